"""The yardstick of test_gpu_index_reference.py can fail: each reference of tests/index_ref.py equals a second, slower
restatement (a dict of lists per row or owner) at every case the GPU test runs; the dense bound holds for the float32 evaluation
by the reference alone; the case tables reach every path, digit boundary and tile edge they claim to; and every deliberately
wrong variant of a kernel (index_ref.PLAN_MUTANTS, ROUTE_MUTANTS) is caught by at least one case on the path whose kernel can
make that mistake."""
import numpy as np
import pytest

import index_ref as IR

PLAN_ALL = IR.PLAN_CASES + [IR.SWITCH] + [c for g in IR.PLAN_JOB_GROUPS for c in IR.plan_job_cases(g)]
ROUTE_ALL = IR.ROUTE_CASES + [c for g in IR.ROUTE_JOB_GROUPS.values() for c in g]
CPU_DENSE = {}


def _same(a, b):
    return all(np.array_equal(x, y) and np.asarray(x).dtype == np.asarray(y).dtype for x, y in zip(a, b))


@pytest.mark.parametrize("c", PLAN_ALL, ids=[c.name for c in PLAN_ALL])
def test_plan_reference_equals_its_restatement(c):
    ids = IR.plan_ids(c)
    ref = IR.plan_reference(ids, c.n_rows)
    assert len(ids) == c.n and _same(ref, IR.plan_slow(ids, c.n_rows))
    assert not IR.plan_problems(ref, IR.evaluate(c))  # the kernels' scheme without a mistake is the reference
    assert ref.seg_begin[ref.n_unique] == c.n and len(ref.seg_begin) == ref.n_unique + 1
    assert ref.flag == int(c.pattern == "oob")


@pytest.mark.parametrize("mut", IR.PLAN_MUTANTS)
def test_plan_mutant_is_caught(mut):
    cases = [c for c in PLAN_ALL if IR.plan_applies(mut, c)]
    caught = [c.name for c in cases if IR.plan_problems(IR.plan_reference(IR.plan_ids(c), c.n_rows), IR.evaluate(c, mut))]
    print(f"index-mutant {mut:<16} caught at {len(caught)} of {len(cases)} cases: {' '.join(caught)}")
    assert caught, f"no plan case catches {mut}"
    for path in ("small", "multi"):  # ... on either sort, where both can make the mistake
        if any(IR.plan_path(c.n) == path for c in cases):
            assert any(n.startswith((path, "jobs") if path == "small" else (path, "switch")) for n in caught), (mut, path)


def test_plan_case_table_reaches_what_it_claims():
    P = IR.PLAN_CASES
    small = [c for c in P if IR.plan_path(c.n) == "small" and c.pattern == "uniform"]
    multi = [c for c in P if IR.plan_path(c.n) == "multi" and c.pattern == "uniform"]
    for cases, ns, rows in ((small, IR.SMALL_N, IR.SMALL_ROWS), (multi, tuple(IR.MULTI_GRID), IR.MULTI_ROWS)):
        assert {c.n for c in cases} == set(ns) and {c.n_rows for c in cases} == set(rows)
        assert all(sum(c.n == n for c in cases) >= 2 for n in ns) and all(sum(c.n_rows == r for c in cases) >= 2 for r in rows)
        for c in cases:  # rows 0 and n_rows - 1 are present
            ids = IR.plan_ids(c)
            assert (c.n_rows - 1) in ids and (c.n == 1 or c.n_rows == 1 or 0 in ids), c.name
    assert {IR.plan_passes(c.n_rows, "small") for c in small} == {0, 1, 2, 4, 5, 8}  # 4-bit digits: a boundary and one beyond
    assert {IR.plan_passes(c.n_rows, "multi") for c in multi} == {1, 2, 3, 4}  # 8-bit digits: both ping-pong starts
    assert not IR.plan_needs_attribute(3584) and IR.plan_needs_attribute(3585)
    assert max(c.n for c in P) == 524289 and -(-524289 // IR.SEG_TILE) > 256  # seg_scan_kernel's second trip
    for path in ("small", "multi"):
        mine = [c for c in P if IR.plan_path(c.n) == path]
        assert {c.pattern for c in mine} == set(IR.PATTERNS) | {"uniform"}
        for c in mine:
            ids, ref = IR.plan_ids(c), IR.plan_reference(IR.plan_ids(c), c.n_rows)
            if c.pattern.startswith("distinct"):
                assert ref.n_unique == c.n  # seg_begin[n] is written
            if c.pattern == "equal":
                assert ref.n_unique == 1
            if c.pattern == "edges":
                assert set(IR.edge_heads(c.n)) == set(ref.seg_begin[:-1].tolist())
                edges = (IR.TILE, IR.SEG_TILE) + ((IR.plan_kpt(c.n),) if path == "small" else ())
                for e in edges:  # a head exactly on the edge and on either side of it
                    assert any({m - 1, m, m + 1} <= set(IR.edge_heads(c.n)) for m in range(e, c.n, e)), (c.name, e)
            if c.pattern == "oob":
                want = [c.n_rows if v is None else v for v in IR.BAD_IDS]
                assert [int(ids[p]) for p in (0, c.n // 3, 2 * c.n // 3, c.n - 1)] == want
    jobs = [IR.plan_job_cases(g) for g in IR.PLAN_JOB_GROUPS]
    assert {len(j) for j in jobs} == {1, 2, 3, 4} and {c.n for j in jobs for c in j} >= {1, 513, 3585, 10240}
    assert any(sum(c.pattern == "oob" for c in j) == 1 and len(j) > 1 for j in jobs)
    assert all(c.n <= IR.PS_MAX for j in jobs for c in j)
    sw = IR.plan_ids(IR.SWITCH)
    assert len(sw) == IR.PS_MAX + 1 and IR.plan_path(len(sw) - 1) == "small"


def _dense(c):
    if c not in CPU_DENSE:
        ids, blocks = IR.dense_inputs(c)
        plan = IR.plan_reference(ids, IR.DENSE_ROWS)
        CPU_DENSE[c] = (ids, blocks, plan, IR.dense_reference(plan, blocks, c.dim))
    return CPU_DENSE[c]


@pytest.mark.parametrize("c", IR.DENSE_CASES, ids=[IR.dense_id(c) for c in IR.DENSE_CASES])
def test_dense_reference_equals_its_restatement_and_float32_is_inside_the_bound(c):
    ids, blocks, plan, ref = _dense(c)
    slow = IR.dense_slow(ids, IR.DENSE_ROWS, blocks, c.dim)
    assert sorted(slow) == ref.rows.tolist()
    for k, r in enumerate(ref.rows.tolist()):  # two float64 summation orders: within the float64 bound of the run
        c_k = int(plan.seg_begin[k + 1] - plan.seg_begin[k])
        assert np.all(np.abs(slow[r] - ref.sum64[k]) <= 2 * c_k * 2.0 ** -53 * np.abs(ref.sum64[k]).max() + ref.E[k] * 1e-6)
    worst = IR.dense_worst(ref, ref.f32)
    print(f"index-ref cpu {IR.dense_id(c)} float32 err/E {worst:.3f}")
    assert worst <= 1.0
    single = np.diff(plan.seg_begin) == 1
    assert np.all(ref.E[single] == 0) and np.array_equal(ref.f32[single].astype(np.float64), ref.sum64[single])
    assert bool(plan.flag) == c.oob and (not c.oob or ref.rows[0] == 0)


def test_dense_case_table_reaches_what_it_claims():
    D = IR.DENSE_CASES
    assert {c.dim for c in D} == {1, 63, 64, 65, 128, 200} and {len(c.blocks) for c in D} >= {1, 2, 4}
    assert any(0 in c.blocks for c in D) and any(c.wide for c in D) and any(c.strided is not None for c in D) and any(c.oob for c in D)
    for c in D:
        ids, _, plan, ref = _dense(c)
        if not c.oob:
            assert set(IR.DENSE_RUNS) <= set(np.diff(plan.seg_begin).tolist())
        assert len(set(range(IR.DENSE_ROWS)) - set(ref.rows.tolist())) >= 10  # rows that must keep their NaN


@pytest.mark.parametrize("c", ROUTE_ALL, ids=[IR.route_id(c) for c in ROUTE_ALL])
def test_route_reference_equals_its_restatement(c):
    ids, R = IR.route_ids(c), IR.route_rows(c)
    cap = IR.route_cap(c, ids)
    assert cap >= 1 and len(ids) == c.n
    ref = IR.route_reference(ids, R, c.rpr, c.world, cap)
    assert _same(ref, IR.route_slow(ids, R, c.rpr, c.world, cap)) and not IR.route_problems(ref, IR.evaluate(c))
    assert ref.oob == int(c.pattern.startswith("oob")) and ref.overflow == int(c.cap == "short")
    assert int((ref.slot_of == -1).sum()) == int(np.maximum(ref.counts.astype(np.int64) - cap, 0).sum())
    if c.pattern == "clamp":
        assert c.rpr * c.world < R and bool((ids // c.rpr >= c.world).any())
    if c.pattern == "empty_tail":
        assert c.rpr * c.world > R and ref.counts[-1] == 0
    if c.pattern == "wave64" and c.n >= 64:
        assert len(set((ids[:64] // c.rpr).tolist())) == 64 and c.world == 64


@pytest.mark.parametrize("mut", IR.ROUTE_MUTANTS)
def test_route_mutant_is_caught(mut):
    caught = [IR.route_id(c) for c in ROUTE_ALL if IR.route_problems(IR.route_case_reference(c), IR.evaluate(c, mut))]
    print(f"index-mutant {mut:<16} caught at {len(caught)} of {len(ROUTE_ALL)} cases: {' '.join(caught)}")
    assert caught, f"no route case catches {mut}"
    assert any(IR.route_id(c) in caught for c in IR.ROUTE_CASES), "only a _jobs group catches it"


def test_route_case_table_reaches_what_it_claims():
    Rc = IR.ROUTE_CASES
    assert {c.n for c in Rc} == set(IR.ROUTE_N) and {c.world for c in Rc} == set(IR.ROUTE_WORLDS)
    assert {c.pattern for c in Rc} == {"uniform", "one_owner", "sorted", "wave64", "clamp", "empty_tail", "oob", "oob_null"}
    assert {c.cap for c in Rc} == {"max", "r64", "short"}
    assert any(IR.route_cap(c) % 64 == 0 and IR.route_cap(c) > IR.route_case_reference(c).max_count for c in Rc if c.cap == "r64")
    G = IR.ROUTE_JOB_GROUPS
    assert {len(g) for g in G.values()} == {3, 8} and all(len({c.world for c in g}) == 1 for g in G.values())
    keys = (lambda c: c.n, IR.route_rows, lambda c: c.rpr, IR.route_cap)
    assert all(len({key(c) for c in g}) > 1 for g in G.values() for key in keys)
    assert all(len({key(c) for c in G["eight-w7"]}) == 8 for key in keys), "n, n_rows, rows_per_rank and cap differ in every job"
    assert any((c.world * IR.route_cap(c)) % 1024 for g in G.values() for c in g)


@pytest.mark.parametrize("c", IR.SERVE_CASES, ids=[IR.serve_id(c) for c in IR.SERVE_CASES])
def test_serve_reference_equals_its_restatement(c):
    ids, table = IR.serve_inputs(c)
    local, rows = IR.serve_reference(ids, IR.SERVE_LO, c.n_local, table, c.dim)
    assert _same((local, rows), IR.serve_slow(ids, IR.SERVE_LO, c.n_local, table, c.dim))
    lo = IR.SERVE_LO
    assert {-1, lo - 1, lo, lo + c.n_local - 1, lo + c.n_local} <= set(ids.tolist())
    mine = (ids >= lo) & (ids < lo + c.n_local)
    assert bool((local[~mine] == c.n_local).all()) and not rows[~mine].any() and bool((local[mine] == ids[mine] - lo).all())
    if c.dtype == "bf16" and c.n_local:  # widening is exact: the bf16 bits are the float's upper half
        assert np.array_equal(rows[mine].view(np.uint32) >> 16, table[local[mine]].astype(np.uint32))


def test_serve_case_table_reaches_what_it_claims():
    S = IR.SERVE_CASES
    assert {c.dim for c in S if c.dtype == "f32"} == {4, 128, 132, 1, 50} and {c.dim for c in S if c.dtype == "bf16"} == {50, 128}
    assert {c.n for c in S} == {7, 8, 9} and any(c.n_local == 0 for c in S)
    assert {len(g) for g in IR.SERVE_GROUPS.values()} == {3, 8}
