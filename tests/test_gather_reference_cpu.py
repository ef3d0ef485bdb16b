"""The yardstick of test_gpu_gather_reference.py can fail: the float32 evaluation of the kernels' arithmetic sits inside the
derived bounds at every case (x bit-equal to the rounded float64 row + pe); the case table reaches every instantiation, both
rounds and both column trips of each path, and the second trip of the pool backward's grid-stride loop; and every way a kernel
of csrc/gather.hip could plausibly go wrong -- evaluated in float64 at the very cases the GPU tests run -- is rejected at every
case where it can change a result."""
import pytest
import torch

import gather_ref as GA

POOL_IDS = [GA.pool_id(c) for c in GA.POOL_CASES]


@pytest.mark.parametrize("c", GA.POOL_CASES, ids=POOL_IDS)
def test_float32_pool_is_inside_the_derived_bound(c):
    """Index-order float32 sum times the rounded reciprocal against the float64 masked mean: within gamma(n + 1) sum|row| / n;
    x the same bits; the flag as the reference says.  The float64 evaluation is the reference itself."""
    inp = GA.pool_inputs(c)
    ref = GA.pool_reference(c, inp)
    x, pooled, flag = GA.pool_evaluate(c, inp, GA.F32)
    assert not GA.pool_problems(ref, x, pooled, flag)
    assert GA.pool_worst(ref, pooled) <= 1.0
    assert bool(torch.isfinite(ref["x"]).all()) and bool(torch.isfinite(ref["pooled"]).all())  # NaN in padded rows never arrives


@pytest.mark.parametrize("mut", GA.POOL_MUTANTS)
def test_pool_mutant_is_rejected_at_every_case_where_it_changes_a_result(mut):
    n_cases, missed = 0, []
    for c in GA.POOL_CASES:
        if not GA.pool_applies(mut, c):
            continue
        n_cases += 1
        inp = GA.pool_inputs(c)
        if not GA.pool_problems(GA.pool_reference(c, inp), *GA.pool_evaluate(c, inp, GA.F64, mut)):
            missed.append(GA.pool_id(c))
    print(f"gather-mutant {mut:<10} rejected at {n_cases - len(missed)} of {n_cases} cases")
    assert n_cases > 0 and not missed, missed


@pytest.mark.parametrize("c", GA.BWD_CASES, ids=[GA.bwd_id(c) for c in GA.BWD_CASES])
def test_float32_pool_backward_is_inside_the_derived_bound_and_its_mutant_is_not(c):
    dx0, dp, lens = GA.bwd_inputs(c)
    assert not GA.bwd_problems(c, dx0, dp, lens, GA.bwd_evaluate(c, dx0, dp, lens, GA.F32))
    if lens:  # the backward reaching padded rows
        assert GA.bwd_problems(c, dx0, dp, lens, GA.bwd_evaluate(c, dx0, dp, lens, GA.F64, "pad"))


def test_case_table_reaches_every_path():
    P = GA.POOL_CASES
    for path in ("v4", "v1"):
        mine = [c for c in P if GA.pool_path(c) == path]
        assert any(c.H > GA.pool_round(c) for c in mine) and any(c.H <= GA.pool_round(c) for c in mine)  # one round, and two
        assert any(c.dim > GA.pool_columns(c) for c in mine)  # a second column trip
        assert {c.lens for c in mine} >= {None, "list", "bad_lo", "bad_hi", "null"} and any(c.oob for c in mine)
        assert {c.form for c in mine} == {"ids", "emb"} and {c.pe for c in mine} == {True, False}
    assert {c.how for c in P if c.group == "switch"} == {"ld", "pe_off", "pooled_off", "x_off", "out1"}
    assert {(c.dim, c.H, c.B) for c in P if c.group == "vec"} == set(GA.VEC_SHAPES)
    assert {(c.dim, c.H) for c in P if c.group == "scalar"} == {(50, 7), (50, 33), (65, 65), (1, 128)}
    for c in P:
        if c.lens == "list":
            raw, lens = GA.pool_lengths(c)
            assert raw == lens and set(raw) == {v for v in (1, 2, 31, 32, 33, 63, 64, 65, c.H - 1, c.H) if v <= c.H}
        if c.oob:  # an out-of-range id in both rounds
            ids = GA.pool_inputs(c)["ids"]
            bad = ((ids < 0) | (ids >= GA.N_ROWS)).any(0)
            assert bool(bad[:GA.pool_round(c)].any()) and bool(bad[GA.pool_round(c):].any())
    G = GA.GATHER_CASES
    assert {GA.gather_instantiation(c) for c in G} == set(GA.GATHER_KERNELS)
    assert {c.dim for c in G} == set(GA.GATHER_DIMS) and {c.how for c in G} == {None, "ld", "out_off"}
    for d in GA.GATHER_DIMS:
        r = GA.rows_per_workgroup(GA.gather_instantiation(GA.Gather(d, 1)))
        assert {c.n_ids for c in G if c.dim == d and c.how is None and c.flag} == {1, r - 1, r + 1, 1000}
        assert any(c.dim == d and not c.flag for c in G)
    assert any(c.B * c.H * c.dim > GA.BWD_GRID for c in GA.BWD_CASES) and any(c.B * c.H * c.dim <= GA.BWD_GRID for c in GA.BWD_CASES)


def test_gather_reference_zero_fills_and_flags():
    for c in GA.GATHER_CASES:
        table, ids = GA.gather_inputs(c)
        out, flag = GA.gather_reference(c, table, ids)
        bad = (ids < 0) | (ids >= GA.GATHER_ROWS)
        assert bool((out[bad] == 0).all()) and bool((out[~bad] == table[ids[~bad]]).all())
        assert flag == int(bool(bad.any()) and c.flag) and (c.n_ids < 4 or bool(bad.any()))
