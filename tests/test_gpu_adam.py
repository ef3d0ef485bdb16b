"""The Adam kernels (csrc/adam.hip) at the C ABI: every schedule against a float64 reference (tests/adam_ref.py) and against
each other bit for bit -- at step counts where the bias corrections have saturated, from states with tiny / denormal /
zero moments, at the chunk tails and fall-backs of the fused sweep, at every row width of the marked sweep, and the
deferred schedule over many steps inside and beyond its step-constant table.  Shapes are the smallest that reach each path.
Every comparison with float64 prints its worst error / bound ratio (profiles/adam_reference_tolerance.txt records them)."""
import ctypes as C
import time

import pytest
import torch

import adam_ref as AR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ZERO = {"p": 0, "m": 0, "v": 0}


@pytest.fixture(scope="module")
def T():
    from two_tower_models_amd import _native as N
    from two_tower_models_amd import ops
    N.load()
    return ops, N


def hyper_at(step):
    """The optimiser's device block with the step count at `step` ([5], [6] are recomputed by every advance)."""
    return torch.tensor([AR.LR, AR.B1, AR.B2, AR.EPS, float(step), 0, 0, 0], dtype=torch.float64, device=DEV)


def dev(ts):
    return [t.clone().to(DEV) for t in ts]


def ptrs(ts):
    return [t.data_ptr() for t in ts]


def same(a, b, what=""):
    for x, y, name in zip(a, b, "pmv"):
        assert torch.equal(x, y), f"{what}: {name} differs in {int((x != y).sum())} elements"


def within(got, ref, group):
    r = AR.ratios(got, ref)
    print(f"[adam-ref] {group}: worst |error| / bound  p {r['p']:.3f}  m {r['m']:.3f}  v {r['v']:.3f}")
    assert AR.violations(got, ref) == ZERO, (group, r)


def lookup(n_rows, D, n, seed):
    """n ids with duplicates, id 0, id n_rows - 1 and one id outside the table (the kernels ignore it) + gradient rows;
    -> ids, rows (CPU) and the dense fp32 gradient, duplicates summed in list order as the plan does."""
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, n_rows, (n,), generator=gen)
    ids[:5] = ids[5:10]
    ids[10], ids[11], ids[12] = 0, n_rows - 1, n_rows + 5
    rows = torch.randn(n, D, generator=gen) * 0.01
    dense = torch.zeros(n_rows, D)
    for i, r in zip(ids.tolist(), rows):
        if i < n_rows:
            dense[i] += r
    return ids, rows, dense


def plan_of(ops, ids_d, rows_d, n_rows):
    plan = ops.RowPlan([ids_d], n_rows + 8)  # ids >= n_rows sort last; the Adam kernels skip their run
    plan.attach([rows_d])
    return plan


def plan_args(plan):
    return [plan.sorted_ids.data_ptr(), plan.perm.data_ptr(), plan.seg_begin.data_ptr(), plan.n_unique.data_ptr()]


def desc_of(N, tables):
    d = (N.AdamTensor * len(tables))()
    for i, (w, m, v) in enumerate(tables):
        d[i].p, d[i].g, d[i].m, d[i].v, d[i].n = w.data_ptr(), None, m.data_ptr(), v.data_ptr(), w.numel()
    return d


def finish_job(N, tabs, n_rows, D, plan, side):
    fj = (N.AdamFinishJob * 1)()
    j = fj[0]
    j.W, j.M, j.V, j.n_rows, j.dim, j.src, j.n_ids = *ptrs(tabs), n_rows, D, C.pointer(plan.sources), plan.n
    j.sorted_ids, j.perm, j.seg_begin, j.n_unique = plan_args(plan)
    j.side, j.side_bytes = (None, 0) if side is None else (side.data_ptr(), side.numel())
    return fj


# ------------------------------------------------------------------ a. one step, every path, against float64
@pytest.mark.parametrize("D", AR.WIDTHS)
@pytest.mark.parametrize("step", [1, 2, 10, 1000, 65536, 10 ** 6])
def test_one_step_every_schedule_against_float64(T, step, D):
    """One step at `step` from edge_state: the single call, plan-stash / sweep / finish, id-stash / fused sweep / merged finish,
    the marked trio (power-of-two widths) and the deferred advance / lazy / flush (table of 2048 steps: steps 65 536 and
    10^6 take the in-kernel constants) give the same bits; the single call and tt_adam_dense on the dense gradient are
    within bounds of adam_step64 for touched and untouched rows; hyper[4..6] are the host's doubles."""
    ops, N = T
    lib = N.load()
    n_rows, n = 97, 64
    state = AR.edge_state(n_rows, D, step % 7)
    ids, rows, dense = lookup(n_rows, D, n, 100 + D)
    ids_d, rows_d = ids.to(DEV), rows.to(DEV)
    ref = AR.bounds(*state, [dense], step)
    side_bytes = lib.tt_adam_table_workspace_bytes(n, D)
    results = {}

    # 1. tt_adam_table
    hyper, tabs = hyper_at(step - 1), dev(state)
    N.check(lib.tt_adam_advance(hyper.data_ptr(), N.stream()), "advance")
    plan = plan_of(ops, ids_d, rows_d, n_rows)
    ws = torch.empty(side_bytes, dtype=torch.uint8, device=DEV)
    N.check(lib.tt_adam_table(*ptrs(tabs), n_rows, D, hyper.data_ptr(), C.byref(plan.sources), n, *plan_args(plan),
                              ws.data_ptr(), side_bytes, N.stream()), "tt_adam_table")
    results["table"] = tabs
    want_h = AR.hyper64(step)
    got_h = [float(x) for x in hyper[4:7].cpu()]
    print(f"[adam-ref] hyper[4..6] at step {step}: device {got_h} host {list(want_h)}")
    assert got_h == list(want_h)
    assert int(hyper.view(torch.int64)[7]) == 0  # the sweep's two chunk counters are re-armed

    # 2. plan-stash -> sweep -> finish
    hyper, tabs = hyper_at(step - 1), dev(state)
    N.check(lib.tt_adam_advance(hyper.data_ptr(), N.stream()), "advance")
    side = torch.empty(side_bytes, dtype=torch.uint8, device=DEV)
    N.check(lib.tt_adam_table_stash(*ptrs(tabs), n_rows, D, n, *plan_args(plan), side.data_ptr(), side_bytes, N.stream()), "stash")
    N.check(lib.tt_adam_table_sweep(*ptrs(tabs), n_rows, D, hyper.data_ptr(), N.stream()), "sweep")
    N.check(lib.tt_adam_table_finish(*ptrs(tabs), n_rows, D, hyper.data_ptr(), C.byref(plan.sources), n, *plan_args(plan),
                                     side.data_ptr(), side_bytes, N.stream()), "finish")
    results["stash/sweep/finish"] = tabs

    # 3. begin_ids (advance + id-stash) -> tables_sweep -> tables_finish
    hyper, tabs = hyper_at(step - 1), dev(state)
    side = torch.empty(side_bytes, dtype=torch.uint8, device=DEV)
    jobs = (N.AdamStashJob * 1)()
    j = jobs[0]
    j.W, j.M, j.V, j.n_rows, j.dim, j.ids, j.n_ids, j.side, j.side_bytes = *ptrs(tabs), n_rows, D, ids_d.data_ptr(), n, side.data_ptr(), side_bytes
    N.check(lib.tt_adam_begin_ids(hyper.data_ptr(), None, 0, jobs, 1, N.stream()), "begin_ids")
    N.check(lib.tt_adam_tables_sweep(desc_of(N, [tabs]), 1, hyper.data_ptr(), 0, N.stream()), "tables_sweep")
    N.check(lib.tt_adam_tables_finish(finish_job(N, tabs, n_rows, D, plan, side), 1, hyper.data_ptr(), N.stream()), "tables_finish")
    results["begin_ids/tables_sweep/tables_finish"] = tabs
    assert [float(x) for x in hyper[4:7].cpu()] == list(want_h)

    # 4. mark -> marked sweep -> finish from the table
    if lib.tt_adam_marked_supported(D):
        hyper, tabs = hyper_at(step - 1), dev(state)
        N.check(lib.tt_adam_advance(hyper.data_ptr(), N.stream()), "advance")
        words = lib.tt_adam_marks_words(n_rows)
        marks = torch.full((words,), -1, dtype=torch.int32, device=DEV)
        N.check(lib.tt_adam_mark_rows(ids_d.data_ptr(), n, n_rows, marks.data_ptr(), words, N.stream()), "mark_rows")
        N.check(lib.tt_adam_tables_sweep_marked(desc_of(N, [tabs]), (C.c_int64 * 1)(D), (C.c_void_p * 1)(marks.data_ptr()), 1,
                                                hyper.data_ptr(), 0, N.stream()), "sweep_marked")
        N.check(lib.tt_adam_tables_finish(finish_job(N, tabs, n_rows, D, plan, None), 1, hyper.data_ptr(), N.stream()), "tables_finish")
        results["marked"] = tabs

    # 5. deferred: advance_tab -> lazy (looked-up rows) -> flush (all others)
    hyper, tabs = hyper_at(step - 1), dev(state)
    tab_steps = 2048
    tab = torch.zeros(2 * tab_steps, dtype=torch.float32, device=DEV)
    last = torch.full((n_rows,), step - 1, dtype=torch.int32, device=DEV)
    N.check(lib.tt_adam_advance_tab(hyper.data_ptr(), tab.data_ptr(), tab_steps, N.stream()), "advance_tab")
    N.check(lib.tt_adam_table_lazy(*ptrs(tabs), n_rows, D, hyper.data_ptr(), C.byref(plan.sources), n, *plan_args(plan),
                                   ws.data_ptr(), side_bytes, last.data_ptr(), tab.data_ptr(), tab_steps, N.stream()), "lazy")
    N.check(lib.tt_adam_table_flush(*ptrs(tabs), n_rows, D, last.data_ptr(), hyper.data_ptr(), tab.data_ptr(), tab_steps,
                                    N.stream()), "flush")
    results["deferred"] = tabs
    assert [float(x) for x in hyper[4:7].cpu()] == list(want_h)
    assert bool((last == step).all())
    if step < tab_steps:  # the table holds what every dense kernel of this step saw
        assert tab[2 * step].item() == torch.tensor(-want_h[1], dtype=torch.float64).float().item()
        assert tab[2 * step + 1].item() == torch.tensor(1.0 / want_h[2], dtype=torch.float64).float().item()
    else:
        assert not bool(tab.any())

    torch.cuda.synchronize()
    first = results["table"]
    for name, tabs in results.items():
        same(first, tabs, name)
    within(first, ref, f"a. one step: tt_adam_table, step {step}, D {D}")
    need = AR.measured_constants([x.cpu() for x in first], *state, dense, step)  # (the oracle needs ORACLE_C; the bound allows 4 x)
    print(f"[adam-ref] a. constants tt_adam_table needs, step {step}, D {D}:  c_p {need['p']:.3f}  c_m {need['m']:.3f}  c_v {need['v']:.3f}")
    touched = torch.zeros(n_rows, dtype=torch.bool)
    touched[ids[ids < n_rows]] = True
    assert not torch.equal(first[1].cpu()[touched], state[1][touched]) and bool((dense[~touched] == 0).all())

    # tt_adam_dense on the same arrays, flattened, with the dense gradient
    hyper, tabs = hyper_at(step - 1), [t.reshape(-1) for t in dev(state)]
    N.check(lib.tt_adam_advance(hyper.data_ptr(), N.stream()), "advance")
    g_d = dense.reshape(-1).to(DEV)
    d = desc_of(N, [tabs])
    d[0].g = g_d.data_ptr()
    N.check(lib.tt_adam_dense(d, 1, hyper.data_ptr(), N.stream()), "tt_adam_dense")
    torch.cuda.synchronize()
    within([t.view(n_rows, D) for t in tabs], ref, f"a. one step: tt_adam_dense, step {step}, D {D}")


def test_zero_moments_leave_p_alone_with_eps_zero(T):
    """eps = 0 is compared with nothing but this: m = v = 0 must leave p unchanged (the 1e-30 floor documented at
    adam_ratio; torch itself returns NaN there)."""
    ops, N = T
    lib = N.load()
    p0, m0, v0 = AR.edge_state(16, 32, 0)
    hyper = torch.tensor([AR.LR, AR.B1, AR.B2, 0.0, 9.0, 0, 0, 0], dtype=torch.float64, device=DEV)
    tabs = dev((p0, m0, v0))
    N.check(lib.tt_adam_advance(hyper.data_ptr(), N.stream()), "advance")
    N.check(lib.tt_adam_table_sweep(*ptrs(tabs), 16, 32, hyper.data_ptr(), N.stream()), "sweep")
    torch.cuda.synchronize()
    for r in (1, 8):
        assert torch.equal(tabs[0][r].cpu(), p0[r]) and not bool(tabs[1][r].any()) and not bool(tabs[2][r].any())
    assert bool(torch.isfinite(tabs[0][9:]).all())


# ------------------------------------------------------------------ b. the fused sweep
SWEEP_STEP = 7


def _sweep_ref(cache, n, seed, k):
    key = (n, seed, k)
    if key not in cache:
        cache[key] = AR.bounds(*AR.edge_flat(n, seed), [None] * k, [SWEEP_STEP] * k)  # (no advance between the launches)
    return cache[key]


_SWEEP_REFS = {}


@pytest.mark.parametrize("n", [4, 4092, 4096, 4100, 3 * 4096 + 40, 4099])
def test_fused_sweep_lengths_and_throttle(T, n):
    """tt_adam_tables_sweep (fused launch: this table + a 4100-element one; alone: the per-table launch with the caller's
    throttle) and tt_adam_table_sweep on flat arrays around the 4096-element chunk: full chunk, tails of 1 and 1023
    float4, three chunks and a bit, and n % 4 != 0 (per-table fall-back, scalar tail) -- for 0 (default), 1, 2 and 7
    workgroups.  Same bits everywhere, within bounds of float64, counters zero after every launch."""
    ops, N = T
    lib = N.load()
    state, other = AR.edge_flat(n, 1), AR.edge_flat(4100, 2)
    hyper = hyper_at(SWEEP_STEP - 1)
    N.check(lib.tt_adam_advance(hyper.data_ptr(), N.stream()), "advance")
    base, base_other = dev(state), dev(other)
    N.check(lib.tt_adam_table_sweep(*ptrs(base), 1, n, hyper.data_ptr(), N.stream()), "table_sweep")
    N.check(lib.tt_adam_table_sweep(*ptrs(base_other), 4100, 1, hyper.data_ptr(), N.stream()), "table_sweep")
    torch.cuda.synchronize()
    assert int(hyper.view(torch.int64)[7]) == 0
    for n_wgs in (0, 1, 2, 7):
        a, b, alone = dev(state), dev(other), dev(state)
        N.check(lib.tt_adam_tables_sweep(desc_of(N, [a, b]), 2, hyper.data_ptr(), n_wgs, N.stream()), "tables_sweep")
        torch.cuda.synchronize()
        assert int(hyper.view(torch.int64)[7]) == 0, n_wgs
        N.check(lib.tt_adam_tables_sweep(desc_of(N, [alone]), 1, hyper.data_ptr(), n_wgs, N.stream()), "tables_sweep")
        torch.cuda.synchronize()
        assert int(hyper.view(torch.int64)[7]) == 0, n_wgs
        same(base, a, f"fused, {n_wgs} workgroups")
        same(base_other, b, f"fused (second table), {n_wgs} workgroups")
        same(base, alone, f"one table, {n_wgs} workgroups")
    within(base, _sweep_ref(_SWEEP_REFS, n, 1, 1), f"b. sweep: n {n}")
    within(base_other, _sweep_ref(_SWEEP_REFS, 4100, 2, 1), "b. sweep: n 4100 (second table)")


@pytest.mark.parametrize("n_wgs", [0, 1, 2, 7])
def test_fused_sweep_four_tables_misaligned_back_to_back_and_a_fifth(T, n_wgs):
    """Four tables (4096, 4, 8200, 4100 elements) in one launch; the same four with the third one 16-byte misaligned
    (x[1:]: every table falls back to its own launch, the misaligned one to the scalar kernel); two launches back to back
    on one hyper block without a host synchronisation (the second starts from counters the first re-armed); a fifth
    table is refused before anything is launched."""
    ops, N = T
    lib = N.load()
    lens = (4096, 4, 8200, 4100)
    states = [AR.edge_flat(L, 10 + i) for i, L in enumerate(lens)]
    hyper = hyper_at(SWEEP_STEP - 1)
    N.check(lib.tt_adam_advance(hyper.data_ptr(), N.stream()), "advance")
    once, twice = [dev(s) for s in states], [dev(s) for s in states]
    for t, L in zip(once, lens):
        N.check(lib.tt_adam_table_sweep(*ptrs(t), 1, L, hyper.data_ptr(), N.stream()), "table_sweep")
    for t, L in zip(twice, lens):
        for _ in range(2):
            N.check(lib.tt_adam_table_sweep(*ptrs(t), L, 1, hyper.data_ptr(), N.stream()), "table_sweep")
            torch.cuda.synchronize()

    fused = [dev(s) for s in states]
    N.check(lib.tt_adam_tables_sweep(desc_of(N, fused), 4, hyper.data_ptr(), n_wgs, N.stream()), "tables_sweep")
    torch.cuda.synchronize()
    assert int(hyper.view(torch.int64)[7]) == 0
    for a, b, L in zip(once, fused, lens):
        same(a, b, f"four tables, n {L}")
    for t, s, L, i in zip(fused, states, lens, range(4)):
        within(t, _sweep_ref(_SWEEP_REFS, L, 10 + i, 1), f"b. four tables: n {L}")

    # the third table one float further into its allocation: not 16-byte aligned
    holders = [[torch.cat([torch.zeros(1), t]).to(DEV) for t in states[2]]]
    mis = [dev(states[0]), dev(states[1]), [h[1:] for h in holders[0]], dev(states[3])]
    assert all(t.data_ptr() % 16 == 4 for t in mis[2])
    N.check(lib.tt_adam_tables_sweep(desc_of(N, mis), 4, hyper.data_ptr(), n_wgs, N.stream()), "tables_sweep")
    torch.cuda.synchronize()
    assert int(hyper.view(torch.int64)[7]) == 0
    for a, b, L in zip(once, mis, lens):
        same(a, b, f"misaligned third table, n {L}")
    assert all(float(h[0]) == 0.0 for h in holders[0])  # the element in front of the view is not the sweep's

    back = [dev(s) for s in states]
    d = desc_of(N, back)
    N.check(lib.tt_adam_tables_sweep(d, 4, hyper.data_ptr(), n_wgs, N.stream()), "tables_sweep")
    N.check(lib.tt_adam_tables_sweep(d, 4, hyper.data_ptr(), n_wgs, N.stream()), "tables_sweep")
    torch.cuda.synchronize()
    assert int(hyper.view(torch.int64)[7]) == 0
    for a, b, L in zip(twice, back, lens):
        same(a, b, f"two launches back to back, n {L}")
    within(back[2], _sweep_ref(_SWEEP_REFS, 8200, 12, 2), "b. two launches back to back: n 8200")

    five = [dev(s) for s in states] + [dev(states[0])]
    assert lib.tt_adam_tables_sweep(desc_of(N, five), 5, hyper.data_ptr(), n_wgs, N.stream()) != 0
    torch.cuda.synchronize()
    for t, s in zip(five, states + [states[0]]):
        same(t, dev(s), "a fifth table: nothing may be launched")


# ------------------------------------------------------------------ c. the marked sweep
def _pattern_ids(pattern, n_rows):
    if pattern == "none":
        return torch.tensor([n_rows + 5, n_rows + 1, n_rows + 5])  # ids outside the table mark nothing
    if pattern == "all":
        return torch.cat([torch.arange(n_rows), torch.tensor([3, 3, n_rows + 5])])
    if pattern == "alternating":
        return torch.cat([torch.arange(0, n_rows, 2), torch.tensor([4, n_rows + 5])])
    if pattern == "last":
        return torch.tensor([n_rows - 1, n_rows - 1, n_rows + 5])
    return torch.tensor([0, n_rows + 5, 0])  # "first"


@pytest.mark.parametrize("pattern", ["none", "all", "alternating", "last", "first"])
@pytest.mark.parametrize("D,n_rows", [(32, 129), (512, 67), (1024, 35), (4096, 9)])
def test_marked_sweep_wide_rows_and_mark_patterns(T, D, n_rows, pattern):
    """tt_adam_tables_sweep_marked where a 16 KB chunk holds 128 rows and one more (D = 32, 129 rows), 2 rows, 1 row and a
    quarter of a row (D = 512, 1024, 4096): marked rows keep their bits, unmarked rows are tt_adam_table_sweep's and within
    bounds, and after the finish from the table (side == NULL) everything is tt_adam_table's."""
    ops, N = T
    lib = N.load()
    assert lib.tt_adam_marked_supported(D) == 1
    state = AR.edge_state(n_rows, D, 3)
    ids = _pattern_ids(pattern, n_rows)
    n = ids.numel()
    gen = torch.Generator().manual_seed(D + n_rows)
    rows = torch.randn(n, D, generator=gen) * 0.01
    ids_d, rows_d = ids.to(DEV), rows.to(DEV)
    marked = torch.zeros(n_rows, dtype=torch.bool)
    marked[ids[ids < n_rows]] = True
    hyper = hyper_at(SWEEP_STEP - 1)
    N.check(lib.tt_adam_advance(hyper.data_ptr(), N.stream()), "advance")

    swept = dev(state)
    N.check(lib.tt_adam_table_sweep(*ptrs(swept), n_rows, D, hyper.data_ptr(), N.stream()), "table_sweep")
    single = dev(state)
    plan = plan_of(ops, ids_d, rows_d, n_rows)
    wsn = lib.tt_adam_table_workspace_bytes(n, D)
    ws = torch.empty(wsn, dtype=torch.uint8, device=DEV)
    N.check(lib.tt_adam_table(*ptrs(single), n_rows, D, hyper.data_ptr(), C.byref(plan.sources), n, *plan_args(plan),
                              ws.data_ptr(), wsn, N.stream()), "tt_adam_table")

    tabs = dev(state)
    words = lib.tt_adam_marks_words(n_rows)
    marks = torch.full((words,), -1, dtype=torch.int32, device=DEV)
    N.check(lib.tt_adam_mark_rows(ids_d.data_ptr(), n, n_rows, marks.data_ptr(), words, N.stream()), "mark_rows")
    N.check(lib.tt_adam_tables_sweep_marked(desc_of(N, [tabs]), (C.c_int64 * 1)(D), (C.c_void_p * 1)(marks.data_ptr()), 1,
                                            hyper.data_ptr(), 0, N.stream()), "sweep_marked")
    torch.cuda.synchronize()
    assert int(hyper.view(torch.int64)[7]) == 0
    for t, s, w, name in zip(tabs, state, swept, "pmv"):
        t, w = t.cpu(), w.cpu()
        assert torch.equal(t[marked].view(torch.int32), s[marked].view(torch.int32)), f"marked rows moved: {name}"
        assert torch.equal(t[~marked], w[~marked]), f"unmarked rows differ from the plain sweep: {name}"
    ref = AR.bounds(*state, [None], SWEEP_STEP)
    keep = ~marked
    if bool(keep.any()):
        sub = AR.Ref(*[x[keep] for x in ref])
        within([t.cpu()[keep] for t in tabs], sub, f"c. marked sweep: D {D}, {pattern}")
    N.check(lib.tt_adam_tables_finish(finish_job(N, tabs, n_rows, D, plan, None), 1, hyper.data_ptr(), N.stream()), "tables_finish")
    torch.cuda.synchronize()
    same(single, tabs, "after the finish from the table")


def test_marked_sweep_two_marked_tables_of_different_widths(T):
    """Two marked tables (D = 32: 300 rows = two chunks and a bit; D = 256: 37 rows) and an unmarked third in ONE launch:
    each table's chunks read their own bitmap at their own rows-per-chunk."""
    ops, N = T
    lib = N.load()
    shapes = [(300, 32), (37, 256), (11, 64)]
    states = [AR.edge_state(r, D, 20 + i) for i, (r, D) in enumerate(shapes)]
    hyper = hyper_at(SWEEP_STEP - 1)
    N.check(lib.tt_adam_advance(hyper.data_ptr(), N.stream()), "advance")
    gen = torch.Generator().manual_seed(9)
    tabs, swept, bitmaps, masks = [dev(s) for s in states], [dev(s) for s in states], [], []
    for (r, D), t in zip(shapes, swept):
        N.check(lib.tt_adam_table_sweep(*ptrs(t), r, D, hyper.data_ptr(), N.stream()), "table_sweep")
    for r, D in shapes[:2]:
        ids = torch.randint(0, r, (r // 3,), generator=gen)
        ids[0], ids[1] = r - 1, r + 5
        mask = torch.zeros(r, dtype=torch.bool)
        mask[ids[ids < r]] = True
        masks.append(mask)
        words = lib.tt_adam_marks_words(r)
        bm = torch.full((words,), -1, dtype=torch.int32, device=DEV)
        ids_d = ids.to(DEV)
        N.check(lib.tt_adam_mark_rows(ids_d.data_ptr(), ids.numel(), r, bm.data_ptr(), words, N.stream()), "mark_rows")
        bitmaps.append(bm)
    masks.append(torch.zeros(shapes[2][0], dtype=torch.bool))
    dims = (C.c_int64 * 3)(*[D for _, D in shapes])
    mp = (C.c_void_p * 3)(bitmaps[0].data_ptr(), bitmaps[1].data_ptr(), None)
    N.check(lib.tt_adam_tables_sweep_marked(desc_of(N, tabs), dims, mp, 3, hyper.data_ptr(), 2, N.stream()), "sweep_marked")
    torch.cuda.synchronize()
    assert int(hyper.view(torch.int64)[7]) == 0
    for t3, s3, w3, mask in zip(tabs, states, swept, masks):
        assert bool(mask.any()) != (mask is masks[2])
        for t, s, w in zip(t3, s3, w3):
            assert torch.equal(t.cpu()[mask].view(torch.int32), s[mask].view(torch.int32))
            assert torch.equal(t.cpu()[~mask], w.cpu()[~mask])


# ------------------------------------------------------------------ d. the deferred schedule over many steps
_DEFERRED_REFS = {}


@pytest.mark.parametrize("tab_steps", [8, 1])
@pytest.mark.parametrize("D", AR.WIDTHS)
def test_deferred_schedule_over_forty_steps(T, D, tab_steps):
    """tt_adam_rows_catchup / tt_adam_advance_tab / tt_adam_table_lazy / tt_adam_table_flush at the ABI, 40 steps from
    step 6 on 257 rows: 48 ids per step from a sliding window (rows recur after 1 .. ~30 idle steps, rows 250 .. 256
    never), duplicates (the atomic claim), one id outside the table, every other step a prefetching catch-up of the next
    step's ids.  A step-constant table of 8 steps makes replays start inside it and end beyond it (replay_consts' double
    arithmetic), one of 1 step keeps them beyond it throughout; all three replay widths (D <= 64, <= 128, wider) and, at
    D = 320, a row whose first 256 columns are dead and whose last 64 live.  Against tt_adam_advance + tt_adam_table on
    a copy, every step: the rows read back after each catch-up, and after the flush everything, bit for bit."""
    ops, N = T
    lib = N.load()
    n_rows, n, K, start = 257, 48, 40, 6
    state = AR.edge_state(n_rows, D, 5)
    gen = torch.Generator().manual_seed(D)
    lookups = []
    for s in range(K):
        ids = (torch.randint(0, 40, (n,), generator=gen) + 7 * s) % 250
        ids[1] = ids[0]
        ids[5] = n_rows + 3
        if s % 9 == 0:
            ids[7] = 2  # the row with dead and live column chunks (D = 320) comes back after long gaps
        rows = torch.randn(n, D, generator=gen) * 0.01
        dense = torch.zeros(n_rows, D)
        for i, r in zip(ids.tolist(), rows):
            if i < n_rows:
                dense[i] += r
        lookups.append((ids.to(DEV), rows.to(DEV), ids[ids < n_rows].to(DEV), dense))

    lazy, comp = dev(state), dev(state)
    h_lazy, h_comp = hyper_at(start), hyper_at(start)
    tab = torch.zeros(2 * tab_steps, dtype=torch.float32, device=DEV)
    last = torch.full((n_rows,), start, dtype=torch.int32, device=DEV)
    wsn = lib.tt_adam_table_workspace_bytes(n, D)
    ws = torch.empty(wsn, dtype=torch.uint8, device=DEV)

    def catch_up(ids_d):
        N.check(lib.tt_adam_rows_catchup(*ptrs(lazy), n_rows, D, ids_d.data_ptr(), n, last.data_ptr(), h_lazy.data_ptr(),
                                         tab.data_ptr(), tab_steps, N.stream()), "rows_catchup")

    for s, (ids_d, rows_d, valid, _) in enumerate(lookups):
        catch_up(ids_d)
        for a, b, name in zip(lazy, comp, "pmv"):
            assert torch.equal(a[valid], b[valid]), f"step {s}: looked-up rows are not current ({name})"
        assert bool((last[valid] == start + s).all())
        plan = plan_of(ops, ids_d, rows_d, n_rows)
        N.check(lib.tt_adam_advance_tab(h_lazy.data_ptr(), tab.data_ptr(), tab_steps, N.stream()), "advance_tab")
        N.check(lib.tt_adam_table_lazy(*ptrs(lazy), n_rows, D, h_lazy.data_ptr(), C.byref(plan.sources), n, *plan_args(plan),
                                       ws.data_ptr(), wsn, last.data_ptr(), tab.data_ptr(), tab_steps, N.stream()), "lazy")
        if s % 2 == 1 and s + 1 < K:
            catch_up(lookups[s + 1][0])  # prefetch: the next step's rows, early
        N.check(lib.tt_adam_advance(h_comp.data_ptr(), N.stream()), "advance")
        N.check(lib.tt_adam_table(*ptrs(comp), n_rows, D, h_comp.data_ptr(), C.byref(plan.sources), n, *plan_args(plan),
                                  ws.data_ptr(), wsn, N.stream()), "tt_adam_table")
    assert torch.equal(h_lazy[:7], h_comp[:7]) and float(h_lazy[4]) == start + K
    assert not torch.equal(lazy[0], comp[0])  # something WAS deferred
    assert bool((last[250:] == start).all())
    flush = lambda: N.check(lib.tt_adam_table_flush(*ptrs(lazy), n_rows, D, last.data_ptr(), h_lazy.data_ptr(), tab.data_ptr(),
                                                    tab_steps, N.stream()), "flush")
    flush()
    torch.cuda.synchronize()
    same(comp, lazy, "after the flush")
    assert bool((last == start + K).all())
    again = [t.clone() for t in lazy]
    flush()
    torch.cuda.synchronize()
    same(again, lazy, "a second flush")
    assert bool((last == start + K).all())
    if D not in _DEFERRED_REFS:
        _DEFERRED_REFS[D] = AR.bounds(*state, [d for _, _, _, d in lookups], start + 1)
    within(comp, _DEFERRED_REFS[D], f"d. 40 steps: D {D}")


# ------------------------------------------------------------------ e. long idle
_IDLE = {}


@pytest.mark.parametrize("tab_steps", [2048, 16])
def test_deferred_flush_after_1200_idle_steps(T, tab_steps):
    """64 rows x 128 columns, no lookups: 1200 x (tt_adam_advance + tt_adam_table_sweep) against 1200 x tt_adam_advance_tab
    and ONE tt_adam_table_flush, constants from the table (2048 steps) and from the kernel's own doubles (16).  fp32
    m <- fma(0.1, -m, m) does not decay to zero: it sticks at a few denormal units after ~940 steps, and a replay (or
    anything that skips rows "that cannot change") has to end on exactly those bits.  The 1200 launch pairs take well
    under a second (printed), so the count is the issue's, not lowered."""
    ops, N = T
    lib = N.load()
    n_rows, D, K = 64, 128, 1200
    state = AR.edge_state(n_rows, D, 4)
    if "swept" not in _IDLE:
        swept, hyper = dev(state), hyper_at(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            N.check(lib.tt_adam_advance(hyper.data_ptr(), N.stream()), "advance")
            N.check(lib.tt_adam_table_sweep(*ptrs(swept), n_rows, D, hyper.data_ptr(), N.stream()), "sweep")
        torch.cuda.synchronize()
        print(f"[adam-ref] e. {K} advance + sweep launch pairs: {time.perf_counter() - t0:.3f} s")
        _IDLE["swept"], _IDLE["hyper"] = swept, hyper
        _IDLE["ref"] = AR.bounds(*state, [None] * K, 1)
    swept = _IDLE["swept"]
    lazy, hyper = dev(state), hyper_at(0)
    tab = torch.zeros(2 * tab_steps, dtype=torch.float32, device=DEV)
    last = torch.zeros(n_rows, dtype=torch.int32, device=DEV)
    for _ in range(K):
        N.check(lib.tt_adam_advance_tab(hyper.data_ptr(), tab.data_ptr(), tab_steps, N.stream()), "advance_tab")
    same(dev(state), lazy, "nothing moves before the flush")
    N.check(lib.tt_adam_table_flush(*ptrs(lazy), n_rows, D, last.data_ptr(), hyper.data_ptr(), tab.data_ptr(), tab_steps,
                                    N.stream()), "flush")
    torch.cuda.synchronize()
    assert torch.equal(hyper[:7], _IDLE["hyper"][:7]) and float(hyper[4]) == K and bool((last == K).all())
    same(swept, lazy, "1200 idle steps")
    for a, b in zip(swept, lazy):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    m = lazy[1].cpu()
    stuck = (m != 0) & (m.abs() < 2.0 ** -126)
    print(f"[adam-ref] e. m after {K} idle steps: {int(stuck.sum())} non-zero subnormals, {int((m == 0).sum())} zeros, "
          f"max |m| {float(m.abs().max()):.3e}")
    assert int(stuck.sum()) > 0 and float(m.abs().max()) < 1e-43
    within(lazy, _IDLE["ref"], f"e. long idle: table of {tab_steps} steps")


# ------------------------------------------------------------------ f. through the optimiser
def _batches(g, base, n, seed, window):
    n_users, n_items = int(g["cfg"][0]), int(g["cfg"][3])
    gen = torch.Generator().manual_seed(seed)
    out = []
    for s in range(n):
        b = [t.clone() for t in base]
        if window:  # ids from a sliding window: rows recur after 1 .. 6 idle steps
            b[0] = ((torch.randint(0, 40, tuple(base[0].shape), generator=gen) + 13 * s) % n_users).to(DEV)
            b[3] = ((torch.randint(0, 50, tuple(base[3].shape), generator=gen) + 17 * s) % n_items).to(DEV)
        else:
            b[0] = torch.randint(0, n_users, tuple(base[0].shape), generator=gen).to(DEV)
            b[3] = torch.randint(0, n_items, tuple(base[3].shape), generator=gen).to(DEV)
        out.append(b)
    return out


def _eager(model, opt, b):
    loss = model.train_forward(*b)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss


def _same_models(a, aopt, b, bopt):
    for (k, x), (_, y) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(x, y), k
    for pa, pb in zip(aopt._params, bopt._params):
        assert torch.equal(aopt.state[pa]["exp_avg"], bopt.state[pb]["exp_avg"])
        assert torch.equal(aopt.state[pa]["exp_avg_sq"], bopt.state[pb]["exp_avg_sq"])


def test_lazy_optimiser_through_table_growths(golden, monkeypatch):
    """test_lazy_adam_is_bit_identical_to_dense's step sequence, 20 steps, with the step-constant table starting at 4 steps:
    DenseExactAdam._advance_lazy doubles it at steps 3, 7 and 15."""
    import two_tower_models_amd as A
    from two_tower_models_amd import optim
    from test_gpu_models import batch_of, make_model
    monkeypatch.setattr(optim, "_TAB_MIN_STEPS", 4)
    g = golden("g1_base_tiny")
    steps = _batches(g, batch_of(g), 20, 77, window=True)
    models, opts = [], []
    for lazy in (False, True):
        model = make_model("base", g)
        opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep=False, lazy=lazy)
        for s, b in enumerate(steps):
            loss = model.train_forward(*b)
            if lazy and s + 1 < len(steps) and s % 2 == 0:
                nb = steps[s + 1]
                opt.prefetch_rows(model._lookup_plan(nb[0], nb[2], nb[3]))
            opt.zero_grad()
            loss.backward()
            opt.step()
        if lazy:
            assert opt._tab_steps == 32 and opt._tab.numel() == 64
            stale = model.item_id_embedding_arch.weight.detach().clone()
            opt.flush()
            assert not torch.equal(stale, model.item_id_embedding_arch.weight)
        torch.cuda.synchronize()
        assert opt.step_count == len(steps)
        models.append(model)
        opts.append(opt)
    _same_models(models[0], opts[0], models[1], opts[1])


@pytest.mark.parametrize("tab_min,replays,eager_step", [(4, 12, False), (4, 12, True), (16, 10, True)])
def test_graphed_lazy_step_beyond_its_captured_table(golden, monkeypatch, tab_min, replays, eager_step):
    """A deferred optimiser inside GraphedTrainStep with a step-constant table of `tab_min` steps: the graph keeps the
    table pointer and size of its capture, so replays past it take the in-kernel constants (the state of every graphed
    deferred run after 65 536 steps).  eager_step: one eager deferred step after the replays, at a step count where the
    optimiser would double its table, and two more replays.  The graph's replays write and read the table they were
    captured with and nothing else, so a replaced table misses every replayed step (idle rows replayed with constants of
    zero: this test failed that way) -- the table is pinned from the capture on.  With a table of 16 steps and 10 replays
    the eager step is step 14, INSIDE the captured table: the replays after it catch rows up across a step whose
    constants the eager step wrote.  Everything against the eager dense schedule, bit for bit."""
    import two_tower_models_amd as A
    from two_tower_models_amd import optim
    from test_gpu_models import batch_of, make_model
    monkeypatch.setattr(optim, "_TAB_MIN_STEPS", tab_min)
    g = golden("g1_base_tiny")
    W = 3
    bs = _batches(g, batch_of(g), 1 + replays + 3, 5, window=True)
    order = [bs[0]] * W + bs[1:1 + replays] + (bs[1 + replays:] if eager_step else [])
    eager = make_model("base", g)
    eopt = A.DenseExactAdam(eager.parameters(), lr=1e-3, overlap_sweep=False, lazy=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for b in order:
            loss = _eager(eager, eopt, b)
    torch.cuda.current_stream().wait_stream(side)
    del loss
    model = make_model("base", g)
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep=False, lazy=True)
    step = A.GraphedTrainStep(model, opt, bs[0], warmup=W)
    captured_tab, captured_steps = opt._tab, opt._tab_steps
    for b in bs[1:1 + replays]:
        step(*b)
    if eager_step:
        loss = _eager(model, opt, bs[1 + replays])
        del loss
        torch.cuda.synchronize()
        # the eager step wanted a bigger table, but the graph reads (and fills) the captured one: it stays
        assert opt._tab is captured_tab and opt._tab_steps == captured_steps and opt._host_steps + 2 >= captured_steps
        for b in bs[2 + replays:]:
            step(*b)
    opt.flush()
    torch.cuda.synchronize()
    assert opt.step_count == len(order) and (tab_min == 16 or len(order) > captured_steps)
    _same_models(eager, eopt, model, opt)


def test_resume_at_step_70000_lazy_equals_dense(golden):
    """A checkpoint whose step count is edited to 70 000 (past the initial 65 536-step table: _init_state sizes the table
    from the resumed step), resumed with the deferred and with the dense schedule for 5 steps."""
    import io
    import two_tower_models_amd as A
    from test_gpu_models import batch_of, make_model
    g = golden("g1_base_tiny")
    bs = _batches(g, batch_of(g), 8, 11, window=True)
    m0 = make_model("base", g)
    o0 = A.DenseExactAdam(m0.parameters(), lr=1e-3)
    for b in bs[:3]:
        _eager(m0, o0, b)
    buf = io.BytesIO()
    torch.save({"opt": o0.state_dict(), "model": m0.state_dict()}, buf)
    out = []
    for lazy in (False, True):
        ck = torch.load(io.BytesIO(buf.getvalue()))
        for st in ck["opt"]["state"].values():
            st["step"] = torch.tensor(70000.0)
        model = make_model("base", g)
        model.load_state_dict(ck["model"])
        opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep=False, lazy=lazy)
        opt.load_state_dict(ck["opt"])
        for b in bs[3:]:
            _eager(model, opt, b)
        opt.flush()
        torch.cuda.synchronize()
        assert opt.step_count == 70005
        if lazy:
            assert opt._tab_steps == 2 * 70002
        out.append((model, opt))
    _same_models(out[0][0], out[0][1], out[1][0], out[1][1])
