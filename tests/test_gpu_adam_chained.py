"""The chained dense-exact step (optim.DenseExactAdam._launch_chained; csrc/adam.hip: adam_sweep_tables_kernel with marks,
tt_adam_mark_advance): a step that looks up few rows marks them, its finish no longer waits for the sweep and the next
step's sweep follows on the sweep's stream behind one launch; once the main stream has run dry the sweep thins itself.

At the C ABI the thinning sweep against tt_adam_tables_sweep_marked, bit for bit, whatever the flag does and whenever it is
written; at the module the chained schedule against the serial and the parked one over a hand-made id schedule, against the
float64 reference of adam_ref.py, in stream order right behind step(), and switched with the other schedules step by step."""
import ctypes as C

import pytest
import torch

import adam_ref as AR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ZERO = {"p": 0, "m": 0, "v": 0}
STEPS, B = 8, 64


@pytest.fixture(scope="module")
def N():
    from two_tower_models_amd import _native as N
    N.load()
    return N


def desc_of(N, tables):
    d = (N.AdamTensor * len(tables))()
    for i, (w, m, v) in enumerate(tables):
        d[i].p, d[i].g, d[i].m, d[i].v, d[i].n = w.data_ptr(), None, m.data_ptr(), v.data_ptr(), w.numel()
    return d


def hyper_at(N, step):
    h = torch.tensor([AR.LR, AR.B1, AR.B2, AR.EPS, float(step - 1), 0, 0, 0], dtype=torch.float64, device=DEV)
    N.check(N.load().tt_adam_advance(h.data_ptr(), N.stream()), "advance")
    return h


# ------------------------------------------------------------------ the ABI: thinning never changes a bit
SHAPES = ((3000, 128), (129, 32))  # 94 chunks; a chunk and one row


@pytest.fixture(scope="module")
def sweep_case(N):
    """Two tables in one launch with some rows marked (first, last, a run across a bitmap word, a chunk's first row), and
    what two plain marked launches (tt_adam_tables_sweep_marked) leave of them: computed once, never modified."""
    lib = N.load()
    state = [[t.to(DEV) for t in AR.edge_state(r, D, 5 + i)] for i, (r, D) in enumerate(SHAPES)]
    marks = []
    for (r, D), rows in zip(SHAPES, ([0, 1, 30, 31, 32, 33, 64, 1500, 2999], [0, 5, 127, 128])):
        ids = torch.tensor(rows, device=DEV)
        bm = torch.full((lib.tt_adam_marks_words(r),), -1, dtype=torch.int32, device=DEV)
        N.check(lib.tt_adam_mark_rows(ids.data_ptr(), ids.numel(), r, bm.data_ptr(), bm.numel(), N.stream()), "mark_rows")
        marks.append(bm)
    dims = (C.c_int64 * 2)(*[D for _, D in SHAPES])
    mp = (C.c_void_p * 2)(*[bm.data_ptr() for bm in marks])
    want = [[t.clone() for t in tab] for tab in state]
    hyper = hyper_at(N, 3)
    for _ in range(2):
        N.check(lib.tt_adam_tables_sweep_marked(desc_of(N, want), dims, mp, 2, hyper.data_ptr(), 0, N.stream()), "sweep_marked")
    torch.cuda.synchronize()
    assert not torch.equal(want[0][0], state[0][0]) and torch.equal(want[0][0][30:34], state[0][0][30:34])
    return state, marks, dims, mp, want


def _chained_twice(N, case, n_wgs, alone_wgs, flag, tag, write=None):
    state, _, dims, mp, want = case
    lib = N.load()
    tabs = [[t.clone() for t in tab] for tab in state]
    hyper = hyper_at(N, 3)
    fp = flag.data_ptr() if flag is not None else None
    for k in range(2):
        N.check(lib.tt_adam_tables_sweep_chained(desc_of(N, tabs), dims, mp, 2, hyper.data_ptr(), n_wgs, alone_wgs, fp, tag,
                                                 N.stream()), "sweep_chained")
        if write is not None and k == 0:
            write()
    torch.cuda.synchronize()
    what = f"n_wgs {n_wgs} alone_wgs {alone_wgs} tag {tag}"
    for got, ref in zip(tabs, want):
        for x, y, name in zip(got, ref, "pmv"):
            assert torch.equal(x, y), f"{what}: {name} differs in {int((x != y).sum())} elements"
    assert int(hyper.view(torch.int64)[7]) == 0, what  # both chunk counters re-armed, whoever left early


def test_chained_sweep_flag_never_equal_to_the_tag(N, sweep_case):
    flag = torch.full((1,), 6, dtype=torch.int32, device=DEV)
    _chained_twice(N, sweep_case, 0, 2, flag, 7)
    _chained_twice(N, sweep_case, 0, 2, None, 7)  # no flag at all


@pytest.mark.parametrize("n_wgs", [0, 4])
@pytest.mark.parametrize("alone", ["1", "2", "grid", "grid+1"])
def test_chained_sweep_thin_from_the_start(N, sweep_case, n_wgs, alone):
    """The flag holds the tag before the launch: every workgroup numbered alone_wgs and up leaves with the one chunk it was
    handed at most, the rest sweep everything; alone_wgs >= the grid never thins."""
    grid = n_wgs or 3 * torch.cuda.get_device_properties(0).multi_processor_count
    alone_wgs = {"1": 1, "2": 2, "grid": grid, "grid+1": grid + 1}[alone]
    flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    _chained_twice(N, sweep_case, n_wgs, alone_wgs, flag, 7)


@pytest.mark.parametrize("n_wgs", [0, 4])
def test_chained_sweep_flag_written_while_it_runs(N, sweep_case, n_wgs):
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    other = torch.cuda.Stream()

    def write():
        with torch.cuda.stream(other):
            flag.fill_(7)

    _chained_twice(N, sweep_case, n_wgs, 1, flag, 7, write)
    other.synchronize()


def test_mark_advance_is_mark_rows_and_advance(N):
    """tt_adam_mark_advance on cleared bitmaps = tt_adam_mark_rows per table + tt_adam_advance, ids outside a table ignored."""
    lib = N.load()
    jobs, got, want = (N.AdamMarkJob * 2)(), [], []
    keep = []
    for i, (r, n) in enumerate(((3000, 700), (129, 40))):
        ids = torch.randint(0, r, (n,), generator=torch.Generator().manual_seed(i)).to(DEV)
        ids[0], ids[1], ids[2], ids[3] = 0, r - 1, r, -1
        words = lib.tt_adam_marks_words(r)
        a = torch.zeros(words, dtype=torch.int32, device=DEV)
        b = torch.full((words,), -1, dtype=torch.int32, device=DEV)
        N.check(lib.tt_adam_mark_rows(ids.data_ptr(), n, r, b.data_ptr(), words, N.stream()), "mark_rows")
        jobs[i].ids, jobs[i].n_ids, jobs[i].n_rows, jobs[i].marks, jobs[i].marks_words = ids.data_ptr(), n, r, a.data_ptr(), words
        got.append(a), want.append(b), keep.append(ids)
    h = torch.tensor([AR.LR, AR.B1, AR.B2, AR.EPS, 999.0, 0, 0, 0], dtype=torch.float64, device=DEV)
    N.check(lib.tt_adam_mark_advance(h.data_ptr(), jobs, 2, N.stream()), "mark_advance")
    assert [float(x) for x in h[4:7].cpu()] == list(AR.hyper64(1000))
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and int(got[0].count_nonzero()) > 0
    N.check(lib.tt_adam_mark_advance(h.data_ptr(), None, 0, N.stream()), "mark_advance")  # no table: the advance alone
    assert float(h[4]) == 1001.0
    jobs[0].marks_words = 3
    assert lib.tt_adam_mark_advance(h.data_ptr(), jobs, 2, N.stream()) == N.TT_E_WORKSPACE


# ------------------------------------------------------------------ the module
def _model(D, n_users, n_items):
    import two_tower_models_amd as A
    torch.manual_seed(11)
    mips = A.BaselineMIPSModule(corpus_size=40, embedding_dim=D)
    return A.TwoTowerBaseRetrieval(num_items=5, user_id_hash_size=n_users, user_id_embedding_dim=D, user_features_size=3,
                                   item_id_hash_size=n_items, item_id_embedding_dim=D, item_features_size=2,
                                   user_value_weights=[1.0], mips_module=mips).to(DEV)


# D = 128: the issue's 300 users x 500 items; D = 32: a user table of B rows, so that EVERY row of one table is looked up in
# every step (no table of 300 or 500 rows can be, by 64 ids), beside an item table of a chunk and one row
SIZES = {128: (300, 500), 32: (B, 129)}


def _ids(n_rows, s):
    """Step s's ids of a table, by hand: row 5 in steps 2 and 3 (n and n + 1); row 9 in steps 2 and 4 only (n and n + 2);
    row 11 twice in step 1; row 0 and the last row in steps 0 and 5; the rest from rows 20 .. n_rows - 2, moving each step."""
    if n_rows == B:
        return torch.randperm(B, generator=torch.Generator().manual_seed(s))  # every row, each step
    special = {0: [0, n_rows - 1], 1: [11, 11], 2: [5, 9], 3: [5], 4: [9], 5: [0, n_rows - 1]}.get(s, [])
    fill = [20 + (13 * s + 3 * k) % (n_rows - 21) for k in range(B - len(special))]
    return torch.tensor(special + fill)


def _batches(D):
    n_users, n_items = SIZES[D]
    gen = torch.Generator().manual_seed(D)
    out = []
    for s in range(STEPS):
        out.append([t.to(DEV) for t in (_ids(n_users, s), torch.randn(B, 3, generator=gen), torch.zeros(B, 2, dtype=torch.long),
                                        _ids(n_items, s), torch.randn(B, 2, generator=gen), torch.zeros(B, dtype=torch.long),
                                        torch.ones(B, 1))])
    return out


def _tables_of(model, opt):
    out = {k: v.clone() for k, v in model.state_dict().items()}
    for i, p in enumerate(opt._tables):
        out[f"exp_avg{i}"], out[f"exp_avg_sq{i}"] = opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()
    return out


def _run(D, modes, sync=False, probe=False, grads=None):
    """STEPS steps (or len(modes)), step s under schedule modes[s]: "chained" | "parked" (forward-announced) | "serial".
    -> per step: loss, every parameter and moment CLONED RIGHT BEHIND step() with no synchronise (and, probe, a no_grad
    train_forward there).  grads: a list that receives each step's dense fp32 table gradients (summed in lookup order)."""
    import two_tower_models_amd as A
    from two_tower_models_amd import optim
    model = _model(D, *SIZES[D])
    opt = A.DenseExactAdam(model.parameters(), lr=AR.LR, overlap_sweep="forward")
    first = {k: v.detach().clone().cpu() for k, v in model.state_dict().items()}
    trace = []
    mark_rows = optim._MARK_ROWS
    try:
        for b, mode in zip(_batches(D), modes):
            optim._MARK_ROWS = mode != "parked"
            opt.overlap_sweep = False if mode == "serial" else "forward"
            loss = model.train_forward(*b)
            if mode != "serial":
                assert opt._chained == (mode == "chained") and opt._begun
                assert all(ts.marked == (mode == "chained") for ts in opt._begun.values())
                assert (model.item_id_embedding_arch.weight._tt_active.p_plane is None) == (mode == "chained")
            opt.zero_grad()
            loss.backward()
            if grads is not None:
                step = []
                for p in opt._tables:
                    g = torch.zeros(p.shape)
                    for blk in sorted(p._tt_rowgrads, key=lambda x: x.index):
                        for i, r in zip(blk.ids.tolist(), blk.rows.cpu()):
                            g[i] += r
                    step.append(g)
                grads.append(step)
            opt.step()
            assert opt._begun is None and not opt._chained
            rec = {"loss": loss.detach().clone(), **_tables_of(model, opt)}
            if probe:
                with torch.no_grad():
                    rec["probe"] = model.train_forward(*b).clone()
            trace.append(rec)
            if sync:
                torch.cuda.synchronize()
    finally:
        optim._MARK_ROWS = mark_rows
    torch.cuda.synchronize()
    assert opt.step_count == len(trace)
    return trace, first, opt


def _same(a, b, what):
    assert len(a) == len(b)
    for s, (x, y) in enumerate(zip(a, b)):
        for k in x:
            assert torch.equal(x[k], y[k]), f"{what}: step {s}: {k} differs"


@pytest.fixture(scope="module")
def serial():
    """The serial schedule's trajectory per width, with its no_grad probes and its table gradients: computed once."""
    out = {}
    for D in SIZES:
        grads = []
        trace, first, _ = _run(D, ["serial"] * STEPS, probe=True, grads=grads)
        out[D] = (trace, first, grads)
    return out


@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("D", [128, 32])
def test_chained_is_bit_identical_to_serial_and_parked(serial, D, sync):
    chained, _, opt = _run(D, ["chained"] * STEPS, sync=sync, probe=True)
    assert opt.sweep_level_note() != "not measured yet" and len(opt._sweep_ctl.pending) + len(opt._sweep_ctl.obs.get(0, [])) > 0
    _same(chained, serial[D][0], f"chained vs serial, D {D}, sync {sync}")  # ... probes included: stream order behind step()
    parked, _, _ = _run(D, ["parked"] * STEPS, sync=sync)
    _same([{k: v for k, v in r.items() if k != "probe"} for r in chained], parked, f"chained vs parked, D {D}, sync {sync}")


@pytest.mark.parametrize("D", [128, 32])
def test_chained_against_float64(serial, D):
    """The chained trajectory's tables against adam_ref.bounds over the STEPS steps, fed the fp32 table gradients of the
    serial run (the schedules agree to the bit, so these are the chained run's gradients too)."""
    _, first, grads = serial[D]
    chained, _, opt = _run(D, ["chained"] * STEPS)
    names = ["user_id_embedding_arch.weight", "item_id_embedding_arch.weight"]
    for i, name in enumerate(names):
        p0 = first[name]
        ref = AR.bounds(p0, torch.zeros_like(p0), torch.zeros_like(p0), [g[i] for g in grads], 1)
        got = [chained[-1][name], chained[-1][f"exp_avg{i}"], chained[-1][f"exp_avg_sq{i}"]]
        r = AR.ratios(got, ref)
        print(f"[adam-ref] chained, D {D}, {name}: worst |error| / bound  p {r['p']:.3f}  m {r['m']:.3f}  v {r['v']:.3f}")
        assert AR.violations(got, ref) == ZERO, (name, r)


@pytest.mark.parametrize("env", [None, "TT_ADAM_CHAIN", "TT_SWEEP_ALONE_WGS"])
def test_switching_schedules_step_by_step(serial, env, monkeypatch):
    """Two chained steps, two serial, two chained = six serial ones; with TT_ADAM_CHAIN=0 the forward-announced steps park
    their rows as before, with TT_SWEEP_ALONE_WGS=0 they chain and the sweep never thins."""
    import two_tower_models_amd as A
    from two_tower_models_amd import optim
    D = 128
    if env is not None:
        monkeypatch.setenv(env, "0")
    fwd = "parked" if env == "TT_ADAM_CHAIN" else "chained"
    if fwd == "parked":  # (the switch alone turns the chain off: _run's `parked` also clears _MARK_ROWS, which is not the point here)
        model = _model(D, *SIZES[D])
        opt = A.DenseExactAdam(model.parameters(), lr=AR.LR, overlap_sweep="forward")
        model.train_forward(*_batches(D)[0])
        assert optim._MARK_ROWS and not opt._chained and model.item_id_embedding_arch.weight._tt_active.p_plane is not None
        opt.release_sweep()
        torch.cuda.synchronize()
    got, _, opt = _run(D, [fwd, fwd, "serial", "serial", fwd, fwd])
    if env == "TT_SWEEP_ALONE_WGS":
        assert opt._alone_tag is None
    elif env is None:
        assert opt._alone_tag == 6 and int(opt._alone_flag) == 6
    want = [{k: v for k, v in r.items() if k != "probe"} for r in serial[D][0][:6]]
    _same(got, want, f"switching, {env}=0" if env else "switching")
