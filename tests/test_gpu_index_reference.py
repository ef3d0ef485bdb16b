"""The index kernels on MI355X (`pytest -m gpu`) against tests/index_ref.py, at the C ABI through ctypes: the row plan on the
one-workgroup sort and the multi-kernel sort (every n and n_rows at which the host code changes the kernel, the LDS attribute,
the pass count or the ping-pong start; every id pattern; the 10240 | 10241 switch with the same ids), tt_rowgrad_plan_jobs with
1 .. 4 mixed lists, tt_rowgrad_dense on plans built by the REFERENCE, owner routing single and _jobs (out-of-range ids, a bucket
over cap, the last owner's clamp, 64 owners in a wave, world up to 1024), the owner side, and every refusal.

Every output is a view into a larger buffer prefilled with a sentinel (NaN, 0x7F7F7F7F, 0x7F7F7F7F7F7F7F7F) and is compared
WHOLE with the buffer the reference predicts: the specified outputs bit for bit, every other byte still the sentinel.  Every
case asserts rc == 0, the exact set and count of kernels launched, and the flag value (0 when nothing is wrong)."""
import ctypes as C

import numpy as np
import pytest
import torch

import index_ref as IR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD_BYTES = 256  # of sentinel on either side of every view
DT = {np.dtype("int32"): (torch.int32, IR.SENT32), np.dtype("int64"): (torch.int64, IR.SENT64),
      np.dtype("float32"): (torch.float32, float("nan")), np.dtype("uint8"): (torch.uint8, 0x7F)}


def _lib():
    from two_tower_models_amd import _native as N
    return N, N.load()


def _counting():
    """with _counting() as n: n[kernel] = launches of every kernel of the three files inside the block."""
    import gemm_ref as GR
    return GR.Launches(IR.KERNELS)


def _launches(n):
    return {k: v for k, v in n.items() if v}


class Buf:
    """`n` elements between two runs of sentinels, sentinel-filled themselves; holds() predicts the whole buffer."""

    def __init__(self, n, dtype):
        self.np_dtype = np.dtype(dtype)
        self.tdtype, self.sent = DT[self.np_dtype]
        self.n, self.pad = n, PAD_BYTES // self.np_dtype.itemsize
        self.t = torch.full((n + 2 * self.pad,), self.sent, dtype=self.tdtype, device=DEV)
        self.ptr = self.t.data_ptr() + PAD_BYTES
        assert self.ptr % 256 == 0

    def bits(self):
        return self.t.cpu().numpy().view({4: np.int32, 8: np.int64, 1: np.uint8}[self.np_dtype.itemsize])

    def get(self, n=None):
        return self.t[self.pad:self.pad + (self.n if n is None else n)].cpu().numpy()

    def holds(self, values=None, at=None):
        """The buffer is the sentinel everywhere but `values` (from element 0, or at the element indices `at`)."""
        want = torch.full(self.t.shape, self.sent, dtype=self.tdtype).numpy()
        if values is not None:
            values = np.asarray(values, self.np_dtype).reshape(-1)
            want[self.pad + (np.arange(len(values)) if at is None else np.asarray(at).reshape(-1))] = values
        return np.array_equal(self.bits(), want.view(self.bits().dtype))

    def outside_clean(self):
        """Nothing but the `n` elements changed."""
        return self.holds(self.get())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Flag:
    """An int32 flag between two sentinels, preset to `v`."""

    def __init__(self, v=0):
        self.t = torch.tensor([-77, v, -77], dtype=torch.int32, device=DEV)
        self.ptr = self.t.data_ptr() + 4

    def value(self):
        f = self.t.cpu().tolist()
        assert f[0] == -77 and f[2] == -77, "a flag's neighbour changed"
        return f[1]


# ------------------------------------------------------------------ the row plan
class PlanRun:
    """One list's plan outputs and the check against the reference."""

    def __init__(self, c, ids=None):
        self.c = c
        self.ids = IR.plan_ids(c) if ids is None else ids
        self.n = len(self.ids)
        self.ids_dev = _dev(self.ids)
        self.sorted_ids, self.perm = Buf(self.n, np.int32), Buf(self.n, np.int32)
        self.seg_begin, self.n_unique = Buf(self.n + 1, np.int32), Buf(1, np.int32)
        self.ref = IR.plan_reference(self.ids, c.n_rows)

    def problems(self):
        r = self.ref
        out = [k for k, ok in (("sorted_ids", self.sorted_ids.holds(r.sorted_ids)), ("perm", self.perm.holds(r.perm)),
                               ("seg_begin", self.seg_begin.holds(r.seg_begin)), ("n_unique", self.n_unique.holds([r.n_unique]))) if not ok]
        return out + ([] if np.array_equal(self.ids_dev.cpu().numpy(), self.ids) else ["ids"])


def _plan_single(run):
    N, lib = _lib()
    flag = Flag()
    ws_bytes = lib.tt_rowgrad_workspace_bytes(run.n)
    ws = Buf(ws_bytes, np.uint8)
    with _counting() as n:
        rc = lib.tt_rowgrad_plan(run.ids_dev.data_ptr(), run.n, run.c.n_rows, run.sorted_ids.ptr, run.perm.ptr, run.seg_begin.ptr,
                                 run.n_unique.ptr, flag.ptr, ws.ptr, ws_bytes, N.stream())
    torch.cuda.synchronize()
    assert ws.outside_clean(), "a byte around the workspace changed"
    return rc, _launches(n), flag.value()


@pytest.mark.parametrize("c", IR.PLAN_CASES, ids=[c.name for c in IR.PLAN_CASES])
def test_rowgrad_plan(c):
    run = PlanRun(c)
    rc, launches, flag = _plan_single(run)
    print(f"index-ref plan {c.name} n_unique {run.ref.n_unique} flag {flag} {launches}")
    assert rc == 0 and launches == IR.plan_launches(c), (rc, launches)
    assert not run.problems() and flag == run.ref.flag, (run.problems(), flag)


def test_rowgrad_plan_switch_between_the_two_sorts():
    """The same 10241 ids through the multi-kernel sort and, the last one removed, through the one-workgroup sort: each equals
    the reference on its own list, and the longer plan with its last id taken out is the shorter plan, bit for bit."""
    c = IR.SWITCH
    ids = IR.plan_ids(c)
    long, short = PlanRun(c, ids), PlanRun(c, ids[:-1].copy())
    for run, path in ((long, "multi"), (short, "small")):
        rc, launches, flag = _plan_single(run)
        assert IR.plan_path(run.n) == path and rc == 0 and launches == IR.plan_launches(c._replace(n=run.n)), (path, rc, launches)
        assert not run.problems() and flag == 0, (path, run.problems())
    keep = long.perm.get() != len(ids) - 1
    assert np.array_equal(long.sorted_ids.get()[keep], short.sorted_ids.get()) and np.array_equal(long.perm.get()[keep], short.perm.get())
    again = IR.plan_reference(ids[long.perm.get()[keep]], c.n_rows)  # the runs, re-derived by the reference from the common prefix
    assert np.array_equal(again.seg_begin, short.seg_begin.get(short.ref.n_unique + 1))


@pytest.mark.parametrize("group", list(IR.PLAN_JOB_GROUPS))
def test_rowgrad_plan_jobs(group):
    N, lib = _lib()
    runs = [PlanRun(c) for c in IR.plan_job_cases(group)]
    jobs = (N.PlanJob * len(runs))()
    for j, r in zip(jobs, runs):
        j.ids, j.n_ids, j.n_rows = r.ids_dev.data_ptr(), r.n, r.c.n_rows
        j.sorted_ids, j.perm, j.seg_begin, j.n_unique = r.sorted_ids.ptr, r.perm.ptr, r.seg_begin.ptr, r.n_unique.ptr
    flag = Flag()
    with _counting() as n:
        rc = lib.tt_rowgrad_plan_jobs(jobs, len(runs), flag.ptr, N.stream())
    torch.cuda.synchronize()
    print(f"index-ref plan-jobs {group} {[(r.n, r.c.n_rows) for r in runs]} flag {flag.value()} {_launches(n)}")
    assert rc == 0 and _launches(n) == {IR.PLAN_JOBS[0]: 1}, (rc, _launches(n))
    assert not [(r.c.name, p) for r in runs for p in r.problems()]
    assert flag.value() == max(r.ref.flag for r in runs)  # one shared flag


# ------------------------------------------------------------------ tt_rowgrad_dense
@pytest.mark.parametrize("c", IR.DENSE_CASES, ids=[IR.dense_id(c) for c in IR.DENSE_CASES])
def test_rowgrad_dense(c):
    """The plan comes from the reference, so this test stands without csrc/rowplan.hip.  dense is NaN-prefilled: an untouched
    row keeps its NaN bits, a touched row is overwritten whole."""
    N, lib = _lib()
    ids, blocks = IR.dense_inputs(c)
    plan = IR.plan_reference(ids, IR.DENSE_ROWS)
    ref = IR.dense_reference(plan, blocks, c.dim)
    n, dim = len(ids), c.dim
    src, keep = N.GradSources(), []
    first = np.cumsum((0,) + c.blocks)
    for k, b in enumerate(blocks):
        ld = 2 * dim if k == c.strided else (dim + 3 if c.wide else dim)
        buf = torch.full((max(len(b), 1) * ld + 64,), float("nan"), device=DEV)
        off = 32 + (dim if k == c.strided else 0)
        buf.as_strided((len(b), dim), (ld, 1), off).copy_(_dev(b))
        keep.append((buf, buf.clone()))
        src.rows[k], src.ld[k], src.first[k] = buf.data_ptr() + 4 * off, ld, int(first[k])
    src.first[len(blocks)], src.n_sources = n, len(blocks)
    seg = np.full(n + 1, IR.SENT32, np.int32)  # the plan as a plan call leaves it: nothing behind seg_begin[n_unique]
    seg[:plan.n_unique + 1] = plan.seg_begin
    plan_dev = [_dev(a) for a in (plan.sorted_ids, plan.perm, seg, np.array([plan.n_unique], np.int32))]
    dense = Buf(IR.DENSE_ROWS * dim, np.float32)
    with _counting() as cnt:
        rc = lib.tt_rowgrad_dense(C.byref(src), n, dim, *[t.data_ptr() for t in plan_dev], dense.ptr, N.stream())
    torch.cuda.synchronize()
    got = dense.get().reshape(IR.DENSE_ROWS, dim)[ref.rows]
    print(f"index-ref {IR.dense_id(c)} err/E {IR.dense_worst(ref, got):.3f} rows {len(ref.rows)} {_launches(cnt)}")
    assert rc == 0 and _launches(cnt) == {IR.DENSE[0]: 1}, (rc, _launches(cnt))
    assert IR.dense_worst(ref, got) <= 1.0
    at = (ref.rows[:, None] * dim + np.arange(dim)[None, :])
    assert dense.holds(ref.f32, at), "the kernel's own float32 sum, bit for bit; every other row still NaN"
    assert all(bool((a.view(torch.int32) == b.view(torch.int32)).all()) for a, b in keep), "a gradient source changed"


# ------------------------------------------------------------------ owner routing
class RouteRun:
    def __init__(self, c):
        self.c, self.ids, self.n_rows = c, IR.route_ids(c), IR.route_rows(c)
        self.cap = IR.route_cap(c, self.ids)
        self.ref = IR.route_reference(self.ids, self.n_rows, c.rpr, c.world, self.cap)
        _, lib = _lib()
        self.ids_dev = _dev(self.ids)
        self.ws_bytes = lib.tt_route_workspace_bytes(c.n, c.world)
        self.fresh()

    def fresh(self):
        c = self.c
        self.ws = Buf(self.ws_bytes, np.uint8)
        self.counts, self.max_count = Buf(c.world, np.int32), Buf(1, np.int32)
        self.send_ids, self.src_of = Buf(c.world * self.cap, np.int64), Buf(c.world * self.cap, np.int64)
        self.slot_of = Buf(c.n, np.int64)

    def count_problems(self, max_count):
        out = [k for k, ok in (("counts", self.counts.holds(self.ref.counts)), ("max_count", self.max_count.holds([max_count])),
                               ("around ws", self.ws.outside_clean())) if not ok]
        return out + [k for k, b in (("send_ids", self.send_ids), ("src_of", self.src_of), ("slot_of", self.slot_of)) if not b.holds()]

    def build_problems(self):
        r = self.ref
        out = [k for k, ok in (("send_ids", self.send_ids.holds(r.send_ids)), ("src_of", self.src_of.holds(r.src_of)),
                               ("slot_of", self.slot_of.holds(r.slot_of)), ("counts", self.counts.holds(r.counts)))
               if not ok]
        return out + ([] if np.array_equal(self.ids_dev.cpu().numpy(), self.ids) else ["ids"])

    def job(self, j):
        c = self.c
        j.ids, j.n_ids, j.n_rows, j.rows_per_rank = self.ids_dev.data_ptr(), c.n, self.n_rows, c.rpr
        j.counts, j.max_count, j.ws, j.ws_bytes = self.counts.ptr, self.max_count.ptr, self.ws.ptr, self.ws_bytes
        j.cap, j.send_ids, j.slot_of, j.src_of = self.cap, self.send_ids.ptr, self.slot_of.ptr, self.src_of.ptr


def _route_jobs(runs, world):
    """count_jobs then build_jobs for all runs in one call each; max_count is written over the sentinel."""
    N, lib = _lib()
    jobs = (N.RouteJob * len(runs))()
    for j, r in zip(jobs, runs):
        r.fresh()
        r.job(j)
    oob, overflow = Flag(), Flag()
    with _counting() as n:
        rc = lib.tt_route_count_jobs(jobs, len(runs), world, oob.ptr, N.stream())
    torch.cuda.synchronize()
    assert rc == 0 and _launches(n) == {k: 1 for k in IR.ROUTE_COUNT_JOBS}, (rc, _launches(n))
    assert not [(IR.route_id(r.c), p) for r in runs for p in r.count_problems(r.ref.max_count)]
    assert oob.value() == max(r.ref.oob for r in runs)
    with _counting() as n:
        rc = lib.tt_route_build_jobs(jobs, len(runs), world, overflow.ptr, N.stream())
    torch.cuda.synchronize()
    assert rc == 0 and _launches(n) == {k: 1 for k in IR.ROUTE_BUILD_JOBS}, (rc, _launches(n))
    assert not [(IR.route_id(r.c), p) for r in runs for p in r.build_problems()]
    assert overflow.value() == max(r.ref.overflow for r in runs) and oob.value() == max(r.ref.oob for r in runs)


@pytest.mark.parametrize("c", IR.ROUTE_CASES, ids=[IR.route_id(c) for c in IR.ROUTE_CASES])
def test_route_count_and_build(c):
    N, lib = _lib()
    run = RouteRun(c)
    ref = run.ref
    args = (run.ids_dev.data_ptr(), c.n, run.n_rows, c.rpr, c.world)
    for preset in (0, ref.max_count + 7):  # *max_count is atomicMax'ed: onto 0, and onto a larger value that stays
        run.fresh()
        run.max_count.t[run.max_count.pad] = preset
        oob = Flag()
        with _counting() as n:
            rc = lib.tt_route_count(*args, run.counts.ptr, run.max_count.ptr, None if c.pattern == "oob_null" else oob.ptr, run.ws.ptr,
                                    run.ws_bytes, N.stream())
        torch.cuda.synchronize()
        assert rc == 0 and _launches(n) == {k: 1 for k in IR.ROUTE_COUNT}, (rc, _launches(n))
        assert not run.count_problems(max(preset, ref.max_count)), run.count_problems(max(preset, ref.max_count))
        assert oob.value() == (0 if c.pattern == "oob_null" else ref.oob)
    overflow = Flag()
    with _counting() as n:
        rc = lib.tt_route_build(*args, run.cap, run.ws.ptr, run.ws_bytes, run.send_ids.ptr, run.slot_of.ptr, run.src_of.ptr, overflow.ptr,
                                N.stream())
    torch.cuda.synchronize()
    print(f"index-ref {IR.route_id(c)} cap {run.cap} max {ref.max_count} oob {ref.oob} overflow {ref.overflow} {_launches(n)}")
    assert rc == 0 and _launches(n) == {k: 1 for k in IR.ROUTE_BUILD}, (rc, _launches(n))
    assert not run.build_problems() and overflow.value() == ref.overflow, (run.build_problems(), overflow.value())
    _route_jobs([run], c.world)  # the same case as the only job of the _jobs entry points


@pytest.mark.parametrize("group", list(IR.ROUTE_JOB_GROUPS))
def test_route_jobs(group):
    cases = IR.ROUTE_JOB_GROUPS[group]
    _route_jobs([RouteRun(c) for c in cases], cases[0].world)
    print(f"index-ref route-jobs {group} {[IR.route_id(c) for c in cases]} {IR.ROUTE_COUNT_JOBS + IR.ROUTE_BUILD_JOBS}")


class ServeRun:
    def __init__(self, c):
        self.c = c
        self.ids, self.table = IR.serve_inputs(c)
        self.ids_dev = _dev(self.ids)
        self.table_dev = None if self.table is None else _dev(self.table.view(np.int16) if c.dtype == "bf16" else self.table)
        self.local, self.rows = Buf(c.n, np.int64), Buf(c.n * c.dim, np.float32)
        self.want = IR.serve_reference(self.ids, IR.SERVE_LO, c.n_local, self.table, c.dim)

    def job(self, j):
        from two_tower_models_amd import _native as N
        c = self.c
        j.ids, j.n_ids, j.lo, j.n_local, j.local = self.ids_dev.data_ptr(), c.n, IR.SERVE_LO, c.n_local, self.local.ptr
        j.table = None if self.table_dev is None else self.table_dev.data_ptr()
        j.dtype, j.dim, j.rows = (N.TT_BF16 if c.dtype == "bf16" else N.TT_F32), c.dim, self.rows.ptr

    def problems(self):
        return [k for k, ok in (("local", self.local.holds(self.want[0])), ("rows", self.rows.holds(self.want[1]))) if not ok]


def _serve(runs):
    N, lib = _lib()
    jobs = (N.RouteServeJob * len(runs))()
    for j, r in zip(jobs, runs):
        r.job(j)
    with _counting() as n:
        rc = lib.tt_route_serve_jobs(jobs, len(runs), N.stream())
    torch.cuda.synchronize()
    assert rc == 0 and _launches(n) == {IR.ROUTE_SERVE[0]: 1}, (rc, _launches(n))
    assert not [(IR.serve_id(r.c), p) for r in runs for p in r.problems()]


@pytest.mark.parametrize("c", IR.SERVE_CASES, ids=[IR.serve_id(c) for c in IR.SERVE_CASES])
def test_route_localize_and_serve(c):
    N, lib = _lib()
    run = ServeRun(c)
    local = Buf(c.n, np.int64)
    with _counting() as n:
        rc = lib.tt_route_localize(run.ids_dev.data_ptr(), c.n, IR.SERVE_LO, c.n_local, local.ptr, N.stream())
    torch.cuda.synchronize()
    assert rc == 0 and _launches(n) == {IR.ROUTE_LOCALIZE[0]: 1} and local.holds(run.want[0]), (rc, _launches(n))
    _serve([run])
    print(f"index-ref {IR.serve_id(c)} {IR.ROUTE_LOCALIZE + IR.ROUTE_SERVE}")


@pytest.mark.parametrize("group", list(IR.SERVE_GROUPS))
def test_route_serve_jobs(group):
    _serve([ServeRun(IR.SERVE_CASES[k]) for k in IR.SERVE_GROUPS[group]])


# ------------------------------------------------------------------ refusals
class Call:
    """A well-formed call of one entry point whose arguments a refusal case then spoils one at a time.  v: scalars and pointers
    by name (for the _jobs entries: the fields of every job); outputs and flags are sentinel-prefilled."""
    PLAN = "ids n_ids n_rows sorted_ids perm seg_begin n_unique flag ws ws_bytes"
    ARGS = {"plan": PLAN, "dense": "src n_ids dim sorted_ids perm seg_begin n_unique dense",
            "count": "ids n_ids n_rows rows_per_rank world counts max_count flag ws ws_bytes",
            "build": "ids n_ids n_rows rows_per_rank world cap ws ws_bytes send_ids slot_of src_of flag",
            "localize": "ids n_ids lo n_local local"}
    JOB_FIELDS = {"plan_jobs": "ids n_ids n_rows sorted_ids perm seg_begin n_unique",
                  "count_jobs": "ids n_ids n_rows rows_per_rank counts max_count ws ws_bytes",
                  "build_jobs": "ids n_ids n_rows rows_per_rank counts max_count ws ws_bytes cap send_ids slot_of src_of",
                  "serve_jobs": "ids n_ids lo n_local local table dtype dim rows"}
    OUT = {"sorted_ids": np.int32, "perm": np.int32, "seg_begin": np.int32, "n_unique": np.int32, "dense": np.float32, "counts": np.int32,
           "max_count": np.int32, "send_ids": np.int64, "slot_of": np.int64, "src_of": np.int64, "local": np.int64, "rows": np.float32}
    MAY_BE_NULL = {"count": ("flag",), "count_jobs": ("flag", "cap", "send_ids", "slot_of", "src_of")}

    def __init__(self, entry):
        N, lib = _lib()
        self.entry, self.n_jobs = entry, 1
        n = 100
        self.v = dict(n_ids=n, n_rows=1000, dim=128 if entry == "serve_jobs" else 8, rows_per_rank=250, world=4, cap=n, lo=0, n_local=16,
                      dtype=N.TT_F32)
        self.v["ws_bytes"] = lib.tt_rowgrad_workspace_bytes(n) if entry == "plan" else lib.tt_route_workspace_bytes(n, 4)
        self.bufs = {k: Buf(n * {"rows": 128, "dense": 8}.get(k, 4), dt) for k, dt in self.OUT.items()}
        self.flag = Flag()
        self.ins = dict(ids=torch.arange(n, dtype=torch.int64, device=DEV), ws=torch.zeros(1 << 16, dtype=torch.uint8, device=DEV),
                        table=torch.ones(16 * 128 + 8, device=DEV), grad=torch.ones(n * 8, device=DEV),
                        sorted_ids=torch.arange(n, dtype=torch.int32, device=DEV), seg_begin=torch.arange(n + 1, dtype=torch.int32, device=DEV),
                        n_unique=torch.tensor([n], dtype=torch.int32, device=DEV), counts=torch.full((4,), 25, dtype=torch.int32, device=DEV))
        for k, b in self.bufs.items():
            self.v[k] = b.ptr
        for k in ("ids", "ws", "table"):
            self.v[k] = self.ins[k].data_ptr()
        if entry == "dense":  # the plan is an input here
            self.v.update(sorted_ids=self.ins["sorted_ids"].data_ptr(), perm=self.ins["sorted_ids"].data_ptr(),
                          seg_begin=self.ins["seg_begin"].data_ptr(), n_unique=self.ins["n_unique"].data_ptr())
        if entry == "build_jobs":  # counts come from the count stage
            self.v["counts"] = self.ins["counts"].data_ptr()
        self.v["flag"] = self.flag.ptr
        self.src = N.GradSources()
        self.src.rows[0], self.src.ld[0], self.src.first[0], self.src.first[1], self.src.n_sources = self.ins["grad"].data_ptr(), 8, 0, n, 1
        self.v["src"] = C.byref(self.src)

    def outputs(self):
        names = (self.ARGS.get(self.entry) or self.JOB_FIELDS[self.entry]).split()
        skip = ("sorted_ids", "perm", "seg_begin", "n_unique") if self.entry == "dense" else (("counts",) if self.entry == "build_jobs" else ())
        return [k for k in names if k in self.OUT and k not in skip]

    def pointers(self):
        names = (self.ARGS.get(self.entry) or (self.JOB_FIELDS[self.entry] + (" flag" if self.entry != "serve_jobs" else ""))).split()
        return [k for k in names if (k in self.OUT or k in ("ids", "ws", "flag", "table", "src")) and k not in self.MAY_BE_NULL.get(self.entry, ())]

    def call(self):
        N, lib = _lib()
        e, v = self.entry, self.v
        with _counting() as n:
            if e in self.ARGS:
                f = {"plan": lib.tt_rowgrad_plan, "dense": lib.tt_rowgrad_dense, "count": lib.tt_route_count, "build": lib.tt_route_build,
                     "localize": lib.tt_route_localize}[e]
                rc = f(*[v[a] for a in self.ARGS[e].split()], N.stream())
            else:
                T = {"plan_jobs": N.PlanJob, "count_jobs": N.RouteJob, "build_jobs": N.RouteJob, "serve_jobs": N.RouteServeJob}[e]
                jobs = (T * max(self.n_jobs, 1))()
                for j in jobs:
                    for k in self.JOB_FIELDS[e].split():
                        setattr(j, k, v[k])
                jp = None if v.get("jobs", 1) is None else jobs
                if e == "plan_jobs":
                    rc = lib.tt_rowgrad_plan_jobs(jp, self.n_jobs, v["flag"], N.stream())
                elif e == "serve_jobs":
                    rc = lib.tt_route_serve_jobs(jp, self.n_jobs, N.stream())
                else:
                    rc = (lib.tt_route_count_jobs if e == "count_jobs" else lib.tt_route_build_jobs)(jp, self.n_jobs, v["world"], v["flag"], N.stream())
        torch.cuda.synchronize()
        untouched = all(self.bufs[k].holds() for k in self.bufs) and self.flag.value() == 0
        return rc, sum(n.values()), untouched


def _set(**kw):
    return lambda call: call.v.update(kw)


def _jobs(k):
    return lambda call: setattr(call, "n_jobs", k)


def _src(**kw):
    def spoil(call):
        for k, val in kw.items():
            if isinstance(val, tuple):
                getattr(call.src, k)[val[0]] = val[1]
            else:
                setattr(call.src, k, val)
    return spoil


def _misaligned_table(call):
    call.v["table"] = call.ins["table"].data_ptr() + 4


BAD, WS, UNS = IR.E_BADARG, IR.E_WORKSPACE, IR.E_UNSUPPORTED
ROUTED = ("count", "build", "count_jobs", "build_jobs")
SIZED = ("plan", "dense") + ROUTED  # id lists of fewer than 2^31 ids: the plan and every count are int32
REFUSALS = [  # (what, entries, rc, how the call is spoiled)
    ("n_ids = 0", SIZED + ("plan_jobs", "localize", "serve_jobs"), BAD, _set(n_ids=0)),
    ("n_ids = -1", SIZED + ("plan_jobs", "localize", "serve_jobs"), BAD, _set(n_ids=-1)),
    ("n_ids = 2^31", SIZED, BAD, _set(n_ids=2 ** 31)),
    ("n_ids = 2^31", ("plan_jobs",), UNS, _set(n_ids=2 ** 31)),
    ("n_ids = 10241", ("plan_jobs",), UNS, _set(n_ids=10241)),
    ("n_rows = 0", ("plan", "plan_jobs") + ROUTED, BAD, _set(n_rows=0)),
    ("n_rows = 2^31 + 1", ("plan", "plan_jobs"), BAD, _set(n_rows=2 ** 31 + 1)),
    ("workspace one byte short", ("plan",) + ROUTED, WS, lambda call: call.v.update(ws_bytes=call.v["ws_bytes"] - 1)),
    ("5 jobs", ("plan_jobs",), BAD, _jobs(5)), ("9 jobs", ("count_jobs", "build_jobs", "serve_jobs"), BAD, _jobs(9)),
    ("0 jobs", ("plan_jobs", "count_jobs", "build_jobs", "serve_jobs"), BAD, _jobs(0)),
    ("jobs = NULL", ("plan_jobs", "count_jobs", "build_jobs", "serve_jobs"), BAD, _set(jobs=None)),
    ("world = 0", ROUTED, BAD, _set(world=0)), ("world = 1025", ROUTED, BAD, _set(world=1025)),
    ("cap = 0", ("build", "build_jobs"), BAD, _set(cap=0)), ("rows_per_rank = 0", ROUTED, BAD, _set(rows_per_rank=0)),
    ("5 sources", ("dense",), BAD, _src(n_sources=5)), ("0 sources", ("dense",), BAD, _src(n_sources=0)),
    ("first[0] != 0", ("dense",), BAD, _src(first=(0, 1))), ("ld < dim", ("dense",), BAD, _src(ld=(0, 7))),
    ("first[n_sources] != n_ids", ("dense",), BAD, _src(first=(1, 99))), ("a source = NULL", ("dense",), BAD, _src(rows=(0, None))),
    ("dim = 0", ("dense", "serve_jobs"), BAD, _set(dim=0)),
    ("table 4 bytes off a 16-byte boundary", ("serve_jobs",), BAD, _misaligned_table), ("dtype 7", ("serve_jobs",), BAD, _set(dtype=7)),
    ("lo = -1", ("localize", "serve_jobs"), BAD, _set(lo=-1)), ("n_local = -1", ("localize", "serve_jobs"), BAD, _set(n_local=-1)),
]
ENTRIES = list(Call.ARGS) + list(Call.JOB_FIELDS)
REFUSAL_CASES = [(w, e, rc, s) for w, es, rc, s in REFUSALS for e in es]


def _null_cases():
    """(entry, pointer) for every pointer that may not be NULL; built without a GPU."""
    out = []
    for e in ENTRIES:
        names = (Call.ARGS.get(e) or (Call.JOB_FIELDS[e] + (" flag" if e != "serve_jobs" else ""))).split()
        out += [(e, k) for k in names if (k in Call.OUT or k in ("ids", "ws", "flag", "table", "src")) and k not in Call.MAY_BE_NULL.get(e, ())]
    return out


@pytest.mark.parametrize("what,entry,want,spoil", REFUSAL_CASES, ids=[f"{e}-{w}".replace(" ", "_") for w, e, _, _ in REFUSAL_CASES])
def test_refusals_return_their_code_before_anything_is_launched_or_written(what, entry, want, spoil):
    call = Call(entry)
    spoil(call)
    rc, launches, untouched = call.call()
    assert rc == want and launches == 0 and untouched, (what, entry, rc, launches, untouched)


@pytest.mark.parametrize("entry,pointer", _null_cases(), ids=[f"{e}-{p}" for e, p in _null_cases()])
def test_null_pointers_are_refused(entry, pointer):
    call = Call(entry)
    assert pointer in call.pointers()
    call.v[pointer] = None
    rc, launches, untouched = call.call()
    assert rc == BAD and launches == 0 and untouched, (entry, pointer, rc, launches, untouched)


LAUNCHES = {"plan": 1, "dense": 1, "count": 2, "build": 2, "localize": 1, "plan_jobs": 1, "count_jobs": 2, "build_jobs": 1, "serve_jobs": 1}


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_refusal_base_call_is_accepted(entry):
    """The unspoiled call of every refusal case runs and writes its outputs."""
    call = Call(entry)
    rc, launches, untouched = call.call()
    assert rc == 0 and launches == LAUNCHES[entry] and not untouched, (rc, launches, untouched)
