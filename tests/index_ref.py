"""Exact yardstick for the index kernels: the row plan (csrc/rowplan.hip: tt_rowgrad_plan, tt_rowgrad_plan_jobs), the dense row
gradient (rowgrad_dense_kernel of csrc/adam.hip: tt_rowgrad_dense) and owner routing (csrc/route.hip: tt_route_count / _build /
_localize and the three _jobs entry points).  A helper, not a test: imported by test_index_reference_cpu.py and
test_gpu_index_reference.py; the product never imports it.  numpy only.

  plan_reference    ids outside [0, n_rows) become 0 and raise the flag; numpy's stable sort; the runs of equal id.  Every
                    output is compared bit for bit.
  dense_reference   per run the float64 sum with its bound and the kernel's own arithmetic (float32, run order, from 0.f), for
                    which bit equality is demanded: the build has no fast-math and the kernel adds in t order.
                      E = gamma(c - 1) sum_t |g_t|,  c = run length,  gamma(k) = k 2^-24 / (1 - k 2^-24)
                    c - 1 roundings (0.f + g_0 is exact), derived, not measured; 0 for c = 1: such rows are bit-equal.
  route_reference   a plain loop over the list, with the three branches OracleRouteKernels asserts away: an id out of range
                    (owner 0, id 0, flag), a bucket over `cap` (slot_of = -1, flag), the last owner's clamp.
                    localize_reference / serve_reference: the owner side (f32 and bf16 tables, zero rows for "not mine").
  *_slow            each reference restated with a dict of lists per row or owner (test_index_reference_cpu.py compares them).
  evaluate          the kernels' arithmetic with one deliberate mistake (`mut`), per family; evaluate(case) without one is the
                    reference.  PLAN_MUTANTS and ROUTE_MUTANTS name them.
  CASES             what test_gpu_index_reference.py runs; the CPU test runs the mutants at the very same cases.

Mutant -> cases that catch it (test_index_reference_cpu.py asserts that some do, on each sort that can make the mistake, and
prints all of them; profiles/index_reference_tolerance.txt keeps the list):
  unstable         an unstable order inside a run                     small-511-r16, multi-10241-r1 ... 43 cases with a run of two
  top_digit        the top digit's pass dropped                       small-511-r65537, multi-10241-r65537 ... 40 cases
  head_256         a run head lost at a 256-key tile edge             multi-edges, multi-distinct_asc ... 16 cases
  head_2048        ... at a 2048-key tile edge                        multi-edges, multi-distinct_asc ... 16 cases
  head_kpt         ... at a thread's kpt edge (one-workgroup sort)    small-edges, small-edges-kpt20 ... 28 cases
  no_sentinel      seg_begin[n_unique] not written                    every case
  oob_low32        an out-of-range id keeping its low 32 bits         small-oob, multi-oob, jobs-four-one-oob-1
  no_wave_prefix   a route rank that ignores earlier waves            route-65-w7-uniform-short ... 29 cases
  no_tile_prefix   a route rank that ignores earlier tiles            route-1025-w2-sorted-short ... 19 cases
  no_clamp         the owner not clamped                              route-5000-w257-clamp-max, route-65-w257-clamp-r64-rpr5, two _jobs cases
  pad_unwritten    padding left unwritten                             route-1-w1024-uniform-r64, route-63-w2-uniform-r64 ... 39 cases
  overflow_placed  an overflowed id placed anyway                     route-64-w7-one_owner-short ... all 13 `short` cases"""
import collections
import zlib

import numpy as np

EPS = 2.0 ** -24
SENT32, SENT64 = 0x7F7F7F7F, 0x7F7F7F7F7F7F7F7F
BAD_IDS = (-1, None, 2 ** 40, -2 ** 63)  # None: n_rows
PS_THREADS, PS_MAX = 512, 10240  # the one-workgroup sort: threads, longest list
TILE, SEG_TILE, RT = 256, 2048, 1024  # keys per radix tile, per run-head tile, ids per route tile
E_BADARG, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -3

PLAN_SMALL = ("plan_small_kernel",)
PLAN_JOBS = ("plan_small_jobs_kernel",)
PLAN_RADIX = ("radix_hist_kernel", "radix_scan_kernel", "radix_scatter_kernel")
PLAN_MULTI = ("plan_init_kernel",) + PLAN_RADIX + ("seg_count_kernel", "seg_scan_kernel", "seg_write_kernel")
DENSE = ("rowgrad_dense_kernel",)
ROUTE_COUNT, ROUTE_BUILD = ("route_hist_kernel", "route_scan_kernel"), ("route_fill_kernel", "route_build_kernel")
ROUTE_COUNT_JOBS, ROUTE_BUILD_JOBS = ("route_hist_jobs_kernel", "route_scan_jobs_kernel"), ("route_build_jobs_kernel",)
ROUTE_LOCALIZE, ROUTE_SERVE = ("route_localize_kernel",), ("route_serve_jobs_kernel",)
KERNELS = (PLAN_SMALL + PLAN_JOBS + PLAN_MULTI + DENSE + ROUTE_COUNT + ROUTE_BUILD + ROUTE_COUNT_JOBS + ROUTE_BUILD_JOBS
           + ROUTE_LOCALIZE + ROUTE_SERVE)


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ------------------------------------------------------------------ the row plan
Plan = collections.namedtuple("Plan", "sorted_ids perm seg_begin n_unique flag")
PlanCase = collections.namedtuple("PlanCase", "name n n_rows pattern")


def plan_path(n):
    return "small" if n <= PS_MAX else "multi"


def plan_kpt(n):
    return -(-n // PS_THREADS)


def plan_passes(n_rows, path):
    """Radix passes the host code runs: 4-bit digits (none for a one-row table) or 8-bit digits."""
    bits = max(1, (n_rows - 1).bit_length())
    if path == "small":
        return 0 if n_rows == 1 else -(-bits // 4)
    return -(-bits // 8)


def plan_needs_attribute(n):
    """The one-workgroup sort's LDS beyond 64 KiB (hipFuncSetAttribute): from 3585 ids on."""
    cap = PS_THREADS * plan_kpt(n) + (PS_THREADS * plan_kpt(n) >> 5) + 1
    return 2 * cap * 4 + 2 * cap * 2 + 4 + 16 * PS_THREADS * 2 > 64 * 1024


def plan_launches(c):
    if plan_path(c.n) == "small":
        return {PLAN_SMALL[0]: 1}
    want = {k: 1 for k in PLAN_MULTI}
    want.update({k: plan_passes(c.n_rows, "multi") for k in PLAN_RADIX})
    return want


def _cut(sorted_keys, n):
    heads = np.flatnonzero(np.r_[True, sorted_keys[1:] != sorted_keys[:-1]])
    return heads, np.r_[heads, n].astype(np.int32)


def plan_reference(ids, n_rows):
    ids = np.asarray(ids, np.int64)
    bad = (ids < 0) | (ids >= n_rows)
    key = np.where(bad, 0, ids)
    perm = np.argsort(key, kind="stable")
    s = key[perm]
    heads, seg = _cut(s, len(ids))
    return Plan(s.astype(np.int32), perm.astype(np.int32), seg, len(heads), int(bad.any()))


def plan_slow(ids, n_rows):
    """The same plan from a dict: row -> the positions that look it up, in list order."""
    rows, flag = {}, 0
    for i, v in enumerate(np.asarray(ids, np.int64).tolist()):
        if v < 0 or v >= n_rows:
            v, flag = 0, 1
        rows.setdefault(v, []).append(i)
    s, perm, seg = [], [], []
    for r in sorted(rows):
        seg.append(len(s))
        s += [r] * len(rows[r])
        perm += rows[r]
    seg.append(len(s))
    return Plan(np.array(s, np.int64).astype(np.int32), np.array(perm, np.int32), np.array(seg, np.int32), len(rows), flag)


PLAN_MUTANTS = ("unstable", "top_digit", "head_256", "head_2048", "head_kpt", "no_sentinel", "oob_low32")


def plan_applies(mut, c):
    """The kernel that can make this mistake runs at this case."""
    path = plan_path(c.n)
    if mut in ("head_256", "head_2048"):
        return path == "multi"
    if mut == "head_kpt":
        return path == "small"
    if mut == "top_digit":
        return plan_passes(c.n_rows, path) > 0
    return True


def plan_evaluate(ids, n_rows, mut=None):
    """An LSD radix sort of the clamped keys (it orders by the bits its passes cover) and the run cut, with one mistake."""
    ids = np.asarray(ids, np.int64)
    n, path = len(ids), plan_path(len(ids))
    bad = (ids < 0) | (ids >= n_rows)
    key = np.where(bad, (ids & 0xFFFFFFFF) if mut == "oob_low32" else 0, ids)
    digit, passes = (4 if path == "small" else 8), plan_passes(n_rows, path)
    if mut == "top_digit":
        passes -= 1
    order = np.argsort(key & ((1 << (digit * max(passes, 0))) - 1), kind="stable")
    s = key[order]
    head = np.r_[True, s[1:] != s[:-1]]
    edge = {"head_256": TILE, "head_2048": SEG_TILE, "head_kpt": plan_kpt(n)}.get(mut)
    if edge:
        head[np.arange(edge, n, edge)] = False
    heads = np.flatnonzero(head)
    if mut == "unstable":
        ends = np.r_[heads[1:], n]
        order = np.concatenate([order[a:b][::-1] for a, b in zip(heads, ends)])
    seg = np.r_[heads, SENT32 if mut == "no_sentinel" else n].astype(np.int32)
    return Plan(s.astype(np.uint32).view(np.int32), order.astype(np.int32), seg, len(heads), int(bad.any()))


def plan_problems(ref, got):
    """Names of the outputs that differ in any bit."""
    out = [k for k in ("sorted_ids", "perm", "seg_begin") if not np.array_equal(getattr(ref, k), getattr(got, k))]
    return out + [k for k in ("n_unique", "flag") if getattr(ref, k) != getattr(got, k)]


def _plant_bad(ids, n_rows):
    n = len(ids)
    for pos, v in zip((0, n // 3, 2 * n // 3, n - 1), BAD_IDS):
        ids[pos] = n_rows if v is None else v
    return ids


def edge_heads(n):
    """Positions at which the `edges` pattern starts a run: every kind of tile edge of the sort that takes n ids, and one
    position to either side."""
    at = set()
    if plan_path(n) == "small":
        kpt = plan_kpt(n)
        at |= {kpt * t for t in list(range(1, PS_THREADS, 5)) + [63, 64, 65, PS_THREADS - 1]}
    at |= set(range(TILE, n, 3 * TILE)) | set(range(SEG_TILE, n, SEG_TILE))
    return sorted({p + d for p in at for d in (-1, 0, 1) if 0 < p + d < n} | {0})


def plan_ids(c):
    rng, n, R = _rng(c.name), c.n, c.n_rows
    if c.pattern in ("uniform", "oob"):
        ids = rng.integers(0, R, n, dtype=np.int64)
        if c.pattern == "oob":
            return _plant_bad(ids, R)
        ids[(n // 2 + 1 + int(rng.integers(0, max(n - 1, 1)))) % n] = 0  # rows 0 and n_rows - 1 are always present
        ids[n // 2] = R - 1  # (a list of one id: the last row)
        return ids
    if c.pattern == "equal":
        return np.full(n, R - 1, np.int64)
    if c.pattern in ("distinct_asc", "distinct_desc"):
        ids = np.arange(n, dtype=np.int64) * ((R - 1) // (n - 1))
        return ids if c.pattern == "distinct_asc" else ids[::-1].copy()
    if c.pattern == "alternating":
        return np.where(np.arange(n) % 2 == 0, R - 1, 3).astype(np.int64)
    if c.pattern == "heavy":
        ids = rng.integers(0, R, n, dtype=np.int64)
        ids[rng.permutation(n)[:n // 2]] = R // 2
        return ids
    if c.pattern == "edges":
        heads = np.array(edge_heads(n))
        vals = np.sort(rng.choice(R, len(heads), replace=False)).astype(np.int64)
        return np.repeat(vals, np.diff(np.r_[heads, n]))[rng.permutation(n)]
    raise ValueError(c.pattern)


def plan_id(c):
    return c.name


SMALL_N = (1, 2, 511, 512, 513, 3584, 3585, 10239, 10240)
SMALL_ROWS = (1, 2, 16, 17, 65536, 65537, 2 ** 28 + 1, 2 ** 31)
MULTI_GRID = {10241: (1, 65537, 2 ** 31), 16384: (256, 2 ** 24 + 1), 16385: (257, 2 ** 31), 20479: (65536, 1),
              20481: (65537, 256, 2 ** 24 + 1), 524289: (257, 65536)}
MULTI_ROWS = (1, 256, 257, 65536, 65537, 2 ** 24 + 1, 2 ** 31)
PATTERNS = ("equal", "distinct_asc", "distinct_desc", "alternating", "heavy", "edges", "oob")
SWITCH = PlanCase("switch-10241-r65537", 10241, 65537, "uniform")  # and its first 10240 ids through the one-workgroup sort
PLAN_CASES = (
    [PlanCase(f"small-{n}-r{r}", n, r, "uniform") for i, n in enumerate(SMALL_N) for r in (SMALL_ROWS[i % 8], SMALL_ROWS[(i + 3) % 8])]
    + [PlanCase(f"multi-{n}-r{r}", n, r, "uniform") for n, rows in MULTI_GRID.items() for r in rows]
    + [PlanCase(f"small-{p}", 3585, 65537, p) for p in PATTERNS] + [PlanCase("small-edges-kpt20", 10240, 65537, "edges")]
    + [PlanCase(f"multi-{p}", 20481 if p == "edges" else 16385, 65537, p) for p in PATTERNS])

# tt_rowgrad_plan_jobs: (n, n_rows, pattern) per job -- a small list under a larger list's LDS size, either way round
PLAN_JOB_GROUPS = {
    "one": ((10240, 65537, "uniform"),),
    "two-small-first": ((1, 2 ** 31, "uniform"), (10240, 17, "uniform")),
    "two-large-first": ((10240, 65536, "heavy"), (513, 2, "uniform")),
    "three": ((513, 16, "uniform"), (3585, 65536, "edges"), (1, 1, "uniform")),
    "four": ((1, 2, "uniform"), (513, 2 ** 28 + 1, "uniform"), (3585, 65537, "distinct_desc"), (10240, 2 ** 31, "uniform")),
    "four-one-oob": ((513, 17, "uniform"), (3585, 65537, "oob"), (1, 1, "uniform"), (10240, 16, "alternating")),
}


def plan_job_cases(group):
    return [PlanCase(f"jobs-{group}-{j}", n, r, p) for j, (n, r, p) in enumerate(PLAN_JOB_GROUPS[group])]


# ------------------------------------------------------------------ tt_rowgrad_dense
# blocks: rows per source block (0: an empty block); wide: ld > dim (False: ld = dim); strided: the index of the block that is the
# [:, 1, :] half of a [rows, 2, dim] buffer; oob: the plan holds out-of-range ids (their gradient rows land in row 0)
DenseCase = collections.namedtuple("DenseCase", "dim blocks wide strided oob")
DENSE_ROWS = 40
DENSE_RUNS = (1, 2, 3, 1000)
DENSE_CASES = [DenseCase(1, (1100,), False, None, False), DenseCase(63, (600, 500), True, None, False),
               DenseCase(64, (1, 599, 400, 100), False, 2, False), DenseCase(65, (700, 0, 400), True, 0, False),
               DenseCase(128, (300, 300, 300, 200), True, 3, False), DenseCase(200, (1100,), True, None, True),
               DenseCase(128, (550, 550), False, 1, True)]


def dense_id(c):
    tags = ("-wide" if c.wide else "") + (f"-strided{c.strided}" if c.strided is not None else "") + ("-oob" if c.oob else "")
    return f"dense-d{c.dim}-{'+'.join(map(str, c.blocks))}" + tags


def dense_inputs(c):
    """(ids, blocks): runs of 1, 2, 3 and 1000 ids on rows 5, 6, 7, 8, the rest uniform over rows 9 .. 29 (rows 0 .. 4 and
    30 .. 39 stay untouched unless out-of-range ids land in row 0); gradient rows of mixed magnitude and sign."""
    rng, n = _rng(dense_id(c)), sum(c.blocks)
    ids = np.concatenate([np.full(k, 5 + j, np.int64) for j, k in enumerate(DENSE_RUNS)])
    ids = np.r_[ids, rng.integers(9, 30, n - len(ids))][rng.permutation(n)]
    if c.oob:
        _plant_bad(ids, DENSE_ROWS)
    g = (rng.standard_normal((n, c.dim)) * 10.0 ** rng.integers(-3, 3, (n, 1))).astype(np.float32)
    first = np.cumsum((0,) + c.blocks)
    return ids, [g[a:b] for a, b in zip(first[:-1], first[1:])]


Dense = collections.namedtuple("Dense", "rows sum64 E f32")


def dense_reference(plan, blocks, dim):
    """rows [n_unique]; sum64, E and f32 [n_unique, dim]."""
    g = np.concatenate(blocks).reshape(-1, dim)[plan.perm]
    seg, u = plan.seg_begin.astype(np.int64), plan.n_unique
    length = np.diff(seg)
    sum64 = np.add.reduceat(g.astype(np.float64), seg[:-1], axis=0)
    E = gamma(length - 1)[:, None] * np.add.reduceat(np.abs(g.astype(np.float64)), seg[:-1], axis=0)
    f32 = np.zeros((u, dim), np.float32)
    for t in range(int(length.max())):
        live = length > t
        f32[live] = f32[live] + g[seg[:-1][live] + t]
    return Dense(plan.sorted_ids[seg[:-1]].astype(np.int64), sum64, E, f32)


def dense_slow(ids, n_rows, blocks, dim):
    """row -> float64 sum of its gradient rows, from a dict of lists."""
    g, rows = np.concatenate(blocks).reshape(-1, dim), {}
    for i, v in enumerate(np.asarray(ids).tolist()):
        rows.setdefault(v if 0 <= v < n_rows else 0, []).append(i)
    return {r: np.sum([g[i].astype(np.float64) for i in at], axis=0) for r, at in rows.items()}


def dense_worst(ref, got):
    """max err / E of `got` [n_unique, dim] against the float64 sum; E = 0 demands equality."""
    err = np.abs(got.astype(np.float64) - ref.sum64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / ref.E)
    return float(np.nan_to_num(q, nan=np.inf).max())


# ------------------------------------------------------------------ owner routing
Route = collections.namedtuple("Route", "counts max_count send_ids slot_of src_of oob overflow")
# pattern: uniform | one_owner | sorted | wave64 (ids k * rows_per_rank, k = 0 .. 63 in turn) | clamp (rows_per_rank * world <
#          n_rows) | empty_tail (rows_per_rank * world > n_rows) | oob (the four out-of-range ids) | oob_null (... oob_flag = NULL)
# cap: max (the largest bucket) | r64 (... rounded up to 64) | short (3 below the largest bucket)
RouteCase = collections.namedtuple("RouteCase", "n world pattern cap rpr", defaults=(37,))
ROUTE_N = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)
ROUTE_WORLDS = (1, 2, 7, 64, 257, 1024)
ROUTE_CASES = [
    RouteCase(1, 1, "uniform", "max"), RouteCase(1, 1024, "uniform", "r64"), RouteCase(63, 2, "uniform", "r64"),
    RouteCase(64, 64, "wave64", "max"), RouteCase(64, 7, "one_owner", "short"), RouteCase(65, 7, "uniform", "short"),
    RouteCase(1023, 257, "uniform", "max"), RouteCase(1024, 1024, "uniform", "r64"), RouteCase(1024, 2, "sorted", "max"),
    RouteCase(1025, 2, "sorted", "short"), RouteCase(1025, 64, "oob", "short"), RouteCase(2049, 7, "one_owner", "short"),
    RouteCase(2049, 1024, "sorted", "max"), RouteCase(2049, 64, "wave64", "r64"), RouteCase(5000, 64, "wave64", "short"),
    RouteCase(5000, 257, "clamp", "max"), RouteCase(5000, 1024, "empty_tail", "r64"), RouteCase(5000, 7, "oob", "max"),
    RouteCase(5000, 1, "uniform", "short"), RouteCase(1023, 7, "oob_null", "max"), RouteCase(65, 257, "clamp", "r64", 5),
    RouteCase(1025, 7, "empty_tail", "short", 1000),
]
# tt_route_*_jobs with 3 and 8 jobs: world per call; n, n_rows, rows_per_rank and cap differ per job; with world = 7 or 257 the
# slot counts world * cap are no multiples of 1024
ROUTE_JOB_GROUPS = {
    "three-w64": [RouteCase(64, 64, "wave64", "max"), RouteCase(1025, 64, "oob", "short", 11), RouteCase(5000, 64, "clamp", "r64", 5)],
    "three-w257": [RouteCase(1023, 257, "uniform", "max", 3), RouteCase(1, 257, "uniform", "max"), RouteCase(2049, 257, "sorted", "short", 101)],
    "eight-w7": [RouteCase(1, 7, "uniform", "max", 2), RouteCase(63, 7, "sorted", "r64", 3), RouteCase(64, 7, "one_owner", "short", 5),
                 RouteCase(65, 7, "uniform", "short", 7), RouteCase(1024, 7, "clamp", "max", 11), RouteCase(1025, 7, "empty_tail", "r64", 13),
                 RouteCase(2049, 7, "oob", "max", 17), RouteCase(5000, 7, "uniform", "short", 19)],
    "eight-w1024": [RouteCase(n, 1024, "uniform", cap, rpr) for n, cap, rpr in
                    ((1, "max", 1), (63, "max", 2), (65, "r64", 3), (1023, "max", 4), (1025, "max", 5), (2049, "short", 1), (64, "max", 7), (5000, "max", 8))],
}


def route_id(c):
    return f"route-{c.n}-w{c.world}-{c.pattern}-{c.cap}" + (f"-rpr{c.rpr}" if c.rpr != 37 else "")


def route_rows(c):
    if c.pattern == "clamp":
        return c.world * c.rpr + c.rpr + 5  # the last owner holds the surplus rows
    if c.pattern == "empty_tail":
        return max(1, c.world // 2) * c.rpr - (1 if c.rpr > 1 else 0)
    return c.world * c.rpr


def route_ids(c):
    rng, R = _rng(route_id(c)), route_rows(c)
    if c.pattern == "one_owner":
        lo = min(3, c.world - 1) * c.rpr
        return rng.integers(lo, lo + c.rpr, c.n, dtype=np.int64)
    if c.pattern == "wave64":
        return (np.arange(c.n, dtype=np.int64) % 64) * c.rpr + rng.integers(0, c.rpr, c.n)
    ids = rng.integers(0, R, c.n, dtype=np.int64)
    if c.pattern == "clamp":
        ids[::3] = rng.integers(c.world * c.rpr, R, len(ids[::3]))  # owner id / rows_per_rank = world without the clamp
    if c.pattern == "sorted":
        ids.sort()
    if c.pattern in ("oob", "oob_null"):
        _plant_bad(ids, R)
    return ids


def route_cap(c, ids=None):
    big = int(route_reference(route_ids(c) if ids is None else ids, route_rows(c), c.rpr, c.world, 1).max_count)
    return {"max": big, "r64": -(-big // 64) * 64, "short": big - 3}[c.cap]


def route_reference(ids, n_rows, rows_per_rank, world, cap):
    counts = [0] * world
    send, src, slot_of, oob, overflow = [-1] * (world * cap), [-1] * (world * cap), [], 0, 0
    for i, v in enumerate(np.asarray(ids, np.int64).tolist()):
        if v < 0 or v >= n_rows:
            v, oob = 0, 1
        o = min(v // rows_per_rank, world - 1)
        r = counts[o]
        counts[o] += 1
        if r >= cap:
            overflow = 1
            slot_of.append(-1)
            continue
        send[o * cap + r], src[o * cap + r] = v, i
        slot_of.append(o * cap + r)
    return Route(np.array(counts, np.int32), max(counts), np.array(send, np.int64), np.array(slot_of, np.int64),
                 np.array(src, np.int64), oob, overflow)


def route_slow(ids, n_rows, rows_per_rank, world, cap):
    """The same routing from a dict: owner -> its (position, id) pairs in list order."""
    ids = np.asarray(ids, np.int64)
    bad = (ids < 0) | (ids >= n_rows)
    v = np.where(bad, 0, ids)
    owner = np.minimum(v // rows_per_rank, world - 1)
    mine = {o: [(int(i), int(v[i])) for i in np.flatnonzero(owner == o)] for o in range(world)}
    send, src = np.full(world * cap, -1, np.int64), np.full(world * cap, -1, np.int64)
    slot_of = np.full(len(ids), -1, np.int64)
    for o, pairs in mine.items():
        for r, (i, x) in enumerate(pairs[:cap]):
            send[o * cap + r], src[o * cap + r], slot_of[i] = x, i, o * cap + r
    counts = np.array([len(mine[o]) for o in range(world)], np.int32)
    return Route(counts, int(counts.max()), send, slot_of, src, int(bad.any()), int((counts > cap).any()))


ROUTE_MUTANTS = ("no_wave_prefix", "no_tile_prefix", "no_clamp", "pad_unwritten", "overflow_placed")


def route_evaluate(ids, n_rows, rows_per_rank, world, cap, mut=None):
    """The kernels' scheme -- tile offsets + earlier waves of the tile + lower lanes of the wave -- with one mistake."""
    pad = SENT64 if mut == "pad_unwritten" else -1
    n_slots = world * cap
    send, src, slot_of, oob, overflow = [pad] * n_slots, [pad] * n_slots, [], 0, 0
    total, tile, wave = collections.Counter(), collections.Counter(), collections.Counter()
    for i, v in enumerate(np.asarray(ids, np.int64).tolist()):
        if i % RT == 0:
            tile_off, tile = collections.Counter(total), collections.Counter()
        if i % 64 == 0:
            wave_off, wave = collections.Counter(tile), collections.Counter()
        if v < 0 or v >= n_rows:
            v, oob = 0, 1
        o = v // rows_per_rank
        if mut != "no_clamp":
            o = min(o, world - 1)
        r = ((0 if mut == "no_tile_prefix" else tile_off[o]) + (0 if mut == "no_wave_prefix" else wave_off[o]) + wave[o])
        total[o] += 1
        tile[o] += 1
        wave[o] += 1
        if r >= cap and mut != "overflow_placed":
            overflow = 1
            slot_of.append(-1)
            continue
        s = o * cap + r
        slot_of.append(s)
        if 0 <= s < n_slots:  # (a kernel with this mistake writes outside its buffers instead)
            send[s], src[s] = v, i
    counts = [total[o] for o in range(world)]
    return Route(np.array(counts, np.int32), max(counts), np.array(send, np.int64), np.array(slot_of, np.int64), np.array(src, np.int64),
                 oob, overflow)


def route_problems(ref, got):
    out = [k for k in ("counts", "send_ids", "slot_of", "src_of") if not np.array_equal(getattr(ref, k), getattr(got, k))]
    return out + [k for k in ("max_count", "oob", "overflow") if getattr(ref, k) != getattr(got, k)]


def route_case_reference(c):
    ids = route_ids(c)
    return route_reference(ids, route_rows(c), c.rpr, c.world, route_cap(c, ids))


# ---- the owner side
# n_local = 0: table = NULL
ServeCase = collections.namedtuple("ServeCase", "dtype dim n n_local", defaults=(23,))
SERVE_CASES = [ServeCase("f32", 4, 7), ServeCase("f32", 128, 8), ServeCase("f32", 132, 9), ServeCase("f32", 1, 9), ServeCase("f32", 50, 7),
               ServeCase("bf16", 50, 8), ServeCase("bf16", 128, 9), ServeCase("f32", 128, 9, 0), ServeCase("bf16", 50, 7, 0), ServeCase("f32", 50, 8, 0)]
SERVE_GROUPS = {"three": (0, 5, 7), "eight": (0, 1, 2, 3, 4, 5, 6, 9)}  # indices into SERVE_CASES
SERVE_LO = 100


def serve_id(c):
    return f"serve-{c.dtype}-d{c.dim}-n{c.n}-local{c.n_local}"


def serve_inputs(c):
    """(ids, table): -1, lo - 1, lo, lo + n_local - 1, lo + n_local in shuffled places among ids around the block; the table as
    float32, or as the uint16 bit patterns of bf16."""
    rng, lo = _rng(serve_id(c)), SERVE_LO
    ids = rng.integers(lo - 5, lo + c.n_local + 5, c.n, dtype=np.int64)
    ids[rng.permutation(c.n)[:5]] = (-1, lo - 1, lo, lo + c.n_local - 1, lo + c.n_local)
    if c.n_local == 0:
        return ids, None
    t = rng.standard_normal((c.n_local, c.dim)).astype(np.float32)
    return ids, t if c.dtype == "f32" else (t.view(np.uint32) >> 16).astype(np.uint16)


def localize_reference(ids, lo, n_local):
    return np.array([v - lo if (v >= 0 and lo <= v < lo + n_local) else n_local for v in np.asarray(ids, np.int64).tolist()], np.int64)


def serve_reference(ids, lo, n_local, table, dim):
    """(local, rows): rows float32 [n, dim], the table's row widened, exact zeros for "not mine"."""
    local = localize_reference(ids, lo, n_local)
    rows = np.zeros((len(local), dim), np.float32)
    for i, r in enumerate(local.tolist()):
        if r < n_local:
            rows[i] = table[r] if table.dtype == np.float32 else (table[r].astype(np.uint32) << 16).view(np.float32)
    return local, rows


def serve_slow(ids, lo, n_local, table, dim):
    """The same from a dict: local row -> the positions that ask for it."""
    asks = {}
    for i, v in enumerate(np.asarray(ids, np.int64).tolist()):
        asks.setdefault(v - lo if v in range(lo, lo + n_local) else n_local, []).append(i)
    local, rows = np.empty(len(ids), np.int64), np.zeros((len(ids), dim), np.float32)
    for r, at in asks.items():
        local[at] = r
        if r != n_local:
            rows[at] = table[r] if table.dtype == np.float32 else (table[r].astype(np.uint32) << 16).view(np.float32)
    return local, rows


# ------------------------------------------------------------------ one entry for both families
def evaluate(c, mut=None):
    """The case's outputs as the kernels compute them, with the mistake `mut`; without one, the reference's."""
    if isinstance(c, PlanCase):
        return plan_evaluate(plan_ids(c), c.n_rows, mut)
    ids = route_ids(c)
    return route_evaluate(ids, route_rows(c), c.rpr, c.world, route_cap(c, ids), mut)
