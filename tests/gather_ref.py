"""Float64 yardstick for the row gathers and the history pool (csrc/gather.hip): tt_gather_rows, tt_hist_embed_pool(_len),
tt_hist_pool_bwd(_len).  A helper, not a test: imported by test_gather_reference_cpu.py and test_gpu_gather_reference.py; the
product never imports it.

  reference   the table indexed in torch.  x = the float32 rounding of the float64 row + pe: ONE add, so bit equality is
              demanded; padded rows are exact zeros, a row with an out-of-range id is zero (+ pe).  pooled = the float64
              masked mean of the raw rows.  tt_gather_rows: bit equality.
  bounds      both derived, none measured:
                pooled of n rows    E = gamma(n + 1) sum_h |row_h| / n,  gamma(k) = k 2^-24 / (1 - k 2^-24): n - 1 adds, the
                                    reciprocal and its product, in any summation order
                pool backward       E = 3 * 2^-24 (|dx0| + |d_pooled| / len): the reciprocal, the product and the sum,
                                    contracted or not
  evaluate    the kernels' arithmetic in float32 (index-order sum, times the rounded reciprocal) or float64; `mut` names a
              deliberately wrong formula.
  CASES       what test_gpu_gather_reference.py runs; the CPU test runs the mutants at the very same cases."""
import collections

import torch

import attention_ref as AR
import gemm_ref as GR

fg, T = AR.fg, AR.T
F64, F32 = torch.float64, torch.float32
EPS = 2.0 ** -24
N_ROWS = 400
Launches = GR.Launches
E_BADARG = GR.E_BADARG
BAD_IDS = (-1, None, 2 ** 40, -2 ** 63)  # None: n_rows

GATHER_KERNELS = {(4, 8): "gather_rows_kernel_v4_l8", (4, 16): "gather_rows_kernel_v4_l16", (4, 32): "gather_rows_kernel_v4_l32",
                  (1, 64): "gather_rows_kernel_v1_l64"}
POOL_KERNELS = {("v4", False): "hist_embed_pool_kernel_v4", ("v4", True): "hist_embed_pool_len_kernel_v4",
                ("v1", False): "hist_embed_pool_kernel_v1", ("v1", True): "hist_embed_pool_len_kernel_v1"}
BWD_KERNELS = {False: "hist_pool_bwd_kernel", True: "hist_pool_bwd_len_kernel"}
KERNELS = tuple(GATHER_KERNELS.values()) + tuple(POOL_KERNELS.values()) + tuple(BWD_KERNELS.values())


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


# ------------------------------------------------------------------ tt_hist_embed_pool(_len)
# form: "ids" | "emb" (ids = NULL: the table is the embedded [B, H, dim] input)
# how (what sends a dim % 4 == 0 call to the scalar path): None | "ld" (ld_pooled % 4 != 0) | "pe_off" | "pooled_off" | "x_off"
#     (one float off a 16-byte boundary) | "out1" (pooled = out[:, 1, :] of [B, 2, dim], dim odd)
# lens: None | "list" (1, 2, 31, 32, 33, 63, 64, 65, H - 1, H; padded ids out of range, padded embedded rows NaN) |
#       "bad_lo" (0 planted) | "bad_hi" (H + 1 planted): clamped, the flag set, each on its own |
#       "null" (tt_hist_embed_pool_len with lengths = NULL)
# oob: ids -1, n_rows, 2^40, -2^63 in valid slots of both rounds
Pool = collections.namedtuple("Pool", "group dim H B form pe how lens oob", defaults=(None, None, False))

VEC_SHAPES = ((128, 50, 9), (128, 64, 3), (128, 65, 3), (128, 128, 3), (128, 200, 2), (8, 65, 2), (132, 70, 2), (256, 129, 2))
SCALAR_SHAPES = ((50, 7, 2), (50, 33, 2), (65, 65, 2), (1, 128, 2))
POOL_CASES = ([Pool("vec", *s, form, pe) for s in VEC_SHAPES for form in ("ids", "emb") for pe in (True, False)]
              + [Pool("scalar", *s, form, pe) for s in SCALAR_SHAPES for form, pe in (("ids", True), ("emb", False))]
              + [Pool("switch", 128, 65, 2, "ids", True, how) for how in ("ld", "pe_off", "pooled_off", "x_off")]
              + [Pool("switch", 65, 65, 2, "ids", True, "out1")]
              + [Pool("oob", 128, 130, 2, "ids", True, None, None, True), Pool("oob", 50, 70, 2, "ids", True, None, None, True)]
              + [Pool("len", dim, H, 10, form, True, None, "list") for dim in (128, 50) for H in (65, 128) for form in ("ids", "emb")]
              + [Pool("len", dim, 65, 10, "ids", True, None, kind) for dim in (128, 50) for kind in ("bad_lo", "bad_hi", "null")])


def pool_id(c):
    return (f"{c.group}-d{c.dim}-H{c.H}-B{c.B}-{c.form}" + ("-pe" if c.pe else "") + (f"-{c.how}" if c.how else "")
            + (f"-len_{c.lens}" if c.lens else "") + ("-oob" if c.oob else ""))


def pool_path(c):
    return "v4" if c.dim % 4 == 0 and c.how is None else "v1"


def pool_round(c):
    """History positions per round of the fused kernel: G * U = 8 * 8 on the float4 path, 4 * 8 on the scalar path."""
    return 64 if pool_path(c) == "v4" else 32


def pool_columns(c):
    """Columns per trip of the column loop: 32 lanes of float4, or 64 lanes."""
    return 128 if pool_path(c) == "v4" else 64


def pool_lengths(c):
    """(what the call is given, what the kernel uses) or (None, None)."""
    if c.lens not in ("list", "bad_lo", "bad_hi"):
        return None, None
    raw = [v for v in (1, 2, 31, 32, 33, 63, 64, 65, c.H - 1, c.H) if v <= c.H][:c.B]
    raw = raw + [c.H] * (c.B - len(raw))
    if c.lens == "bad_lo":
        raw[0] = 0
    if c.lens == "bad_hi":
        raw[1] = c.H + 1
    return raw, [min(max(v, 1), c.H) for v in raw]


def pool_inputs(c):
    seed = 5000 + 17 * c.dim + c.H
    raw, lens = pool_lengths(c)
    valid = torch.arange(c.H)[None, :] < torch.tensor(lens if lens else [c.H] * c.B)[:, None]
    inp = dict(pe=T(fg.gaussianish((c.H, c.dim), seed + 2)) if c.pe else None, lengths=raw, lens=lens, valid=valid, ids=None)
    if c.form == "ids":
        inp["table"] = T(fg.gaussianish((N_ROWS, c.dim), seed))
        ids = T(fg.uniform_ids((c.B, c.H), N_ROWS, seed + 1)).clone()
        if c.oob:  # both rounds of the path, both samples
            R = pool_round(c)
            for (b, h), v in zip(((0, 3), (0, R + 6), (1, 5), (1, c.H - 1)), BAD_IDS):
                ids[b, h] = N_ROWS if v is None else v
        pad = torch.tensor([N_ROWS + 5, -7, 2 ** 40, -2 ** 63])[(torch.arange(c.B)[:, None] + torch.arange(c.H)[None, :]) % 4]
        inp["ids"] = torch.where(valid, ids, pad)
    else:
        emb = T(fg.gaussianish((c.B, c.H, c.dim), seed + 3))
        inp["table"] = torch.where(valid[:, :, None], emb, torch.full_like(emb, float("nan")))
    return inp


def pool_evaluate(c, inp, dtype=F64, mut=None):
    """(x [B, H, dim] float32, pooled [B, dim] in dtype, flag) the way hist_embed_pool_kernel forms them.  mut: "round2" the
    second round dropped; "pe_pad" pe added on padded slots; "mean_H" the mean over H; "oob_row0" an out-of-range id reads row
    0; "pooled_pe" pooled from x + pe; "col_trip" the column trips beyond the first dropped."""
    B, H, dim = c.B, c.H, c.dim
    valid = inp["valid"]
    if c.form == "ids":
        ok = (inp["ids"] >= 0) & (inp["ids"] < N_ROWS)
        rows = inp["table"][torch.where(ok, inp["ids"], torch.zeros_like(inp["ids"]))]
        if mut != "oob_row0":
            rows = torch.where(ok[:, :, None], rows, torch.zeros_like(rows))
    else:
        ok = torch.ones(B, H, dtype=torch.bool)
        rows = inp["table"]
    rows = torch.where(valid[:, :, None], rows, torch.zeros_like(rows))  # padded rows are not read
    pe = inp["pe"] if c.pe else torch.zeros(H, dim)
    x = (rows.double() + pe.double()[None]).float()
    x = torch.where(valid[:, :, None], x, (pe[None].expand(B, H, dim) if mut == "pe_pad" else torch.zeros_like(x)))
    src = (x if mut == "pooled_pe" else rows).to(dtype)
    n = torch.full((B,), float(H)) if mut == "mean_H" else valid.sum(1).float()
    took = valid.clone()
    if mut == "round2":
        took[:, pool_round(c):] = False
        x = torch.where((torch.arange(H) < pool_round(c))[None, :, None], x, torch.full_like(x, float("nan")))
    src = torch.where(took[:, :, None], src, torch.zeros_like(src))
    if dtype == F64:
        pooled = src.sum(1) / n.double()[:, None]
    else:
        acc = torch.zeros(B, dim)
        for h in range(H):
            acc = acc + src[:, h]
        pooled = acc * (1.0 / n)[:, None]
    if mut == "col_trip":
        cut = pool_columns(c)
        x = torch.cat([x[..., :cut], torch.full_like(x[..., cut:], float("nan"))], dim=-1)
        pooled = torch.cat([pooled[..., :cut], torch.full_like(pooled[..., cut:], float("nan"))], dim=-1)
    raw = inp["lengths"]
    flag = int(bool((valid & ~ok).any()) or (raw is not None and any(v < 1 or v > H for v in raw)))
    return x, pooled, flag


def pool_applies(mut, c):
    _, lens = pool_lengths(c)
    short = lens is not None and min(lens) < c.H
    return {"round2": c.H > pool_round(c), "pe_pad": short and c.pe, "mean_H": short, "oob_row0": c.oob, "pooled_pe": c.pe,
            "col_trip": c.dim > pool_columns(c)}[mut]


POOL_MUTANTS = ("round2", "pe_pad", "mean_H", "oob_row0", "pooled_pe", "col_trip")


def pool_reference(c, inp):
    """{"x": float32, "pooled": float64, "E": the bound on pooled, "flag"}."""
    x, pooled, flag = pool_evaluate(c, inp)
    if c.form == "ids":
        ok = (inp["ids"] >= 0) & (inp["ids"] < N_ROWS)
        raw_rows = torch.where((ok & inp["valid"])[:, :, None], inp["table"][torch.where(ok, inp["ids"], torch.zeros_like(inp["ids"]))], torch.zeros(1))
    else:
        raw_rows = torch.where(inp["valid"][:, :, None], inp["table"], torch.zeros(1))
    n = inp["valid"].sum(1).double()
    E = torch.tensor([gamma(int(k) + 1) for k in n])[:, None] * raw_rows.double().abs().sum(1) / n[:, None]
    return dict(x=x, pooled=pooled, E=E, flag=flag)


def pool_problems(ref, x, pooled, flag):
    """What is wrong with a result, as a list (empty: nothing)."""
    bad = []
    if not bool((x.contiguous().view(torch.int32) == ref["x"].contiguous().view(torch.int32)).all()):
        bad.append("x is not the rounded row + pe bit for bit")
    err = (pooled.double() - ref["pooled"]).abs()
    if not bool((err <= ref["E"]).all()):  # NaN fails
        bad.append(f"pooled outside E: worst err / E {float((err / ref['E'].clamp_min(1e-300)).nan_to_num(float('inf')).max()):.3f}")
    if flag != ref["flag"]:
        bad.append(f"flag {flag}, want {ref['flag']}")
    return bad


def pool_worst(ref, pooled):
    """Worst err / E (an error where E = 0 counts as inf)."""
    err = (pooled.double() - ref["pooled"]).abs().nan_to_num(float("inf"))
    q = torch.where(ref["E"] > 0, err / ref["E"].clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")).double())
    return float(q.max())


# ------------------------------------------------------------------ tt_gather_rows
# how: None (ld_out = dim + 4, or dim + 3 on the scalar dims) | "ld" (ld_out % 4 != 0) | "out_off" (out one float off)
Gather = collections.namedtuple("Gather", "dim n_ids flag how", defaults=(True, None))
GATHER_DIMS = (4, 32, 36, 64, 68, 128, 256, 2, 50, 130)
GATHER_ROWS = 97


def gather_instantiation(c):
    if c.dim % 4 or c.how:
        return (1, 64)
    return (4, 8) if c.dim <= 32 else (4, 16) if c.dim <= 64 else (4, 32)


def rows_per_workgroup(inst):
    return 256 // inst[1]


def _gather_n(dim):
    r = rows_per_workgroup(gather_instantiation(Gather(dim, 1)))
    return (1, r - 1, r + 1, 1000)


GATHER_CASES = ([Gather(d, n) for d in GATHER_DIMS for n in _gather_n(d)]
                + [Gather(d, _gather_n(d)[2], False) for d in GATHER_DIMS]
                + [Gather(64, n, True, how) for how in ("ld", "out_off") for n in (5, 1000)])


def gather_id(c):
    return f"d{c.dim}-n{c.n_ids}" + ("" if c.flag else "-noflag") + (f"-{c.how}" if c.how else "")


def gather_inputs(c):
    table = T(fg.gaussianish((GATHER_ROWS, c.dim), 4000 + c.dim))
    ids = T(fg.uniform_ids((c.n_ids,), GATHER_ROWS, 4100 + c.dim + c.n_ids)).clone()  # 1000 ids of 97 rows: they repeat
    for k, i in enumerate(range(3, c.n_ids, 7)):
        v = BAD_IDS[k % 4]
        ids[i] = GATHER_ROWS if v is None else v
    return table, ids


def gather_reference(c, table, ids):
    """(out [n_ids, dim], flag): rows copied bit for bit, zeros for an id out of range."""
    ok = (ids >= 0) & (ids < GATHER_ROWS)
    out = torch.where(ok[:, None], table[torch.where(ok, ids, torch.zeros_like(ids))], torch.zeros(1))
    return out, int(bool((~ok).any()) and c.flag)


# ------------------------------------------------------------------ tt_hist_pool_bwd(_len)
Bwd = collections.namedtuple("Bwd", "B H dim lens")  # lens: None | "cycle" | "null"
BWD_CASES = [Bwd(B, H, dim, lens) for (B, H, dim) in ((3, 7, 50), (100, 128, 128)) for lens in (None, "cycle", "null")]
BWD_GRID = 4096 * 256  # elements one trip of the grid-stride loop covers


def bwd_id(c):
    return f"B{c.B}-H{c.H}-d{c.dim}" + (f"-len_{c.lens}" if c.lens else "")


def bwd_inputs(c):
    dx0 = T(fg.gaussianish((c.B, c.H, c.dim), 6000 + c.dim))
    dp = T(fg.gaussianish((c.B, c.dim), 6001 + c.dim))
    lens = [1 + (b % c.H) for b in range(c.B)] if c.lens == "cycle" else None
    return dx0, dp, lens


def bwd_evaluate(c, dx0, dp, lens, dtype=F64, mut=None):
    """dx0[b, h < len] + d_pooled[b] / len, rows behind len left as they are.  mut "pad": the padded rows take it too."""
    n = torch.tensor(lens if lens else [c.H] * c.B)
    valid = (torch.arange(c.H)[None, :] < n[:, None])[:, :, None]
    if dtype == F64:
        add = dp.double()[:, None, :] / n.double()[:, None, None]
    else:
        add = dp[:, None, :] * (1.0 / n.float())[:, None, None]
    out = dx0.to(dtype) + add
    return out if mut == "pad" else torch.where(valid, out, dx0.to(dtype))


def bwd_problems(c, dx0, dp, lens, got):
    n = torch.tensor(lens if lens else [c.H] * c.B)
    valid = (torch.arange(c.H)[None, :] < n[:, None])[:, :, None].expand_as(dx0)
    ref = bwd_evaluate(c, dx0, dp, lens)
    E = 3 * EPS * (dx0.double().abs() + dp.double().abs()[:, None, :] / n.double()[:, None, None])
    bad = []
    if not bool(((got.double() - ref).abs() <= E)[valid].all()):
        bad.append(f"outside E: worst err / E {float(((got.double() - ref).abs() / E)[valid].nan_to_num(float('inf')).max()):.3f}")
    if not bool((got.double() == dx0.double())[~valid].all()):  # dx0 is finite: equal values are equal bits
        bad.append("a padded dx row changed")
    return bad


def bwd_worst(c, dx0, dp, lens, got):
    n = torch.tensor(lens if lens else [c.H] * c.B)
    E = 3 * EPS * (dx0.double().abs() + dp.double().abs()[:, None, :] / n.double()[:, None, None])
    valid = (torch.arange(c.H)[None, :] < n[:, None])[:, :, None].expand_as(dx0)
    return float(((got.double() - bwd_evaluate(c, dx0, dp, lens)).abs() / E)[valid].nan_to_num(float("inf")).max())


# ------------------------------------------------------------------ the GPU calls (test_gpu_gather_reference.py)
def _guard():
    import encoder_last_ref as ER
    return ER.Guard


def _flag(dev):
    """An int32 flag between two sentinels."""
    return torch.tensor([-77, 0, -77], dtype=torch.int32, device=dev)


def gpu_pool(c, inp, dev, how="case", lengths="case"):
    """One call -> dict(rc, launches, x, pooled, flag, clean).  how / lengths override the case's (for the bit comparisons
    with the float4 path and with the call without `_len`)."""
    from two_tower_models_amd import _native as N
    lib, Guard = N.load(), _guard()
    how = c.how if how == "case" else how
    B, H, dim = c.B, c.H, c.dim
    tbl = inp["table"].reshape(-1, dim)
    table = Guard(dev, tbl.shape[0], dim, fill=tbl)
    pe = Guard(dev, H, dim, off=1 if how == "pe_off" else 0, fill=inp["pe"]) if c.pe else None
    x = Guard(dev, B * H, dim, off=1 if how == "x_off" else 0)
    ld, off = {None: (dim + 4 if dim % 4 == 0 else dim + 3, 0), "ld": (dim + 2, 0), "pe_off": (dim + 4, 0), "x_off": (dim + 4, 0),
               "pooled_off": (dim + 4, 1), "out1": (2 * dim, dim)}[how]
    pooled = Guard(dev, B, dim, ld=ld, off=off)
    ids = inp["ids"].to(dev) if inp["ids"] is not None else None
    flag = _flag(dev)
    use_len = c.lens is not None and lengths is not False
    ln = torch.tensor(inp["lengths"], dtype=torch.int32, device=dev) if (use_len and inp["lengths"] is not None and lengths == "case") else None
    head = (table.ptr, N_ROWS if ids is not None else 0, dim, None if ids is None else ids.data_ptr(), B, H)
    tail = (None if pe is None else pe.ptr, x.ptr, pooled.ptr, ld, flag.data_ptr() + 4, N.stream())
    with Launches(KERNELS) as n:
        if use_len:
            rc = lib.tt_hist_embed_pool_len(*head, None if ln is None else ln.data_ptr(), *tail)
        else:
            rc = lib.tt_hist_embed_pool(*head, *tail)
    torch.cuda.synchronize()
    f = flag.cpu().tolist()
    clean = (x.outside_clean() and pooled.outside_clean() and table.unchanged() and (pe is None or pe.unchanged())
             and f[0] == -77 and f[2] == -77 and (ids is None or bool((ids.cpu() == inp["ids"]).all())))
    return dict(rc=rc, launches={k: v for k, v in n.items() if v}, x=x.get().reshape(B, H, dim), pooled=pooled.get(), flag=f[1], clean=clean)


def gpu_gather(c, table, ids, dev):
    from two_tower_models_amd import _native as N
    lib, Guard = N.load(), _guard()
    ld, off = {None: (c.dim + 4 if c.dim % 4 == 0 else c.dim + 3, 0), "ld": (c.dim + 3, 0), "out_off": (c.dim + 4, 1)}[c.how]
    tb, out, flag, idd = Guard(dev, GATHER_ROWS, c.dim, fill=table), Guard(dev, c.n_ids, c.dim, ld=ld, off=off), _flag(dev), ids.to(dev)
    with Launches(KERNELS) as n:
        rc = lib.tt_gather_rows(tb.ptr, GATHER_ROWS, c.dim, idd.data_ptr(), c.n_ids, out.ptr, ld, flag.data_ptr() + 4 if c.flag else None,
                                N.stream())
    torch.cuda.synchronize()
    f = flag.cpu().tolist()
    return dict(rc=rc, launches={k: v for k, v in n.items() if v}, out=out.get(), flag=f[1],
                clean=out.outside_clean() and tb.unchanged() and f[0] == -77 and f[2] == -77)


def gpu_bwd(c, dx0, dp, lens, dev, entry_len):
    """d_pooled as the [:, 1, :] half of a [B, 2, dim] NaN buffer (ld = 2 dim)."""
    from two_tower_models_amd import _native as N
    lib, Guard = N.load(), _guard()
    dx, d_pooled = Guard(dev, c.B * c.H, c.dim, fill=dx0), Guard(dev, c.B, c.dim, ld=2 * c.dim, off=c.dim + (-c.dim) % 4, fill=dp)
    ln = torch.tensor(lens, dtype=torch.int32, device=dev) if lens else None
    with Launches(KERNELS) as n:
        if entry_len:
            rc = lib.tt_hist_pool_bwd_len(dx.ptr, c.B, c.H, c.dim, None if ln is None else ln.data_ptr(), d_pooled.ptr, 2 * c.dim, N.stream())
        else:
            rc = lib.tt_hist_pool_bwd(dx.ptr, c.B, c.H, c.dim, d_pooled.ptr, 2 * c.dim, N.stream())
    torch.cuda.synchronize()
    return dict(rc=rc, launches={k: v for k, v in n.items() if v}, dx=dx.get().reshape(c.B, c.H, c.dim),
                clean=dx.outside_clean() and d_pooled.unchanged())
