"""Float64 yardstick for the fp32 GEMM family (csrc/gemm.hip, gemm_ws.hip, gemm_ws16.hip, gemm_tn_stream.hip behind
tt_gemm_f32, tt_gemm_tn_colsum_f32, tt_colsum_f32 and tt_hist_dx_pool_bwd).  A helper, not a test: imported by
test_gemm_reference_cpu.py and test_gpu_gemm_reference.py the way mips_ref.py is imported by its tests; the product never
imports it.

  inputs      four classes, all from fixture_gen, hashed by ELEMENT INDEX of one flat stream per operand kind: the seeds leave
              the shape out, so the operand of a smaller M is a prefix of a larger one's.
                exact      fg.trits for operands, bias, aux and old C; row m of op(A) times 2^((m % 5) - 2).  Every product and
                           partial sum is a multiple of 2^-2 below 2^22: ANY summation order gives the float64 result exactly,
                           and the checker demands equality at every K, 49 173 included.
                flat       fg.gaussianish, never rounded
                positive   |a|, |b|: no cancellation (K <= 8195 only: beyond it the index-order yardstick is too wide to
                           catch a dropped term)
                range      rows of op(A) scaled by 2^(4 g), g gaussianish per row
  reference   float64: s64 = op(A) op(B); pre = s64 + bias (+ scale pool[m / group]); ReLU or the (aux > 0) mask -- on aux,
              not on the value, and BEFORE the accumulate; + C_old.  aux carries -0.0, +0.0, 2^-126, -2^-126 at
              aux_plants(): only 2^-126 passes.  tt_gemm_tn_colsum_f32 also db = colsum(A).
  YARD        the worst |s32 - s64| / (2^-24 Abs) of a float32 index-order evaluation (one rounding per multiply and per add,
              numpy ufuncs, no BLAS) per (class, K band), over the leading YARD_ROWS x YARD_COLS block of every distinct
              (entry, layout, N, K, class) of the case table (the block is a prefix: see inputs).  `python tests/gemm_ref.py`
              prints the table, test_gemm_reference_cpu.py re-measures it.  Never calibrated against a kernel.
  bound       per element  E = 4 YARD 2^-24 Abs + 2^-24 |result|,  Abs = |A||B| + |bias| + |C_old| (+ |pool term|).  The factor
              4 is the project's (mips_ref.py, profiles/adam_reference_tolerance.txt).  Where ReLU's argument is within E of
              zero either branch is accepted; those elements are counted, and at most BAND_SHARE of a case may be there.
  CASES       every call test_gpu_gemm_reference.py makes, each with the path it must land on; route() restates the
              dispatch (plan_gemm, the rowgroups formula, Ws16Cfg::ROWS, tns_s / tns_nwg, the alignment predicates) the way
              mips_ref.py restates GROUP / CHUNK, and gives tiles / stages per workgroup.
  buffers     every operand is a view into a larger NaN-filled buffer (padding columns, rows before and after); C without
              accumulate is NaN-prefilled too.  check() wants every result finite and within E and every byte outside the C
              view unchanged.

profiles/gemm_reference_tolerance.txt records the tables and what the GPU showed."""
import collections
import os
import sys

import numpy as np
import torch

try:
    import fixture_gen as fg
except ImportError:  # run as a script or from a child process: pytest's conftest.py is what puts tests/golden on the path
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import fixture_gen as fg

EPS = 2.0 ** -24
FACTOR = 4.0
BAND_SHARE = 1e-3
NT, NN, TN = 0, 1, 2
EPI_NONE, EPI_RELU, EPI_MASK = 0, 1, 2
E_BADARG, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -3
LAYOUT = {NT: "NT", NN: "NN", TN: "TN"}
KERNELS = ("gemm_tile64", "gemm_tile64_full", "gemm_tile128", "gemm_tile128_full", "splitk_reduce_kernel", "gemm_ws_kernel",
           "gemm_ws16_kernel", "tn_stream_kernel")
STREAM_ALL = "TT_GEMM_TN_STREAM_ALL"

# constants of csrc/ the cases rest on
BK, BI, BJ = 32, 128, 64  # gemm.hip K-tile; mfma_stream.hpp: columns per gemm_ws workgroup, rows per gemm_ws tile
WS_MIN_M, WS_MAX_K, WS_PASS_K = 16384, 512, 256

# worst |s32 - s64| / (2^-24 Abs) of the float32 index-order evaluation per (class, K band): see main()
BANDS = (64, 512, 8195, 1 << 30)
YARD = {
    "flat": {64: 4.4, 512: 4.3, 8195: 5.3, 1 << 30: 4.3},
    "positive": {64: 7.1, 512: 11.6, 8195: 98.0},
    "range": {64: 4.2, 512: 5.7, 8195: 3.8},
}
YARD_ROWS, YARD_COLS = 64, 128

Case = collections.namedtuple(
    "Case", "group entry layout M N K cls padA offA padB offB padC offC padX offX bias epi acc H env path need")


def _c(group, entry, layout, M, N, K, path, cls="flat", padA=4, offA=0, padB=4, offB=0, padC=4, offC=0, padX=4, offX=0,
       bias=None, epi=EPI_NONE, acc=0, H=0, env="", **need):
    return Case(group, entry, layout, M, N, K, cls, padA, offA, padB, offB, padC, offC, padX, offX, bias, epi, acc, H, env,
                path, tuple(sorted(need.items())))


def case_id(c):
    s = f"{c.group}-{c.entry}-{LAYOUT[c.layout]}-M{c.M}-N{c.N}-K{c.K}-{c.cls}"
    s += f"-a{c.padA}.{c.offA}-b{c.padB}.{c.offB}-c{c.padC}.{c.offC}"
    if c.epi == EPI_MASK:
        s += f"-x{c.padX}.{c.offX}"
    if c.bias:
        s += "-bias" if c.bias == "yes" else "-biasmis"
    s += ("", "-relu", "-mask")[c.epi] + ("-acc" if c.acc else "") + (f"-H{c.H}" if c.H else "") + ("-all" if c.env else "")
    return s


# ------------------------------------------------------------------ the dispatch, restated
def ceil_div(a, b):
    return -(-a // b)


def round_up(a, b):
    return ceil_div(a, b) * b


def plan_gemm(M, N, K):
    """gemm.hip plan_gemm -> (tile, splits, k_per_split)."""
    t128 = ceil_div(M, 128) * ceil_div(N, 128)
    bm = 128 if (t128 >= 192 or (K >= 8192 and M >= 128 and N >= 128 and t128 >= 2)) else 64
    tiles = ceil_div(M, bm) * ceil_div(N, bm)
    ktiles = ceil_div(K, BK)
    splits = 1
    if tiles < 256 and ktiles >= 16:
        splits = max(1, min(256 // tiles, ktiles // 4, 256))
    kps = ceil_div(ktiles, splits) * BK
    return bm, ceil_div(K, kps), kps


def ws16_rows(kb, nb):
    """Ws16Cfg<KB, NB>::ROWS."""
    return 32 if kb == 3 else 48 if kb == 2 else 48 if nb == 3 else 64 if nb == 2 else 96


def tns_s(cg):
    return 12 if cg == 3 else 16 if cg == 2 else 8


def tns_nwg(M, K):
    chunks = ceil_div(K, 2 * tns_s(M // 128))
    return min(chunks, 768 if M == 128 else 256)


def tns_ws_floats(M, N, K, stream_all):
    if N != 128 or not (M == 384 or (stream_all and M in (128, 256))) or K < 8192:
        return 0
    cg = M // 128
    return tns_nwg(M, K) * (4 * cg * 4 * 16 * 64 + cg * 4 * 32)


def workspace_bytes(layout, M, N, K, stream_all=False):
    """tt_gemm_workspace_bytes."""
    if M <= 0 or N <= 0 or K <= 0:
        return 0
    _, splits, _ = plan_gemm(M, N, K)
    generic = round_up(splits * M * (N + 1) * 4, 256) if splits > 1 else 0
    stream = round_up(tns_ws_floats(M, N, K, stream_all) * 4, 256) if layout == TN else 0
    return max(generic, stream)


def colsum_rows_per_part(M):
    r = 64
    while ceil_div(M, r) > 512:
        r *= 2
    return r


def per_workgroup(n, groups):
    """(fewest, most) items a workgroup gets under the balanced partition t0 = n g / G, t1 = n (g + 1) / G."""
    sizes = [n * (g + 1) // groups - n * g // groups for g in range(groups)]
    return min(sizes), max(sizes)


def dims(c):
    """(rows, width) of A, B as stored."""
    a = (c.M, c.K) if c.layout != TN else (c.K, c.M)
    b = (c.N, c.K) if c.layout == NT else (c.K, c.N)
    return a, b


def lds(c):
    (_, wa), (_, wb) = dims(c)
    return wa + c.padA, wb + c.padB, c.N + c.padC, c.N + c.padX


def _ws_one(c, K, lda, ldw, ldc, a_al, w_al, c_al, x_al, bias, epi, aux, acc):
    """ws_launch_one of gemm_ws.hip -> its launch parameters."""
    dp8 = 4 if K <= 32 else 8 if K <= 64 else 16 if K <= 128 else 32
    a_vec = lda % 4 == 0 and a_al
    c_vec = ldc % 4 == 0 and c_al and (not aux or ((c.N + c.padX) % 4 == 0 and x_al))
    dma = a_vec and K == dp8 * 8 and lda <= (1 << 22)
    tiles, colblocks = ceil_div(c.M, BJ), ceil_div(c.N, BI)
    slots = 256 * (2 if (dma and dp8 <= 16) else 1)
    rowgroups = min(max(slots // colblocks // 8 * 8, 8), tiles)
    mode = "GENERIC"
    if c_vec and c.N % 32 == 0 and epi == EPI_NONE:
        mode = "ACC" if acc else "PLAIN"
    return {"dp8": dp8, "dma": dma, "mode": mode, "rowgroups": rowgroups, "tiles": per_workgroup(tiles, rowgroups)}


def route(c):
    """The path a case takes: {"path", "launches" {kernel: count}, and the parameters of that path}.  Pointer alignment is
    the base offset's (buffers() puts every view an offset of `off` floats behind a 16-byte boundary)."""
    none = {k: 0 for k in KERNELS}

    def out(path, **kw):
        n = dict(none)
        n.update(kw.pop("launches", {}))
        return dict(path=path, launches=n, **kw)

    if c.entry == "colsum":
        rpp = colsum_rows_per_part(c.M)
        return out("colsum", rows_per_part=rpp, parts=ceil_div(c.M, rpp))
    if c.entry == "pool":
        rows = ws16_rows(3, 1)
        nst = ceil_div(c.M, rows)
        return out("pool", launches={"gemm_ws16_kernel": 1}, rows=rows, stages=per_workgroup(nst, min(nst, 256)),
                   last_rows=c.M - (nst - 1) * rows)
    M, N, K, layout = c.M, c.N, c.K, c.layout
    if M == 0 or N == 0:
        return out("none")
    lda, ldb, ldc, ldx = lds(c)
    a_al, b_al, c_al, x_al = c.offA % 4 == 0, c.offB % 4 == 0, c.offC % 4 == 0, c.offX % 4 == 0
    bias_al = c.bias != "mis"
    aux = c.epi == EPI_MASK  # the tests pass aux only with the mask epilogue
    colsum = c.entry == "tncs"
    if layout == TN and not c.bias and c.epi == EPI_NONE and tns_ws_floats(M, N, K, bool(c.env)):
        if a_al and b_al and lda % 4 == 0 and ldb % 4 == 0 and lda < (1 << 22) and ldb < (1 << 22):
            cg = M // 128
            nst = ceil_div(K, 2 * tns_s(cg))
            nwg = tns_nwg(M, K)
            return out("tns", launches={"tn_stream_kernel": 1}, cg=cg, nwg=nwg, stages=per_workgroup(nst, nwg),
                       last_rows=K - (nst - 1) * 2 * tns_s(cg))
    if not colsum and layout != TN and M >= WS_MIN_M:
        if (N % 128 == 0 and K % 128 == 0 and N >= 128 and K >= 128 and (N // 128) * (K // 128) <= 3 and c.epi == EPI_NONE
                and not c.acc and a_al and b_al and c_al and bias_al and lda % 4 == 0 and ldb % 4 == 0 and ldc % 4 == 0
                and lda <= (1 << 20)):
            kb, nb = K // 128, N // 128
            rows = ws16_rows(kb, nb)
            nst = ceil_div(M, rows)
            return out("ws16", launches={"gemm_ws16_kernel": 1}, cfg=(kb, nb), rows=rows,
                       stages=per_workgroup(nst, min(nst, 256)), last_rows=M - (nst - 1) * rows)
        if 1 <= K <= WS_MAX_K and M * ldc < (1 << 31) and (not aux or M * ldx < (1 << 31)):
            if K <= WS_PASS_K:
                one = _ws_one(c, K, lda, ldb, ldc, a_al, b_al, c_al, x_al, c.bias, c.epi, aux, c.acc)
                return out("ws", launches={"gemm_ws_kernel": 1}, passes=[one], last_rows=M - (ceil_div(M, BJ) - 1) * BJ)
            bypass = (M % 128 == 0 and N % 128 == 0 and K % 32 == 0 and lda % 4 == 0 and ldb % 4 == 0 and a_al and b_al)
            if not (c.acc and c.epi != EPI_NONE) and not bypass:
                p1 = _ws_one(c, WS_PASS_K, lda, ldb, ldc, a_al, b_al, c_al, x_al, c.bias, EPI_NONE, False, c.acc)
                p2 = _ws_one(c, K - WS_PASS_K, lda, ldb, ldc, a_al, b_al, c_al, x_al, None, c.epi, aux, 1)
                return out("ws2", launches={"gemm_ws_kernel": 2}, passes=[p1, p2], last_rows=M - (ceil_div(M, BJ) - 1) * BJ)
    a_vec, b_vec = lda % 4 == 0 and a_al, ldb % 4 == 0 and b_al
    bm, splits, kps = plan_gemm(M, N, max(K, 1))
    if K == 0:
        splits = 1
    full = M % bm == 0 and N % bm == 0 and K % BK == 0 and a_vec and b_vec
    name = f"gemm_tile{bm}" + ("_full" if full else "")
    path = f"t{bm}" + ("f" if full else "") + ("+sk" if splits > 1 else "")
    return out(path, launches={name: 1, "splitk_reduce_kernel": int(splits > 1)}, tile=bm, full=full, splits=splits,
               k_per_split=kps, last_split=K - (splits - 1) * kps, a_vec=a_vec, b_vec=b_vec,
               last_rows=M - (ceil_div(M, bm) - 1) * bm,
               ws_need=round_up(splits * M * (N + 1) * 4, 256) if splits > 1 else 0)


def claims(c, r):
    """[(claim, what the case table says, what route() gives)] for every claim a case makes beyond its path."""
    got = {}
    if r["path"] in ("ws", "ws2"):
        p = r["passes"]
        got.update(dp8=p[0]["dp8"], dma=p[0]["dma"], mode=p[0]["mode"], tiles=p[0]["tiles"], mode1=p[0]["mode"],
                   mode2=p[-1]["mode"], dma2=p[-1]["dma"])
    return [(k, v, got.get(k, r.get(k))) for k, v in c.need]


def row_unit(c, r):
    """Rows of one tile or stage along the streamed / tiled M of the case's path."""
    return {"ws": BJ, "ws2": BJ}.get(r["path"], r.get("rows", r.get("tile", 0)))


# ------------------------------------------------------------------ inputs
_SEED = {"a": 71001, "b": 71002, "bias": 71003, "aux": 71004, "cold": 71005, "pool": 71006, "g": 71007}
_streams = {}


def _need(kind, trit):
    n = 4
    for c in CASES:
        if (c.cls == "exact") != trit:
            continue
        (ra, wa), (rb, wb) = dims(c) if c.entry != "colsum" else ((c.M, c.N), (0, 0))
        n = max(n, {"a": ra * wa, "b": rb * wb, "bias": c.N, "aux": c.M * c.N, "cold": c.M * c.N,
                    "pool": (c.M // c.H if c.H else 0) * c.N, "g": max(c.M, c.N)}[kind])
    return n


def stream(kind, trit, n):
    """The first n values of the operand kind's flat stream (float32): a hash of the element index."""
    k = (kind, trit)
    if k not in _streams or _streams[k].shape[0] < n:
        m = max(n, _need(kind, trit))
        _streams[k] = (fg.trits if trit else fg.gaussianish)((m,), _SEED[kind] + (500 if trit else 0))
    return _streams[k][:n]


def aux_plants(M, N):
    """[(m, n, value)]: -0.0, +0.0, 2^-126 and -2^-126 in aux; only 2^-126 passes the mask."""
    vals = (-0.0, 0.0, 2.0 ** -126, -(2.0 ** -126))
    flat = sorted({0, (M * N) // 3, (M * N) // 2, M * N - 1})
    return [(f // N, f % N, v) for f, v in zip(flat, vals)] if M * N >= 4 and len(flat) == 4 else []


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def operands(c, rows=None):
    """(A, B) float32 numpy as stored ([M, K] / [K, M]; [N, K] / [K, N]); rows: only the first `rows` rows of op(A)."""
    trit = c.cls == "exact"
    (ra, wa), (rb, wb) = dims(c)
    A = stream("a", trit, ra * wa).reshape(ra, wa)
    B = stream("b", trit, rb * wb).reshape(rb, wb)
    M = c.M
    if c.cls == "positive":
        A, B = np.abs(A), np.abs(B)
    elif c.cls == "range":
        s = np.exp2(4.0 * stream("g", False, M).astype(np.float64)).astype(np.float32)
        A = A * (s[None, :] if c.layout == TN else s[:, None])
    elif c.cls == "exact":
        s = np.exp2((np.arange(M) % 5) - 2.0).astype(np.float32)
        A = A * (s[None, :] if c.layout == TN else s[:, None])
    elif c.cls != "flat":
        raise KeyError(c.cls)
    if rows is not None:
        A = A[:, :rows] if c.layout == TN else A[:rows]
    return np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(B, dtype=np.float32)


def colsum_input(c):
    """X [M, N] float32 of a tt_colsum_f32 case."""
    X = stream("a", c.cls == "exact", c.M * c.N).reshape(c.M, c.N)
    if c.cls == "exact":
        X = X * np.exp2((np.arange(c.M) % 5) - 2.0).astype(np.float32)[:, None]
    elif c.cls == "positive":
        X = np.abs(X)
    return np.ascontiguousarray(X, dtype=np.float32)


def op_matrices(c, A, B):
    """(op(A) [M, K], op(B) [K, N]) torch views of the stored operands."""
    A, B = T(A), T(B)
    return (A.t() if c.layout == TN else A), (B.t() if c.layout == NT else B)


def band_of(K):
    return next(b for b in BANDS if K <= b)


def reduction(c):
    return c.M if c.entry == "colsum" else c.K


def band_name(b):
    return f"K <= {b}" if b < BANDS[-1] else f"K > {BANDS[-2]}"


def yard_of(c):
    return 0.0 if c.cls == "exact" else YARD[c.cls][band_of(reduction(c))]


_cache = collections.OrderedDict()


def _key(c):
    return (c.entry, c.layout, c.M, c.N, c.K, c.cls, c.H)


def shape_data(c):
    """Per (entry, layout, M, N, K, class): the stored operands, s64 = op(A) op(B), Abs = |op(A)| |op(B)| (None for the
    exact class) and the float32 BLAS product s32; shared by every epilogue / accumulate / stride variant of the shape.  The
    last six shapes are kept, the last two once a result has more than 2^22 elements."""
    k = _key(c)
    if k in _cache:
        _cache.move_to_end(k)
        return _cache[k]
    while len(_cache) >= (2 if c.M * c.N > (1 << 22) else 6):
        _cache.popitem(last=False)
    trit = c.cls == "exact"
    d = {}
    if c.entry == "colsum":
        X = colsum_input(c)
        x64 = T(X).double()
        d.update(A=X, s64=x64.sum(0)[None, :], Abs=None if trit else x64.abs().sum(0)[None, :], s32=T(X).sum(0)[None, :])
    else:
        A, B = operands(c)
        oa, ob = op_matrices(c, A, B)
        oa64, ob64 = oa.double(), ob.double()
        d.update(A=A, B=B, s64=oa64 @ ob64 if c.K else torch.zeros(c.M, c.N, dtype=torch.float64),
                 Abs=None if trit else (oa64.abs() @ ob64.abs() if c.K else torch.zeros(c.M, c.N, dtype=torch.float64)),
                 s32=oa @ ob if c.K else torch.zeros(c.M, c.N))
        if c.entry == "tncs":
            d.update(db64=oa64.sum(1), dbAbs=None if trit else oa64.abs().sum(1), db32=oa.sum(1))
    _cache[k] = d
    return d


def drop_cache():
    _cache.clear()


def side_inputs(c):
    """{"bias", "aux", "cold", "pool"} float32 torch tensors (or None) of the case."""
    trit = c.cls == "exact"
    M, N = c.M, c.N
    s = {"bias": None, "aux": None, "cold": None, "pool": None}
    if c.bias:
        s["bias"] = T(stream("bias", trit, N).copy())
    if c.epi == EPI_MASK:
        aux = stream("aux", trit, M * N).reshape(M, N).copy()
        for m, n, v in aux_plants(M, N):
            aux[m, n] = v
        s["aux"] = T(aux)
    if c.acc:
        s["cold"] = T(stream("cold", trit, M * N).reshape(M, N).copy())
    if c.entry == "pool":
        s["pool"] = T(stream("pool", trit, (M // c.H) * N).reshape(M // c.H, N).copy())
    return s


def pool_scale(c):
    return float(np.float32(1.0) / np.float32(c.H))


def reference(c, d=None, s=None):
    """{"ref", "E", "band" (bool, elements whose ReLU argument is within E of zero and not zero), "alt" (the other branch's
    result), and for tt_gemm_tn_colsum_f32 "db", "Edb"}; float64.  E is None for the exact class: equality."""
    d = shape_data(c) if d is None else d
    s = side_inputs(c) if s is None else s
    y = FACTOR * yard_of(c) * EPS
    exact = c.cls == "exact"
    pre = d["s64"].clone()
    Abs = None if exact else d["Abs"].clone()
    if s["bias"] is not None:
        pre += s["bias"].double()[None, :]
        if not exact:
            Abs += s["bias"].double().abs()[None, :]
    if c.entry == "pool":
        term = pool_scale(c) * s["pool"].double()[torch.arange(c.M) // c.H]
        pre += term
        if not exact:
            Abs += term.abs()
    band = torch.zeros_like(pre, dtype=torch.bool)
    alt = None
    if c.epi == EPI_RELU:
        val = pre.clamp(min=0.0)
        if not exact:
            band = (pre.abs() <= y * Abs + EPS * pre.abs()) & (pre != 0)
        alt = torch.where(pre > 0, torch.zeros_like(pre), pre)
    elif c.epi == EPI_MASK:
        val = torch.where(s["aux"] > 0, pre, torch.zeros_like(pre))
    else:
        val = pre
    ref = val
    if c.acc:
        ref = val + s["cold"].double()
        if alt is not None:
            alt = alt + s["cold"].double()
        if not exact:
            Abs += s["cold"].double().abs()
    r = {"ref": ref, "E": None if exact else y * Abs + EPS * ref.abs(), "band": band, "alt": alt}
    if c.entry == "tncs":
        r["db"] = d["db64"]
        r["Edb"] = None if exact else y * d["dbAbs"] + EPS * d["db64"].abs()
    return r


# ------------------------------------------------------------------ buffers
class Buffers:
    """The operands of a case as views into larger NaN-filled float32 buffers (CPU).  view(name) is the logical operand;
    C holds C_old with accumulate and NaN without.  view(name, buf) reads the same geometry out of another copy of the buffer
    (the one a call wrote, brought back from the device)."""

    def __init__(self, c, d, s):
        self.c, self.buf, self.geom = c, {}, {}
        if c.entry == "colsum":
            self._add("A", T(d["A"]), c.padA, c.offA)
            self._add("C", torch.full((1, c.N), float("nan")), 0, c.offC)
            return
        if c.entry == "pool":
            self._add("A", T(d["A"]), 0, 0)
            self._add("B", T(d["B"]), 0, 0)
            self._add("pool", s["pool"], c.padX, 0)
            self._add("C", torch.full((c.M, c.N), float("nan")), 0, 0)
            return
        self._add("A", T(d["A"]), c.padA, c.offA)
        self._add("B", T(d["B"]), c.padB, c.offB)
        self._add("C", s["cold"] if c.acc else torch.full((c.M, c.N), float("nan")), c.padC, c.offC)
        if s["bias"] is not None:
            self._add("bias", s["bias"][None, :], 0, 1 if c.bias == "mis" else 0)
        if s["aux"] is not None:
            self._add("aux", s["aux"], c.padX, c.offX)
        if c.entry == "tncs":
            self._add("db", torch.full((1, c.M), float("nan")), 0, 0)

    def _add(self, name, x, pad, off):
        rows, w = x.shape
        ld = w + pad
        guard = round_up(2 * ld, 4) + 64
        buf = torch.full((guard + off + rows * ld + guard,), float("nan"), dtype=torch.float32)
        self.buf[name], self.geom[name] = buf, (rows, w, ld, guard + off)
        self.view(name).copy_(x)

    def view(self, name, buf=None):
        rows, w, ld, start = self.geom[name]
        return torch.as_strided(self.buf[name] if buf is None else buf, (rows, w), (ld, 1), start)

    def ld(self, name):
        return self.geom[name][2]


def outside_unchanged(bufs, name, after):
    """Every element of buffer `name` outside its view has the bits it had (`after`: the whole buffer after the call)."""
    a, b = after.clone(), bufs.buf[name].clone()
    bufs.view(name, a).zero_()
    bufs.view(name, b).zero_()
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------ the checker
class Report:
    """worst = the largest err / E (exact class: 0 or inf); band = elements in the ReLU band; bad = elements outside E;
    nonfinite; clean = nothing outside the C view changed; db_worst likewise for the column sums."""

    def __init__(self):
        self.worst, self.band, self.bad, self.nonfinite, self.clean, self.db_worst = 0.0, 0, 0, 0, True, 0.0

    @property
    def ok(self):
        return self.bad == 0 and self.nonfinite == 0 and self.clean and self.db_worst <= 1.0

    def __repr__(self):
        return (f"Report(worst err/E {self.worst:.3g}, band {self.band}, outside E {self.bad}, non-finite {self.nonfinite}, "
                f"surroundings {'clean' if self.clean else 'CHANGED'}, colsum err/E {self.db_worst:.3g})")


def _ratio(err, E):
    if E is None:
        return torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf")))
    r = err / E
    return torch.where(err == 0, torch.zeros_like(err), torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r))


def check(c, ref, bufs, c_after, db_after=None):
    """The whole C buffer after a call (CPU float32) against the reference -> Report."""
    rep = Report()
    got = bufs.view("C", c_after)
    rep.nonfinite = int((~torch.isfinite(got)).sum())
    rep.clean = outside_unchanged(bufs, "C", c_after)
    if ref["E"] is None and c.entry != "tncs":  # the exact class: equality, in float32 (the reference is representable)
        rep.bad = int((~(got == ref["ref"].float())).sum())
        rep.worst = float("inf") if rep.bad else 0.0
        return rep
    got = got.double()
    want = ref["ref"]
    err = (got - want).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    ratio = _ratio(err, ref["E"])
    if ref["alt"] is not None and bool(ref["band"].any()):
        err2 = (got - ref["alt"]).abs()
        err2 = torch.where(torch.isnan(err2), torch.full_like(err2, float("inf")), err2)
        ratio = torch.where(ref["band"], torch.minimum(ratio, _ratio(err2, ref["E"])), ratio)
    rep.band = int(ref["band"].sum())
    rep.bad = int((ratio > 1.0).sum())
    rep.worst = float(ratio.max()) if ratio.numel() else 0.0
    if c.entry == "tncs":
        db = bufs.view("db", db_after).double()[0]
        e = (db - ref["db"]).abs()
        e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
        rep.db_worst = float(_ratio(e, ref["Edb"]).max())
        rep.clean = rep.clean and outside_unchanged(bufs, "db", db_after)
    return rep


# ------------------------------------------------------------------ float32 evaluations and the mutants
MUTANTS = ("last_k", "ragged_row", "tile_unwritten", "swap_cols", "bias_per_split", "bias_omitted", "acc_ignored",
           "cold_before_epi", "mask_from_value", "mask_ge0", "pass2_overwrites", "colsum_last_part", "pool_index")


def run_f32(c, d, s, bufs, mutant=None):
    """torch's float32 matmul plus the epilogue in float32, written through the C view of a copy of the buffers ->
    (C buffer, db buffer or None); with a mutant, that way of going wrong (None where the case gives it nothing to do)."""
    r = route(c)
    M, N, K = c.M, c.N, c.K
    f32 = torch.float32
    sm = d["s32"]
    bias = s["bias"]
    db = None
    if c.entry == "colsum":
        if mutant not in (None, "colsum_last_part", "last_k"):
            return None
        if mutant == "colsum_last_part":
            rpp = r["rows_per_part"]
            sm = T(d["A"])[:(r["parts"] - 1) * rpp].sum(0)[None, :] if r["parts"] > 1 else torch.zeros(1, N)
        if mutant == "last_k":
            sm = T(d["A"])[:M - 1].sum(0)[None, :] if M > 1 else torch.zeros(1, N)
        out = bufs.buf["C"].clone()
        bufs.view("C", out).copy_(sm)
        return out, None
    oa, ob = op_matrices(c, d["A"], d["B"])
    if mutant == "last_k":
        if K < 1:
            return None
        sm = sm - oa[:, K - 1:K] * ob[K - 1:K, :]
    if mutant == "pass2_overwrites":
        if r["path"] != "ws2":
            return None
        sm, bias = oa[:, WS_PASS_K:] @ ob[WS_PASS_K:, :], None
    if mutant == "bias_per_split":
        if bias is None or r.get("splits", 1) < 2:
            return None
        bias = bias * float(r["splits"])
    if mutant == "bias_omitted":
        if bias is None:
            return None
        bias = None
    pre = sm if bias is None else sm + bias[None, :]
    if c.entry == "pool":
        grp = c.H + 1 if mutant == "pool_index" else c.H
        pre = pre + s["pool"][torch.arange(M) // grp] * torch.tensor(pool_scale(c), dtype=f32)
    elif mutant == "pool_index":
        return None
    cold = s["cold"]
    if mutant == "cold_before_epi":
        if cold is None or c.epi == EPI_NONE:
            return None
        pre, cold = pre + cold, None
    if mutant == "acc_ignored":
        if cold is None:
            return None
        cold = None
    if mutant in ("mask_from_value", "mask_ge0") and c.epi != EPI_MASK:
        return None
    if c.epi == EPI_RELU:
        val = pre.clamp(min=0.0)
    elif c.epi == EPI_MASK:
        mask = pre > 0 if mutant == "mask_from_value" else s["aux"] >= 0 if mutant == "mask_ge0" else s["aux"] > 0
        val = torch.where(mask, pre, torch.zeros_like(pre))
    else:
        val = pre
    res = val if cold is None else val + cold
    if mutant == "swap_cols":
        if N < 5:
            return None
        perm = torch.arange(N)
        for n0 in range(0, N - 4, 32):
            perm[n0], perm[n0 + 4] = n0 + 4, n0
        res = res[:, perm]
    out = bufs.buf["C"].clone()
    view = bufs.view("C", out)
    keep = view.clone()
    view.copy_(res)
    if mutant == "ragged_row":
        unit = row_unit(c, r)
        if not unit or M % unit == 0:
            return None
        view[M - 1] = keep[M - 1]
    if mutant == "tile_unwritten":
        if M < 1:
            return None
        t = (ceil_div(M, BJ) - 1) // 2
        view[t * BJ:(t + 1) * BJ] = keep[t * BJ:(t + 1) * BJ]
    if c.entry == "tncs":
        dbv = d["db32"]
        if mutant == "colsum_last_part":
            dbv = oa[:, :max(K - BJ, 0)].sum(1)
        db = bufs.buf["db"].clone()
        bufs.view("db", db).copy_(dbv[None, :])
    elif mutant == "colsum_last_part":
        return None
    return out, db


def same_bits(a, b):
    return a is b or (a is not None and b is not None and torch.equal(a.view(torch.int32), b.view(torch.int32)))


def index_order_f32(oa, ob):
    """op(A) op(B) in float32, one rounding per multiply and per add, summed in index order (numpy ufuncs: no BLAS, no fma)."""
    an, bn = np.ascontiguousarray(oa.numpy().T), np.ascontiguousarray(ob.numpy())  # [K, M], [K, N]
    acc = np.zeros((an.shape[1], bn.shape[1]), dtype=np.float32)
    tmp = np.empty_like(acc)
    for k in range(an.shape[0]):
        np.multiply(an[k][:, None], bn[k][None, :], out=tmp)
        np.add(acc, tmp, out=acc)
    return T(acc)


def index_order_sum_f32(x):
    """Column sums of x [R, N] in float32, index order."""
    xn = x.numpy()
    acc = np.zeros(xn.shape[1], dtype=np.float32)
    for r in range(xn.shape[0]):
        np.add(acc, xn[r], out=acc)
    return T(acc)


def yard_shapes(cls, band):
    """One case per distinct (entry kind, layout, N, K) of the (class, band): the yardstick reads its leading block only."""
    best = {}
    for c in CASES:
        if c.cls != cls or band_of(reduction(c)) != band or min(c.M, c.N) == 0 or reduction(c) == 0:
            continue
        k = ("colsum", c.M, min(c.N, YARD_COLS)) if c.entry == "colsum" else (c.layout, min(c.N, YARD_COLS), c.K, c.entry == "tncs")
        if k not in best or best[k].M < c.M:
            best[k] = c
    return list(best.values())


def measure(cls, band):
    """(worst |s32 - s64| / (2^-24 Abs), case id) of the index-order float32 evaluation over yard_shapes."""
    worst = (0.0, None)
    for c in yard_shapes(cls, band):
        if c.entry == "colsum":
            x = T(np.ascontiguousarray(colsum_input(c)[:, :YARD_COLS]))
            r = float(((index_order_sum_f32(x).double() - x.double().sum(0)).abs() / (EPS * x.double().abs().sum(0))).max())
        else:
            A, B = operands(c, rows=YARD_ROWS)
            oa, ob = op_matrices(c, A, B)
            oa, ob = oa.contiguous(), ob[:, :YARD_COLS].contiguous()
            s64, Abs = oa.double() @ ob.double(), oa.double().abs() @ ob.double().abs()
            r = float(((index_order_f32(oa, ob).double() - s64).abs() / (EPS * Abs)).max())
            if c.entry == "tncs":  # the column sums of A: the same reduction, adds only
                x = oa.t().contiguous()
                r = max(r, float(((index_order_sum_f32(x).double() - x.double().sum(0)).abs() / (EPS * x.double().abs().sum(0))).max()))
        if r >= worst[0]:
            worst = (r, case_id(c))
    return worst


# ------------------------------------------------------------------ the GPU call (test_gpu_gemm_reference.py and its child)
class Launches:
    """with Launches() as n: ...  -> n[kernel] = launches the library counted inside the block, for every name of KERNELS
    (or of `kernels`: tower_ref.py counts its own family)."""

    def __init__(self, kernels=KERNELS):
        self.n, self.kernels = {}, tuple(kernels)

    def __enter__(self):
        from two_tower_models_amd import _native as N
        lib = N.load()
        lib.tt_profile_filter(",".join(self.kernels).encode())
        lib.tt_profile_enable(1)
        return self.n

    def __exit__(self, *exc):
        import ctypes as C
        from two_tower_models_amd import _native as N
        lib = N.load()
        torch.cuda.synchronize()
        try:
            for k in self.kernels:
                ms, cnt = C.c_double(0.0), C.c_int64(0)
                N.check(lib.tt_profile_read(k.encode(), C.byref(ms), C.byref(cnt)), "tt_profile_read")
                self.n[k] = cnt.value
        finally:
            lib.tt_profile_enable(0)
            lib.tt_profile_filter(None)
        return False


def run_gpu(c, bufs, dev="cuda:0", ws_short=0):
    """One call of the case's entry point at the C ABI with explicit pointers and leading dimensions ->
    {"rc", "C" (whole buffer, CPU), "db", "launches", "ws_bytes"}.  ws_short: bytes withheld from the workspace size."""
    from two_tower_models_amd import _native as N
    lib = N.load()
    g = {k: v.to(dev) for k, v in bufs.buf.items()}
    ptr = {}
    for k, v in g.items():
        assert v.data_ptr() % 16 == 0
        ptr[k] = v.data_ptr() + 4 * bufs.geom[k][3]
    with Launches() as n:
        if c.entry == "colsum":
            wsn = lib.tt_colsum_workspace_bytes(c.M, c.N)
            ws = torch.empty(max(wsn, 16), dtype=torch.uint8, device=dev)
            rc = lib.tt_colsum_f32(ptr["A"], c.M, c.N, bufs.ld("A"), ptr["C"], ws.data_ptr(), wsn - ws_short, N.stream())
        elif c.entry == "pool":
            wsn = 0
            rc = lib.tt_hist_dx_pool_bwd(ptr["A"], ptr["B"], c.M // c.H, c.H, c.N, ptr["pool"], bufs.ld("pool"), ptr["C"], N.stream())
        else:
            wsn = lib.tt_gemm_workspace_bytes(c.layout, c.M, c.N, c.K)
            ws = torch.empty(max(wsn, 16), dtype=torch.uint8, device=dev)
            if c.entry == "tncs":
                rc = lib.tt_gemm_tn_colsum_f32(c.M, c.N, c.K, ptr["A"], bufs.ld("A"), ptr["B"], bufs.ld("B"), ptr["C"], bufs.ld("C"),
                                               c.acc, ptr["db"], ws.data_ptr(), wsn - ws_short, N.stream())
            else:
                rc = lib.tt_gemm_f32(c.layout, c.M, c.N, c.K, ptr["A"], bufs.ld("A"), ptr["B"], bufs.ld("B"), ptr["C"], bufs.ld("C"),
                                     ptr.get("bias"), c.epi, ptr.get("aux"), bufs.ld("aux") if "aux" in ptr else 0, c.acc,
                                     ws.data_ptr(), wsn - ws_short, N.stream())
    torch.cuda.synchronize()
    return {"rc": rc, "C": g["C"].cpu(), "db": g["db"].cpu() if "db" in g else None, "launches": dict(n), "ws_bytes": wsn}


def gpu_case(c, dev="cuda:0"):
    """Everything test_gpu_gemm_reference.py asserts of one case, as a JSON-able dict (the child process returns these)."""
    d, s = shape_data(c), side_inputs(c)
    ref, r = reference(c, d, s), route(c)
    bufs = Buffers(c, d, s)
    res = {"id": case_id(c), "want_launches": r["launches"], "short_rc": None, "short_clean": None, "repeat_same": None}
    if c.entry in ("gemm", "tncs"):
        res["ws_want"] = workspace_bytes(c.layout, c.M, c.N, c.K, bool(c.env))
        if r.get("splits", 1) > 1 and r["ws_need"] == res["ws_want"]:  # one byte less: refused, nothing written
            short = run_gpu(c, bufs, dev, ws_short=1)
            res["short_rc"] = short["rc"]
            res["short_clean"] = same_bits(short["C"], bufs.buf["C"]) and sum(short["launches"].values()) == 0
    out = run_gpu(c, bufs, dev)
    rep = check(c, ref, bufs, out["C"], out["db"])
    if r["path"] == "tns" or r.get("splits", 1) > 1:  # deterministic: a second call gives the same bits
        again = run_gpu(c, bufs, dev)
        res["repeat_same"] = same_bits(again["C"], out["C"]) and same_bits(again["db"], out["db"])
    res.update(rc=out["rc"], launches=out["launches"], ws_bytes=out["ws_bytes"], worst=rep.worst, band=rep.band, bad=rep.bad,
               nonfinite=rep.nonfinite, clean=rep.clean, db_worst=rep.db_worst, ok=rep.ok, path=r["path"])
    return res


def gpu_line(res):
    ran = {k: v for k, v in res["launches"].items() if v}
    return (f"gemm-ref {res['id']} err/E {res['worst']:.3f} colsum err/E {res['db_worst']:.3f} band {res['band']} "
            f"path {res['path']} launches {ran}")


def assert_gpu_case(c, res):
    assert res["rc"] == 0, res
    assert res["launches"] == res["want_launches"], (res["launches"], res["want_launches"])
    if "ws_want" in res:
        assert res["ws_bytes"] == res["ws_want"], (res["ws_bytes"], res["ws_want"])
    if res["short_rc"] is not None:
        assert res["short_rc"] == E_WORKSPACE and res["short_clean"], res
    assert res["repeat_same"] in (None, True), res
    assert res["ok"], res


# ------------------------------------------------------------------ the cases
EPIS = (("yes", EPI_NONE, 0), ("yes", EPI_RELU, 0), ("yes", EPI_MASK, 0), (None, EPI_NONE, 1), ("yes", EPI_RELU, 1),
        ("yes", EPI_MASK, 1))
L3 = (NT, NN, TN)


def _generic64():
    cs = []
    for L in L3:
        for cls in ("flat", "exact"):
            # ragged, scalar loads because ld % 4 != 0 / because the base pointer is one float off; and the FULL form
            cs.append(_c("g64", "gemm", L, 200, 96, 41, "t64", cls, padA=1, padB=1, bias="yes", a_vec=False, b_vec=False))
            cs.append(_c("g64", "gemm", L, 128, 64, 64, "t64", cls, offA=1, offB=1, bias="yes", a_vec=False, b_vec=False))
            cs.append(_c("g64", "gemm", L, 128, 64, 64, "t64f", cls, bias="yes"))
            for K in (1, 31, 32, 33):
                cs.append(_c("g64", "gemm", L, 70, 50, K, "t64", cls, bias="yes"))
            cs.append(_c("g64", "gemm", L, 70, 50, 0, "t64", cls, bias="yes"))
            cs.append(_c("g64", "gemm", L, 70, 50, 0, "t64", cls))
            cs.append(_c("g64", "gemm", L, 1, 50, 41, "t64", cls, bias="yes"))
            cs.append(_c("g64", "gemm", L, 70, 1, 41, "t64", cls, bias="yes"))
        for cls in ("positive", "range"):
            cs.append(_c("g64", "gemm", L, 200, 96, 41, "t64", cls, padA=1, padB=1, bias="yes"))
        # 16-byte aligned rows whose width is no multiple of 4: vector loads up to a scalar tail
        wa, wb = (41, 41) if L == NT else (41, 98) if L == NN else (202, 98)
        for cls in ("flat", "exact"):
            cs.append(_c("g64", "gemm", L, 202, 98, 41, "t64", cls, padA=-wa % 4, padB=-wb % 4, bias="yes", a_vec=True, b_vec=True))
    for L in (NT, NN):
        for bias, epi, acc in EPIS[1:]:  # strided, misaligned C and aux
            cs.append(_c("g64", "gemm", L, 200, 96, 41, "t64", "flat", padC=1, offC=1, padX=3, offX=2, bias=bias, epi=epi, acc=acc))
            cs.append(_c("g64", "gemm", L, 200, 96, 41, "t64", "exact", padC=1, offC=1, padX=3, offX=2, bias=bias, epi=epi, acc=acc))
    cs.append(_c("g64", "gemm", NT, 0, 50, 41, "none"))
    cs.append(_c("g64", "gemm", NT, 70, 0, 41, "none"))
    return cs


def _generic128():
    cs = []
    for L in (NT, NN):  # >= 192 tiles of 128^2
        cs.append(_c("g128", "gemm", L, 2048, 1536, 64, "t128f", "flat", bias="yes"))
        cs.append(_c("g128", "gemm", L, 2048, 1536, 64, "t128f", "exact", bias="yes", epi=EPI_RELU))
        cs.append(_c("g128", "gemm", L, 2053, 1539, 41, "t128", "flat", padA=1, offA=1, padB=1, offB=1, padC=1, offC=1, bias="yes",
                     a_vec=False, b_vec=False))
        cs.append(_c("g128", "gemm", L, 2053, 1539, 41, "t128", "flat", padA=3, padB=3 if L == NT else 1, bias="yes", a_vec=True, b_vec=True))
        cs.append(_c("g128", "gemm", L, 2053, 1539, 41, "t128", "exact", padA=1, offA=1, padB=1, offB=1, padC=1, offC=1, bias="yes",
                     epi=EPI_MASK, acc=1, a_vec=False, b_vec=False))
    return cs


def _splitk():
    cs = []
    for L in L3:  # 128^2 through K >= 8192: 64 whole splits at 8192, 52 at 8195 with a last split of 35
        for cls in ("flat", "exact"):
            cs.append(_c("sk128", "gemm", L, 256, 128, 8192, "t128f+sk", cls, splits=64))
            cs.append(_c("sk128", "gemm", L, 256, 128, 8195, "t128+sk", cls, splits=52, last_split=35))
        cs.append(_c("sk128", "gemm", L, 256, 128, 8195, "t128+sk", "positive", splits=52))
        cs.append(_c("sk128", "gemm", L, 256, 128, 8195, "t128+sk", "range", splits=52))
    for cls in ("flat", "exact"):
        for K, path in ((8192, "t128f+sk"), (8195, "t128+sk")):
            cs.append(_c("sk128", "tncs", TN, 256, 128, K, path, cls))
            cs.append(_c("sk128", "tncs", TN, 256, 128, K, path, cls, acc=1))
    for L in (NT, NN):
        for bias, epi, acc in EPIS:
            for cls in ("flat", "exact"):
                cs.append(_c("sk128", "gemm", L, 256, 128, 8195, "t128+sk", cls, bias=bias, epi=epi, acc=acc, splits=52))
                # 64^2: 4 tiles, 32 K-tiles: splits at the cap ktiles / 4 = 8, the last one 104 long
                cs.append(_c("sk64", "gemm", L, 100, 70, 1000, "t64+sk", cls, bias=bias, epi=epi, acc=acc, splits=8, last_split=104))
        # one tile, 1024 K-tiles: splits at the cap 256
        cs.append(_c("sk64", "gemm", L, 60, 50, 32768, "t64+sk", "flat", bias="yes", splits=256))
        cs.append(_c("sk64", "gemm", L, 60, 50, 32768, "t64+sk", "exact", bias="yes", epi=EPI_RELU, acc=1, splits=256))
    cs.append(_c("sk64", "tncs", TN, 100, 70, 1000, "t64+sk", "flat", splits=8))
    cs.append(_c("sk64", "tncs", TN, 100, 70, 1000, "t64+sk", "exact", acc=1, splits=8))
    cs.append(_c("sk64", "tncs", TN, 100, 70, 300, "t64", "flat"))
    return cs


M_WS = WS_MIN_M + 5  # 257 tiles of 64 rows, the last one 5 rows: its second 32-row sub-tile is empty


def _ws():
    cs = []
    for L in (NT, NN):
        # launch variants: dp8 = 4 / 8 / 16 / 32 with LDS-DMA and with register staging, in each store mode
        forms = [(32, 4, True, 0), (64, 8, True, 0), (128, 16, True, 0), (256, 32, True, 0),
                 (31, 4, False, 0), (50, 8, False, 0), (100, 16, False, 0), (200, 32, False, 0), (128, 16, False, 1)]
        for i, (K, dp8, dma, offA) in enumerate(forms):
            cls = "exact" if (i + L) % 2 else "flat"
            cs.append(_c("ws", "gemm", L, M_WS, 96, K, "ws", cls, offA=offA, bias="yes", dp8=dp8, dma=dma, mode="PLAIN"))
            cs.append(_c("ws", "gemm", L, M_WS, 96, K, "ws", cls, offA=offA, acc=1, dp8=dp8, dma=dma, mode="ACC"))
            cs.append(_c("ws", "gemm", L, M_WS, 100, K, "ws", cls, offA=offA, bias="yes", epi=EPI_RELU, dp8=dp8, dma=dma, mode="GENERIC"))
        # aligned rows of 50: vector loads up to a scalar tail, for the streamed rows and (NT) the stationary ones
        cs.append(_c("ws", "gemm", L, M_WS, 96, 50, "ws", "flat", padA=2, padB=2 if L == NT else 4, bias="yes", dp8=8, dma=False, mode="PLAIN"))
        cs.append(_c("ws", "gemm", L, M_WS, 96, 50, "ws", "exact", padA=2, padB=2 if L == NT else 4, acc=1, dp8=8, dma=False, mode="ACC"))
        # WS_GENERIC: ragged columns, a misaligned C, a misaligned aux, every epilogue with and without accumulate
        cs.append(_c("ws", "gemm", L, M_WS, 100, 64, "ws", "flat", bias="yes", mode="GENERIC"))
        cs.append(_c("ws", "gemm", L, M_WS, 96, 64, "ws", "flat", offC=1, bias="yes", mode="GENERIC"))
        cs.append(_c("ws", "gemm", L, M_WS, 96, 64, "ws", "exact", padC=1, acc=1, mode="GENERIC"))
        cs.append(_c("ws", "gemm", L, M_WS, 96, 64, "ws", "flat", offX=1, bias="yes", epi=EPI_MASK, mode="GENERIC"))
        for bias, epi, acc in EPIS[1:]:
            if epi != EPI_NONE:
                cs.append(_c("ws", "gemm", L, M_WS, 96, 64, "ws", "flat", bias=bias, epi=epi, acc=acc, mode="GENERIC"))
                cs.append(_c("ws", "gemm", L, M_WS, 100, 44, "ws", "exact", bias=bias, epi=epi, acc=acc, mode="GENERIC"))
        cs.append(_c("ws", "gemm", L, M_WS, 96, 128, "ws", "positive", bias="yes", mode="PLAIN"))
        cs.append(_c("ws", "gemm", L, M_WS, 96, 128, "ws", "range", bias="yes", mode="PLAIN"))
        # the tile loop: 1-2, 2-3, 3-4 and 5-6 tiles per workgroup; last tile of 5 rows and of 37
        for M in (M_WS, WS_MIN_M + 64 + 37):
            cs.append(_c("wsloop", "gemm", L, M, 384, 32, "ws", "flat", bias="yes", tiles=(1, 2), dma=True, mode="PLAIN"))
            cs.append(_c("wsloop", "gemm", L, M, 640, 32, "ws", "exact", bias="yes", tiles=(2, 3), dma=True, mode="PLAIN"))
            cs.append(_c("wsloop", "gemm", L, M, 384, 31, "ws", "flat", bias="yes", tiles=(3, 4), dma=False, mode="PLAIN"))
            cs.append(_c("wsloop", "gemm", L, M, 640, 31, "ws", "exact", bias="yes", tiles=(5, 6), dma=False, mode="PLAIN"))
        cs.append(_c("wsloop", "gemm", L, M_WS, 640, 32, "ws", "exact", acc=1, tiles=(2, 3), dma=True, mode="ACC"))
        cs.append(_c("wsloop", "gemm", L, M_WS, 384, 31, "ws", "flat", bias="yes", epi=EPI_MASK, acc=1, tiles=(3, 4), mode="GENERIC"))
        # K in (256, 512]: two passes, the second one accumulating (WS_ACC when nothing else is asked of it)
        for K, dma2 in ((384, True), (300, False), (257, False)):
            cls = "exact" if K == 300 else "flat"
            cs.append(_c("ws2", "gemm", L, M_WS, 96, K, "ws2", cls, bias="yes", mode2="ACC", dma2=dma2))
            cs.append(_c("ws2", "gemm", L, M_WS, 96, K, "ws2", cls, bias="yes", epi=EPI_RELU, mode2="GENERIC", dma2=dma2))
            cs.append(_c("ws2", "gemm", L, M_WS, 96, K, "ws2", cls, bias="yes", epi=EPI_MASK, mode2="GENERIC", dma2=dma2))
            cs.append(_c("ws2", "gemm", L, M_WS, 96, K, "ws2", cls, acc=1, mode1="ACC", mode2="ACC", dma2=dma2))
        # back to the generic kernel: K > 512; the aligned bypass; accumulate plus an epilogue at K > 256
        cs.append(_c("wsfall", "gemm", L, M_WS, 96, 513, "t64", "flat", bias="yes"))
        cs.append(_c("wsfall", "gemm", L, WS_MIN_M, 128, 320, "t64f", "exact", bias="yes"))
        cs.append(_c("wsfall", "gemm", L, M_WS, 96, 300, "t64", "flat", bias="yes", epi=EPI_RELU, acc=1))
        cs.append(_c("wsfall", "gemm", L, M_WS, 96, 300, "t64", "exact", bias="yes", epi=EPI_MASK, acc=1))
    return cs


WS16_CFGS = ((1, 1), (2, 1), (3, 1), (1, 2), (1, 3))


def _ws16():
    cs = []
    for L in (NT, NN):
        for kb, nb in WS16_CFGS:
            rows, K, N = ws16_rows(kb, nb), 128 * kb, 128 * nb
            # one stage per workgroup; exactly three; a wrapped ring (4 - 5 stages) with a ragged last stage of 5 rows
            cs.append(_c("ws16", "gemm", L, WS_MIN_M, N, K, "ws16", "flat", bias="yes", cfg=(kb, nb),
                         stages={96: (1, 1), 64: (1, 1), 48: (1, 2), 32: (2, 2)}[rows]))
            cs.append(_c("ws16", "gemm", L, 3 * 256 * rows, N, K, "ws16", "exact", bias="yes", cfg=(kb, nb), stages=(3, 3)))
            cs.append(_c("ws16", "gemm", L, 4 * 256 * rows + rows + 5, N, K, "ws16", "flat" if (L == NT and kb == 3) else "exact", bias="yes",
                         cfg=(kb, nb), stages=(4, 5), last_rows=5))
        cs.append(_c("ws16", "gemm", L, WS_MIN_M, 128, 128, "ws16", "positive", cfg=(1, 1)))
        cs.append(_c("ws16", "gemm", L, WS_MIN_M, 128, 128, "ws16", "range", cfg=(1, 1)))
        # what sends the call on to gemm_ws: a misaligned bias, ld % 4 != 0, accumulate
        for K, path in ((128, "ws"), (384, "ws2")):
            cs.append(_c("ws16fall", "gemm", L, M_WS, 128, K, path, "flat", bias="mis"))
            cs.append(_c("ws16fall", "gemm", L, M_WS, 128, K, path, "exact", padA=1, bias="yes"))
            cs.append(_c("ws16fall", "gemm", L, M_WS, 128, K, path, "exact", acc=1))
    return cs


def _pool():
    cs = []
    for cls in ("flat", "exact"):  # (exact: 1 / H must be a power of two)
        cs.append(_c("pool", "pool", NN, 16384, 128, 384, "pool", cls, H=1, padX=0, stages=(2, 2)))
        cs.append(_c("pool", "pool", NN, 512 * 32, 128, 384, "pool", cls, H=32, padX=4, stages=(2, 2)))
        cs.append(_c("pool", "pool", NN, 1026 * 32 - 32, 128, 384, "pool", cls, H=32, padX=0, stages=(4, 5)))
    cs.append(_c("pool", "pool", NN, 565 * 29, 128, 384, "pool", "flat", H=29, padX=4, last_rows=1))  # a group straddles a stage
    cs.append(_c("pool", "pool", NN, 1132 * 29, 128, 384, "pool", "flat", H=29, padX=0, stages=(4, 5), last_rows=28))  # wrapped, ragged
    return cs


def _tns():
    cs = []
    # M = 384: the streaming kernel in every process.  24 rows per stage: > 768 stages give a workgroup four
    for K, st in ((8192, (1, 2)), (8193, (1, 2)), (24576 + 24 + 5, (4, 5))):
        for cls in ("flat", "exact"):
            cs.append(_c("tns", "gemm", TN, 384, 128, K, "tns", cls, stages=st))
            cs.append(_c("tns", "tncs", TN, 384, 128, K, "tns", cls, acc=1, stages=st))
        cs.append(_c("tns", "gemm", TN, 384, 128, K, "tns", "exact", acc=1, padA=0, padB=0, stages=st))
        cs.append(_c("tns", "tncs", TN, 384, 128, K, "tns", "flat", padA=0, padB=0, stages=st))
    cs.append(_c("tns", "tncs", TN, 384, 128, 8195, "tns", "positive"))
    cs.append(_c("tns", "tncs", TN, 384, 128, 8195, "tns", "range"))
    # a misaligned pointer and K = 8191 fall to the tiled kernel
    cs.append(_c("tnsfall", "tncs", TN, 384, 128, 8192, "t128+sk", "flat", offA=1))
    cs.append(_c("tnsfall", "gemm", TN, 384, 128, 8192, "t128+sk", "exact", offB=1, acc=1))
    cs.append(_c("tnsfall", "tncs", TN, 384, 128, 8191, "t64+sk", "flat", splits=20))
    # M = 256 (32 rows per stage) and 128 (16 rows, 768 workgroups): streaming only under TT_GEMM_TN_STREAM_ALL, in a child
    # process; the same shapes in the default process take the tiled kernel
    for M, Ks in ((256, (8192, 8193, 32768 + 32 + 5)), (128, (8192, 8193, 49152 + 16 + 5))):
        for K in Ks:
            st = (4, 5) if K > 8193 else None
            tiled = ("t128" if M == 256 else "t64") + ("f" if K % 32 == 0 else "") + "+sk"
            for env, path in ((STREAM_ALL, "tns"), ("", tiled)):
                kw = {"stages": st} if (st and env) else {}
                cs.append(_c("tnsall", "gemm", TN, M, 128, K, path, "flat", env=env, **kw))
                cs.append(_c("tnsall", "tncs", TN, M, 128, K, path, "exact", acc=1, env=env, **kw))
            cs.append(_c("tnsall", "tncs", TN, M, 128, K, "tns", "flat", env=STREAM_ALL, padA=0, padB=0))
            cs.append(_c("tnsall", "gemm", TN, M, 128, K, "tns", "exact", acc=1, env=STREAM_ALL))
        cs.append(_c("tnsall", "tncs", TN, M, 128, 8192, tiled_for(M, 8192), "flat", env=STREAM_ALL, offA=1))
        cs.append(_c("tnsall", "tncs", TN, M, 128, 8191, "t64+sk", "flat", env=STREAM_ALL))  # (K < 8192: the 64^2 tile)
    return cs


def tiled_for(M, K):
    """The tiled path of a TN product the streaming kernel refuses (a misaligned operand or K < 8192: never the FULL form)."""
    return ("t128" if M == 256 else "t64") + "+sk"


def _colsum():
    cs = []
    for cls in ("flat", "exact"):
        for M in (1, 63, 64, 65):
            cs.append(_c("colsum", "colsum", NT, M, 65, 0, "colsum", cls))
        for N in (1, 63):
            cs.append(_c("colsum", "colsum", NT, 65, N, 0, "colsum", cls, padA=0))
        # more than 512 parts of 64 rows: rows_per_part doubles
        cs.append(_c("colsum", "colsum", NT, 512 * 64 + 65, 65, 0, "colsum", cls, padA=3, offA=1, rows_per_part=128))
    cs.append(_c("colsum", "colsum", NT, 5000, 130, 0, "colsum", "positive"))
    return cs


CASES = []
CASES += _generic64() + _generic128() + _splitk() + _ws() + _ws16() + _pool() + _tns() + _colsum()
_DUP = [k for k, v in collections.Counter(case_id(c) for c in CASES).items() if v > 1]
assert not _DUP, ("case ids must be distinct", _DUP)
DEFAULT_CASES = [c for c in CASES if not c.env]
CHILD_CASES = [c for c in CASES if c.env]

# every path the suite must reach, by the name check_paths_named() looks for in the routes of the cases
PATHS = ("t64", "t64f", "t128", "t128f", "t64+sk", "t64f+sk", "t128+sk", "t128f+sk", "ws", "ws2", "ws16", "pool", "tns", "colsum", "none")


def main():
    print("float32 index-order evaluation against float64: worst |s32 - s64| / (2^-24 Abs) per class and K band")
    print(f"{'class':<9} {'band':<10} {'shapes':>6} {'measured':>9} {'YARD':>7}   worst case")
    ok = True
    for cls in YARD:
        for band in YARD[cls]:
            w = measure(cls, band)
            print(f"{cls:<9} {band_name(band):<10} {len(yard_shapes(cls, band)):>6} {w[0]:9.3f} {YARD[cls][band]:7.2f}   {w[1]}")
            ok = ok and w[0] <= YARD[cls][band] <= 1.1 * w[0]
    print("\nReLU band: elements whose ReLU argument is within E of zero (either branch accepted), worst share per group")
    worst = {}
    for c in CASES:
        if c.epi == EPI_RELU:
            ref = reference(c)
            share = float(ref["band"].double().mean()) if ref["band"].numel() else 0.0
            worst[c.group] = max(worst.get(c.group, 0.0), share)
            ok = ok and share <= BAND_SHARE
    for g, sh in worst.items():
        print(f"{g:<9} {100 * sh:8.4f} %")
    print(f"\n{len(CASES)} cases, {len(CHILD_CASES)} of them in the {STREAM_ALL} child process")
    assert ok, "YARD is below the measured worst case or more than 10 % above it, or a case misses the band condition"


if __name__ == "__main__":
    main()
