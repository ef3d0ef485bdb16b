"""Float64 yardstick for the in-batch softmax cross entropy (csrc/inbatch_ce.hip, ce_wide.hip and the staging code of
mfma_stream.hpp).  A helper, not a test: imported by test_ce_reference_cpu.py and test_gpu_ce_reference.py the way
attention_ref.py and mips_ref.py are imported by theirs; the product never imports it.

  evaluate    the formulas, in the dtype of the input:
                S = U I^T (+ b[None, :]),  lse_i = logsumexp_j S_ij,  ce_i = lse_i - S[i, i + off],  P = softmax(S),
                du_unit = P I - I[i + off],  dU = coef (.) du_unit,  dI = ((P - onehot) (.) coef)^T U,
                logits = S log2 e (what the kept-logits forward writes).
              float64: matmul.  float32: one rounding per multiply and per add, summed in index order, exp and log
              correctly rounded (float64's, rounded) -- no BLAS, no host math library in float32: the same bits on every
              IEEE machine.  `mut` names a deliberately wrong formula (MUTANTS).
  reference   float64 forward + torch autograd (ref:src/two_tower_base_retrieval.py:287 the logits, :301-312 the row-wise
              cross entropy against the diagonal, :322 and :334-343 the weighted mean; the per-item term is the log-Q
              correction :289-295 names as missing), written from those lines; the float32 oracle is not called.
  inputs      four classes from fixture_gen.gaussianish.  Each operand is scaled by (128 / D)^(1/4), i.e. the LOGITS by
              sqrt(128 / D), so their statistics do not depend on D:
                flat     scale 0.5: logits of s.d. ~2.8 (the older tests' inputs)
                peaked   scale 5: logits of s.d. ~280, rows near one-hot.  (Scale 3, logits of s.d. ~100, leaves 78 - 89 %
                         of the rows of these shapes with a largest probability above 0.99 -- the gap between a row's two
                         largest of 200 - 1000 logits is ~sd / 3.7 on average -- and scale 4 still misses one case; the
                         class's condition, 90 %, is what was kept.)
                shifted  flat with the component along v = ones / sqrt(D) removed, plus +-c v on U (+ even user rows,
                         - odd ones) and c v on I, c^2 = 80: every logit of an even row sits near +80, of an odd row near
                         -80.  Without the max subtraction fp32 exp overflows in the first and the row sum underflows in
                         the second; the online rescale and the split merge carry the whole result.
                planted  flat; for every fourth user row I[i + off] = 4 U[i] / |U[i]|^2 * 20 (the positive's logit is 80:
                         it holds all the mass, du_unit = E - I[pos] cancels), for every fourth-plus-one row the negated
                         vector (logit -80: it holds none).
              coef = g / M with both signs, every 16th exactly 0.  bias: None, the Zipf -log q term, the signed +-30 term.
  layout      how an operand sits in a larger buffer: dense (ld = D), strided16 (ld = D + 8, 16-B aligned: still LDS-DMA
              eligible at D = 32 / 64 / 128), pad4 (ld = the next multiple of 4 above D, aligned: D = 50 in 52, 98 in
              100 -- vector loads with a scalar tail), odd_ld (ld = D + 3) and misaligned (ld = D + 4, base one float
              off): no vector loads, register staging.  Slack of an input is NaN, of an output the sentinel 7.0.
  plan        plan_ce, can_dma, wide_chunk_rows and the workspace formulas restated in Python.
  CASES       what test_gpu_ce_reference.py runs; coverage() lists the cells of the issue's matrix a case list reaches.

Tolerances.  |got - ref| <= a + m * max|ref| + r * |ref| element-wise.
  flat keeps the project's figures (tests/test_gpu_kernels.py, test_gpu_logq.py), now against float64: ce a = 2e-5,
  r = 1e-5; du_unit, dU, dI m = 1e-5, r = 1e-4; kept logits m = 1e-5.
  Everything else (lse of every class; every quantity of peaked, shifted, planted): a = 0, the same r (0 for lse and the
  logits) and m = 4 x YARD[class][quantity], where YARD is the worst max((|fp32 - f64| - r |f64|)+) / max|f64| of the
  float32 evaluation above over the class's cases -- measured by `python tests/ce_ref.py`, rounded up to two digits, never
  below 2^-24, re-measured by test_ce_reference_cpu.py.  The factor 4 is the project's (Adam, attention, MIPS): the
  hardware's 1-ulp exp2 / log2 and a matrix-core summation order.  profiles/ce_reference_tolerance.txt records the table
  and what the GPU showed."""
import collections
import functools
import math
import os
import sys

import numpy as np
import torch

try:
    import fixture_gen as fg
except ImportError:  # run as a script: pytest's conftest.py is what puts tests/golden on the path
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import fixture_gen as fg

F64 = torch.float64
F32 = torch.float32
SENTINEL = 7.0
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
CLASSES = ("flat", "peaked", "shifted", "planted")
BIASES = ("none", "zipf", "pm30")
QUANTITIES = ("ce", "lse", "logits", "du_unit", "dU", "dI")
RTOL = {"ce": 1e-5, "lse": 0.0, "logits": 0.0, "du_unit": 1e-4, "dU": 1e-4, "dI": 1e-4}
FLAT_TOL = {"ce": (2e-5, 0.0, 1e-5), "logits": (0.0, 1e-5, 0.0), "du_unit": (0.0, 1e-5, 1e-4), "dU": (0.0, 1e-5, 1e-4),
            "dI": (0.0, 1e-5, 1e-4)}
FLOOR = 2.0 ** -24
FACTOR = 4.0
PEAKED_SCALE = 5.0

# worst normalised error of the float32 CPU evaluation against float64 per class over CASES: see main()
YARD = {
    "flat": {"ce": 6.0e-08, "lse": 3.2e-07, "logits": 4.5e-07, "du_unit": 6.0e-07, "dU": 3.5e-07, "dI": 2.3e-07},
    "peaked": {"ce": 6.0e-08, "lse": 4.6e-07, "logits": 5.2e-07, "du_unit": 8.1e-05, "dU": 2.9e-05, "dI": 2.1e-05},
    "shifted": {"ce": 3.3e-07, "lse": 3.8e-07, "logits": 6.7e-07, "du_unit": 5.3e-06, "dU": 5.0e-06, "dI": 3.0e-06},
    "planted": {"ce": 6.0e-08, "lse": 4.9e-07, "logits": 6.0e-07, "du_unit": 1.6e-06, "dU": 4.7e-07, "dI": 5.5e-07},
}


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


# ------------------------------------------------------------------ bias terms (shared with test_gpu_logq.py)
def zipf_bias(n, seed=71):
    """-log q of a Zipf(1.0) popularity over 10^6 items at n seeded ids."""
    ids = torch.from_numpy(fg.uniform_ids((n,), 10 ** 6, seed).astype(np.int64))
    harmonic = float(np.sum(1.0 / np.arange(1, 10 ** 6 + 1, dtype=np.float64)))
    return (torch.log(ids.double() + 1.0) + math.log(harmonic)).float()


def signed_bias(n, seed=72):
    b = torch.from_numpy(fg.gaussianish((n,), seed))
    return b * (30.0 / float(b.abs().max()))


# ------------------------------------------------------------------ layouts
LAYOUTS = ("dense", "strided16", "pad4", "odd_ld", "misaligned")


def layout(name, D):
    """(ld, offset of the first element in floats) of an operand of width D inside its buffer (the buffer itself is
    16-byte aligned)."""
    return {"dense": (D, 0), "strided16": (D + 8, 0), "pad4": ((D // 4 + 1) * 4, 0), "odd_ld": (D + 3, 0),
            "misaligned": (D + 4, 1)}[name]


def place(x, name, fill, device="cpu"):
    """-> (buffer, view): a 1-D float32 buffer filled with `fill` and the [rows, D] view of layout `name` inside it,
    holding x (a tensor, or a (rows, D) shape for an output: the view keeps the fill)."""
    rows, D = x if isinstance(x, tuple) else x.shape
    ld, off = layout(name, D)
    buf = torch.full((off + rows * ld,), fill, dtype=F32, device=device)
    view = torch.as_strided(buf, (rows, D), (ld, 1), off)
    if not isinstance(x, tuple):
        view.copy_(x)
    return buf, view


def slack_intact(buf, view, fill=SENTINEL):
    """Every element of the buffer outside the view still holds the fill."""
    mask = torch.ones_like(buf, dtype=torch.bool)
    torch.as_strided(mask, view.shape, view.stride(), view.storage_offset()).fill_(False)
    return bool((buf[mask] == fill).all())


# ------------------------------------------------------------------ the dispatch plan, restated
def _ceil_div(a, b):
    return -(-a // b)


def _round_up(a, b):
    return _ceil_div(a, b) * b


def plan_ce(RX, RY, D):
    """plan_ce (csrc/inbatch_ce.hip): (dp8, splits, tiles_per_split) for RX stationary and RY streamed rows."""
    dp8 = 4 if D <= 32 else 8 if D <= 64 else 16 if D <= 128 else None
    if dp8 is None:
        return None
    rowblocks, tiles = _ceil_div(RX, 128), _ceil_div(RY, 64)
    splits = _ceil_div(512, rowblocks)
    while rowblocks * splits < 1024 and tiles >= 32 * splits:
        splits *= 2
    splits = max(1, min(splits, _ceil_div(tiles, 4), 64))
    tps = _ceil_div(tiles, splits)
    return dp8, _ceil_div(tiles, tps), tps


def wide_chunk_rows(M, N):
    """wide_chunk_rows (csrc/ce_wide.hip)."""
    mc = max((512 << 20) // (N * 4) // 128 * 128, 128)
    return min(mc, M)


def plan(M, N, D, lay_u="dense", lay_i="dense", lay_du="dense", lay_di="dense", gemm_ws=None):
    """A pure-Python statement of the host code that picks the kernels of a call: plan_ce, can_dma, the x_vec / y_vec
    flags of fwd_impl / fwd_du_impl / bwd_impl, launch_slab_reduce's choice, tt_inbatch_ce_workspace_bytes,
    tt_inbatch_ce_bias_workspace_bytes, tt_inbatch_ce_logits_bytes (csrc/inbatch_ce.hip) and wide_chunk_rows,
    ce_wide_workspace_bytes, the chunk loop of ce_wide_run (csrc/ce_wide.hip).  For D > 128 the workspace needs the
    library GEMM's own query, `gemm_ws(kind, m, n, k)` with kind in "NT", "NN", "TN"; without it "ws" is None.
    Returns dp8 (None: the wide path); user / item: (splits, tiles_per_split, tiles of every split) of the user side
    (users stationary, items streamed: forward, forward + dU, dU) and the item side (dI); stage_fwd = stage_du: how the
    item rows are staged; stage_di: how the user rows are staged; vec_u / vec_i; reduce_du / reduce_di: which slab
    reduce runs (None: one split, the product kernel writes the output itself); chunks: the row chunks of the wide path;
    ws / ws_bias / logits_bytes."""
    (ldu, offu), (ldi, offi) = layout(lay_u, D), layout(lay_i, D)
    vec_u, vec_i = ldu % 4 == 0 and offu % 4 == 0, ldi % 4 == 0 and offi % 4 == 0
    out = dict(vec_u=vec_u, vec_i=vec_i, logits_bytes=_round_up(M, 128) * _round_up(N, 128) * 4)
    if D > 128:
        mc = wide_chunk_rows(M, N)
        chunks = [min(mc, M - r0) for r0 in range(0, M, mc)]
        ws = None
        if gemm_ws is not None:
            g = 0
            for rows in (mc, M % mc):
                if rows > 0:
                    g = max(g, gemm_ws("NT", rows, N, D), gemm_ws("NN", rows, D, N), gemm_ws("TN", N, D, rows))
            ws = _round_up(mc * N * 4, 256) + _round_up(g, 256)
        out.update(dp8=None, user=None, item=None, stage_fwd="gemm", stage_du="gemm", stage_di="gemm", reduce_du=None,
                   reduce_di=None, chunks=chunks, ws=ws, ws_bias=None if ws is None else ws + _round_up(N * 4, 256))
        return out
    dp8, su, tu = plan_ce(M, N, D)
    _, si, ti = plan_ce(N, M, D)

    def split_tiles(rows, s, t):
        tiles = _ceil_div(rows, 64)
        return [min(t, tiles - z * t) for z in range(s)]

    def can_dma(ld, off):
        return D == dp8 * 8 and ld % 4 == 0 and ld <= (1 << 22) and off % 4 == 0

    def reduce_of(splits, lay_out):
        if splits == 1:
            return None
        ldo, offo = layout(lay_out, D)
        return "reduce4" if D % 4 == 0 and ldo % 4 == 0 and offo % 4 == 0 else "scalar"

    fwd = _round_up((2 * su * M + M) * 4, 256)
    du = _round_up(su * M * D * 4, 256) if su > 1 else 0
    di = _round_up(si * N * D * 4, 256) if si > 1 else 0
    fwd_du = fwd + _round_up(su * M * D * 4, 256)
    ws = max(fwd, du + di, fwd_du) + 256
    stage_i = "dma" if can_dma(ldi, offi) else "reg"
    out.update(dp8=dp8, user=(su, tu, split_tiles(N, su, tu)), item=(si, ti, split_tiles(M, si, ti)), stage_fwd=stage_i,
               stage_du=stage_i, stage_di="dma" if can_dma(ldu, offu) else "reg", reduce_du=reduce_of(su, lay_du),
               reduce_di=reduce_of(si, lay_di), chunks=None, ws=ws, ws_bias=ws + _round_up(N * 4, 256))
    return out


# ------------------------------------------------------------------ the cases
# group, entry, shape, class, bias, and the layouts of U, I, dU, dI, du_unit
Case = collections.namedtuple("Case", "group entry M N D off cls bias lu li ldu ldi ldun")
ENTRIES = ("fwd", "fwd_du", "keep", "loss", "bwd", "bwd_nodu", "bias_plain", "bias_du", "bias_keep", "bias_loss")
BIAS_ENTRIES = ("bias_plain", "bias_du", "bias_keep", "bias_loss")
KEEP_ENTRIES = ("keep", "bias_keep")
# what an entry calls after its forward: (backward entry point, with dU)
BACKWARD = {"fwd": None, "fwd_du": None, "loss": None, "keep": ("kept", False), "bwd": ("bwd", True), "bwd_nodu": ("bwd", False),
            "bias_plain": ("bwd", True), "bias_du": ("bwd", False), "bias_keep": ("kept", False), "bias_loss": ("bwd", False)}
FULL = {4: 32, 8: 64, 16: 128}
NARROW = {4: (8, 24), 8: (40, 50), 16: (72, 98, 100)}
WIDE = (132, 200)
ALL_D = (8, 24, 32, 40, 50, 64, 72, 98, 100, 128, 132, 200)
STAGINGS = ("dma_dense", "dma_strided16", "reg_narrow", "reg_odd_ld", "reg_misaligned")
# (M, N, off) with the split plans of the issue's table (D does not enter plan_ce's splits):
#   77 x 203    1 / 1, off 126: the positives end in the last, ragged tile
#   130 x 700   user side 3 splits of 4 / 4 / 3 tiles, off 200: the positives cross the split boundary at item 256
#   300 x 300   2 splits of 3 / 2 tiles; 2 splits
#   321 x 577   3 splits of 4 / 4 / 2 tiles; 2 splits of 3 tiles; off 256: positives cross item 512 and end in the one-row tile
#   385 x 449   2 splits of 4 tiles; 2 splits of 4 / 3 tiles
#   129 x 1000  4 splits of 4 tiles; 1 split; off 871: the positives end in the last, ragged tile
SHAPES = ((77, 203, 126), (130, 700, 200), (300, 300, 0), (321, 577, 256), (385, 449, 64), (129, 1000, 871))
TWO_CHUNK = (130, 524352, 132, 524352 - 130)  # wide_chunk_rows = 128: a second chunk of two rows


def _matrix():
    """One case per (entry, width class, staging of the item rows, input class); shapes, narrow widths, bias terms and
    the remaining layouts rotate with the indices, as functions of (D, class) only so that few distinct references are
    needed."""
    cases = []
    for ie, entry in enumerate(ENTRIES):
        cells = [(dp8, st) for dp8 in (4, 8, 16) for st in STAGINGS] + [(None, "gemm")]
        for dp8, st in cells:
            if entry in KEEP_ENTRIES and not st.startswith("dma"):
                continue  # the kept-logits pair exists in the LDS-DMA form only
            for ic, cls in enumerate(CLASSES):
                if dp8 is None:
                    D = WIDE[ic % 2]
                elif st == "reg_narrow":
                    D = NARROW[dp8][(ic + ie) % len(NARROW[dp8])]
                else:
                    D = FULL[dp8]
                if cls == "planted" and D < 32:
                    D = 24  # (at D = 8 the planted items of OTHER rows outweigh a row's own positive; test_ce_reference_cpu.py checks the conditions)
                iD = ALL_D.index(D)
                M, N, off = SHAPES[0 if (cls == "planted" and D <= 32) else (iD + ic) % len(SHAPES)]
                # a term on top of +-80 would break the classes' conditions: none for shifted, none / Zipf for planted
                if entry not in BIAS_ENTRIES or cls == "shifted":
                    bias = "none"
                elif dp8 is None:
                    bias = {"flat": "pm30", "peaked": "zipf", "planted": "none"}[cls]
                else:
                    bias = BIASES[(iD + ie) % 2] if cls == "planted" else BIASES[(iD + ie + ic) % 3]
                rot = lambda k: LAYOUTS[(ic + ie + k) % len(LAYOUTS)]
                li = {"dma_dense": "dense", "dma_strided16": "strided16", "reg_odd_ld": "odd_ld", "reg_misaligned": "misaligned",
                      "reg_narrow": rot(1), "gemm": rot(1)}[st]
                if entry in KEEP_ENTRIES:
                    lu = ("dense", "strided16")[(ic + ie) % 2]
                elif st.startswith("dma"):
                    lu = ("dense", "odd_ld", "strided16", "misaligned")[ic]  # dI stages U by DMA, registers, DMA, registers
                elif st in ("reg_odd_ld", "reg_misaligned"):
                    lu = ("dense", "misaligned", "strided16", "odd_ld")[ic]
                else:
                    lu = rot(3)
                cases.append(Case("matrix", entry, M, N, D, off, cls, bias, lu, li, rot(0), rot(2), rot(4)))
    return cases


def _edges():
    """M = N = 1 (one tile, one row) through every entry and width class; the vector-load tails the issue names (D = 50
    in ld = 52, D = 98 in ld = 100) on both operands; the two-chunk wide case in modes 0, 1, 2 with and without a term."""
    cases = []
    for ie, entry in enumerate(ENTRIES):
        for D in (8, 64, 100, 132) if entry not in KEEP_ENTRIES else (32, 64, 128):
            # planted: the one logit is 80, a sum of D terms of one sign (a flat 1 x 1 logit is whatever cancellation left,
            # and its error relative to itself says nothing)
            cases.append(Case("one", entry, 1, 1, D, 0, "planted", "zipf" if entry in BIAS_ENTRIES else "none",
                              "dense", "dense", LAYOUTS[ie % 5], LAYOUTS[(ie + 1) % 5], LAYOUTS[(ie + 2) % 5]))
    for entry in ("fwd_du", "bwd", "bias_du", "bias_plain"):
        for D, (M, N, off) in ((50, SHAPES[1]), (98, SHAPES[3])):
            cases.append(Case("tail", entry, M, N, D, off, "flat", "zipf" if entry in BIAS_ENTRIES else "none",
                              "pad4", "pad4", "pad4", "odd_ld", "pad4"))
    M, N, D, off = TWO_CHUNK
    for entry, bias in (("fwd", "none"), ("fwd_du", "none"), ("bwd", "none"), ("bias_plain", "zipf"), ("bias_du", "zipf")):
        cases.append(Case("two_chunk", entry, M, N, D, off, "flat", bias, "strided16", "dense", "strided16", "dense", "strided16"))
    return cases


CASES = _matrix() + _edges()


def case_id(c):
    return (f"{c.group}-{c.entry}-{c.M}x{c.N}x{c.D}+{c.off}-{c.cls}-{c.bias}-U.{c.lu}-I.{c.li}-dU.{c.ldu}-dI.{c.ldi}"
            f"-du.{c.ldun}")


def math_key(c):
    """What the reference of a case depends on."""
    return (c.M, c.N, c.D, c.off, c.cls, c.bias)


def case_plan(c, gemm_ws=None):
    return plan(c.M, c.N, c.D, c.lu, c.li, c.ldu if BACKWARD[c.entry] == ("bwd", True) else "dense", c.ldi, gemm_ws)


def staging_of(c):
    """The issue's name for how the item rows of a case are staged, from the plan (not from how the case was meant)."""
    p = case_plan(c)
    if p["dp8"] is None:
        return "gemm"
    if p["stage_fwd"] == "dma":
        return "dma_dense" if c.li == "dense" else "dma_strided16"
    if c.D != 8 * p["dp8"]:
        return "reg_narrow"
    return "reg_odd_ld" if layout(c.li, c.D)[0] % 4 else "reg_misaligned"


def coverage(cases):
    """The cells of the issue's matrix that a case list reaches, each a tuple."""
    got = set()
    for c in cases:
        p = case_plan(c)
        st, dp8, back = staging_of(c), p["dp8"], BACKWARD[c.entry]
        got.add(("entry", c.entry))
        got.add(("width", c.D))
        got.add(("staging", st))
        got.add(("class", c.entry, dp8, st, c.cls))
        if c.entry in BIAS_ENTRIES:
            got.add(("bias", c.entry, st, c.bias))
        if c.M == 1 and c.N == 1:
            got.add(("ragged", "1x1"))
        if c.entry in KEEP_ENTRIES and _ceil_div(c.N, 64) % 2:
            got.add(("keep_pad", c.entry, "unwritten_columns"))  # an odd number of 64-column tiles in the 128-padded buffer
        for name, hit in (("M%32", c.M % 32), ("M%128", c.M % 128), ("N%64", c.N % 64)):
            if hit:
                got.add(("ragged", name))
        if dp8 is None:
            got.add(("wide", "one_chunk") if len(p["chunks"]) == 1 else
                    ("wide", "two_chunks_ragged", c.entry, c.bias != "none", c.lu) if p["chunks"][-1] < p["chunks"][0] else ("wide", "even"))
            continue
        if back == ("bwd", True) or back == ("bwd", False):
            got.add(("bwd_pair", c.entry, p["stage_di"] + "/" + p["stage_du"]))
        for ld_name, v, lay in (("U", p["vec_u"], c.lu), ("I", p["vec_i"], c.li)):
            got.add(("vec", "vec0" if not v else "vec1_d4" if c.D % 4 == 0 else "vec1_tail"))
            if v and c.D % 4:
                got.add(("vec1_tail", c.D, layout(lay, c.D)[0]))
        (su, tu, tiles_u), (si, ti, tiles_i) = p["user"], p["item"]
        got.add(("splits", "1/1" if su == 1 and si == 1 else ">1/1" if si == 1 else "1/>1" if su == 1 else ">1/>1"))
        for s, t, tiles in (p["user"], p["item"]):
            got.add(("splits", "tps_odd" if t % 2 else "tps_even"))
            if tiles[-1] < t and s > 1:
                got.add(("splits", "short_last"))
            if s == 1 and tiles == [1]:
                got.add(("splits", "one_tile"))
        if back is not None:
            for r in ((p["reduce_du"],) if back == ("bwd", True) else ()) + (p["reduce_di"],):
                if r:
                    got.add(("reduce", r))
        if c.N % 64 and c.off + c.M - 1 >= c.N // 64 * 64:
            got.add(("ragged", "pos_last_ragged_tile"))
        if su > 1 and c.off // (tu * 64) != (c.off + c.M - 1) // (tu * 64):
            got.add(("ragged", "pos_straddle_split"))
    return got


def required_cells():
    """Every cell of the issue's matrix, as coverage() names them."""
    need = {("entry", e) for e in ENTRIES} | {("width", D) for D in ALL_D} | {("staging", s) for s in STAGINGS + ("gemm",)}
    for e in ENTRIES:
        for dp8 in (4, 8, 16, None):
            for st in (("gemm",) if dp8 is None else STAGINGS):
                if e in KEEP_ENTRIES and not st.startswith("dma"):
                    continue
                need |= {("class", e, dp8, st, cls) for cls in CLASSES}
                if e in BIAS_ENTRIES:
                    need |= {("bias", e, st, b) for b in BIASES}
        if BACKWARD[e] is not None and BACKWARD[e][0] == "bwd":
            need |= {("bwd_pair", e, pair) for pair in ("dma/dma", "dma/reg", "reg/dma", "reg/reg")}
    need |= {("vec", v) for v in ("vec0", "vec1_d4", "vec1_tail")} | {("vec1_tail", 50, 52), ("vec1_tail", 98, 100)}
    need |= {("splits", s) for s in ("1/1", ">1/1", ">1/>1", "tps_odd", "tps_even", "short_last", "one_tile")}
    need |= {("reduce", "reduce4"), ("reduce", "scalar")}
    need |= {("ragged", r) for r in ("M%32", "M%128", "N%64", "pos_last_ragged_tile", "pos_straddle_split", "1x1")}
    need |= {("wide", "one_chunk")} | {("keep_pad", e, "unwritten_columns") for e in KEEP_ENTRIES}
    need |= {("wide", "two_chunks_ragged", e, b, "strided16")
             for e, b in (("fwd", False), ("fwd_du", False), ("bwd", False), ("bias_plain", True), ("bias_du", True))}
    return need


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _operands(M, N, D, off, cls):
    seed = 9000 + 7 * M + 13 * N + 131 * D
    k = (128.0 / D) ** 0.25
    scale = (PEAKED_SCALE if cls == "peaked" else 0.5) * k
    U = T(fg.gaussianish((M, D), seed)).double() * scale
    I = T(fg.gaussianish((N, D), seed + 1)).double() * scale
    if cls == "shifted":
        v = torch.full((D,), 1.0 / math.sqrt(D), dtype=F64)
        c = math.sqrt(80.0)
        sign = torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0).double()
        U = U - (U @ v)[:, None] * v + sign[:, None] * c * v
        I = I - (I @ v)[:, None] * v + c * v
    if cls == "planted":
        rows = torch.arange(M)
        hi, lo = rows[rows % 4 == 0], rows[rows % 4 == 1]
        unit = 80.0 * U / (U * U).sum(dim=1, keepdim=True)
        I[hi + off] = unit[hi]
        I[lo + off] = -unit[lo]
    coef = T(fg.gaussianish((M,), seed + 2)).double() / M
    coef[15::16] = 0.0
    labels = (T(fg.gaussianish((M, 3), seed + 3)) > 0.3).float()
    return U.float().contiguous(), I.float().contiguous(), coef.float().contiguous(), labels


@functools.lru_cache(maxsize=None)
def _bias(N, bias):
    return None if bias == "none" else zipf_bias(N) if bias == "zipf" else signed_bias(N)


UVW = torch.tensor([0.1, 0.2, 0.3])


def inputs(key):
    """fp32 (U, I, b or None, coef, labels [M, 3]) of a math_key."""
    M, N, D, off, cls, bias = key
    U, I, coef, labels = _operands(M, N, D, off, cls)
    return U, I, _bias(N, bias), coef, labels


# ------------------------------------------------------------------ the formulas
def _nt(a, b):
    """[n, d] x [m, d] -> [n, m], reduced over d."""
    if a.dtype == F64:
        return a @ b.t()
    acc, tmp = torch.zeros(a.shape[0], b.shape[0], dtype=a.dtype), torch.empty(a.shape[0], b.shape[0], dtype=a.dtype)
    for k in range(a.shape[1]):
        torch.mul(a[:, k, None], b[None, :, k], out=tmp)
        acc.add_(tmp)
    return acc


def _nn(p, v):
    """[n, m] x [m, d] -> [n, d], reduced over m in index order."""
    if p.dtype == F64:
        return p @ v
    acc, tmp = torch.zeros(p.shape[0], v.shape[1], dtype=p.dtype), torch.empty(p.shape[0], v.shape[1], dtype=p.dtype)
    pt = p.t().contiguous()
    for j in range(p.shape[1]):
        torch.mul(pt[j][:, None], v[j][None, :], out=tmp)
        acc.add_(tmp)
    return acc


def _tn(g, u):
    """[m, n]^T x [m, d] -> [n, d], reduced over m in index order."""
    if g.dtype == F64:
        return g.t() @ u
    acc, tmp = torch.zeros(g.shape[1], u.shape[1], dtype=g.dtype), torch.empty(g.shape[1], u.shape[1], dtype=g.dtype)
    for i in range(g.shape[0]):
        torch.mul(g[i][:, None], u[i][None, :], out=tmp)
        acc.add_(tmp)
    return acc


def _exp(x):
    """exp in x's dtype; float32: the correctly rounded one (float64's, rounded), not the host library's vector form."""
    return torch.exp(x) if x.dtype == F64 else torch.exp(x.double()).to(x.dtype)


def _log(x):
    return torch.log(x) if x.dtype == F64 else torch.log(x.double()).to(x.dtype)


def _sum(x):
    """Sum over the last index; float32: in index order, one rounding per add (numpy's accumulate is sequential)."""
    if x.dtype == F64:
        return x.sum(dim=-1)
    with np.errstate(over="ignore"):  # (the mutant without the max subtraction overflows: that is its point)
        return T(np.add.accumulate(x.contiguous().numpy(), axis=-1, dtype=np.float32)[..., -1])


# name -> the cases (by shape, plan and inputs) at which the mutant can differ from the true formula
MUTANTS = {
    # the last streamed tile's missing rows count as logits of 0 (seen where a row's lse leaves e^0 a part of 1e-5 or more)
    "ragged_tile_zero": lambda k, p: k[1] % 64 != 0 and float(key_reference(k)["lse"].min()) < 11.5,
    # the last item takes no part in the statistics (seen where it holds a part of 1e-3 or more of some row's mass)
    "last_item_ignored": lambda k, p: k[1] > 1 and float(key_reference(k)["p_last"].max()) > 1e-3,
    "last_user_ignored": lambda k, p: True,
    "no_diag_offset": lambda k, p: k[3] != 0,                   # positives taken at i
    "diag_first_split": lambda k, p: p["user"] is not None and p["user"][0] > 1 and k[3] + k[0] - 1 >= p["user"][1] * 64,
    "no_max": lambda k, p: k[4] == "shifted",
    "merge_no_factor_lse": lambda k, p: p["user"] is not None and p["user"][0] > 1,
    "merge_no_factor_du": lambda k, p: p["user"] is not None and p["user"][0] > 1,
    "bias_fwd_only": lambda k, p: k[5] != "none",
    "bias_by_user_row": lambda k, p: k[5] != "none" and k[0] > 1,
    "bias_ln_units": lambda k, p: k[5] != "none",
    "abs_coef": lambda k, p: bool((inputs(k)[3] < 0).any()),
    "zero_coef_neighbour": lambda k, p: k[0] >= 16,
    "slack_read": lambda k, p: True,                            # (applied where a case of the key has a strided U or I)
    "chunk_overwrite_dI": lambda k, p: p["chunks"] is not None and len(p["chunks"]) > 1,
    "chunk_diag_local": lambda k, p: p["chunks"] is not None and len(p["chunks"]) > 1,
}
# derived from the unmutated result and its logits without another pass over the products
POSTHOC = ("chunk_overwrite_dI", "chunk_diag_local", "last_user_ignored", "diag_first_split")


def heavy(key):
    """The two-chunk wide case: 68 M logits.  It is left out of the yardstick -- float32 summed in index order over
    524 352 terms is itself 6e-5 of max|lse| and 3e-4 of max|du_unit| off (measured), worse than every bound here, and
    no tolerance of the case derives from YARD: it is `flat`, held to the project's fixed figures, and the wide path's
    row_lse is not compared -- and it takes the POSTHOC mutants only, applied to the float64 reference rounded to float32."""
    return key[0] * key[1] > 10 ** 7


_ALL = frozenset(QUANTITIES)
# the quantities a mutant stands for in the kernels (evaluate() may move others along: a backward's dU is recomputed by
# its own kernel, not taken from the forward's merge or from wide_sub_diag_kernel)
AFFECTS = {
    "ragged_tile_zero": _ALL - {"logits"}, "last_item_ignored": _ALL - {"logits"}, "last_user_ignored": _ALL,
    "no_diag_offset": frozenset({"ce", "du_unit", "dU", "dI"}), "diag_first_split": frozenset({"ce"}),
    "no_max": _ALL - {"logits"}, "merge_no_factor_lse": frozenset({"ce", "lse"}), "merge_no_factor_du": frozenset({"du_unit"}),
    "bias_fwd_only": frozenset({"dU", "dI"}), "bias_by_user_row": frozenset({"dI"}), "bias_ln_units": _ALL,
    "abs_coef": frozenset({"dU", "dI"}), "zero_coef_neighbour": frozenset({"dU", "dI"}), "slack_read": _ALL,
    "chunk_overwrite_dI": frozenset({"dI"}), "chunk_diag_local": frozenset({"du_unit"}),
}


def compared(c):
    """The quantities test_gpu_ce_reference.py compares for case c (it asserts that it compares exactly these)."""
    q = {"ce"} | ({"lse"} if c.D <= 128 else set())
    if c.entry in ("fwd_du", "keep", "loss", "bias_du", "bias_keep", "bias_loss"):
        q.add("du_unit")
    if c.entry in KEEP_ENTRIES:
        q.add("logits")
    if BACKWARD[c.entry] is not None:
        q.add("dI")
        if BACKWARD[c.entry][1]:
            q.add("dU")
    return frozenset(q)


@functools.lru_cache(maxsize=None)
def key_compared(key):
    """Every quantity that some case of a math key compares."""
    return frozenset().union(*[compared(c) for c in CASES if math_key(c) == key])


def watched(mut, key):
    """The quantities through which a mutant at a key can be seen by the GPU test: only these count when it is rejected."""
    affects = AFFECTS[mut]
    if key[1] == 1 and mut in ("slack_read", "bias_ln_units"):
        affects = frozenset({"lse", "logits"})  # one logit: it moves, p = 1 stays (and the wide path's lse is not compared)
    return affects & key_compared(key)


def applies(mut, key, pl):
    if key[1] == 1 and mut not in ("slack_read", "bias_ln_units", "bias_fwd_only", "last_user_ignored"):
        return False  # one logit: p = 1, ce = 0 and every gradient is 0 whatever the coefficient or the statistics
    return bool(watched(mut, key)) and MUTANTS[mut](key, pl) and (mut in POSTHOC or not heavy(key))


def evaluate(U, I, b, coef, off, dtype, mut=None, pl=None, memo=None):
    """{"ce", "lse", "logits", "du_unit", "dU", "dI"} in `dtype`; lse in natural-log units.  mut: a key of MUTANTS
    (pl = plan(M, N, D), needed by the split and chunk mutants).  memo: a dict that carries the logits and the unmutated
    result of the same inputs and dtype from one call to the next."""
    memo = {} if memo is None else memo
    U, I, coef = U.to(dtype), I.to(dtype), coef.to(dtype)
    b = None if b is None else b.to(dtype)
    M, N = U.shape[0], I.shape[0]
    rows = torch.arange(M)
    if mut in POSTHOC:
        if "base" not in memo:
            memo["base"] = evaluate(U, I, b, coef, off, dtype, None, pl, memo)
        out = {k: v.clone() for k, v in memo["base"].items()}
        if mut == "last_user_ignored":  # its outputs are never written, and it adds nothing to dI
            for k in ("ce", "lse", "logits", "du_unit", "dU"):
                out[k][M - 1] = SENTINEL
            g = _exp(memo["Sb"][M - 1] - memo["base"]["lse"][M - 1])
            g[M - 1 + off] -= 1.0
            out["dI"] = out["dI"] - (g * coef[M - 1])[:, None] * U[M - 1][None, :]
        elif mut == "diag_first_split":  # the rows whose positive lies in a later split find diag = 0
            late = rows + off >= pl["user"][1] * 64
            out["ce"][late] = out["lse"][late]
        elif mut == "chunk_diag_local":  # r counted from the chunk start
            r0 = pl["chunks"][0]
            out["du_unit"][r0:] = out["du_unit"][r0:] + I[rows[r0:] + off] - I[rows[r0:] - r0 + off]
            out["dU"][r0:] = coef[r0:, None] * out["du_unit"][r0:]
        else:  # chunk_overwrite_dI: the last chunk's product replaces the sum
            r0 = M - pl["chunks"][-1]
            g = _exp(memo["Sb"][r0:] - memo["base"]["lse"][r0:, None])
            g[rows[r0:] - r0, rows[r0:] + off] -= 1.0
            out["dI"] = _tn(g * coef[r0:, None], U[r0:])
        return out
    if mut == "slack_read":  # column D - 1 of the item rows comes from the slack (NaN taken as 1.0)
        I = I.clone()
        I[:, -1] = 1.0
        S = _nt(U, I)
    else:
        if "S" not in memo:
            memo["S"] = _nt(U, I)
        S = memo["S"]
    if mut == "abs_coef":
        coef = coef.abs()
    if mut == "zero_coef_neighbour":
        coef = coef.clone()
        zero = (coef == 0).nonzero()[:, 0]
        coef[zero] = coef[zero - 1]
    bf = b
    if mut == "bias_ln_units" and b is not None:  # fma(acc, log2 e, b) with b not yet scaled by log2 e
        bf = b * LN2
    Sb = S if bf is None else S + bf[None, :]
    if mut is None:
        memo["Sb"] = Sb
    pos = rows if mut == "no_diag_offset" else rows + off
    stat = Sb
    if mut == "ragged_tile_zero":
        stat = torch.cat([Sb, torch.zeros(M, 64 - N % 64, dtype=dtype)], dim=1)
    if mut == "last_item_ignored":
        stat = Sb[:, :N - 1]
    mx = torch.zeros(M, dtype=dtype) if mut == "no_max" else stat.max(dim=1).values
    e = _exp(stat - mx[:, None])
    l = _sum(e)
    lse = mx + _log(l)
    if mut == "merge_no_factor_lse":  # sum_z s_z instead of sum_z s_z 2^(m_z - M)
        width = pl["user"][1] * 64
        ez = torch.cat([_exp(Sb[:, z:z + width] - Sb[:, z:z + width].max(dim=1, keepdim=True).values) for z in range(0, N, width)], dim=1)
        lse_out = mx + _log(_sum(ez))
    else:
        lse_out = lse
    ce = lse_out - Sb[rows, pos]
    P = e[:, :N] / l[:, None]
    if mut == "last_item_ignored":
        P = torch.cat([P, torch.zeros(M, 1, dtype=dtype)], dim=1)
    if mut == "merge_no_factor_du":  # sum_z O_z instead of sum_z O_z 2^(m_z - M)
        width = pl["user"][1] * 64
        ez = torch.cat([_exp(Sb[:, z:z + width] - Sb[:, z:z + width].max(dim=1, keepdim=True).values) for z in range(0, N, width)], dim=1)
        E = _nn(ez / l[:, None], I)
    else:
        E = _nn(P, I)
    du_unit = E - I[pos]
    Pb = P
    if mut == "bias_fwd_only":  # the backward forms its probabilities from the plain logits
        Pb = _exp(S - lse[:, None])
    if mut == "bias_by_user_row":
        Pb = _exp(S + b[:M, None] - lse[:, None])
    if Pb is P:
        dU = coef[:, None] * du_unit
    else:
        dU = coef[:, None] * (_nn(Pb, I) - I[pos])
    G = Pb.clone()
    G[rows, pos] -= 1.0
    dI = _tn(G * coef[:, None], U)
    out = {"ce": ce, "lse": lse_out, "logits": Sb * LOG2E, "du_unit": du_unit, "dU": dU, "dI": dI}
    if mut is None:
        memo["base"] = out
    return out


def weighted_loss(ce, labels):
    """(w, coef, loss) of the weighted-mean loss head in ce's dtype (ref :322, :334-343): nuv = labels . uvw clamped at
    1e-6, w = nuv / max nuv, loss = sum(ce w) / M, coef = w / M."""
    nuv = torch.clamp((labels.to(ce.dtype) * UVW.to(ce.dtype)).sum(dim=-1), min=0.000001)
    w = nuv / nuv.max()
    return w, w / ce.shape[0], (ce * w).sum() / ce.shape[0]


def reference(key):
    """float64 quantities of a math_key: the forward, torch autograd through sum(coef ce) for dU and dI, and the weighted
    mean loss (w, coef_w, loss) of the fused loss entries."""
    U32, I32, b, coef, labels = inputs(key)
    M, off = key[0], key[3]
    U, I = U32.double().requires_grad_(True), I32.double().requires_grad_(True)
    S = U @ I.t()
    if b is not None:
        S = S + b.double()[None, :]
    rows = torch.arange(M)
    lse = torch.logsumexp(S, dim=1)
    ce = lse - S[rows, rows + off]
    dU, dI = torch.autograd.grad((ce * coef.double()).sum(), [U, I])
    with torch.no_grad():
        P = torch.exp(S - lse[:, None])
        du_unit = P @ I - I[rows + off]
        p_pos, p_max = P[rows, rows + off].clone(), P.max(dim=1).values
        w, coef_w, loss = weighted_loss(ce, labels)
        out = {"ce": ce.detach(), "lse": lse.detach(), "logits": (S * LOG2E).detach(), "du_unit": du_unit, "dU": dU, "dI": dI,
               "w": w, "coef_w": coef_w, "loss": loss, "p_pos": p_pos, "p_max": p_max, "row_max": S.detach().max(dim=1).values,
               "p_last": P[:, -1].clone()}
    return out


_ref_cache = {}


def key_reference(key):
    """reference(key), computed once per key.  Leave it unchanged."""
    if key not in _ref_cache:
        _ref_cache[key] = reference(key)
    return _ref_cache[key]


def case_reference(c):
    return key_reference(math_key(c))


# ------------------------------------------------------------------ tolerances
def tol(cls, name):
    """(a, m, r) of |got - ref| <= a + m max|ref| + r |ref|."""
    if cls == "flat" and name in FLAT_TOL:
        return FLAT_TOL[name]
    return (0.0, FACTOR * YARD[cls][name], RTOL[name])


def ratio(got, ref, t):
    """Worst |got - ref| / bound over every element (NaN counts as inf); <= 1 means within tolerance."""
    got = got.detach().to(F64)  # (on the device the result is on: the two-chunk case has 69 M elements)
    ref = ref.detach().to(got.device, F64)
    bound = t[0] + t[1] * float(ref.abs().max()) + t[2] * ref.abs()
    err = (got - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)  # (an exact result passes a bound of 0: M = N = 1)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    return float(q.max())


def ratios(got, ref, cls):
    """{quantity: worst err / bound} of the quantities in `got` against reference()'s dict."""
    return {n: ratio(got[n], ref[n], tol(cls, n)) for n in got if n in QUANTITIES}


def normalised_error(got, ref, name):
    """The yardstick's unit: max((|got - ref| - r |ref|)+) / max|ref|."""
    got, ref = got.detach().to("cpu", F64), ref.detach().to("cpu", F64)
    top = float(ref.abs().max())
    return float(((got - ref).abs() - RTOL[name] * ref.abs()).clamp_min(0.0).max()) / (top if top > 0 else 1.0)


# the fused loss head (one 1024-thread workgroup: 3 products and 2 adds, a clamp, a division, another by M; partial sums
# of ce w in 1024 threads, then wave and block reductions).  Each of w and coef is at most 6 roundings of half an ulp
# from the exact value: 8 x 2^-24 of max|ref|.  The loss inherits every row's ce bound weighted by w <= 1, plus the
# rounding of at most M / 1024 + 6 + 16 additions and a product per term, each at most 2^-24 of sum |ce| w / M.
def loss_tolerances(ref, cls):
    ce_t = tol(cls, "ce")
    ce_bound = ce_t[0] + ce_t[1] * float(ref["ce"].abs().max()) + ce_t[2] * ref["ce"].abs()
    M = ref["ce"].shape[0]
    adds = M / 1024 + 6 + 16 + 2
    loss_bound = float((ce_bound * ref["w"]).sum()) / M + (adds + 8) * FLOOR * float((ref["ce"].abs() * ref["w"]).sum()) / M
    return {"w": (0.0, 8 * FLOOR, 0.0), "coef_w": (0.0, 8 * FLOOR, 0.0), "loss": (loss_bound, 0.0, 0.0)}


def yardstick_keys():
    return sorted(set(math_key(c) for c in CASES if not heavy(math_key(c))), key=str)


def measure(keys=None):
    """Worst normalised error of the float32 evaluation per (class, quantity) over the cases' math keys, and where."""
    worst = {cls: {q: (0.0, None) for q in QUANTITIES} for cls in CLASSES}
    for key in (yardstick_keys() if keys is None else keys):
        U, I, b, coef, _ = inputs(key)
        ref = key_reference(key)
        got = evaluate(U, I, b, coef, key[3], F32)
        for q in QUANTITIES:
            e = normalised_error(got[q], ref[q], q)
            if e >= worst[key[4]][q][0]:
                worst[key[4]][q] = (e, key)
    return worst


def main():
    print("float32 CPU evaluation against float64: worst max((|err| - r |ref|)+) / max|ref| per class")
    worst = measure()
    ok = True
    for cls in CLASSES:
        print(f"{cls:<8} " + " ".join(f"{q} {worst[cls][q][0]:.3e}" for q in QUANTITIES))
        print(f"{'':<8} recorded " + " ".join(f"{q} {YARD[cls][q]:.1e}" for q in QUANTITIES))
        print(f"{'':<8} worst dI at {worst[cls]['dI'][1]}")
        ok = ok and all(worst[cls][q][0] <= YARD[cls][q] for q in QUANTITIES)
    assert ok, "YARD is below the measured worst case"


if __name__ == "__main__":
    main()
