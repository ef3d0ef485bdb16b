"""Float64 yardstick for the collapsed last encoder layer (csrc/encoder_last.hip).  A helper, not a test: imported by
test_encoder_last_reference_cpu.py and test_gpu_encoder_last_reference.py the way attention_ref.py is imported by its tests;
the product never imports it.  `python tests/encoder_last_ref.py` prints the yardstick table.

  reference    the UNCOLLAPSED layer -- Q, K and V projected at every position, softmax, output projection, row 0 taken -- in
               float64, gradients by torch autograd; with lengths, one sample at a time by truncation.  The saved tensors
               (q0, t, probs, xbar, ctx0) from the definitions of include/tt_hotpath.h, in float64.
  collapsed    the kernels' algebra (t_h = W_k,h^T q0_h, xbar_h, 32-sample weight partials, four-chain reduce) in float64
               (matmul) or float32 (one rounding per multiply and per add, sums in index order, exp correctly rounded:
               attention_ref's helpers).  `mut` names a deliberately wrong formula.
  inputs       four classes from fixture_gen.gaussianish, seeded from (H, D, heads): a smaller batch is a prefix of a larger one
                 flat     x of scale 1 (the older tests' inputs)
                 peaked   x of scale 3
                 shifted  flat + a per-sample vector on rows 1 .. H-1, solved in float64 from t so that every head's scores
                          there sit near +200 (even samples: exp overflows without the max subtraction, row 0 underflows)
                          or near -200 (odd samples: row 0 takes all the mass).  H = 1 has no such rows.
                 kbias    flat with b_in[D:2D] * 1e3: the reference keeps it, the kernels' algebra drops it
  CASES / tol  the cases test_gpu_encoder_last_reference.py runs and the tolerance of each (class, quantity), shared with the
               CPU tests, which measure the yardstick and run the mutants at the very same cases.

Tolerances.  |got - ref| <= a + m max|ref| + r |ref| element-wise.  The flat class keeps the project's figures
(tests/test_gpu_kernels.py): recent a = 4e-6, r = 1e-5; gradients a = 1e-8, m = 4e-6, r = 2e-4.  Everything else (the saved
tensors of every class; every quantity of peaked, shifted, kbias): a = 0, r = 1e-5 (gradients 2e-4) and m = 4 x YARD[class]
[quantity], YARD = the worst max((|fp32 - f64| - r |f64|)+) / max|f64| of the float32 CPU evaluation over the class's cases,
rounded up to two digits, never below 2^-24; the factor 4 is the Adam reference's (the hardware's 1-ulp exp and reciprocal,
the matrix cores' summation order).  Never calibrated against a kernel.  profiles/encoder_last_reference_tolerance.txt
records the table and what the GPU showed."""
import collections
import math
import sys

import torch

import attention_ref as AR
import gemm_ref as GR

fg = AR.fg
F64, F32 = torch.float64, torch.float32
T = AR.T
Launches = GR.Launches
E_BADARG, E_WORKSPACE, E_UNSUPPORTED = GR.E_BADARG, GR.E_WORKSPACE, GR.E_UNSUPPORTED

CLASSES = ("flat", "peaked", "shifted", "kbias")
SAVED = ("q0", "t", "probs", "xbar", "ctx0")
GRADS = ("dx", "dW_in", "db_in", "dW_out", "db_out")
NAMES = SAVED + ("recent",) + GRADS
FWD_NAMES = SAVED + ("recent",)
RTOL = {n: (2e-4 if n in GRADS else 1e-5) for n in NAMES}
FLAT_TOL = dict({"recent": (4e-6, 0.0, 1e-5)}, **{n: (1e-8, 4e-6, 2e-4) for n in GRADS})
FLOOR = 2.0 ** -24
FACTOR = 4.0
GARBAGE = 50.0  # scale of what the backward's copy of x holds in padded rows

K_PRE, K_MAIN, K_MAIN_LEN, K_POST = "enc_last_pre_kernel", "enc_last_main_fwd_kernel", "enc_last_main_fwd_len_kernel", "enc_last_post_kernel"
K_A, K_BWD, K_B, K_WGRAD, K_REDUCE = ("enc_last_bwd_a_kernel", "enc_last_main_bwd_kernel", "enc_last_bwd_b_kernel",
                                      "enc_last_wgrad_kernel", "enc_last_reduce_kernel")
KERNELS = (K_PRE, K_MAIN, K_MAIN_LEN, K_POST, K_A, K_BWD, K_B, K_WGRAD, K_REDUCE)

# worst normalised error of the float32 CPU evaluation against float64 per (class, quantity): see main()
YARD = {
    "flat": dict(q0=1.4e-07, t=1.8e-07, probs=6.0e-08, xbar=4.6e-07, ctx0=3.3e-07, recent=4.1e-07,
                 dx=2.4e-07, dW_in=2.8e-07, db_in=6.0e-08, dW_out=3.0e-07, db_out=6.0e-08),
    "peaked": dict(q0=9.9e-08, t=2.7e-07, probs=1.1e-06, xbar=4.5e-06, ctx0=2.2e-06, recent=2.0e-06,
                   dx=1.1e-06, dW_in=1.7e-06, db_in=1.3e-06, dW_out=1.4e-06, db_out=6.0e-08),
    "shifted": dict(q0=1.2e-07, t=1.8e-07, probs=1.5e-05, xbar=2.4e-07, ctx0=2.6e-07, recent=2.6e-07,
                    dx=5.2e-03, dW_in=6.5e-05, db_in=5.8e-03, dW_out=1.9e-07, db_out=6.0e-08),
    "kbias": dict(q0=1.2e-07, t=1.8e-07, probs=6.0e-08, xbar=4.1e-07, ctx0=2.6e-07, recent=3.2e-07,
                  dx=1.5e-07, dW_in=1.8e-07, db_in=6.0e-08, dW_out=2.0e-07, db_out=6.0e-08),
}

# ------------------------------------------------------------------ the cases
# lens: None | "cycle" (1 .. H in turn; B < H: spread evenly over 1 .. H) | "bad" (0, -3, H + 1, 2^31 - 1 planted) | "null" (tt_enc_last_fwd_len, lengths = NULL)
# place: 0 packed, aligned | 1 recent one float off a 16-byte boundary with ld = D + 3 | 2 recent = out[:, 0, :] of [B, 2, D];
#        1 and 2: d_recent with ld = 2D; q0, ctx0, probs, b_in, b_out one float off
Case = collections.namedtuple("Case", "group B H D heads cls lens place", defaults=(None, 0))

BATCHES = (1, 31, 32, 33, 64, 65, 97, 129, 225, 257)  # G = 1, 1, 1, 2, 2, 3, 4, 5, 8, 9 partials
WIDTHS = ((4, 1), (8, 2), (36, 3), (64, 16), (64, 1), (68, 1), (72, 2), (96, 2), (100, 5), (124, 1), (128, 1), (128, 4), (128, 16))
HISTORIES = (1, 2, 31, 32, 33, 50, 63, 64)
LEN_SHAPES = ((33, 50, 128, 4), (65, 64, 64, 16), (4, 3, 4, 1))
BAD_LENGTHS = (0, -3, None, 2 ** 31 - 1)  # None: H + 1

CASES = ([Case("batch", B, 50, 128, 4, "flat") for B in BATCHES]
         + [Case("width", 33, 7, D, h, c) for (D, h) in WIDTHS for c in ("flat", "peaked")]
         + [Case("history", 3, H, D, h, c) for (D, h) in ((128, 4), (64, 16)) for H in HISTORIES for c in CLASSES
            if not (c == "shifted" and H == 1)]
         + [Case("lengths", *s, c, "cycle") for s in LEN_SHAPES for c in ("flat", "peaked")]
         + [Case("lengths", *s, "flat", "bad") for s in LEN_SHAPES]
         + [Case("lengths", *s, "flat", "null") for s in LEN_SHAPES]
         + [Case("placement", *s, "flat", None, p) for s in ((33, 50, 128, 4), (33, 10, 100, 5)) for p in (1, 2)]
         + [Case("kbias", *s, "kbias") for s in ((33, 50, 128, 4), (33, 7, 36, 3))])


def case_id(c):
    return (f"{c.group}-B{c.B}-H{c.H}-D{c.D}-h{c.heads}-{c.cls}" + (f"-len_{c.lens}" if c.lens else "")
            + (f"-place{c.place}" if c.place else ""))


def groups_of(B):
    return [(lo, min(lo + 32, B)) for lo in range(0, B, 32)]


def lengths_of(c):
    """(what the call is given, what the kernels use: clamped to [1, H]) or (None, None)."""
    if c.lens not in ("cycle", "bad"):
        return None, None
    # 1 .. H in turn where the batch is at least H long, else B lengths spread evenly over 1 .. H, both ends included
    raw = [1 + b % c.H if c.B >= c.H else 1 + (b * (c.H - 1)) // (c.B - 1) for b in range(c.B)]
    if c.lens == "bad":
        for b, v in enumerate(BAD_LENGTHS):
            raw[b] = c.H + 1 if v is None else v
    return raw, [min(max(v, 1), c.H) for v in raw]


def inputs(c):
    """fp32 operands of a case: x [B, H, D] (x_fwd: NaN in padded rows, x_bwd: finite garbage there), the layer's
    parameters, the cotangent g [B, D], lengths (raw, as passed) and lens (clamped, as used)."""
    B, H, D, heads = c.B, c.H, c.D, c.heads
    seed = 9000 + 131 * H + 7 * D + heads
    x = T(fg.gaussianish((B, H, D), seed)) * (3.0 if c.cls == "peaked" else 1.0)
    w_in = T(fg.gaussianish((3 * D, D), seed + 1)) * (1.0 / math.sqrt(D))
    b_in = T(fg.gaussianish((3 * D,), seed + 2)) * 0.1
    w_out = T(fg.gaussianish((D, D), seed + 3)) * (1.0 / math.sqrt(D))
    b_out = T(fg.gaussianish((D,), seed + 4)) * 0.1
    g = T(fg.gaussianish((B, D), seed + 5))
    if c.cls == "kbias":
        b_in[D:2 * D] *= 1e3
    if c.cls == "shifted":
        dh = D // heads
        q0 = x[:, 0].double() @ w_in[:D].double().t() + b_in[:D].double()
        t = torch.einsum("bhk,hkd->bhd", q0.reshape(B, heads, dh), w_in[D:2 * D].double().reshape(heads, dh, D))
        sign = torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0).double()
        want = (200.0 * math.sqrt(dh)) * sign[:, None, None] * torch.ones(B, heads, 1, dtype=F64)
        v = (torch.linalg.pinv(t) @ want)[:, :, 0]  # scale * t_h . v = +-200 for every head
        x = x.double()
        x[:, 1:] += v[:, None, :]
        x = x.float()
    raw, lens = lengths_of(c)
    x_fwd = x_bwd = x.contiguous()
    if lens is not None:
        pad = torch.arange(H)[None, :] >= torch.tensor(lens)[:, None]
        x_fwd = torch.where(pad[:, :, None], torch.full_like(x, float("nan")), x)
        x_bwd = torch.where(pad[:, :, None], T(fg.gaussianish((B, H, D), seed + 6)) * GARBAGE, x)
    return dict(x_fwd=x_fwd, x_bwd=x_bwd, w_in=w_in, b_in=b_in, w_out=w_out, b_out=b_out, g=g, lengths=raw, lens=lens,
                heads=heads)


# ------------------------------------------------------------------ the float64 reference
def uncollapsed(x, w_in, b_in, w_out, b_out, heads):
    """The whole layer at every position -> (out [B, H, D], prob [B, heads, H, H], ctx [B, H, D])."""
    B, H, D = x.shape
    dh = D // heads
    qkv = x.reshape(B * H, D) @ w_in.t() + b_in
    q, k, v = (qkv[:, i * D:(i + 1) * D].reshape(B, H, heads, dh).permute(0, 2, 1, 3) for i in range(3))
    s = (q * (1.0 / math.sqrt(dh))) @ k.transpose(-1, -2)
    p = torch.softmax(s, dim=-1)
    ctx = (p @ v).permute(0, 2, 1, 3).reshape(B, H, D)
    return (ctx.reshape(B * H, D) @ w_out.t() + b_out).reshape(B, H, D), p, ctx


def reference(inp):
    """{name: float64 tensor} of all eleven quantities."""
    heads, lens = inp["heads"], inp["lens"]
    leaves = [inp[k].double().requires_grad_(True) for k in ("x_bwd", "w_in", "b_in", "w_out", "b_out")]
    x, w_in, b_in, w_out, b_out = leaves
    B, H, D = x.shape
    dh = D // heads
    if lens is None:
        out, p, ctx = uncollapsed(x, w_in, b_in, w_out, b_out, heads)
        recent, probs, ctx0 = out[:, 0], p[:, :, 0, :], ctx[:, 0]
        xv = x
    else:
        rows = [uncollapsed(x[b:b + 1, :n], w_in, b_in, w_out, b_out, heads) for b, n in enumerate(lens)]
        recent = torch.cat([r[0][:, 0] for r in rows])
        probs = torch.cat([torch.cat([r[1][:, :, 0, :], x.new_zeros(1, heads, H - n)], dim=-1) for r, n in zip(rows, lens)])
        ctx0 = torch.cat([r[2][:, 0] for r in rows])
        xv = torch.where((torch.arange(H)[None, :] < torch.tensor(lens)[:, None])[:, :, None], x, torch.zeros_like(x))
    grads = torch.autograd.grad((recent * inp["g"].double()).sum(), leaves)
    with torch.no_grad():
        q0 = x[:, 0] @ w_in[:D].t() + b_in[:D]
        t = torch.einsum("bhk,hkd->bhd", q0.reshape(B, heads, dh), w_in[D:2 * D].reshape(heads, dh, D))
        xbar = torch.einsum("bhj,bjd->bhd", probs, xv)
    res = dict(q0=q0, t=t, probs=probs, xbar=xbar, ctx0=ctx0, recent=recent, dx=grads[0], dW_in=grads[1], db_in=grads[2],
               dW_out=grads[3], db_out=grads[4])
    return {k: v.detach() for k, v in res.items()}


# ------------------------------------------------------------------ the kernels' algebra
MUTANTS = ("scale", "no_max", "no_bv", "tile_head", "cols64", "last_pos", "dx0", "wgrad_last_sample", "reduce_last",
           "reduce_tail", "db_out_dctx0", "db_k", "len_ignored", "len_plus_one", "probs_pad")


def applies(mut, c):
    """Whether the wrong formula can change a result at this case."""
    G, dh = len(groups_of(c.B)), c.D // c.heads
    _, lens = lengths_of(c)
    longest = max(lens) if lens else c.H
    live = longest - (1 if c.cls == "shifted" else 0)  # shifted: row 0 holds all of the mass or none of it
    if mut in ("scale", "last_pos", "dx0"):  # a one-row softmax is 1 whatever the score: no score gradient either
        return live >= 2
    if mut == "no_max":
        return c.cls == "shifted"
    if mut == "tile_head":
        return live >= 2 and any((i // dh) != ((32 * (i // 32)) // dh) for i in range(c.D))  # one live row: every head's xbar is it
    if mut == "cols64":
        return c.D > 64
    if mut == "reduce_last":
        return G >= 2
    if mut == "reduce_tail":
        return G % 4 != 0
    if mut in ("len_ignored", "len_plus_one", "probs_pad"):
        return lens is not None and min(lens) < c.H
    return True


def _partials(a, bm, B, dtype, drop_last):
    """[G, M, N]: per 32-sample group, sum_b a[b, :, None] * bm[b] (bm [B, N] or [B, M, N]); a = None: sum_b bm[b]."""
    out = []
    for lo, hi in groups_of(B):
        hi = hi - 1 if drop_last else hi
        term = (lambda b: bm[b]) if a is None else (lambda b: a[b][:, None] * (bm[b] if bm[b].dim() == 2 else bm[b][None, :]))
        if dtype == F64:
            acc = (bm[lo:hi].sum(0) if a is None else a[lo:hi].t() @ bm[lo:hi] if bm.dim() == 2
                   else torch.einsum("bm,bmn->mn", a[lo:hi], bm[lo:hi]))
        else:
            acc = torch.zeros_like(term(lo))
            for b in range(lo, hi):
                acc = acc + term(b)
        out.append(acc)
    return torch.stack(out)


def _reduce(parts, mut):
    """enc_last_reduce_kernel's el_sum_parts: four interleaved chains, the tail on the first, (s0 + s1) + (s2 + s3)."""
    n = parts.shape[0] - (1 if mut == "reduce_last" else 0)
    s = [torch.zeros_like(parts[0]) for _ in range(4)]
    w = 0
    while w + 3 < n:
        for i in range(4):
            s[i] = s[i] + parts[w + i]
        w += 4
    if mut != "reduce_tail":
        for w in range(w, n):
            s[0] = s[0] + parts[w]
    return (s[0] + s[1]) + (s[2] + s[3])


def collapsed(inp, dtype=F64, mut=None):
    """{name: tensor in dtype} of all eleven quantities, the way csrc/encoder_last.hip forms them."""
    heads = inp["heads"]
    x, w_in, b_in, w_out, b_out, g = (inp[k].to(dtype) for k in ("x_bwd", "w_in", "b_in", "w_out", "b_out", "g"))
    B, H, D = x.shape
    dh = D // heads
    _nt, _nn, _sum, _exp = AR._nt, AR._nn, AR._sum, AR._exp
    Wq, Wk, Wv, bq, bv = w_in[:D], w_in[D:2 * D], w_in[2 * D:], b_in[:D], b_in[2 * D:]
    scale = torch.tensor(float(dh + 1 if mut == "scale" else dh), dtype=dtype).sqrt().reciprocal()
    head_of = torch.arange(D) // dh
    pick = lambda full, hd: full.gather(1, hd[None, None, :].expand(B, 1, D))[:, 0]  # [B, heads, D] -> [B, D], column i of head hd[i]
    # forward
    q0 = _nt(x[:, 0], Wq) + bq
    t = _nn(q0.reshape(B, heads, 1, dh), Wk.reshape(heads, dh, D))[:, :, 0]
    s = _nt(t, x) * scale  # [B, heads, H]
    Hv = torch.tensor(inp["lens"] if inp["lens"] is not None else [H] * B)
    if mut == "len_ignored":
        Hv = torch.full_like(Hv, H)
    if mut == "len_plus_one":
        Hv = (Hv + 1).clamp(max=H)
    pos = torch.arange(H)[None, :]
    valid = pos < Hv[:, None]
    if mut == "last_pos":
        valid = valid & ((pos != Hv[:, None] - 1) | (Hv[:, None] < 2))
    valid = valid[:, None, :]
    sm = s.masked_fill(~valid, float("-inf"))
    mx = torch.zeros_like(sm[..., :1]) if mut == "no_max" else sm.max(dim=-1, keepdim=True).values
    e = _exp(sm - mx)
    p = e / _sum(e)[..., None]
    xbar = _nn(p, torch.where(valid.transpose(1, 2), x, torch.zeros_like(x)))
    if mut == "probs_pad":
        p = torch.where(valid, p, _exp(s - mx))
    if mut == "cols64":
        xbar = torch.cat([xbar[..., :64], torch.zeros_like(xbar[..., 64:])], dim=-1)
    ctx_head = (32 * (torch.arange(D) // 32)) // dh if mut == "tile_head" else head_of
    ctx0 = pick(_nt(xbar, Wv), ctx_head)
    if mut != "no_bv":
        ctx0 = ctx0 + bv
    recent = _nt(ctx0, w_out) + b_out
    # backward, data
    d_ctx0 = _nn(g, w_out)
    d_xbar = _nn(d_ctx0.reshape(B, heads, 1, dh), Wv.reshape(heads, dh, D))[:, :, 0]
    dp = _nt(d_xbar, x)
    delta = _sum(p * dp)
    ds = scale * p * (dp - delta[..., None])
    dt = _nn(ds, x)
    if mut == "cols64":
        dt = torch.cat([dt[..., :64], torch.zeros_like(dt[..., 64:])], dim=-1)
    dx = _nn(p.transpose(-1, -2), d_xbar) + _nn(ds.transpose(-1, -2), t)
    dq0 = pick(_nt(dt, Wk), head_of)
    if mut != "dx0":
        dx = torch.cat([(dx[:, 0] + _nn(dq0, Wq))[:, None], dx[:, 1:]], dim=1)
    # backward, weights: one partial per 32 samples, then the fixed-order reduce
    drop = mut == "wgrad_last_sample"
    per_row = lambda v: v.repeat_interleave(dh, dim=1)  # [B, heads, D] -> [B, D (row m of head(m)), D]
    part = lambda a, bm: _reduce(_partials(a, bm, B, dtype, drop), mut)
    dW_out, dW_v = part(g, ctx0), part(d_ctx0, per_row(xbar))
    dW_q, dW_k = part(dq0, x[:, 0]), part(q0, per_row(dt))
    db_out, db_v, db_q = part(None, g), part(None, d_ctx0), part(None, dq0)
    if mut == "db_out_dctx0":
        db_out = db_v
    db_k = db_v if mut == "db_k" else torch.zeros_like(db_q)
    return dict(q0=q0, t=t, probs=p, xbar=xbar, ctx0=ctx0, recent=recent, dx=dx, dW_in=torch.cat([dW_q, dW_k, dW_v]),
                db_in=torch.cat([db_q, db_k, db_v]), dW_out=dW_out, db_out=db_out)


# ------------------------------------------------------------------ cached inputs and references
_cache = {}


def _math_key(c):
    return (c.B, c.H, c.D, c.heads, c.cls, c.lens if c.lens in ("cycle", "bad") else None)


def case_inputs(c):
    k = _math_key(c)
    if k not in _cache:
        inp = inputs(c)
        _cache[k] = (inp, reference(inp))
    return _cache[k][0]


def case_reference(c):
    """reference() of a case's inputs, computed once per distinct (shape, class, lengths).  Leave it unchanged."""
    case_inputs(c)
    return _cache[_math_key(c)][1]


def distinct_cases():
    """CASES with those that repeat another's arithmetic (placements, lengths = NULL) dropped."""
    seen, out = set(), []
    for c in CASES:
        if _math_key(c) not in seen:
            seen.add(_math_key(c))
            out.append(c)
    return out


# ------------------------------------------------------------------ tolerances and the verdict
def tol(cls, name):
    """(a, m, r) of |got - ref| <= a + m max|ref| + r |ref|."""
    if cls == "flat" and name in FLAT_TOL:
        return FLAT_TOL[name]
    return (0.0, FACTOR * YARD[cls][name], RTOL[name])


ratio = AR.ratio


def normalised_error(got, ref, name):
    got, ref = got.detach().to("cpu", F64).reshape(ref.shape), ref.detach().to("cpu", F64)
    return float(((got - ref).abs() - RTOL[name] * ref.abs()).clamp_min(0.0).max()) / float(ref.abs().max())


def verdict(c, got, ref):
    """({name: worst |got - ref| / bound}, [what is not exactly as the header states it]) over the quantities in `got`."""
    D = c.D
    ratios = {n: ratio(got[n].reshape(ref[n].shape), ref[n], tol(c.cls, n)) for n in got}
    exact = []
    if "db_in" in got and float(got["db_in"].reshape(-1)[D:2 * D].abs().max()) != 0.0:
        exact.append("db_in[D:2D] != 0")
    _, lens = lengths_of(c)
    if lens is not None:
        pad = torch.arange(c.H)[None, :] >= torch.tensor(lens)[:, None]
        if "probs" in got and not bool((got["probs"].reshape(c.B, c.heads, c.H).cpu()[pad[:, None, :].expand(-1, c.heads, -1)] == 0).all()):
            exact.append("padded probs != 0")
        if "dx" in got and not bool((got["dx"].reshape(c.B, c.H, D).cpu()[pad] == 0).all()):
            exact.append("padded dx rows != 0")
    return ratios, exact


def rejected(c, got, ref):
    r, exact = verdict(c, got, ref)
    return bool(exact) or max(r.values()) > 1.0


def measure(cls):
    """Worst normalised error of the float32 evaluation per quantity over the class's cases, and where."""
    worst = {n: (0.0, None) for n in NAMES}
    for c in distinct_cases():
        if c.cls != cls:
            continue
        got, ref = collapsed(case_inputs(c), F32), case_reference(c)
        for n in NAMES:
            e = normalised_error(got[n], ref[n], n)
            if e >= worst[n][0]:
                worst[n] = (e, case_id(c))
    return worst


def round_up(v):
    """Two significant digits, upwards, never below 2^-24."""
    v = max(v, FLOOR)
    e = math.floor(math.log10(v)) - 1
    return math.ceil(v / 10 ** e - 1e-9) * 10 ** e


# ------------------------------------------------------------------ the GPU calls (test_gpu_encoder_last_reference.py)
class Guard:
    """A [rows, cols] fp32 view with row stride ld, `off` floats behind a 128-byte boundary of a NaN-filled buffer."""

    def __init__(self, dev, rows, cols, ld=None, off=0, fill=None):
        ld = ld or cols
        n = 32 + off + max(rows, 1) * ld + 32
        self.buf = torch.full((n,), float("nan"), dtype=F32, device=dev)
        assert self.buf.data_ptr() % 128 == 0
        self.view = self.buf.as_strided((rows, cols), (ld, 1), 32 + off)
        self.inside = torch.zeros(n, dtype=torch.bool, device=dev)
        self.inside.as_strided((rows, cols), (ld, 1), 32 + off).fill_(True)
        if fill is not None:
            self.view.copy_(fill.reshape(rows, cols))
        self.before = self.buf.clone()
        self.ptr = self.buf.data_ptr() + 4 * (32 + off)

    def get(self):
        return self.view.cpu()

    def outside_clean(self):
        return bool((self.buf.view(torch.int32) == self.before.view(torch.int32))[~self.inside].all())

    def unchanged(self):
        return bool((self.buf.view(torch.int32) == self.before.view(torch.int32)).all())


def same_bits(a, b):
    return all(bool((a[k].contiguous().view(torch.int32) == b[k].contiguous().view(torch.int32)).all()) for k in a)


def gpu_forward(c, inp, dev, len_entry=None, lengths="case"):
    """One forward call -> (rc, launches, {name: Guard}, operands).  len_entry: call tt_enc_last_fwd_len (default: when the
    case has lengths); lengths: "case" or None (NULL)."""
    from two_tower_models_amd import _native as N
    lib = N.load()
    B, H, D, heads, mis = c.B, c.H, c.D, c.heads, 1 if c.place else 0
    ops = dict(x=Guard(dev, B * H, D, fill=inp["x_fwd"]), w_in=Guard(dev, 3 * D, D, fill=inp["w_in"]),
               b_in=Guard(dev, 1, 3 * D, off=mis, fill=inp["b_in"]), w_out=Guard(dev, D, D, fill=inp["w_out"]),
               b_out=Guard(dev, 1, D, off=mis, fill=inp["b_out"]))
    ld_recent, off_recent = {0: (D, 0), 1: (D + 3, 1), 2: (2 * D, 0)}[c.place]
    outs = dict(recent=Guard(dev, B, D, ld=ld_recent, off=off_recent), q0=Guard(dev, B, D, off=mis), t=Guard(dev, B * heads, D),
                probs=Guard(dev, B * heads, H, off=mis), xbar=Guard(dev, B * heads, D), ctx0=Guard(dev, B, D, off=mis))
    use_len = (inp["lengths"] is not None) if len_entry is None else len_entry
    ln = torch.tensor(inp["lengths"], dtype=torch.int32, device=dev) if (use_len and lengths == "case" and inp["lengths"] is not None) else None
    tail = (ops["w_in"].ptr, ops["b_in"].ptr, ops["w_out"].ptr, ops["b_out"].ptr, outs["recent"].ptr, ld_recent, outs["q0"].ptr,
            outs["t"].ptr, outs["probs"].ptr, outs["xbar"].ptr, outs["ctx0"].ptr, N.stream())
    with Launches(KERNELS) as n:
        if use_len:
            rc = lib.tt_enc_last_fwd_len(ops["x"].ptr, B, H, D, heads, None if ln is None else ln.data_ptr(), *tail)
        else:
            rc = lib.tt_enc_last_fwd(ops["x"].ptr, B, H, D, heads, *tail)
    torch.cuda.synchronize()
    return rc, {k: v for k, v in n.items() if v}, outs, ops


def gpu_backward(c, inp, fwd, dev, mode, prev=None):
    """mode "halves": tt_enc_last_bwd_data then _weights (the workspace left alone in between); "whole": tt_enc_last_bwd.
    prev: the outputs and workspace of an earlier call to run into again.  The workspace is NaN-filled and exactly
    tt_enc_last_bwd_workspace_bytes long inside a larger NaN buffer."""
    from two_tower_models_amd import _native as N
    lib = N.load()
    B, H, D, heads = c.B, c.H, c.D, c.heads
    nb = lib.tt_enc_last_bwd_workspace_bytes(B, H, D, heads)
    if prev is None:
        ld_dr = 2 * D if c.place else D
        ops = dict(x=Guard(dev, B * H, D, fill=inp["x_bwd"]), w_in=Guard(dev, 3 * D, D, fill=inp["w_in"]),
                   w_out=Guard(dev, D, D, fill=inp["w_out"]), g=Guard(dev, B, D, ld=ld_dr, fill=inp["g"]))
        outs = dict(dx=Guard(dev, B * H, D), dW_in=Guard(dev, 3 * D, D), db_in=Guard(dev, 1, 3 * D), dW_out=Guard(dev, D, D),
                    db_out=Guard(dev, 1, D), ws=Guard(dev, 1, nb // 4))
    else:
        ops, outs = prev
    ld_dr = ops["g"].view.stride(0)
    f, o, ws = fwd, outs, outs["ws"]
    head = (ops["x"].ptr, B, H, D, heads)
    launches = {}
    if mode == "whole":
        with Launches(KERNELS) as n:
            rc = lib.tt_enc_last_bwd(*head, ops["w_in"].ptr, ops["w_out"].ptr, ops["g"].ptr, ld_dr, f["q0"].ptr, f["t"].ptr,
                                     f["probs"].ptr, f["xbar"].ptr, f["ctx0"].ptr, o["dx"].ptr, o["dW_in"].ptr, o["db_in"].ptr,
                                     o["dW_out"].ptr, o["db_out"].ptr, ws.ptr, nb, N.stream())
        launches["whole"] = {k: v for k, v in n.items() if v}
    else:
        with Launches(KERNELS) as n:
            rc = lib.tt_enc_last_bwd_data(*head, ops["w_in"].ptr, ops["w_out"].ptr, ops["g"].ptr, ld_dr, f["t"].ptr, f["probs"].ptr,
                                          o["dx"].ptr, ws.ptr, nb, N.stream())
        launches["data"] = {k: v for k, v in n.items() if v}
        with Launches(KERNELS) as n:
            rc2 = lib.tt_enc_last_bwd_weights(*head, ops["g"].ptr, ld_dr, f["q0"].ptr, f["xbar"].ptr, f["ctx0"].ptr, o["dW_in"].ptr,
                                              o["db_in"].ptr, o["dW_out"].ptr, o["db_out"].ptr, ws.ptr, nb, N.stream())
        launches["weights"] = {k: v for k, v in n.items() if v}
        rc = rc or rc2
    torch.cuda.synchronize()
    return rc, launches, outs, ops, nb


def workspace_bytes(B, H, D, heads):
    """tt_enc_last_bwd_workspace_bytes, from the header's layout: d_xbar, dt [B, heads, D], d_ctx0, dq0 [B, D], one partial
    of 2 D^2 + 2 D and one of 2 D^2 + D floats per 32 samples, each block rounded up to 256 bytes."""
    up = lambda v: (v + 255) // 256 * 256
    G = len(groups_of(B))
    return 2 * up(B * heads * D * 4) + 2 * up(B * D * 4) + up(G * (2 * D * D + 2 * D) * 4) + up(G * (2 * D * D + D) * 4)


def gpu_case(c, dev="cuda:0"):
    """Everything test_gpu_encoder_last_reference.py asserts of one case, as a dict."""
    inp, ref = case_inputs(c), case_reference(c)
    has_len = inp["lengths"] is not None
    res = {"id": case_id(c), "cls": c.cls, "group": c.group}
    rc, n, fo, fops = gpu_forward(c, inp, dev, len_entry=True if c.lens == "null" else None, lengths=None if c.lens == "null" else "case")
    res["rc_fwd"], res["launches_fwd"] = rc, n
    res["want_fwd"] = {K_PRE: 1, (K_MAIN_LEN if has_len else K_MAIN): 1, K_POST: 1}
    got = {k: fo[k].get() for k in FWD_NAMES}
    clean = all(g.outside_clean() for g in fo.values()) and all(g.unchanged() for g in fops.values())
    if c.lens == "null":  # lengths = NULL: the very bits of the call without `_len`
        rc0, n0, fo0, _ = gpu_forward(c, inp, dev, len_entry=False)
        res["null_same"] = rc0 == 0 and n0 == res["want_fwd"] and same_bits(got, {k: fo0[k].get() for k in FWD_NAMES})
    halves = gpu_backward(c, inp, fo, dev, "halves")
    whole = gpu_backward(c, inp, fo, dev, "whole")
    first = {k: whole[2][k].get() for k in GRADS}
    again = gpu_backward(c, inp, fo, dev, "whole", prev=(whole[3], whole[2]))
    res["rc_bwd"] = [halves[0], whole[0], again[0]]
    res["launches_bwd"] = dict(halves[1], **whole[1], again=again[1]["whole"])
    res["want_bwd"] = {"data": {K_A: 1, K_BWD: 1, K_B: 1}, "weights": {K_WGRAD: 1, K_REDUCE: 1},
                       "whole": {K_A: 1, K_BWD: 1, K_B: 1, K_WGRAD: 1, K_REDUCE: 1}}
    res["want_bwd"]["again"] = res["want_bwd"]["whole"]
    res["ws_bytes"], res["ws_want"] = halves[4], workspace_bytes(c.B, c.H, c.D, c.heads)
    got.update({k: halves[2][k].get() for k in GRADS})
    res["halves_same"] = same_bits({k: got[k] for k in GRADS}, first)
    res["repeat_same"] = same_bits(first, {k: again[2][k].get() for k in GRADS})
    for run in (halves, whole):
        clean = clean and all(g.outside_clean() for g in run[2].values()) and all(g.unchanged() for g in run[3].values())
    clean = clean and all(g.outside_clean() for g in fo.values())
    clean = clean and same_bits({k: got[k] for k in FWD_NAMES}, {k: fo[k].get() for k in FWD_NAMES})  # the backward leaves them alone
    res["clean"] = clean
    res["finite"] = all(bool(torch.isfinite(v).all()) for v in got.values())
    res["ratios"], res["exact"] = verdict(c, got, ref)
    return res


def gpu_line(res):
    r = res["ratios"]
    return f"enc-last-ref {res['id']} err/bound " + " ".join(f"{n} {r[n]:.3f}" for n in NAMES)


def assert_gpu_case(c, res):
    assert res["rc_fwd"] == 0 and res["rc_bwd"] == [0, 0, 0], res
    assert res["launches_fwd"] == res["want_fwd"], (res["launches_fwd"], res["want_fwd"])
    assert res["launches_bwd"] == res["want_bwd"], (res["launches_bwd"], res["want_bwd"])
    assert res["ws_bytes"] == res["ws_want"], (res["ws_bytes"], res["ws_want"])
    assert res["finite"], res["id"]
    assert not res["exact"], res["exact"]
    assert max(res["ratios"].values()) <= 1.0, res["ratios"]
    assert res["clean"], "a byte outside an output view, or past the reported workspace size, changed"
    assert res["halves_same"], "tt_enc_last_bwd != _data then _weights bit for bit"
    assert res["repeat_same"], "a second backward call gave other bits"
    assert res.get("null_same", True), "lengths = NULL is not the call without _len bit for bit"


def main():
    print("float32 CPU evaluation against float64: worst max((|err| - r |ref|)+) / max|ref| per class and quantity")
    ok = True
    for cls in CLASSES:
        w = measure(cls)
        print(cls)
        for n in NAMES:
            y = YARD[cls][n]
            ok = ok and w[n][0] <= y
            print(f"  {n:<7} measured {w[n][0]:.3e}  rounded up {round_up(w[n][0]):.1e}  recorded {y:.1e}  m = {tol(cls, n)[1]:.2e}   {w[n][1]}")
    assert ok, "YARD is below the measured worst case"


if __name__ == "__main__":
    sys.exit(main())
