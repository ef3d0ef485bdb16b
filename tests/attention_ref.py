"""Float64 yardstick for the attention kernels (csrc/attention.hip, attention_mfma.hip, attention_wg.hip).  A helper, not
a test: imported by test_attention_reference_cpu.py and test_gpu_attention.py the way adam_ref.py is imported by its tests;
the product never imports it.

  forward / backward   the kernels' own formulas (row max, lse = max + log(sum); P = exp(S - lse), delta_i = dO_i . O_i,
                       dS = P (dP - delta)) over the packed qkv [B*H, 3D], vectorised over samples and heads, in the
                       dtype of the input: float64 (matmul) or float32 (one rounding per multiply and per add, summed in
                       index order, exp and log correctly rounded -- no BLAS, no vector-width dependent summation, no host
                       math library in float32: the same bits on every IEEE machine).  `mut` names a deliberately wrong formula.
  reference            float64 forward + torch autograd: what the GPU tests compare against.
  inputs               the three input classes, from fixture_gen.gaussianish:
                         flat     scale 0.6: logits of s.d. ~0.4, every softmax nearly uniform (the older tests' inputs)
                         peaked   scale 3:   logits of s.d. ~9, rows near one-hot
                         shifted  flat + a common component c u (u = ones / sqrt(dh), c^2 / sqrt(dh) = 200) on Q and
                                  +-c u on K: every logit of an even sample sits near +200, of an odd sample near -200.
                                  Without the max subtraction fp32 exp overflows in the first and the row sum underflows
                                  to zero in the second.
  CASES / tol / ratio  the shapes test_gpu_attention.py runs, per group, and the tolerance each (family, class, quantity)
                       is held to -- shared with the CPU tests, which measure the yardstick and run the mutants at the
                       very same shapes.

Tolerances.  |got - ref| <= a + m * max|ref| + r * |ref| element-wise.
  flat ctx and d_qkv keep the project's figures (tests/test_gpu_history_lengths.py): ctx a = 2e-6, r = 1e-5;
  d_qkv a = 1e-7, m = 2e-6, r = 2e-4.
  Everything else (lse of every class; ctx and d_qkv of peaked and shifted): a = 0, the same r (0 for lse), and
  m = 4 x YARD[family][class][quantity], where YARD is the worst max((|fp32 - f64| - r |f64|)+) / max|f64| of the float32
  CPU evaluation above over the family's cases -- measured by `python tests/attention_ref.py`, rounded up to two digits,
  never below 2^-24 (half an ulp of max|ref|: no fp32 result can be held tighter), and re-measured by
  test_attention_reference_cpu.py.  The factor 4 is the Adam reference's: the hardware's 1-ulp exp, log and reciprocal and
  another summation order (matrix cores, fmaf chains).  profiles/attention_reference_tolerance.txt records the table and
  what the GPU showed."""
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
CLASSES = ("flat", "peaked", "shifted")
RTOL = {"ctx": 1e-5, "lse": 0.0, "dqkv": 2e-4}
FLAT_TOL = {"ctx": (2e-6, 0.0, 1e-5), "dqkv": (1e-7, 2e-6, 2e-4)}
FLOOR = 2.0 ** -24
FACTOR = 4.0

# worst normalised error of the float32 CPU evaluation against float64 per (family, class): see main()
YARD = {
    "wg": {"flat": {"ctx": 1.6e-07, "lse": 1.8e-07, "dqkv": 1.6e-07},
           "peaked": {"ctx": 2.9e-06, "lse": 2.7e-07, "dqkv": 8.8e-07}},
    "mfma": {"flat": {"ctx": 1.4e-07, "lse": 2.5e-07, "dqkv": 1.6e-07},
             "peaked": {"ctx": 1.8e-06, "lse": 2.9e-07, "dqkv": 1.2e-06},
             "shifted": {"ctx": 3.0e-05, "lse": 2.5e-07, "dqkv": 1.4e-05}},
    "valu": {"flat": {"ctx": 1.7e-07, "lse": 2.0e-07, "dqkv": 3.9e-07},
             "peaked": {"ctx": 1.2e-06, "lse": 2.3e-07, "dqkv": 1.3e-06},
             "shifted": {"ctx": 4.1e-05, "lse": 3.1e-07, "dqkv": 1.1e-05}},
}


# ------------------------------------------------------------------ the cases of test_gpu_attention.py: (B, H, D, heads, class)
WG_H = (1, 2, 8, 9, 31, 32, 33, 47, 48, 49, 50)
WG_EDGES = [(2, H, 128, 4, c) for H in WG_H for c in ("flat", "peaked")]
TRIP_B = (257, 512, 513, 769)
WG_TRIPS = [(B, H, 128, 4, c) for H in (50, 49, 33) for B in TRIP_B for c in (("flat", "peaked") if H == 50 else ("flat",))]
ALIGN = (2, 50, 128, 4, "flat")
THREE = (9, 50, 128, 4, "flat")
MFMA_H = (1, 31, 32, 33, 63, 64)
# B * heads = 3, 5, 9 pairs: a tail block for 4 waves per block and for the dh = 64 backward's 2; 32 pairs of 16 heads
MFMA = ([(B, H, D, heads, c) for (B, heads, D) in ((3, 1, 64), (5, 1, 32), (3, 3, 48)) for H in MFMA_H for c in CLASSES]
        + [(2, 64, 256, 16, c) for c in CLASSES])
# shapes next to the matrix-core class that the VALU pair takes: H = 65 at dh = 32; 16 heads of dh = 8
MFMA_EDGE_VALU = [(5, 65, 32, 1, c) for c in CLASSES] + [(2, 64, 128, 16, c) for c in CLASSES]
VALU_LONG = [(1, H, 8, 2, c) for H in (255, 256, 257, 300) for c in CLASSES] + [(1, 300, 32, 2, c) for c in CLASSES]
VALU_DH = (1, 4, 5, 16, 17, 33, 65, 128)
VALU_WIDTH = [(2, 7, 2 * dh, 2, c) for dh in VALU_DH for c in CLASSES]
LDS_REFUSED = (1, 700, 16, 1, "flat")  # backward LDS (4 H dhp + 2 H) 4 = 184 800 B > 160 KiB; the forward's 89 600 B fit
FAMILY_CASES = {"wg": WG_EDGES + WG_TRIPS + [ALIGN, THREE],
                "mfma": MFMA,
                "valu": MFMA_EDGE_VALU + VALU_LONG + VALU_WIDTH + [LDS_REFUSED]}


def case_id(case):
    B, H, D, heads, c = case
    return f"B{B}-H{H}-D{D}-h{heads}-{c}"


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def inputs(case):
    """fp32 (qkv [B*H, 3D], d_ctx [B*H, D]) of a case.  The seed leaves B out and the values are a hash of the element
    index, so a smaller batch of the same (H, D, heads, class) is a PREFIX of a larger one (and so is its reference)."""
    B, H, D, heads, cls = case
    dh = D // heads
    seed = 7000 + 131 * H + 7 * D + heads
    scale = {"flat": 0.6, "peaked": 3.0, "shifted": 0.6}[cls]
    qkv = T(fg.gaussianish((B * H, 3 * D), seed)) * scale
    d_ctx = T(fg.gaussianish((B * H, D), seed + 1))
    if cls == "shifted":
        c = math.sqrt(200.0 * math.sqrt(dh)) / math.sqrt(dh)  # each of the dh components of c u
        sign = torch.where(torch.arange(B) % 2 == 0, 1.0, -1.0).repeat_interleave(H)[:, None]
        qkv[:, :D] += c
        qkv[:, D:2 * D] += sign * c
    return qkv.contiguous(), d_ctx.contiguous()


# ------------------------------------------------------------------ the formulas
def _split(t, B, H, heads):
    return t.reshape(B, H, heads, -1).permute(0, 2, 1, 3)


def _rows(t):
    B, heads, H, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * H, heads * dh)


def _nt(a, b):
    """[..., n, d] x [..., m, d] -> [..., n, m], reduced over d."""
    if a.dtype == F64:
        return a @ b.transpose(-1, -2)
    acc = torch.zeros(*a.shape[:-1], b.shape[-2], dtype=a.dtype)
    for i in range(a.shape[-1]):
        acc = acc + a[..., :, None, i] * b[..., None, :, i]
    return acc


def _nn(p, v):
    """[..., n, m] x [..., m, d] -> [..., n, d], reduced over m."""
    if p.dtype == F64:
        return p @ v
    acc = torch.zeros(*p.shape[:-1], v.shape[-1], dtype=p.dtype)
    for j in range(p.shape[-1]):
        acc = acc + p[..., :, j, None] * v[..., None, j, :]
    return acc


def _exp(x):
    """exp in x's dtype; float32: the correctly rounded one (float64's, rounded), not the host library's 1-ulp vector form."""
    return torch.exp(x) if x.dtype == F64 else torch.exp(x.double()).to(x.dtype)


def _log(x):
    return torch.log(x) if x.dtype == F64 else torch.log(x.double()).to(x.dtype)


def _sum(x):
    if x.dtype == F64:
        return x.sum(dim=-1)
    acc = torch.zeros(x.shape[:-1], dtype=x.dtype)
    for j in range(x.shape[-1]):
        acc = acc + x[..., j]
    return acc


FORWARD_MUTANTS = ("scale", "lse_no_max", "keys32")
BACKWARD_MUTANTS = ("stale_k", "stale_q", "stale_do", "delta_48_49")


def forward(qkv, B, H, D, heads, mut=None):
    """-> (ctx [B*H, D], lse [B, heads, H]) in qkv's dtype.  mut: "scale" 1 / sqrt(dh + 1); "lse_no_max" the max is not
    added back; "keys32" keys >= 32 take no part."""
    dh = D // heads
    scale = 1.0 / math.sqrt(dh + 1 if mut == "scale" else dh)
    q, k, v = (_split(qkv[:, i * D:(i + 1) * D], B, H, heads) for i in range(3))
    s = _nt(q * scale, k)
    if mut == "keys32":
        s = torch.cat([s[..., :32], torch.full_like(s[..., 32:], float("-inf"))], dim=-1)
    mx = s.max(dim=-1, keepdim=True).values
    p = _exp(s - mx)
    l = _sum(p)
    ctx = _rows(_nn(p / l[..., None], v))
    lse = _log(l) if mut == "lse_no_max" else mx[..., 0] + _log(l)
    return ctx, lse


def backward(qkv, ctx, lse, d_ctx, B, H, D, heads, mut=None):
    """d_qkv [B*H, 3D] from the saved ctx and lse, as the kernels form it.  mut: "scale", "keys32" as above;
    "stale_k" / "stale_q" / "stale_do": sample b >= 256 takes that operand's rows from sample b - 256 (what a persistent
    workgroup of a 256-wide grid still holds from its previous trip); "delta_48_49": rows 48 and 49 have no part in
    delta_i = dO_i . O_i (the remainder rows of the workgroup kernel's staging)."""
    dh = D // heads
    scale = 1.0 / math.sqrt(dh + 1 if mut == "scale" else dh)
    q, k, v = (_split(qkv[:, i * D:(i + 1) * D], B, H, heads) for i in range(3))
    g, o = _split(d_ctx, B, H, heads), _split(ctx, B, H, heads)
    if mut in ("stale_k", "stale_q", "stale_do"):
        idx = torch.arange(B)
        idx[256:] -= 256
        if mut == "stale_k":
            k = k[idx]
        elif mut == "stale_q":
            q = q[idx]
        else:
            g = g[idx]
    qs = q * scale
    P = _exp(_nt(qs, k) - lse[..., None])
    if mut == "keys32":
        P = torch.cat([P[..., :32], torch.zeros_like(P[..., 32:])], dim=-1)
    dP = _nt(g, v)
    delta = _sum(g * o)
    if mut == "delta_48_49":
        delta = torch.cat([delta[..., :48], torch.zeros_like(delta[..., 48:50]), delta[..., 50:]], dim=-1)
    dS = P * (dP - delta[..., None])
    dq = _nn(dS, k) * scale
    dk = _nn(dS.transpose(-1, -2), qs)
    dv = _nn(P.transpose(-1, -2), g)
    return torch.cat([_rows(dq), _rows(dk), _rows(dv)], dim=1)


def evaluate(qkv, d_ctx, B, H, D, heads, dtype, mut=None):
    """Forward, then the backward on the forward's own ctx and lse, all in `dtype` -> (ctx, lse, d_qkv).
    mut "last_pair": the correct result with the last (sample, head) pair's outputs left at the sentinel."""
    x, g = qkv.to(dtype), d_ctx.to(dtype)
    ctx, lse = forward(x, B, H, D, heads, mut if mut in FORWARD_MUTANTS else None)
    dq = backward(x, ctx, lse, g, B, H, D, heads, mut if mut != "lse_no_max" else None)
    if mut == "last_pair":
        dh = D // heads
        ctx, lse, dq = ctx.clone(), lse.clone(), dq.clone()
        ctx[(B - 1) * H:, D - dh:] = SENTINEL
        lse[B - 1, heads - 1] = SENTINEL
        for t in range(3):
            dq[(B - 1) * H:, (t + 1) * D - dh:(t + 1) * D] = SENTINEL
    return ctx, lse, dq


def reference(qkv, d_ctx, B, H, D, heads):
    """float64 (ctx, lse, d_qkv): the vectorised forward and torch autograd through it."""
    x = qkv.detach().to("cpu", F64).requires_grad_(True)
    ctx, lse = forward(x, B, H, D, heads)
    (dq,) = torch.autograd.grad((ctx * d_ctx.detach().to("cpu", F64)).sum(), [x])
    return ctx.detach(), lse.detach(), dq


_ref_cache = {}


def _cached(case):
    B, H, D, heads, cls = case
    key = (H, D, heads, cls)
    if key not in _ref_cache or _ref_cache[key][0] < B:
        Bmax = max([c[0] for cases in FAMILY_CASES.values() for c in cases if c[1:] == case[1:]] + [B])
        qkv, d_ctx = inputs((Bmax,) + tuple(case[1:]))
        _ref_cache[key] = (Bmax, qkv, d_ctx) + reference(qkv, d_ctx, Bmax, H, D, heads)
    return _ref_cache[key]


def case_inputs(case):
    """inputs(case), cut from the cached largest batch of its (H, D, heads, class)."""
    B, H = case[0], case[1]
    _, qkv, d_ctx, _, _, _ = _cached(case)
    return qkv[:B * H], d_ctx[:B * H]


def case_reference(case):
    """reference() of a case's inputs, computed once per (H, D, heads, class) at the largest batch any group runs it with
    and sliced: samples are independent and a smaller batch's inputs are a prefix (see inputs).  Leave it unchanged."""
    B, H = case[0], case[1]
    _, _, _, ctx, lse, dq = _cached(case)
    return {"ctx": ctx[:B * H], "lse": lse[:B], "dqkv": dq[:B * H]}


# ------------------------------------------------------------------ tolerances
def family_of(case):
    for fam, cases in FAMILY_CASES.items():
        if tuple(case) in cases:
            return fam
    raise KeyError(case)


def tol(family, cls, name):
    """(a, m, r) of |got - ref| <= a + m max|ref| + r |ref|."""
    if cls == "flat" and name in FLAT_TOL:
        return FLAT_TOL[name]
    return (0.0, FACTOR * YARD[family][cls][name], RTOL[name])


def ratio(got, ref, t):
    """Worst |got - ref| / bound over every element (NaN counts as inf); <= 1 means within tolerance."""
    got, ref = got.detach().to("cpu", F64), ref.detach().to("cpu", F64)
    bound = t[0] + t[1] * float(ref.abs().max()) + t[2] * ref.abs()
    q = (got - ref).abs() / bound
    return float(torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q).max())


def ratios(got, ref, family, cls):
    """{"ctx": .., "lse": .., "dqkv": ..} of a result triple / dict against case_reference's dict."""
    if not isinstance(got, dict):
        got = dict(zip(("ctx", "lse", "dqkv"), got))
    return {n: ratio(got[n], ref[n], tol(family, cls, n)) for n in got}


def normalised_error(got, ref, name):
    """The yardstick's unit: max((|got - ref| - r |ref|)+) / max|ref|."""
    got, ref = got.detach().to("cpu", F64), ref.detach().to("cpu", F64)
    return float(((got - ref).abs() - RTOL[name] * ref.abs()).clamp_min(0.0).max()) / float(ref.abs().max())


def yardstick_cases(family):
    """The family's cases with every batch below the largest of its (H, D, heads, class) dropped: the smaller batches are
    prefixes of the largest, so its worst error covers theirs."""
    best = {}
    for c in FAMILY_CASES[family]:
        if c[1:] not in best or best[c[1:]][0] < c[0]:
            best[c[1:]] = c
    return sorted(best.values(), key=lambda c: (CLASSES.index(c[4]), c[2], c[3], c[1]))


def measure(family, cls):
    """Worst normalised error of the float32 evaluation per quantity over the family's cases of one class, and where."""
    worst = {"ctx": (0.0, None), "lse": (0.0, None), "dqkv": (0.0, None)}
    for case in yardstick_cases(family):
        if case[4] != cls:
            continue
        B, H, D, heads, _ = case
        qkv, d_ctx = case_inputs(case)
        ref = case_reference(case)
        got = dict(zip(("ctx", "lse", "dqkv"), evaluate(qkv, d_ctx, B, H, D, heads, F32)))
        for n in worst:
            e = normalised_error(got[n], ref[n], n)
            if e >= worst[n][0]:
                worst[n] = (e, case_id(case))
    return worst


def main():
    print("float32 CPU evaluation against float64: worst max((|err| - r |ref|)+) / max|ref| per family and class")
    print(f"{'family':<6} {'class':<8} {'ctx':>10} {'lse':>10} {'d_qkv':>10}   recorded (YARD)               worst case (d_qkv)")
    ok = True
    for fam in FAMILY_CASES:
        for cls in YARD[fam]:
            w = measure(fam, cls)
            y = YARD[fam][cls]
            print(f"{fam:<6} {cls:<8} {w['ctx'][0]:10.3e} {w['lse'][0]:10.3e} {w['dqkv'][0]:10.3e}   "
                  f"{y['ctx']:.1e} {y['lse']:.1e} {y['dqkv']:.1e}   {w['dqkv'][1]}")
            ok = ok and all(w[n][0] <= y[n] for n in y)
    assert ok, "YARD is below the measured worst case"


if __name__ == "__main__":
    main()
