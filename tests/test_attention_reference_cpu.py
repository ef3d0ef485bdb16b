"""The yardstick of test_gpu_attention.py can fail: attention_ref's vectorised float64 attention IS the per-sample form of
history_lengths_ref and nn.MultiheadAttention's functional form; the float32 evaluation of the same formulas stays within
the recorded yardstick (YARD) at every shape the GPU tests run; and every wrong formula a kernel could plausibly implement
falls outside the tolerances those tests use, at the very shape and input class where they run it -- while the unmutated
formula falls inside."""
import pytest
import torch

import attention_ref as AR
import history_lengths_ref as HR

F64 = torch.float64


@pytest.mark.parametrize("case", [(3, 50, 128, 4, "flat"), (2, 7, 34, 2, "peaked"), (4, 33, 48, 3, "shifted"), (2, 1, 8, 2, "flat")],
                         ids=AR.case_id)
def test_vectorised_reference_is_the_per_sample_core_and_multi_head_attention(case):
    """ctx, lse and d_qkv of attention_ref against (a) HR.attention_core with full lengths + autograd, logsumexp of the
    plain scores; (b) torch.nn.functional.multi_head_attention_forward on the same projection weights (output and the
    gradients of the input and of both projections, which pass through ctx and d_qkv); (c) the explicit backward formulas
    (the ones the float32 yardstick and the mutants are built from) against autograd.  float64, 1e-12 of max|.|."""
    B, H, D, heads, cls = case
    qkv, d_ctx = AR.inputs(case)
    ctx, lse, dq = AR.reference(qkv, d_ctx, B, H, D, heads)

    def same(a, b, what):
        err = float((a - b).abs().max()) / max(float(b.abs().max()), 1.0)
        assert err < 1e-12, (what, err)

    x = qkv.to(F64).requires_grad_(True)
    c2 = HR.attention_core(x, B, H, D, heads, [H] * B)
    (dq2,) = torch.autograd.grad((c2 * d_ctx.to(F64)).sum(), [x])
    same(ctx, c2.detach(), "ctx")
    same(dq, dq2, "d_qkv")
    dh = D // heads
    q, k = (AR._split(qkv.to(F64)[:, i * D:(i + 1) * D], B, H, heads) for i in range(2))
    same(lse, torch.logsumexp(q @ k.transpose(-1, -2) / dh ** 0.5, dim=-1), "lse")
    e = AR.evaluate(qkv, d_ctx, B, H, D, heads, F64)
    same(e[0], ctx, "explicit ctx")
    same(e[1], lse, "explicit lse")
    same(e[2], dq, "explicit d_qkv")
    # nn.MultiheadAttention's functional form around the core: qkv = x W_in^T + b_in, out = ctx W_out^T + b_out
    gen = torch.Generator().manual_seed(5)
    scale_in = {"flat": 0.6, "peaked": 3.0, "shifted": 0.6}[cls]
    leaves = [torch.randn(B, H, D, generator=gen, dtype=F64), torch.randn(3 * D, D, generator=gen, dtype=F64) * scale_in / D ** 0.5,
              torch.randn(3 * D, generator=gen, dtype=F64) * 0.3, torch.randn(D, D, generator=gen, dtype=F64) / D ** 0.5,
              torch.randn(D, generator=gen, dtype=F64) * 0.3]
    cot = torch.randn(B, H, D, generator=gen, dtype=F64)
    res = []
    for form in ("ours", "torch"):
        xs, w_in, b_in, w_out, b_out = (t.clone().requires_grad_(True) for t in leaves)
        if form == "ours":
            c, _ = AR.forward(xs.reshape(B * H, D) @ w_in.t() + b_in, B, H, D, heads)
            out = (c @ w_out.t() + b_out).reshape(B, H, D)
        else:
            xt = xs.transpose(0, 1)  # [H, B, D]
            out, _ = torch.nn.functional.multi_head_attention_forward(
                xt, xt, xt, D, heads, w_in, b_in, None, None, False, 0.0, w_out, b_out, training=False, need_weights=False)
            out = out.transpose(0, 1)
        res.append((out.detach(),) + torch.autograd.grad((out * cot).sum(), [xs, w_in, b_in, w_out, b_out]))
    for a, b, what in zip(res[0], res[1], ("out", "dx", "dW_in", "db_in", "dW_out", "db_out")):
        same(a, b, "multi_head_attention_forward " + what)


@pytest.mark.parametrize("family,cls", [(f, c) for f in AR.YARD for c in AR.YARD[f]])
def test_float32_evaluation_is_within_the_recorded_yardstick(family, cls):
    """The same formulas in float32 (index-order sums) against float64, every case of the family and class: the worst
    normalised error per quantity is what YARD records (rounded up) -- the number the GPU tolerances hang on."""
    worst = AR.measure(family, cls)
    y = AR.YARD[family][cls]
    print(f"yardstick {family:<5} {cls:<8} " + " ".join(f"{n} {worst[n][0]:.3e} (recorded {y[n]:.1e}, at {worst[n][1]})" for n in y))
    for n in y:
        assert worst[n][0] <= y[n], (n, worst[n], y[n])
        assert y[n] >= AR.FLOOR


def mutants_of(case, family):
    """(wrong formula, quantities, every) that differ from the right one at this case: outside the tolerance in every one of
    the quantities named, or (every = False) in at least one."""
    B, H, D, heads, cls = case
    out = [("scale", ("ctx", "lse", "dqkv"), False), ("lse_no_max", ("lse",), True), ("last_pair", ("ctx", "lse", "dqkv"), True)]
    if H >= 33:
        out.append(("keys32", ("ctx", "dqkv"), True))
    if family == "wg" and H >= 49:
        out.append(("delta_48_49", ("dqkv",), True))
    if family == "wg" and B > 256:
        out += [(m, ("dqkv",), True) for m in ("stale_k", "stale_q", "stale_do")]
    return out


ALL_CASES = [(f, c) for f in AR.FAMILY_CASES for c in AR.FAMILY_CASES[f]]


@pytest.mark.parametrize("family,case", ALL_CASES, ids=[f"{f}-{AR.case_id(c)}" for f, c in ALL_CASES])
def test_mutated_formulas_fall_outside_the_gpu_tolerances(family, case):
    """Every case of test_gpu_attention.py, with the tolerance it uses there.  A float64 (otherwise exact) evaluation of:
    the previous trip's K, Q or dO rows (sample b - 256) in sample b's gradient; rows 48 and 49 missing from delta; the
    scale 1 / sqrt(dh + 1); lse without the max; keys >= 32 dropped; the last (sample, head) pair unwritten -- each where it
    can differ (B > 256; H >= 49; everywhere; everywhere; H >= 33; everywhere) -- is outside the tolerance in the quantity
    named (for the scale: in at least one -- at H = 1 the softmax is 1 whatever the scale, and only lse sees it).  The
    unmutated float64 formula is inside by a factor > 100."""
    B, H, D, heads, cls = case
    qkv, d_ctx = AR.case_inputs(case)
    ref = AR.case_reference(case)
    good = AR.ratios(AR.evaluate(qkv, d_ctx, B, H, D, heads, F64), ref, family, cls)
    assert max(good.values()) < 1e-2, good
    for mut, names, every in mutants_of(case, family):
        r = AR.ratios(AR.evaluate(qkv, d_ctx, B, H, D, heads, F64, mut), ref, family, cls)
        print(f"{AR.case_id(case)} {mut:<12} err / bound: " + " ".join(f"{n} {r[n]:.3g}" for n in r))
        assert (min if every else max)(r[n] for n in names) > 1.0, (mut, r)
