"""Which library call each form of the in-batch softmax makes, on MI355X (`pytest -m gpu`): ops.InBatchSoftmaxCE and
ops.InBatchSoftmaxWeightedLoss over {no term, term} x {no keys, keys} x {no gradient, U and I, I alone}, forward and
backward under `_native.trace`, against the literal list of entry points -- the NARROWEST call for the form.  The values
of every form are checked against float64 elsewhere (test_gpu_ce_reference.py, test_gpu_ce_hits_reference.py); here only the
routing, and that the number of arguments given to `apply` does not matter."""
import pytest
import torch

from test_gpu_logq import DEV

pytestmark = pytest.mark.gpu

# (term, keys, gradients) -> the calls of one forward (and backward), in host order
CE_CALLS = {
    # no gradient: the forward alone
    ("-", "-", "none"): ["tt_inbatch_ce_fwd"],
    ("b", "-", "none"): ["tt_inbatch_ce_bias_fwd"],
    ("-", "k", "none"): ["tt_inbatch_ce_masked_fwd"],
    ("b", "k", "none"): ["tt_inbatch_ce_masked_fwd"],
    # U and I: the forward leaves du_unit, the backward scales it and runs the item side
    ("-", "-", "UI"): ["tt_inbatch_ce_fwd_du", "tt_scale_rows", "tt_inbatch_ce_bwd"],
    ("b", "-", "UI"): ["tt_inbatch_ce_bias_fwd", "tt_scale_rows", "tt_inbatch_ce_bias_bwd"],
    ("-", "k", "UI"): ["tt_inbatch_ce_masked_fwd", "tt_scale_rows", "tt_inbatch_ce_masked_bwd"],
    ("b", "k", "UI"): ["tt_inbatch_ce_masked_fwd", "tt_scale_rows", "tt_inbatch_ce_masked_bwd"],
    # I alone: no du_unit was saved, the recompute backward writes dU itself
    ("-", "-", "I"): ["tt_inbatch_ce_fwd", "tt_inbatch_ce_bwd"],
    ("b", "-", "I"): ["tt_inbatch_ce_bias_fwd", "tt_inbatch_ce_bias_bwd"],
    ("-", "k", "I"): ["tt_inbatch_ce_masked_fwd", "tt_inbatch_ce_masked_bwd"],
    ("b", "k", "I"): ["tt_inbatch_ce_masked_fwd", "tt_inbatch_ce_masked_bwd"],
}
KEPT_CALLS = {  # keep_logits=True at N >= 4 M, D = 128: the item side reads the logits the forward kept
    ("-", "-"): ["tt_inbatch_ce_fwd_du_keep", "tt_scale_rows", "tt_inbatch_ce_bwd_kept"],
    ("b", "-"): ["tt_inbatch_ce_bias_fwd", "tt_scale_rows", "tt_inbatch_ce_bwd_kept"],
    ("-", "k"): ["tt_inbatch_ce_masked_fwd", "tt_scale_rows", "tt_inbatch_ce_bwd_kept"],
    ("b", "k"): ["tt_inbatch_ce_masked_fwd", "tt_scale_rows", "tt_inbatch_ce_bwd_kept"],
}
LOSS_CALLS = {
    ("-", "-"): ["tt_inbatch_ce_fwd_du_loss", "tt_scale_rows_g", "tt_inbatch_ce_bwd"],
    ("b", "-"): ["tt_inbatch_ce_bias_fwd", "tt_scale_rows_g", "tt_inbatch_ce_bias_bwd"],
    ("-", "k"): ["tt_inbatch_ce_masked_fwd", "tt_scale_rows_g", "tt_inbatch_ce_masked_bwd"],
    ("b", "k"): ["tt_inbatch_ce_masked_fwd", "tt_scale_rows_g", "tt_inbatch_ce_masked_bwd"],
}
FORMS = [("-", "-"), ("b", "-"), ("-", "k"), ("b", "k")]


def operands(M, Nn, D, term, keys, grads):
    g = torch.Generator().manual_seed(1000 * M + Nn + D)
    U = (0.3 * torch.randn(M, D, generator=g)).to(DEV).requires_grad_(grads == "UI")
    I = (0.3 * torch.randn(Nn, D, generator=g)).to(DEV).requires_grad_(grads in ("UI", "I"))
    b = torch.randn(Nn, generator=g).to(DEV) if term == "b" else None
    k = (torch.arange(Nn, dtype=torch.int32) % 61).to(DEV) if keys == "k" else None
    return U, I, b, k


def traced(fn):
    from two_tower_models_amd import _native as N
    N.trace = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, list(N.trace)
    finally:
        N.trace = None


def run_ce(U, I, *rest):
    from two_tower_models_amd import ops
    ce = ops.InBatchSoftmaxCE.apply(U, I, *rest)
    if ce.requires_grad:
        ce.sum().backward()
    return ce.detach(), U.grad, I.grad


@pytest.mark.parametrize("grads", ["none", "UI", "I"])
@pytest.mark.parametrize("term,keys", FORMS)
def test_row_ce_calls_the_narrowest_entry_point(term, keys, grads):
    """130 x 130, D = 32: two row blocks, an edge tile; N < 4 M, so the logits are recomputed."""
    U, I, b, k = operands(130, 130, 32, term, keys, grads)
    _, calls = traced(lambda: run_ce(U, I, 0, None, b, k))
    assert calls == CE_CALLS[(term, keys, grads)]


@pytest.mark.parametrize("term,keys", FORMS)
def test_row_ce_with_kept_logits(term, keys):
    U, I, b, k = operands(130, 700, 128, term, keys, "UI")
    _, calls = traced(lambda: run_ce(U, I, 0, True, b, k))
    assert calls == KEPT_CALLS[(term, keys)]


@pytest.mark.parametrize("term,keys", FORMS)
def test_fused_loss_calls_the_narrowest_entry_point(term, keys):
    from two_tower_models_amd import ops
    U, I, b, k = operands(130, 130, 32, term, keys, "UI")
    labels = torch.rand(130, 2, generator=torch.Generator().manual_seed(5)).to(DEV)
    uvw = torch.tensor([1.0, 0.5], device=DEV)
    _, calls = traced(lambda: ops.InBatchSoftmaxWeightedLoss.apply(U, I, labels, uvw, b, k).backward())
    assert calls == LOSS_CALLS[(term, keys)]
    assert U.grad is not None and I.grad is not None


@pytest.mark.parametrize("grads", ["none", "UI", "I"])
def test_trailing_none_arguments_change_nothing(grads):
    """apply(U, I, 0) and apply(U, I, 0, None, None, None): the same call, the same bits."""
    from two_tower_models_amd import ops
    res = []
    for rest in ((0,), (0, None, None, None)):
        U, I, _, _ = operands(130, 130, 32, "-", "-", grads)
        res.append(traced(lambda: run_ce(U, I, *rest)))
    (short, calls_short), (full, calls_full) = res
    assert calls_short == calls_full == CE_CALLS[("-", "-", grads)]
    for a, c in zip(short, full):
        assert (a is None and c is None) or torch.equal(a, c)
    if grads == "UI":
        labels, uvw = torch.ones(130, 1, device=DEV), torch.ones(1, device=DEV)
        out = []
        for rest in ((), (None, None)):
            U, I, _, _ = operands(130, 130, 32, "-", "-", grads)
            loss = ops.InBatchSoftmaxWeightedLoss.apply(U, I, labels, uvw, *rest)
            loss.backward()
            out.append((loss.detach(), U.grad, I.grad))
        assert all(torch.equal(a, c) for a, c in zip(*out))
