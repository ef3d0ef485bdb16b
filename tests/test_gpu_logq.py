"""Log-Q sampling-bias correction and mixed negatives on MI355X (`pytest -m gpu`): the per-item logit term inside the
in-batch softmax kernels, from the C ABI up to `train_forward`, against torch-CPU expressions on top of oracle.cpu_ref:

    scores = R.inbatch_logits(U, I) + b[None, :];  F.cross_entropy(scores, arange(M) + off, reduction="none");  autograd

The term is b = -log q of a Zipf(1.0) popularity over 10^6 items taken at N seeded ids (2.7 .. 16.5), or a signed vector
scaled to +-30.  Tolerances are the unbiased kernels' own (tests/test_gpu_kernels.py): row_ce atol 2e-5 / rtol 1e-5,
gradients 1e-5 * max|g| + rtol 1e-4; the +-30 case takes test_inbatch_ce_large_logits_stable's (fp64 reference, atol 1e-3,
rtol 1e-5).  The float32 oracle itself, measured on the CPU against its float64 twin over every shape of KERNEL_SHAPES with
both terms (inputs scaled 0.5): at most 0.071 of the row_ce bound and 1.31e-6 * max|g| on the gradients, i.e. under a
seventh of either bound (worst case of both: (130, 700, 200, off 400) with the Zipf term)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fixture_gen as fg
from ce_ref import signed_bias, zipf_bias  # the two terms (shared with the float64 CE reference's cases)
from oracle import cpu_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (M, N, D, off): D = 128 aligned (LDS-DMA form), 40 / 50 (register-staged form), 2, 200 / 256 (ce_wide), ragged M,
# N > M with off > 0, N not a multiple of 64, one row, and several splits
KERNEL_SHAPES = [(256, 256, 128, 0), (1000, 1000, 128, 0), (200, 200, 40, 0), (130, 700, 50, 400), (64, 64, 2, 0),
                 (300, 300, 256, 0), (130, 700, 200, 400), (128, 512, 128, 256), (77, 203, 128, 50), (100, 300, 64, 200),
                 (1, 1, 8, 0), (8192, 8192, 128, 0)]


@pytest.fixture(scope="module")
def T():
    from two_tower_models_amd import _native as N
    from two_tower_models_amd import ops
    N.load()
    return ops, N


def g(shape, seed):
    return torch.from_numpy(fg.gaussianish(shape, seed))


def oracle_rows(U, I, b, off):
    scores = R.inbatch_logits(U, I) + b[None, :]
    return F.cross_entropy(scores, torch.arange(U.shape[0]) + off, reduction="none")


def oracle(U, I, b, off, coef, dtype=torch.float32):
    U, I = U.detach().to(dtype).requires_grad_(True), I.detach().to(dtype).requires_grad_(True)
    ce = oracle_rows(U, I, b.to(dtype), off)
    (ce * coef.to(dtype)).sum().backward()
    return ce.detach(), U.grad, I.grad


def close_grad(got, want, rtol=1e-4):
    return torch.allclose(got.cpu().to(want.dtype), want, atol=1e-5 * float(want.abs().max()) + 1e-9, rtol=rtol)


def _ld(t):
    """Leading dimension of a row-major (possibly row-strided) [rows, D] view."""
    return max(t.stride(0), t.shape[1])


def abi_workspace(T, M, Nn, D):
    """The scratch tensor the abi_* helpers hand to the library (at least the biased calls' size)."""
    ops, N = T
    return N.scratch.get(torch.device(DEV), N.load().tt_inbatch_ce_bias_workspace_bytes(M, Nn, D), "logq_test")


def abi_fwd(T, U, I, off, bias, form="plain", labels=None, uvw=None, *, entry="bias", du_unit=None, logits=None, fill=None):
    """tt_inbatch_ce_bias_fwd in one of its forms; bias None = NULL.  Returns a dict of its outputs.
    U, I (and du_unit, if given: a preallocated output view) may be row-strided views: their row stride is the leading
    dimension passed.  entry="plain": the calls without the term argument (tt_inbatch_ce_fwd, _fwd_du, _fwd_du_keep,
    _fwd_du_loss) instead.  logits: a preallocated buffer of at least tt_inbatch_ce_logits_bytes.  fill: the value the
    outputs allocated here hold before the call (default: uninitialised)."""
    ops, N = T
    lib = N.load()
    M, D = U.shape
    Nn = I.shape[0]
    e = lambda *shape: torch.empty(*shape, device=DEV) if fill is None else torch.empty(*shape, device=DEV).fill_(fill)
    out = dict(lse=e(M), ce=e(M))
    wsp, wsn = ops._ws(torch.device(DEV), lib.tt_inbatch_ce_bias_workspace_bytes(M, Nn, D), "logq_test")
    du = None
    zn = 0
    tail = (None, 1, None, None, None, None)
    if form != "plain":
        du = out["du_unit"] = e(M, D) if du_unit is None else du_unit
    if form == "keep":
        zn = lib.tt_inbatch_ce_logits_bytes(M, Nn)
        logits = out["logits"] = torch.empty(zn, dtype=torch.uint8, device=DEV) if logits is None else logits
    else:
        logits = None
    if form == "loss":
        out.update(w=e(M), coef=e(M), loss=e(()))
        tail = (N.ptr(labels), labels.shape[1] if labels is not None else 1, uvw.data_ptr(), out["w"].data_ptr(),
                out["coef"].data_ptr(), out["loss"].data_ptr())
    ld_du = _ld(du) if du is not None else D
    head = (U.data_ptr(), _ld(U), I.data_ptr(), _ld(I), M, Nn, D, off)
    stats = (out["lse"].data_ptr(), out["ce"].data_ptr())
    if entry == "bias":
        N.check(lib.tt_inbatch_ce_bias_fwd(*head, N.ptr(bias), *stats, N.ptr(du), ld_du, N.ptr(logits), zn, *tail, wsp, wsn,
                                           N.stream()), "tt_inbatch_ce_bias_fwd")
        return out
    assert entry == "plain" and bias is None
    if form == "plain":
        N.check(lib.tt_inbatch_ce_fwd(*head, *stats, wsp, wsn, N.stream()), "tt_inbatch_ce_fwd")
    elif form == "du":
        N.check(lib.tt_inbatch_ce_fwd_du(*head, *stats, du.data_ptr(), ld_du, wsp, wsn, N.stream()), "tt_inbatch_ce_fwd_du")
    elif form == "keep":
        N.check(lib.tt_inbatch_ce_fwd_du_keep(*head, *stats, du.data_ptr(), ld_du, logits.data_ptr(), zn, wsp, wsn, N.stream()),
                "tt_inbatch_ce_fwd_du_keep")
    else:
        N.check(lib.tt_inbatch_ce_fwd_du_loss(*head, tail[0], tail[1], tail[2], *stats, du.data_ptr(), ld_du, *tail[3:], wsp, wsn,
                                              N.stream()), "tt_inbatch_ce_fwd_du_loss")
    return out


def abi_bwd(T, U, I, off, bias, lse, coef, with_du=True, *, entry="bias", dU=None, dI=None):
    """tt_inbatch_ce_bias_bwd (entry="plain": tt_inbatch_ce_bwd); U, I and the preallocated dU / dI may be row-strided."""
    ops, N = T
    lib = N.load()
    M, D = U.shape
    Nn = I.shape[0]
    wsp, wsn = ops._ws(torch.device(DEV), lib.tt_inbatch_ce_bias_workspace_bytes(M, Nn, D), "logq_test")
    if with_du and dU is None:
        dU = torch.empty(M, D, device=DEV)
    dU = dU if with_du else None
    dI = torch.empty(Nn, D, device=DEV) if dI is None else dI
    head = (U.data_ptr(), _ld(U), I.data_ptr(), _ld(I), M, Nn, D, off)
    rest = (lse.data_ptr(), coef.data_ptr(), N.ptr(dU), _ld(dU) if dU is not None else D, dI.data_ptr(), _ld(dI), wsp, wsn, N.stream())
    if entry == "bias":
        N.check(lib.tt_inbatch_ce_bias_bwd(*head, N.ptr(bias), *rest), "tt_inbatch_ce_bias_bwd")
    else:
        assert entry == "plain" and bias is None
        N.check(lib.tt_inbatch_ce_bwd(*head, *rest), "tt_inbatch_ce_bwd")
    return dU, dI


def abi_bwd_kept(T, U, Nn, off, lse, coef, logits, *, dI=None):
    ops, N = T
    lib = N.load()
    M, D = U.shape
    wsp, wsn = ops._ws(torch.device(DEV), lib.tt_inbatch_ce_workspace_bytes(M, Nn, D), "logq_test")
    dI = torch.empty(Nn, D, device=DEV) if dI is None else dI
    N.check(lib.tt_inbatch_ce_bwd_kept(U.data_ptr(), _ld(U), M, Nn, D, off, lse.data_ptr(), coef.data_ptr(), logits.data_ptr(),
                                       lib.tt_inbatch_ce_logits_bytes(M, Nn), dI.data_ptr(), _ld(dI), wsp, wsn, N.stream()),
            "tt_inbatch_ce_bwd_kept")
    return dI


# ------------------------------------------------------------------ 1. kernel parity
@pytest.mark.parametrize("path", ["op", "abi"])
@pytest.mark.parametrize("M,Nn,D,off", KERNEL_SHAPES)
def test_biased_ce_matches_the_torch_expression(T, M, Nn, D, off, path):
    """`op`: InBatchSoftmaxCE with item_bias (forward fused with dU, item-side backward; without a gradient the plain
    forward).  `abi`: the plain forward and the recomputing backward WITH its dU kernel, called directly."""
    ops, N = T
    U, I = g((M, D), 21) * 0.5, g((Nn, D), 22) * 0.5
    coef = g((M,), 23).abs() / M
    b = zipf_bias(Nn)
    ce_ref, dU_ref, dI_ref = oracle(U, I, b, off, coef)
    Ud, Id, bd, cd = U.to(DEV), I.to(DEV), b.to(DEV), coef.to(DEV)
    if path == "op":
        Ud, Id = Ud.requires_grad_(True), Id.requires_grad_(True)
        ce = ops.InBatchSoftmaxCE.apply(Ud, Id, off, None, bd)
        (ce * cd).sum().backward()
        dU, dI = Ud.grad, Id.grad
        ce_plain = ops.InBatchSoftmaxCE.apply(Ud.detach(), Id.detach(), off, None, bd)  # no gradient: the plain forward
        assert torch.allclose(ce_plain.cpu(), ce_ref, atol=2e-5, rtol=1e-5)
    else:
        f = abi_fwd(T, Ud, Id, off, bd, "plain")
        ce = f["ce"]
        dU, dI = abi_bwd(T, Ud, Id, off, bd, f["lse"], cd, with_du=True)
    err = (ce.detach().cpu() - ce_ref).abs() - 1e-5 * ce_ref.abs()
    print(f"row_ce err {float(err.max()):.3e} (bound 2e-5)  dU {float((dU.cpu() - dU_ref).abs().max() / dU_ref.abs().max()):.3e}"
          f"  dI {float((dI.cpu() - dI_ref).abs().max() / dI_ref.abs().max()):.3e} of max|g| (bound 1e-5 + rtol 1e-4)")
    assert torch.allclose(ce.detach().cpu(), ce_ref, atol=2e-5, rtol=1e-5)
    assert close_grad(dU, dU_ref) and close_grad(dI, dI_ref)


@pytest.mark.parametrize("M,Nn,D,off", [(256, 256, 128, 0), (130, 700, 50, 400), (300, 300, 256, 0), (1000, 1000, 128, 0)])
def test_biased_ce_with_a_signed_term_of_30_is_stable(T, M, Nn, D, off):
    """b of both signs scaled to +-30 (logit columns e^60 apart): finite, and within atol 1e-3 / rtol 1e-5 of float64."""
    ops, N = T
    U, I = g((M, D), 31) * 0.5, g((Nn, D), 32) * 0.5
    coef = g((M,), 33).abs() / M
    b = signed_bias(Nn)
    ce_ref, dU_ref, dI_ref = oracle(U, I, b, off, coef, torch.float64)
    Ud, Id = U.to(DEV).requires_grad_(True), I.to(DEV).requires_grad_(True)
    ce = ops.InBatchSoftmaxCE.apply(Ud, Id, off, None, b.to(DEV))
    (ce * coef.to(DEV)).sum().backward()
    assert torch.isfinite(ce).all() and torch.isfinite(Ud.grad).all() and torch.isfinite(Id.grad).all()
    assert torch.allclose(ce.detach().cpu().double(), ce_ref, atol=1e-3, rtol=1e-5)
    assert torch.allclose(Ud.grad.cpu().double(), dU_ref, atol=1e-3 * float(dU_ref.abs().max()), rtol=1e-5)
    assert torch.allclose(Id.grad.cpu().double(), dI_ref, atol=1e-3 * float(dI_ref.abs().max()), rtol=1e-5)
    f = abi_fwd(T, Ud.detach(), Id.detach(), off, b.to(DEV), "plain")
    assert torch.allclose(f["ce"].cpu().double(), ce_ref, atol=1e-3, rtol=1e-5)


# ------------------------------------------------------------------ 2. zero bias is no bias, bit for bit
@pytest.mark.parametrize("M,Nn,D,off", [(300, 300, 128, 0), (130, 700, 50, 400), (256, 1024, 128, 512), (200, 200, 200, 0),
                                        (4096, 4096, 128, 0)])
def test_zero_bias_is_no_bias_bit_for_bit(T, M, Nn, D, off):
    """item_bias = zeros(N) against item_bias = NULL (the BIAS = false kernels): row_lse, row_ce, du_unit, dU, dI and the
    fused loss, torch.equal, for the plain, fwd_du, kept and fused-loss forms -- and NULL against the calls without the
    argument, which it dispatches to."""
    ops, N = T
    lib = N.load()
    Ud, Id = (g((M, D), 41) * 0.5).to(DEV), (g((Nn, D), 42) * 0.5).to(DEV)
    coef = (g((M,), 43).abs() / M).to(DEV)
    zero = torch.zeros(Nn, device=DEV)
    labels = (g((M, 3), 44) > 0.3).float().to(DEV)
    uvw = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    forms = ["plain", "du"] + (["keep"] if (D in (32, 64, 128)) else []) + (["loss"] if off == 0 else [])
    for form in forms:
        kw = dict(labels=labels, uvw=uvw) if form == "loss" else {}
        a, z = abi_fwd(T, Ud, Id, off, None, form, **kw), abi_fwd(T, Ud, Id, off, zero, form, **kw)
        for k in a:
            if k != "logits":  # (-0.0 == +0.0 in value; the kept buffer is compared through the gradient it yields)
                assert torch.equal(a[k], z[k]), (form, k)
        if form == "keep":
            dIa = abi_bwd_kept(T, Ud, Nn, off, a["lse"], coef, a["logits"])
            dIz = abi_bwd_kept(T, Ud, Nn, off, z["lse"], coef, z["logits"])
            assert torch.equal(dIa, dIz)
        if form == "plain":
            (dUa, dIa), (dUz, dIz) = abi_bwd(T, Ud, Id, off, None, a["lse"], coef), abi_bwd(T, Ud, Id, off, zero, a["lse"], coef)
            assert torch.equal(dUa, dUz) and torch.equal(dIa, dIz)
            # NULL is the call without the argument
            wsp, wsn = ops._ws(torch.device(DEV), lib.tt_inbatch_ce_workspace_bytes(M, Nn, D), "logq_test")
            lse0, ce0, dU0, dI0 = (torch.empty(M, device=DEV), torch.empty(M, device=DEV), torch.empty(M, D, device=DEV),
                                   torch.empty(Nn, D, device=DEV))
            N.check(lib.tt_inbatch_ce_fwd(Ud.data_ptr(), D, Id.data_ptr(), D, M, Nn, D, off, lse0.data_ptr(), ce0.data_ptr(), wsp, wsn,
                                          N.stream()), "fwd")
            N.check(lib.tt_inbatch_ce_bwd(Ud.data_ptr(), D, Id.data_ptr(), D, M, Nn, D, off, lse0.data_ptr(), coef.data_ptr(),
                                          dU0.data_ptr(), D, dI0.data_ptr(), D, wsp, wsn, N.stream()), "bwd")
            assert torch.equal(lse0, a["lse"]) and torch.equal(ce0, a["ce"]) and torch.equal(dU0, dUa) and torch.equal(dI0, dIa)
    # the ops: zeros against None, loss and gradients
    outs = []
    for bias in (None, zero):
        U, I = Ud.clone().requires_grad_(True), Id.clone().requires_grad_(True)
        ce = ops.InBatchSoftmaxCE.apply(U, I, off, None, bias)
        (ce * coef).sum().backward()
        outs.append((ce.detach(), U.grad, I.grad))
    assert all(torch.equal(x, y) for x, y in zip(*outs))


# ------------------------------------------------------------------ 3. a constant bias changes nothing
@pytest.mark.parametrize("M,Nn,D,off", [(256, 256, 128, 0), (130, 700, 50, 400), (300, 300, 256, 0)])
def test_constant_bias_changes_nothing(T, M, Nn, D, off):
    """Softmax shift invariance: b = 7.25 on every column leaves row_ce and the gradients where they were (within the
    tolerances of the parity test; the logits are rounded at another magnitude, so not bit for bit)."""
    ops, N = T
    U0, I0 = (g((M, D), 51) * 0.5).to(DEV), (g((Nn, D), 52) * 0.5).to(DEV)
    coef = (g((M,), 53).abs() / M).to(DEV)
    outs = []
    for bias in (None, torch.full((Nn,), 7.25, device=DEV)):
        U, I = U0.clone().requires_grad_(True), I0.clone().requires_grad_(True)
        ce = ops.InBatchSoftmaxCE.apply(U, I, off, None, bias)
        (ce * coef).sum().backward()
        outs.append((ce.detach().cpu(), U.grad.cpu(), I.grad.cpu()))
    (ce0, dU0, dI0), (ce1, dU1, dI1) = outs
    assert not torch.equal(ce0, ce1) or M == 1
    assert torch.allclose(ce1, ce0, atol=2e-5, rtol=1e-5)
    assert close_grad(dU1, dU0) and close_grad(dI1, dI0)


# ------------------------------------------------------------------ 4. kept and recomputed backward agree
@pytest.mark.parametrize("M,Nn,D,off", [(130, 700, 128, 400), (256, 2048, 128, 1536)])
def test_kept_and_recomputed_backward_agree_under_a_bias(T, M, Nn, D, off):
    """ce_bwd_kept_kernel is unchanged: the logits the biased forward kept already include the term."""
    ops, N = T
    U0, I0 = (g((M, D), 61) * 0.5).to(DEV), (g((Nn, D), 62) * 0.5).to(DEV)
    coef = (g((M,), 63).abs() / M).to(DEV)
    b = zipf_bias(Nn).to(DEV)
    outs, calls = [], []
    for keep in (True, False):
        U, I = U0.clone().requires_grad_(True), I0.clone().requires_grad_(True)
        N.trace = []
        try:
            ce = ops.InBatchSoftmaxCE.apply(U, I, off, keep, b)
            (ce * coef).sum().backward()
            calls.append(list(N.trace))
        finally:
            N.trace = None
        outs.append((ce.detach(), U.grad, I.grad))
    assert "tt_inbatch_ce_bwd_kept" in calls[0] and "tt_inbatch_ce_bias_bwd" not in calls[0]
    assert "tt_inbatch_ce_bias_bwd" in calls[1] and "tt_inbatch_ce_bwd_kept" not in calls[1]
    (ce_k, dU_k, dI_k), (ce_r, dU_r, dI_r) = outs
    assert torch.allclose(ce_k, ce_r, atol=2e-5, rtol=1e-5)
    assert torch.allclose(dI_k, dI_r, atol=1e-6 * float(dI_r.abs().max()) + 1e-12, rtol=1e-5)
    # ... and against the oracle, like the recomputed one
    ce_ref, dU_ref, dI_ref = oracle(U0.cpu(), I0.cpu(), b.cpu(), off, coef.cpu())
    assert torch.allclose(ce_k.cpu(), ce_ref, atol=2e-5, rtol=1e-5) and close_grad(dU_k, dU_ref) and close_grad(dI_k, dI_ref)


# ------------------------------------------------------------------ 5. fused loss head = two-op path, bit for bit
@pytest.mark.parametrize("M,Nn,D,Tn", [(8192, 8192, 128, 3), (4096, 4096, 128, 0), (777, 777, 64, 3), (17, 17, 32, 1), (300, 300, 256, 3),
                                       (256, 293, 128, 3), (256, 512, 128, 1)])
def test_biased_fused_loss_head_is_the_two_op_path_bit_for_bit(T, M, Nn, D, Tn):
    """InBatchSoftmaxWeightedLoss(..., item_bias) against InBatchSoftmaxCE(..., item_bias) + WeightedMeanLoss: loss and every
    gradient identical, run after run; extra item rows (mixed negatives) included; and the loss against the CPU oracle."""
    ops, N = T
    gen = torch.Generator().manual_seed(M + D)
    U0, I0 = torch.randn(M, D, generator=gen) * 0.4, torch.randn(Nn, D, generator=gen) * 0.4
    labels = (torch.rand(M, Tn, generator=gen) < 0.4).float() if Tn else None
    uvw = torch.tensor([0.1, 0.2, 0.3][:max(Tn, 1)])
    b = zipf_bias(Nn)
    labd, uvwd, bd = (labels.to(DEV) if Tn else None), uvw.to(DEV), b.to(DEV)
    outs = []
    for fused in (True, False, True):
        U, I = U0.clone().to(DEV).requires_grad_(True), I0.clone().to(DEV).requires_grad_(True)
        if fused:
            assert ops.fused_loss_supported(U, I, labd, uvwd, bd)
            loss = ops.InBatchSoftmaxWeightedLoss.apply(U, I, labd, uvwd, bd)
        else:
            loss = ops.WeightedMeanLoss.apply(ops.InBatchSoftmaxCE.apply(U, I, 0, None, bd), labd, uvwd)
        (loss * 1.75).backward()  # an upstream gradient other than 1
        outs.append((loss.detach().clone(), U.grad.clone(), I.grad.clone()))
    for a, c in ((outs[0], outs[1]), (outs[0], outs[2])):
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and torch.equal(a[2], c[2])
    ce = oracle_rows(U0, I0, b, 0)
    w = R.normalise_value_weights(R.net_user_value(labels, uvw)) if Tn else torch.ones(M)
    assert abs(outs[0][0].item() - float((ce * w).mean())) < 1e-5 * max(1.0, float(ce.mean()))


# ------------------------------------------------------------------ 6. model level
def Tn_(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def state_of(gd, prefix="p."):
    return {k[len(prefix):]: Tn_(v) for k, v in gd.items() if k.startswith(prefix)}


def batch_of(gd, prefix="in.", dev=DEV):
    names = ("user_id", "user_features", "user_history", "item_id", "item_features", "position", "labels")
    return [Tn_(gd[prefix + n]).to(dev) for n in names]


def make_model(kind, gd):
    import two_tower_models_amd as A
    n_users, du, iu, n_items, di, ii, Tn, B, H = (int(v) for v in gd["cfg"])
    mips = A.BaselineMIPSModule(corpus_size=64, embedding_dim=di)
    common = dict(num_items=10, user_id_hash_size=n_users, user_id_embedding_dim=du, user_features_size=iu,
                  item_id_hash_size=n_items, item_id_embedding_dim=di, item_features_size=ii,
                  user_value_weights=[float(v) for v in gd["uvw"]], mips_module=mips)
    if kind == "base":
        m = A.TwoTowerBaseRetrieval(**common)
    elif kind == "hist":
        m = A.TwoTowerWithUserHistoryEncoder(user_history_seqlen=H, **common)
    else:
        m = A.TwoTowerWithDebiasing(user_history_seqlen=H, **common)
    m.load_state_dict(state_of(gd), strict=True)
    return m.to(DEV)


MODELS = {"base": ("g2_base_aligned", R.debias_identity), "hist": ("g4_hist_d128", R.debias_identity),
          "debias": ("g6_debias_d128", R.debias_combined)}


def candidates(gd, Bn, seed, log_q=True, collide=False):
    """Bn extra items (ids, features) and the log q of every candidate: a Zipf(1.0) popularity over the item table's rows."""
    n_items, ii, B = int(gd["cfg"][3]), int(gd["cfg"][5]), int(gd["cfg"][7])
    harmonic = float(np.sum(1.0 / np.arange(1, n_items + 1)))
    table = -(torch.log(torch.arange(1, n_items + 1).double()) + math.log(harmonic)).float()  # log q per item id
    item_id = Tn_(gd["in.item_id"])
    kw = {}
    if log_q:
        kw["item_log_q"] = table[item_id]
    if Bn:
        neg = Tn_(fg.uniform_ids((Bn,), n_items, seed).astype(np.int64))
        if collide:  # duplicates across blocks: batch items, history items, and repeats inside the block
            hist = Tn_(gd["in.user_history"]).reshape(-1)
            neg[0::5] = item_id[: len(neg[0::5])]
            neg[1::5] = hist[: len(neg[1::5])]
            neg[2::5] = neg[3::5][: len(neg[2::5])] if len(neg[3::5]) >= len(neg[2::5]) else neg[2::5]
        kw["negative_item_id"] = neg
        kw["negative_item_features"] = g((Bn, ii), seed + 1) * 0.5
        if log_q:
            kw["negative_log_q"] = table[neg]
    return kw


def oracle_loss(params, batch, uvw, extra, kind, gd, debias):
    """The reference's train_forward (oracle.cpu_ref) with the corrected logits and the widened item block."""
    user_id, user_features, user_history, item_id, item_features, position, labels = batch
    fkw = dict(with_history=True, heads=4, pos_table=Tn_(gd["pe_table"])) if kind != "base" else dict(with_history=False)
    u = R.user_embedding(params, user_id, user_features, user_history, **fkw)
    ids, feats = item_id, item_features
    if "negative_item_id" in extra:
        ids = torch.cat([item_id, extra["negative_item_id"]])
        feats = torch.cat([item_features, extra["negative_item_features"].to(item_features.dtype)])
    it = R.item_embeddings(params, ids, feats)
    scores = R.inbatch_logits(u, it)
    if "item_log_q" in extra:
        log_q = torch.cat([extra["item_log_q"], extra["negative_log_q"]]) if "negative_log_q" in extra else extra["item_log_q"]
        scores = scores - log_q.to(scores.dtype)[None, :]
    ce = F.cross_entropy(scores, torch.arange(u.shape[0]), reduction="none")
    nuv = R.net_user_value(labels, uvw)
    nuv, aux = debias(nuv, position, u, params)
    return (ce * R.normalise_value_weights(nuv)).sum() / ce.shape[0] + aux


ZERO_GRADIENT = ("item_tower_arch.bias", "item_features_arch.2.bias")  # softmax shift invariance


@pytest.mark.parametrize("Bn", [0, 37, "B"])
@pytest.mark.parametrize("kind", ["base", "hist", "debias"])
def test_models_with_log_q_and_mixed_negatives_match_the_oracle(golden, kind, Bn):
    """Loss 1e-4 and every parameter gradient 1e-5 * max|g| + 2e-4 rel against the oracle at the golden weights and
    inputs, with item_log_q and Bn extra negatives.  The oracle is the float32 torch-CPU expression for all three models
    (measured on the MI355X box: the debias model, whose sum-MSE terms put a loss of 3108 next to a CE of ~5, stays
    within the bound against it with or without the new arguments, while a float64 oracle sits 2-7e-5 * max|g| away from
    BOTH float32 sides on four of its tensors -- also with no new argument, i.e. on the parent's path)."""
    name, debias = MODELS[kind]
    gd = golden(name)
    Bn = int(gd["cfg"][7]) if Bn == "B" else Bn
    extra = candidates(gd, Bn, seed=300 + Bn)
    leaves = {k: v.requires_grad_(True) for k, v in state_of(gd).items()}
    want = oracle_loss(leaves, batch_of(gd, dev="cpu"), Tn_(gd["uvw"]), extra, kind, gd, debias)
    grads = dict(zip(leaves, torch.autograd.grad(want, list(leaves.values()), allow_unused=True)))
    model = make_model(kind, gd)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = model.train_forward(*batch_of(gd), **{k: v.to(DEV) for k, v in extra.items()})
    print(f"{kind} Bn={Bn}: loss {loss.item():.6f} oracle {float(want):.6f}")
    assert loss.dim() == 0 and abs(loss.item() - float(want)) < 1e-4 * max(1.0, abs(float(want)))
    loss.backward()  # no optimiser attached: dense embedding gradients
    worst = ("", 0.0)
    for pname, p in model.named_parameters():
        w = grads[pname]
        w = torch.zeros_like(p, device="cpu") if w is None else w.float()
        assert p.grad is not None, pname
        got = p.grad.cpu()
        tol = max(1e-5 * float(w.abs().max()), 1e-7)  # floor: the analytically-zero gradients hold ~1e-8 of rounding noise
        rel = float(((got - w).abs() - 2e-4 * w.abs()).max()) / tol
        worst = max(worst, (pname, rel), key=lambda t: t[1])
        print(f"  {pname}: max|g| {float(w.abs().max()):.3e} excess/tol {rel:.3f}")
        assert torch.allclose(got, w, atol=tol, rtol=2e-4), (pname, float((got - w).abs().max()), tol)
    print("  worst", worst)


# ------------------------------------------------------------------ 7. three optimiser steps
@pytest.mark.parametrize("kind", ["base", "hist"])
def test_three_optimiser_steps_with_colliding_negatives(golden, kind):
    """Negatives whose ids collide with batch items and with history ids, three steps under overlap_sweep=True, "forward"
    and lazy=True: tables, dense parameters and both moments against three steps of the oracle, the three schedules
    bit-identical to each other, and a row that only a negative looked up has moved like a looked-up row.
    Bounds: DESIGN.md section 3, as tests/test_gpu_models.py::assert_reference_trajectory writes them -- the zero-gradient
    tensors by 2 * steps * lr; everything else <= 5e-6 (+ 1e-5 rel) with <= 0.2 % of a tensor's elements outside and
    none beyond 2e-4: Adam's first updates are lr * g / (|g| + eps), so an element whose gradient is ~1e-4 of the typical
    size turns a 1e-7 relative summation-order difference into a ~1e-5 step difference between ANY two float32
    implementations."""
    import two_tower_models_amd as A
    name, debias = MODELS[kind]
    gd = golden(name)
    steps, lr = 3, 1e-3
    extras = [candidates(gd, 37, seed=500 + s, collide=True) for s in range(steps)]
    uvw = Tn_(gd["uvw"])
    # oracle: three Adam steps on every element of every parameter
    params = {k: v.clone() for k, v in state_of(gd).items()}
    state = R.AdamState(params)
    batch = batch_of(gd, dev="cpu")
    want_losses = []
    for s in range(steps):
        leaves = {k: v.detach().requires_grad_(True) for k, v in params.items()}
        loss = oracle_loss(leaves, batch, uvw, extras[s], kind, gd, debias)
        grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
        state.step += 1
        with torch.no_grad():
            for (pname, p), gr in zip(params.items(), grads):
                if gr is not None:
                    R.adam_update(p, gr, state.m[pname], state.v[pname], state.step, lr)
        want_losses.append(loss.item())
    finals = []
    for schedule in (dict(overlap_sweep=True), dict(overlap_sweep="forward"), dict(lazy=True)):
        model = make_model(kind, gd)
        opt = A.DenseExactAdam(model.parameters(), lr=lr, **schedule)
        b = batch_of(gd)
        got_losses = []
        for s in range(steps):
            loss = model.train_forward(*b, **{k: v.to(DEV) for k, v in extras[s].items()})
            opt.zero_grad()
            loss.backward()
            opt.step()
            got_losses.append(loss.item())
        opt.flush()
        torch.cuda.synchronize()
        assert opt.step_count == steps and np.allclose(got_losses, want_losses, atol=1e-4), (got_losses, want_losses)
        fin = {k: v.detach().clone() for k, v in model.state_dict().items()}
        for pname, p in model.named_parameters():
            fin["m." + pname] = opt.state[p]["exp_avg"].detach().clone()
            fin["v." + pname] = opt.state[p]["exp_avg_sq"].detach().clone()
        finals.append(fin)
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]) and torch.equal(finals[0][k], finals[2][k]), k
    fin = finals[0]
    for k, want in params.items():
        noise_only = k in ZERO_GRADIENT or k.endswith("in_proj_bias")  # (in_proj_bias: its K third)
        err = (fin[k].cpu() - want).abs() - 1e-5 * want.abs()
        n_out = int((err > 5e-6).sum())
        print(f"{k}: max err {float(err.max()):.3e}, {n_out} of {err.numel()} elements over 5e-6")
        assert float(err.max()) <= 2 * steps * lr * 1.05, (k, float(err.max()))
        if not noise_only:
            assert n_out <= max(1, int(2e-3 * err.numel())) and float(err.max()) <= 2e-4, (k, n_out, float(err.max()))
            # moments: m is linear in the three gradients, v in their squares (no division by a small number), so they
            # inherit the gradient tolerance (1e-5 * max + 2e-4 rel) once and twice over, with no outliers
            for tag, ref, f in (("m.", state.m[k], 1.0), ("v.", state.v[k], 2.0)):
                got = fin[tag + k].cpu()
                assert torch.allclose(got, ref, atol=f * 1e-5 * float(ref.abs().max()) + 1e-12, rtol=f * 2e-4), \
                    (tag + k, float((got - ref).abs().max()), float(ref.abs().max()))
    # a row only a negative looked up: moved like a looked-up row (Adam's first steps are ~lr each), not like an idle one
    if kind == "base":
        touched = torch.zeros(int(gd["cfg"][3]), dtype=torch.bool)
        touched[Tn_(gd["in.item_id"])] = True
        only_neg = torch.zeros_like(touched)
        for e in extras:
            only_neg[e["negative_item_id"]] = True
        only_neg &= ~touched
        assert bool(only_neg.any())
        w0 = state_of(gd)["item_id_embedding_arch.weight"]
        moved = (fin["item_id_embedding_arch.weight"].cpu() - w0)[only_neg].abs().max(dim=1).values
        idle = ~(touched | only_neg)
        assert float(moved.min()) > 0.5 * lr
        if bool(idle.any()):
            assert float((fin["item_id_embedding_arch.weight"].cpu() - w0)[idle].abs().max()) == 0.0


# ------------------------------------------------------------------ 8. nothing old moved
@pytest.mark.parametrize("kind", ["base", "hist"])
def test_the_reference_call_is_untouched(golden, kind):
    """train_forward with the reference's seven arguments: the loss is torch.equal to the four-argument
    InBatchSoftmaxWeightedLoss.apply(U, I, lab, uvw) on the same tower outputs, and no call with a term is made."""
    from two_tower_models_amd import _native as N
    from two_tower_models_amd import ops
    gd = golden(MODELS[kind][0])
    model = make_model(kind, gd)
    b = batch_of(gd)
    N.trace = []
    try:
        loss = model.train_forward(*b)
        calls = list(N.trace)
    finally:
        N.trace = None
    assert "tt_inbatch_ce_fwd_du_loss" in calls and not any("bias" in c for c in calls)
    u = model.compute_user_embedding(b[0], b[1], b[2])
    it = model.compute_item_embeddings(b[3], b[4])
    direct = ops.InBatchSoftmaxWeightedLoss.apply(u, it, b[6], model.user_value_weights)
    assert torch.equal(loss.detach(), direct.detach())


# ------------------------------------------------------------------ 9. refusals
def test_refusals(golden):
    import two_tower_models_amd as A
    from two_tower_models_amd import ops, parallel
    gd = golden("g2_base_aligned")
    b = batch_of(gd)
    B = b[0].shape[0]
    ok = {k: v.to(DEV) for k, v in candidates(gd, 8, seed=900).items()}
    model = make_model("base", gd)
    assert torch.isfinite(model.train_forward(*b, **ok))
    # negatives with half of the log q
    for drop in ("item_log_q", "negative_log_q"):
        with pytest.raises(ValueError, match="half-corrected"):
            model.train_forward(*b, **{k: v for k, v in ok.items() if k != drop})
    # a bias of the wrong length, dtype, or on the CPU
    with pytest.raises(ValueError, match="one value per item row"):
        model.train_forward(*b, item_log_q=ok["item_log_q"][:-1])
    with pytest.raises(RuntimeError, match="item_bias is on cpu"):
        model.train_forward(*b, item_log_q=ok["item_log_q"].cpu())
    with pytest.raises(TypeError, match="float32"):
        model.train_forward(*b, item_log_q=ok["item_log_q"].double())
    U, I = torch.zeros(8, 32, device=DEV), torch.zeros(12, 32, device=DEV)
    with pytest.raises(ValueError):
        ops.InBatchSoftmaxCE.apply(U, I, 0, None, torch.zeros(8, device=DEV))
    with pytest.raises(RuntimeError):
        ops.InBatchSoftmaxWeightedLoss.apply(U.requires_grad_(True), I, None, torch.ones(1, device=DEV), torch.zeros(12))
    # row-sharded model
    sharded = make_model("base", gd)
    w = sharded.item_id_embedding_arch.weight
    w._tt_shard = parallel.RowShard(w.shape[0], w.shape[1], 1, 0)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        sharded.train_forward(*b, **ok)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        sharded.train_forward(*b, item_log_q=ok["item_log_q"])
    # light ranker
    mips = A.BaselineMIPSModule(corpus_size=64, embedding_dim=32)
    lr = A.TwoTowerPlusLightRanker(num_items=5, num_mips_items=16, num_ranker_user_embeddings=2, user_id_hash_size=256,
                                   user_id_embedding_dim=32, user_features_size=8, user_history_seqlen=4, item_id_hash_size=256,
                                   item_id_embedding_dim=32, item_features_size=8, user_value_weights=[1.0],
                                   mips_module=mips).to(DEV)
    with pytest.raises(NotImplementedError, match="light-ranker"):
        lr.train_forward(*b, item_log_q=ok["item_log_q"])


# ------------------------------------------------------------------ a subclass with the reference's signature; graphs
def test_subclass_with_the_reference_loss_signature_keeps_working(golden):
    import two_tower_models_amd as A
    gd = golden("g2_base_aligned")

    class Mine(A.TwoTowerBaseRetrieval):
        def compute_training_loss(self, user_embedding, item_embeddings, position, labels):
            return super().compute_training_loss(user_embedding, item_embeddings, position, labels)

    base = make_model("base", gd)
    base.__class__ = Mine
    b = batch_of(gd)
    assert torch.isfinite(base.train_forward(*b))
    with pytest.raises(TypeError):  # the term is passed on only when it is given
        base.train_forward(*b, item_log_q=torch.zeros(b[0].shape[0], device=DEV))


def test_graphed_train_step_takes_the_new_tensors_as_extra_batch_members(golden):
    """GraphedTrainStep replays train_forward(*static_inputs) positionally: item_log_q, negative ids / features / log q as
    members 8..11 of the example batch.  Warm-up plus three replayed steps equal as many eager steps bit for bit."""
    import two_tower_models_amd as A
    gd = golden("g2_base_aligned")
    ex = candidates(gd, 37, seed=700)
    order = ("item_log_q", "negative_item_id", "negative_item_features", "negative_log_q")
    full = batch_of(gd) + [ex[k].to(DEV) for k in order]
    W, n = 2, 3  # GraphedTrainStep's warm-up = W real steps on the example batch, then n replays
    finals = []
    for graphed in (False, True):
        model = make_model("base", gd)
        opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep=False, lazy=True)
        losses = []
        if graphed:
            step = A.GraphedTrainStep(model, opt, full, warmup=W)
            losses = [step(*full).item() for _ in range(n)]
        else:
            side = torch.cuda.Stream()  # eager reference on a side stream as well (same autograd stream rules)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(W + n):
                    loss = model.train_forward(*full)
                    opt.zero_grad()
                    loss.backward()
                    opt.step()
                    losses.append(loss.item())
            torch.cuda.current_stream().wait_stream(side)
            del loss
        opt.flush()
        torch.cuda.synchronize()
        assert opt.step_count == W + n
        finals.append(({k: v.detach().clone() for k, v in model.state_dict().items()}, losses))
    assert finals[1][1] == finals[0][1][W:]
    for k in finals[0][0]:
        assert torch.equal(finals[0][0][k], finals[1][0][k]), k
