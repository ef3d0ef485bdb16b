"""Cosine logits without a GPU: the float64 reference of the row-normalise op against torch autograd, the C ABI's new
symbols and every refusal they make before a HIP call, and the model's switch (`use_cosine_logits`)."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import l2norm_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("log_scale", L.LOG_SCALES)
@pytest.mark.parametrize("D,rows", [(1, 5), (3, 7), (50, 10), (128, 63)])
def test_closed_form_equals_autograd(D, rows, log_scale):
    """s * F.normalize(x.double(), dim=1, eps) through autograd against the closed form, clamped rows (gaussian * 1e-15 and
    the exactly zero row) included, and d_log_scale against autograd's."""
    x, dy = L.make_rows(rows, D, seed=D * 31 + rows)
    eps = L.EPS32
    xd = x.double().requires_grad_(True)
    ls = torch.tensor(0.0 if log_scale is None else float(torch.tensor(log_scale, dtype=torch.float32)), dtype=torch.float64,
                      requires_grad=True)
    y = torch.exp(ls) * F.normalize(xd, dim=1, eps=eps)
    y.backward(dy.double())
    y64, inv64 = L.forward64(x, log_scale)
    dx64, dls64, terms = L.backward64(x, dy, log_scale)
    assert torch.allclose(y64, y.detach(), rtol=1e-13, atol=0)
    clamped = x.double().norm(dim=1) <= eps
    assert clamped.any() and (~clamped).any() or rows < 2
    assert torch.equal(inv64[clamped], torch.full_like(inv64[clamped], 1.0 / eps))
    # (autograd's dy - n <n, dy> and the closed form round differently, and at D = 1 both are rounding noise around 0:
    # relative to the size of the terms that cancel, s * inv * max|dy_r|)
    scale = (math.exp(float(ls.detach())) * inv64 * dy.double().abs().amax(dim=1)).unsqueeze(1)
    assert float(((dx64 - xd.grad).abs() / scale).max()) < 1e-12
    assert abs(float(dls64) - float(ls.grad)) <= 1e-13 * float(terms.abs().sum()) + 1e-300
    zero = (x == 0).all(dim=1)
    assert torch.equal(y64[zero], torch.zeros_like(y64[zero]))


def test_fp32_restatement_stays_inside_its_own_yardstick():
    w = L.measure()
    assert max(w["rel_inv"], w["rel_y"]) <= L.Y_REL and w["dx_rowmax"] <= L.Y_DX and w["dls_sumabs"] <= L.Y_DLS
    assert w["d1_abs"] <= L.D1_ABS
    assert 40 <= sum(1 for _ in L.cases()) <= 60


def test_new_symbols_are_exported_and_the_version_stays_6():
    from two_tower_models_amd import _native as N
    lib = N.load()
    for name in ("tt_l2norm_fwd", "tt_l2norm_bwd", "tt_l2norm_bwd_workspace_bytes"):
        assert name in N.SIGNATURES and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "tt_hotpath.h")).read()
    assert re.search(r"#define TT_ABI_VERSION 6\b", header) and lib.tt_abi_version() == 6 == N.ABI_VERSION
    assert lib.tt_l2norm_bwd_workspace_bytes(0) == 0
    assert lib.tt_l2norm_bwd_workspace_bytes(L.ROWS_BEYOND_ONE_PASS) >= 4 * (L.ROWS_BEYOND_ONE_PASS + L.ROWS_PER_WG - 1) // L.ROWS_PER_WG


def _fwd_side(N, rows=4, ld=8, x=64, y=64, inv=64):
    return N.L2NormFwdSide(x, ld, y, ld, inv, rows, None)


def _bwd_side(N, rows=4, ld=8, x=64, dy=64, inv=64, dx=64, d_log_scale=None):
    return N.L2NormBwdSide(x, ld, dy, ld, inv, dx, ld, rows, None, d_log_scale)


def test_every_refusal_is_made_without_a_gpu():
    """(The pointers are never dereferenced: every call below returns before any HIP call.)"""
    from two_tower_models_amd import _native as N
    lib = N.load()
    BAD = N.TT_E_BADARG

    def refused(rc, word):
        return rc == BAD and word in lib.tt_last_error_string().decode()

    fwd = lambda sides, n, D=8, eps=1e-12: lib.tt_l2norm_fwd(sides, n, D, eps, None)
    bwd = lambda sides, n, D=8, eps=1e-12, ws=None, wsb=0: lib.tt_l2norm_bwd(sides, n, D, eps, ws, wsb, None)
    for call, side in ((fwd, _fwd_side), (bwd, _bwd_side)):
        arr = lambda *s: (type(s[0]) * len(s))(*s)
        ok = side(N)
        assert refused(call(None, 1), "null side array")
        assert refused(call(arr(ok, ok, ok), 0), "n_sides") and refused(call(arr(ok, ok, ok), 3), "n_sides")
        assert refused(call(arr(ok), 1, D=0), "D < 1")
        assert refused(call(arr(side(N, ld=7)), 1), "ld < D")
        assert refused(call(arr(ok, side(N, ld=7)), 2), "ld < D")  # the second side is checked as well
        assert refused(call(arr(side(N, rows=-1)), 1), "rows < 0")
        for eps in (0.0, -1e-12, float("inf"), float("nan"), 1e-45):
            assert refused(call(arr(ok), 1, eps=eps), "eps")
        for field in ("x", "inv"):
            assert refused(call(arr(side(N, **{field: None})), 1), "null")
    assert refused(fwd((N.L2NormFwdSide * 1)(_fwd_side(N, y=None)), 1), "null")
    for field in ("dy", "dx"):
        assert refused(bwd((N.L2NormBwdSide * 1)(_bwd_side(N, **{field: None})), 1), "null")
    # a d_log_scale needs the workspace: NULL, or smaller than the sum over the sides that ask
    asks = (N.L2NormBwdSide * 2)(_bwd_side(N, rows=1025, d_log_scale=64), _bwd_side(N, rows=5, d_log_scale=64))
    need = lib.tt_l2norm_bwd_workspace_bytes(1025) + lib.tt_l2norm_bwd_workspace_bytes(5)
    assert refused(bwd(asks, 2, ws=None, wsb=need), "workspace")
    assert refused(bwd(asks, 2, ws=64, wsb=need - 1), "workspace")
    # rows == 0 everywhere and nothing asked for: nothing to do, no launch, no device needed
    assert fwd((N.L2NormFwdSide * 1)(_fwd_side(N, rows=0, x=None, y=None, inv=None)), 1) == 0
    assert bwd((N.L2NormBwdSide * 1)(_bwd_side(N, rows=0, x=None, dy=None, inv=None, dx=None)), 1) == 0


def _base(A, **kw):
    return A.TwoTowerBaseRetrieval(4, 10, 8, 4, 10, 8, 4, [1.0], A.BaselineMIPSModule(16, 8), **kw)


@pytest.mark.parametrize("learnable", [False, True])
def test_use_cosine_logits_adds_exactly_logit_log_scale(learnable):
    import two_tower_models_amd as A
    plain, m = _base(A), _base(A)
    before = list(plain.state_dict())
    assert not hasattr(plain, "logit_log_scale") and not hasattr(plain, "logit_temperature")
    assert m.use_cosine_logits(temperature=0.05, learnable=learnable) is m
    assert sorted(m.state_dict()) == sorted(before + ["logit_log_scale"]) and list(plain.state_dict()) == before
    t = m.logit_log_scale
    assert t.dtype == torch.float32 and tuple(t.shape) == (1,)
    assert float(t.detach()) == float(torch.tensor(math.log(1 / 0.05), dtype=torch.float32))
    assert isinstance(t, torch.nn.Parameter) == learnable
    assert ("logit_log_scale" in dict(m.named_parameters())) == learnable
    assert ("logit_log_scale" in dict(m.named_buffers())) == (not learnable)
    assert not getattr(t, "_tt_is_table", False)  # DenseExactAdam: the dense path
    assert abs(m.logit_temperature - 0.05) < 1e-8
    with pytest.raises(ValueError, match="already"):
        m.use_cosine_logits()


@pytest.mark.parametrize("bad", [0.0, -0.05, float("inf"), float("nan")])
def test_use_cosine_logits_refuses_a_bad_temperature(bad):
    import two_tower_models_amd as A
    m = _base(A)
    with pytest.raises(ValueError, match="temperature"):
        m.use_cosine_logits(temperature=bad)
    assert not hasattr(m, "logit_log_scale")


def test_history_and_debias_models_inherit_the_switch_and_the_light_ranker_refuses():
    import two_tower_models_amd as A
    mips = A.BaselineMIPSModule(16, 8)
    for cls in (A.TwoTowerWithUserHistoryEncoder, A.TwoTowerWithDebiasing):
        m = cls(4, 10, 8, 4, 6, 10, 8, 4, [1.0], mips).use_cosine_logits(1.0, learnable=True)
        assert float(m.logit_log_scale.detach()) == 0.0
    lr = A.TwoTowerPlusLightRanker(4, 8, 2, 10, 8, 4, 6, 10, 8, 4, [1.0], mips)
    with pytest.raises(NotImplementedError, match="cosine"):
        lr.use_cosine_logits()
    assert not hasattr(lr, "logit_log_scale")


def test_a_model_sharded_after_the_switch_refuses_before_any_kernel(monkeypatch):
    import two_tower_models_amd as A
    m = _base(A).use_cosine_logits()
    monkeypatch.setattr(A.TwoTowerBaseRetrieval, "_sharded", lambda self: True)
    B = 4
    args = (torch.zeros(B, dtype=torch.long), torch.zeros(B, 4), torch.zeros(B, 2, dtype=torch.long),
            torch.zeros(B, dtype=torch.long), torch.zeros(B, 4), torch.zeros(B, dtype=torch.long), torch.ones(B, 1))
    with pytest.raises(NotImplementedError, match="cosine"):
        m.train_forward(*args)
    with pytest.raises(NotImplementedError, match="cosine"):
        m.index_corpus(torch.zeros(B, dtype=torch.long), torch.zeros(B, 4))
    with pytest.raises(NotImplementedError, match="cosine"):
        m.forward(*args[:3])
    with pytest.raises(NotImplementedError, match="cosine"):
        _base(A).use_cosine_logits()
