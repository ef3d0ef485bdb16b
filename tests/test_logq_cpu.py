"""CPU-side checks of the log-Q correction / mixed-negatives surface: the C-ABI entry points and their argument
validation, the model methods' signatures, the sampling helpers against hand-computed values, and train.py's flags."""
import inspect
import math
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tt_inbatch_ce_bias_workspace_bytes", "tt_inbatch_ce_bias_fwd", "tt_inbatch_ce_bias_bwd")


def test_entry_points_exist_and_abi_version_is_6():
    from two_tower_models_amd import _native as N
    lib = N.load()
    assert lib.tt_abi_version() == 6 and N.ABI_VERSION == 6
    header = open(os.path.join(ROOT, "include", "tt_hotpath.h")).read()
    assert re.search(r"#define TT_ABI_VERSION 6\b", header)
    for name in NEW:
        assert name in N.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name
    # the correction is documented against the lines that name it as missing
    assert "base_retrieval.py:289-295" in header and header.count("ref:src/two_tower_base_retrieval.py:287-312, :289-295") >= 2
    # the pre-scaled copy of the term rides behind the plain calls' workspace, which keeps its size
    for M, Nn, D in ((8192, 8192, 128), (130, 700, 50), (300, 300, 256)):
        base = lib.tt_inbatch_ce_workspace_bytes(M, Nn, D)
        assert lib.tt_inbatch_ce_bias_workspace_bytes(M, Nn, D) >= base + 4 * Nn
    assert lib.tt_inbatch_ce_workspace_bytes(8192, 8192, 128) > 0


def test_bias_entry_points_validate_arguments_without_a_gpu():
    """Null pointers and a diagonal outside the item block: TT_E_BADARG before any HIP call (no device here)."""
    from two_tower_models_amd import _native as N
    lib = N.load()
    x = 0x1000  # never dereferenced: every call below is refused by the argument checks
    M, Nn, D = 8, 16, 32

    def fwd(U=x, I=x, off=0, bias=x, lse=x, ce=x, du=None, logits=None, uvw=None, outs=(None, None, None), ws=x, m=M, n=Nn):
        return lib.tt_inbatch_ce_bias_fwd(U, D, I, D, m, n, D, off, bias, lse, ce, du, D, logits, 0, None, 1, uvw, *outs, ws, 1 << 30,
                                          None)

    def bwd(U=x, I=x, off=0, bias=x, lse=x, coef=x, dU=None, dI=x, ws=x, m=M, n=Nn):
        return lib.tt_inbatch_ce_bias_bwd(U, D, I, D, m, n, D, off, bias, lse, coef, dU, D, dI, D, ws, 1 << 30, None)

    for kw in (dict(U=None), dict(I=None), dict(lse=None), dict(ce=None), dict(ws=None)):
        assert fwd(**kw) == N.TT_E_BADARG and b"null pointer" in lib.tt_last_error_string(), kw
    for kw in (dict(U=None), dict(I=None), dict(lse=None), dict(coef=None), dict(dI=None), dict(ws=None)):
        assert bwd(**kw) == N.TT_E_BADARG and b"null pointer" in lib.tt_last_error_string(), kw
    for call in (fwd, bwd):
        assert call(off=Nn - M + 1) == N.TT_E_BADARG and b"diagonal outside the item block" in lib.tt_last_error_string()
        assert call(off=-1) == N.TT_E_BADARG
        assert call(m=0) == N.TT_E_BADARG and call(n=0) == N.TT_E_BADARG
    # kept logits / the loss tail need the du_unit form; the tail needs its three outputs
    assert fwd(logits=x) == N.TT_E_BADARG and fwd(uvw=x) == N.TT_E_BADARG
    assert fwd(du=x, uvw=x) == N.TT_E_BADARG and b"null pointer" in lib.tt_last_error_string()
    assert fwd(du=x, logits=x, uvw=x, outs=(x, x, x)) == N.TT_E_UNSUPPORTED
    # a workspace that only fits the plain calls is refused when there is a term to pre-scale
    need = lib.tt_inbatch_ce_workspace_bytes(M, Nn, D)
    assert lib.tt_inbatch_ce_bias_fwd(x, D, x, D, M, Nn, D, 0, x, x, x, None, D, None, 0, None, 1, None, None, None, None, x, need,
                                      None) == N.TT_E_WORKSPACE


def test_model_signatures_keep_the_reference_parameters_first():
    import two_tower_models_amd as A
    ref_train = ["self", "user_id", "user_features", "user_history", "item_id", "item_features", "position", "labels"]
    new_train = ["item_log_q", "negative_item_id", "negative_item_features", "negative_log_q"]
    for cls in (A.TwoTowerBaseRetrieval, A.TwoTowerWithUserHistoryEncoder, A.TwoTowerWithDebiasing,
                A.TwoTowerWithPositionDebiasedWeights, A.TwoTowerWithUserDebiasedWeights, A.TwoTowerPlusLightRanker):
        sig = inspect.signature(cls.train_forward)
        names = list(sig.parameters)
        assert names[:8] == ref_train and names[8:] == new_train + ["remove_accidental_hits"], (cls.__name__, names)
        assert all(sig.parameters[n].default is inspect.Parameter.empty for n in ref_train[1:])
        assert all(sig.parameters[n].default is None for n in new_train)
        hits = sig.parameters["remove_accidental_hits"]
        assert hits.kind is inspect.Parameter.KEYWORD_ONLY and hits.default is False
    sig = inspect.signature(A.TwoTowerBaseRetrieval.compute_training_loss)
    assert list(sig.parameters) == ["self", "user_embedding", "item_embeddings", "position", "labels", "item_log_q", "item_id"]
    assert sig.parameters["item_log_q"].default is None
    assert sig.parameters["item_id"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["item_id"].default is None
    from two_tower_models_amd import ops
    for fn, names in ((ops.InBatchSoftmaxCE.forward, ["U", "I", "diag_offset", "keep_logits", "item_bias", "item_key"]),
                      (ops.InBatchSoftmaxWeightedLoss.forward, ["U", "I", "labels", "uvw", "item_bias", "item_key"])):
        sig = inspect.signature(fn)
        assert list(sig.parameters)[1:] == names and sig.parameters["item_key"].default is None


def test_new_arguments_are_refused_where_they_are_not_implemented():
    """No GPU needed: the refusals come before any kernel."""
    import pytest
    import two_tower_models_amd as A
    from two_tower_models_amd import parallel
    mips = A.BaselineMIPSModule(16, 8)
    B = 4
    args = [torch.zeros(B, dtype=torch.long), torch.zeros(B, 4), torch.zeros(B, 2, dtype=torch.long),
            torch.zeros(B, dtype=torch.long), torch.zeros(B, 4), torch.zeros(B, dtype=torch.long), torch.ones(B, 1)]
    lq, neg_id, neg_f, neg_lq = torch.zeros(B), torch.zeros(3, dtype=torch.long), torch.zeros(3, 4), torch.zeros(3)
    m = A.TwoTowerBaseRetrieval(4, 10, 8, 4, 10, 8, 4, [1.0], mips)
    for kw in (dict(negative_item_id=neg_id, negative_item_features=neg_f, item_log_q=lq),
               dict(negative_item_id=neg_id, negative_item_features=neg_f, negative_log_q=neg_lq),
               dict(negative_item_id=neg_id), dict(negative_item_features=neg_f), dict(negative_log_q=neg_lq)):
        with pytest.raises(ValueError):
            m.train_forward(*args, **kw)
    m.item_id_embedding_arch.weight._tt_shard = parallel.RowShard(20, 8, 2, 0)
    assert m._sharded()
    with pytest.raises(NotImplementedError, match="row-sharded"):
        m.train_forward(*args, item_log_q=lq)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        m.compute_training_loss(torch.zeros(B, 8), torch.zeros(B, 8), args[5], args[6], item_log_q=lq)
    lr = A.TwoTowerPlusLightRanker.__new__(A.TwoTowerPlusLightRanker)  # refused before anything of the model is used
    with pytest.raises(NotImplementedError, match="light-ranker"):
        A.TwoTowerPlusLightRanker.train_forward(lr, *args, item_log_q=lq)


def test_sampling_helpers_against_hand_computed_values():
    import two_tower_models_amd as A
    from two_tower_models_amd import sampling
    assert A.sampling is sampling and "sampling" in A.__all__
    counts = torch.tensor([0, 1, 3, 4])  # total 8; the zero count is treated as one occurrence
    got = sampling.log_q_from_counts(counts)
    want = torch.tensor([math.log(1 / 8), math.log(1 / 8), math.log(3 / 8), math.log(4 / 8)])
    assert got.dtype == torch.float32 and got.shape == (4,) and torch.allclose(got, want, atol=1e-7)
    ids = torch.tensor([3, 0, 2, 2])
    # n_uniform = 0: the unigram table, looked up
    assert torch.equal(sampling.mixture_log_q(got, ids, 5, 0, 4), got[ids])
    # 6 in-batch + 2 uniform draws over 4 items: q_j = (6 p_j + 2 / 4) / 8
    p = torch.tensor([1 / 8, 1 / 8, 3 / 8, 4 / 8])
    want = torch.log((6 * p[ids] + 0.5) / 8)
    mix = sampling.mixture_log_q(got, ids, 6, 2, 4)
    assert mix.dtype == torch.float32 and torch.allclose(mix, want, atol=1e-6)
    assert abs(float(mix[0]) - math.log((6 * 0.5 + 0.5) / 8)) < 1e-6
    # all uniform: log(1 / num_items) whatever the table says
    assert torch.allclose(sampling.mixture_log_q(got, ids, 0, 7, 4), torch.full((4,), math.log(0.25)), atol=1e-6)


def test_train_parser_knows_the_flags_and_they_are_off_by_default():
    from two_tower_models_amd import train
    p = train.build_parser()
    d = p.parse_args([])
    assert d.logq is False and d.num_random_negatives == 0
    a = p.parse_args(["--logq", "--num_random_negatives", "32"])
    assert a.logq is True and a.num_random_negatives == 32
    assert list(inspect.signature(train.train_one_epoch).parameters)[:4] == ["model", "dataloader", "optimizer", "device"]
    extra = list(inspect.signature(train.train_one_epoch).parameters.values())[4:]
    assert extra and all(q.default is None for q in extra)
