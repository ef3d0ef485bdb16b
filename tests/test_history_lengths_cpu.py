"""CPU-side checks of variable-length histories: the float64 reference against itself and against torch's own
key_padding_mask, the C-ABI entry points and their argument validation, the public keywords, and the refusals."""
import inspect
import os
import re

import pytest
import torch

import history_lengths_ref as HR
from oracle import cpu_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tt_hist_embed_pool_len", "tt_hist_pool_bwd_len", "tt_attn_fwd_len", "tt_attn_bwd_len", "tt_enc_last_fwd_len")


def _layers(L, D, gen):
    return [(torch.randn(3 * D, D, generator=gen, dtype=HR.F64) * 0.3, torch.randn(3 * D, generator=gen, dtype=HR.F64) * 0.3,
             torch.randn(D, D, generator=gen, dtype=HR.F64) * 0.3, torch.randn(D, generator=gen, dtype=HR.F64) * 0.3)
            for _ in range(L)]


def test_reference_truncation_mask_and_torch_key_padding_mask_agree():
    """B=5, H=7, D=16, 4 heads, 3 layers, non-zero biases, float64: the per-sample truncation form, the vectorised
    additive-mask form and nn.MultiheadAttention(key_padding_mask=arange(H)[None] >= lengths[:, None]) agree to rounding --
    forward and the gradient of the input (exactly zero on padded rows)."""
    gen = torch.Generator().manual_seed(5)
    B, H, D, heads, L = 5, 7, 16, 4, 3
    lengths = [1, 3, 7, 4, 6]
    layers = _layers(L, D, gen)
    pe = R.positional_table(H, D).to(HR.F64)
    x = torch.randn(B, H, D, generator=gen, dtype=HR.F64)
    cot = torch.randn(B, 2, D, generator=gen, dtype=HR.F64)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya = HR.encoder_truncated(xa, lengths, layers, heads, pe)
    yb = HR.encoder_masked(xb, lengths, layers, heads, pe)
    assert float((ya - yb).detach().abs().max()) < 1e-13
    (ga,), (gb,) = torch.autograd.grad((ya * cot).sum(), [xa]), torch.autograd.grad((yb * cot).sum(), [xb])
    assert float((ga - gb).abs().max()) < 1e-13
    valid = torch.arange(H)[None, :] < torch.tensor(lengths)[:, None]
    assert float(ga[~valid].abs().max()) == 0.0 and float(gb[~valid].abs().max()) == 0.0
    # torch's own module, slot 0 only (the pooled slot is a plain masked mean)
    h = x + pe[None]
    for w_in, b_in, w_out, b_out in layers:
        mha = torch.nn.MultiheadAttention(D, heads, batch_first=True, dtype=HR.F64)
        with torch.no_grad():
            mha.in_proj_weight.copy_(w_in), mha.in_proj_bias.copy_(b_in)
            mha.out_proj.weight.copy_(w_out), mha.out_proj.bias.copy_(b_out)
        h = mha(h, h, h, key_padding_mask=~valid, need_weights=False)[0]
    assert float((h[:, 0, :] - ya[:, 0, :]).abs().max()) < 1e-13
    # garbage in the padded rows does not reach the masked form
    xg = x.clone()
    xg[~valid] = float("nan")
    assert torch.equal(HR.encoder_masked(xg, lengths, layers, heads, pe), yb.detach())


def test_reference_attention_core_is_the_oracles_layer():
    """attention_core between the two projections = oracle.cpu_ref.self_attention_layer (full lengths)."""
    gen = torch.Generator().manual_seed(6)
    B, H, D, heads = 3, 5, 8, 2
    (w_in, b_in, w_out, b_out), = _layers(1, D, gen)
    x = torch.randn(B, H, D, generator=gen, dtype=HR.F64)
    want = R.self_attention_layer(x, w_in, b_in, w_out, b_out, heads)
    assert float((HR.layer_from_core(x, w_in, b_in, w_out, b_out, heads) - want).abs().max()) < 1e-14
    # and truncated: rows of a short sample are the oracle's layer on the truncated sample, its padded ctx rows zero
    lengths = [2, 5, 1]
    qkv = x.reshape(B * H, D) @ w_in.t() + b_in
    ctx = HR.attention_core(qkv, B, H, D, heads, lengths).reshape(B, H, D)
    for b, n in enumerate(lengths):
        got = ctx[b, :n] @ w_out.t() + b_out
        assert float((got - R.self_attention_layer(x[b:b + 1, :n], w_in, b_in, w_out, b_out, heads)[0]).abs().max()) < 1e-14
        assert float(ctx[b, n:].abs().sum()) == 0.0


def test_entry_points_exist_in_header_library_and_bindings():
    from two_tower_models_amd import _native as N
    lib = N.load()
    header = open(os.path.join(ROOT, "include", "tt_hotpath.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert name in N.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert "key_padding_mask" in header and "WRITTEN AS ZERO" in header


def test_len_entry_points_validate_arguments_without_a_gpu():
    """Null pointers and bad sizes: TT_E_BADARG before any HIP call (no device here), with lengths given or not."""
    from two_tower_models_amd import _native as N
    lib = N.load()
    x = 0x1000  # never dereferenced: every call below is refused by the argument checks
    B, H, D, heads = 4, 6, 16, 4
    for ln in (x, None):
        assert lib.tt_hist_embed_pool_len(None, 10, D, x, B, H, ln, x, x, x, 2 * D, x, None) == N.TT_E_BADARG
        assert b"null pointer" in lib.tt_last_error_string()
        assert lib.tt_hist_embed_pool_len(x, 10, D, x, B, H, ln, x, None, x, 2 * D, x, None) == N.TT_E_BADARG
        assert lib.tt_hist_embed_pool_len(x, 10, D, x, B, H, ln, x, x, x, 2 * D, None, None) == N.TT_E_BADARG  # the flag
        assert lib.tt_hist_embed_pool_len(x, 10, D, x, B, 0, ln, x, x, x, 2 * D, x, None) == N.TT_E_BADARG
        assert lib.tt_hist_embed_pool_len(x, 10, D, x, B, H, ln, x, x, x, D - 1, x, None) == N.TT_E_BADARG
        assert lib.tt_hist_pool_bwd_len(None, B, H, D, ln, x, 2 * D, None) == N.TT_E_BADARG
        assert lib.tt_hist_pool_bwd_len(x, B, H, D, ln, None, 2 * D, None) == N.TT_E_BADARG
        assert lib.tt_hist_pool_bwd_len(x, B, H, 0, ln, x, 2 * D, None) == N.TT_E_BADARG
        assert lib.tt_attn_fwd_len(None, B, H, D, heads, ln, x, x, None) == N.TT_E_BADARG
        assert lib.tt_attn_fwd_len(x, B, H, D, heads, ln, None, x, None) == N.TT_E_BADARG
        assert lib.tt_attn_fwd_len(x, B, H, D, 3, ln, x, x, None) == N.TT_E_BADARG  # D % heads
        assert lib.tt_attn_bwd_len(x, x, x, None, B, H, D, heads, ln, x, None) == N.TT_E_BADARG
        assert lib.tt_attn_bwd_len(x, x, x, x, B, H, D, heads, ln, None, None) == N.TT_E_BADARG
        assert lib.tt_attn_bwd_len(x, x, x, x, B, -1, D, heads, ln, x, None) == N.TT_E_BADARG
        assert lib.tt_enc_last_fwd_len(None, B, H, D, heads, ln, x, x, x, x, x, 2 * D, x, x, x, x, x, None) == N.TT_E_BADARG
        assert lib.tt_enc_last_fwd_len(x, B, H, D, heads, ln, x, x, x, x, x, 2 * D, x, x, None, x, x, None) == N.TT_E_BADARG
    assert lib.tt_enc_last_fwd_len(x, B, 65, D, heads, x, x, x, x, x, x, 2 * D, x, x, x, x, x, None) == N.TT_E_UNSUPPORTED
    # an empty batch is a no-op, lengths or not
    assert lib.tt_attn_fwd_len(x, 0, H, D, heads, x, x, x, None) == 0
    assert lib.tt_hist_pool_bwd_len(x, 0, H, D, x, x, 2 * D, None) == 0


def test_public_keywords():
    import two_tower_models_amd as A
    from two_tower_models_amd import ops
    for meth, names in ((A.UserHistoryEncoder.forward, ["self", "user_history", "lengths"]),
                        (A.UserHistoryEncoder.encode_ids, ["self", "item_table", "history_ids", "lengths"])):
        sig = inspect.signature(meth)
        assert list(sig.parameters) == names and sig.parameters["lengths"].default is None
    for cls in (A.TwoTowerBaseRetrieval, A.TwoTowerWithUserHistoryEncoder, A.TwoTowerWithDebiasing,
                A.TwoTowerWithPositionDebiasedWeights, A.TwoTowerWithUserDebiasedWeights, A.TwoTowerPlusLightRanker):
        for meth in (cls.train_forward, cls.forward):
            # the keyword sits on the wrapper (`takes_history_lengths`), behind everything the method itself takes ...
            outer = inspect.signature(meth, follow_wrapped=False).parameters
            assert list(outer)[-2] == "user_history_lengths" or list(outer)[-1] == "user_history_lengths", cls.__name__
            q = outer["user_history_lengths"]
            assert q.default is None and q.kind is inspect.Parameter.KEYWORD_ONLY
            # ... whose own parameter list is what it was
            assert "user_history_lengths" not in inspect.signature(meth).parameters
        # the overridable hooks keep their three-argument signatures
        for hook in (cls.process_user_features, cls.compute_user_embedding):
            assert list(inspect.signature(hook).parameters) == ["self", "user_id", "user_features", "user_history"]
    assert inspect.signature(ops.HistoryEncoder.apply).parameters["lengths"].default is None


def test_lengths_reach_the_summary_for_the_call_only_and_refusals(monkeypatch):
    """No GPU needed.  The lengths are visible to `_history_summary` while train_forward / forward runs -- through a
    subclass hook that calls super() too --, a user-supplied encoder gets `lengths=` only when lengths were given, nothing
    stays set after the call returns or raises; row-sharded models and the light-ranker model refuse the keyword."""
    import two_tower_models_amd as A
    from two_tower_models_amd import parallel
    mips = A.BaselineMIPSModule(16, 8)
    B, H = 4, 2
    args = [torch.zeros(B, dtype=torch.long), torch.zeros(B, 4), torch.zeros(B, H, dtype=torch.long),
            torch.zeros(B, dtype=torch.long), torch.zeros(B, 4), torch.zeros(B, dtype=torch.long), torch.ones(B, 1)]
    lengths = torch.tensor([1, 2, 2, 1])
    seen = []

    class Stop(Exception):
        pass

    class Probe(A.TwoTowerWithUserHistoryEncoder):
        def process_user_features(self, user_id, user_features, user_history):  # a hook that calls super()
            return super().process_user_features(user_id, user_features, user_history)

        def _history_summary(self, user_history):
            seen.append(self._tt_history_lengths)
            raise Stop()

    m = Probe(4, 10, 8, 4, H, 10, 8, 4, [1.0], mips)
    for call in (lambda **kw: m.train_forward(*args, **kw), lambda **kw: m(*args[:3], **kw)):
        with pytest.raises(Stop):
            call(user_history_lengths=lengths)
        assert seen.pop() is lengths and m._tt_history_lengths is None  # cleared although the call raised
        with pytest.raises(Stop):
            call()
        assert seen.pop() is None

    class Enc(torch.nn.Module):  # a user-supplied encoder: called with `lengths=` only when lengths were given
        def forward(self, *a, **kw):
            seen.append(kw)
            raise Stop()

    m2 = A.TwoTowerWithUserHistoryEncoder(4, 10, 8, 4, H, 10, 8, 4, [1.0], mips)
    m2.user_history_encoder = Enc()
    monkeypatch.setattr(A.ops.EmbeddingLookup, "apply", staticmethod(lambda w, ids: w[ids]))  # (the product lookup needs the GPU)
    for kw, want in ((dict(user_history_lengths=lengths), {"lengths": lengths}), (dict(), {})):
        with pytest.raises(Stop):
            with m2._history_lengths(kw.get("user_history_lengths")):
                m2._history_summary(args[2])
        got = seen.pop()
        assert set(got) == set(want) and all(got[k] is want[k] for k in want)
    monkeypatch.undo()
    # the base model takes the keyword and ignores it, as it ignores user_history (it stops at the CPU tensors)
    base = A.TwoTowerBaseRetrieval(4, 10, 8, 4, 10, 8, 4, [1.0], mips)
    with pytest.raises(RuntimeError, match="no CPU path"):
        base.train_forward(*args, user_history_lengths=lengths)
    assert base._tt_history_lengths is None
    # refusals
    base.item_id_embedding_arch.weight._tt_shard = parallel.RowShard(20, 8, 2, 0)
    m.item_id_embedding_arch.weight._tt_shard = parallel.RowShard(20, 8, 2, 0)
    for model in (base, m):
        with pytest.raises(NotImplementedError, match="row-sharded"):
            model.train_forward(*args, user_history_lengths=lengths)
        with pytest.raises(NotImplementedError, match="row-sharded"):
            model(*args[:3], user_history_lengths=lengths)
    lr = A.TwoTowerPlusLightRanker.__new__(A.TwoTowerPlusLightRanker)  # refused before anything of the model is used
    with pytest.raises(NotImplementedError, match="light-ranker"):
        A.TwoTowerPlusLightRanker.train_forward(lr, *args, user_history_lengths=lengths)
    with pytest.raises(NotImplementedError, match="light-ranker"):
        A.TwoTowerPlusLightRanker.forward(lr, *args[:3], user_history_lengths=lengths)


def test_history_encoder_op_checks_the_lengths_tensor():
    """Type and shape errors of `lengths` come before any kernel (and before the device check of the other inputs)."""
    from two_tower_models_amd import ops
    chk = ops.HistoryEncoder._lengths_i32
    assert chk(None, 4, torch.device("cpu")) is None
    with pytest.raises(TypeError):
        chk(torch.ones(4), 4, torch.device("cpu"))
    with pytest.raises(TypeError):
        chk([1, 2, 3, 4], 4, torch.device("cpu"))
    with pytest.raises(ValueError):
        chk(torch.ones(3, dtype=torch.long), 4, torch.device("cpu"))
    with pytest.raises(ValueError):
        chk(torch.ones(4, 1, dtype=torch.int32), 4, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        chk(torch.ones(4, dtype=torch.long), 4, torch.device("cpu"))


def test_train_parser_min_history_len_is_off_by_default():
    from two_tower_models_amd import train
    p = train.build_parser()
    assert p.parse_args([]).min_history_len is None
    assert p.parse_args(["--min_history_len", "3"]).min_history_len == 3
