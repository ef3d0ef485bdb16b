"""Pin the CPU oracle (oracle/cpu_ref.py) to the reference: every function is
checked against golden vectors the reference itself produced
(tests/golden/make_golden.py).  CPU-only."""
import numpy as np
import pytest
import torch

import fixture_gen as fg
from oracle import cpu_ref as R


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def params_of(g, prefix="p."):
    return {k[len(prefix):]: T(v) for k, v in g.items() if k.startswith(prefix)}


def batch_of(g, prefix="in.", labels_key="labels"):
    names = ("user_id", "user_features", "user_history", "item_id", "item_features", "position")
    return [T(g[prefix + n]) for n in names] + [T(g[prefix + labels_key])]


def grads_of(loss, leaves):
    gs = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    return {k: g for k, g in zip(leaves, gs) if g is not None}


# ---------------------------------------------------------------- encoder
def test_reference_known_answer_vectors(golden):
    """ref:tests/test_user_history_enc.py:48-124 through the oracle."""
    g = golden("g3_encoder_kat")
    x = T(g["x"])
    for tag, table in (("nope", None), ("pe", R.positional_table(3, 2))):
        layers = [(T(g[f"{tag}.p.multihead_attn_layers.0.in_proj_weight"]),
                   T(g[f"{tag}.p.multihead_attn_layers.0.in_proj_bias"]),
                   T(g[f"{tag}.p.multihead_attn_layers.0.out_proj.weight"]),
                   T(g[f"{tag}.p.multihead_attn_layers.0.out_proj.bias"]))]
        y = R.history_encoder_forward(x, layers, 1, table)
        assert torch.allclose(y, T(g[f"expected_{tag}"]), atol=1e-3)  # upstream's own tolerance
        assert torch.allclose(y, T(g[f"{tag}.out"]), atol=1e-6)


def test_positional_tables_bit_exact(golden):
    g = golden("g7_pe_tables")
    for key, want in g.items():
        _, H, D = key.split("_")
        got = R.positional_table(int(H), int(D)).numpy()
        assert np.array_equal(got, want), key


@pytest.mark.parametrize("name", ["g3_encoder_d128", "g3_encoder_d128_nope", "g3_encoder_odd"])
def test_encoder_forward_and_grads(golden, name):
    g = golden(name)
    D, H, heads, L, B, pe = (int(v) for v in g["cfg"])
    leaves = {k: v.requires_grad_(True) for k, v in params_of(g).items()}
    x = T(g["x"]).requires_grad_(True)
    table = T(g["pe_table"]) if pe else None
    if pe:
        assert np.array_equal(R.positional_table(H, D).numpy(), g["pe_table"])
    y = R.history_encoder_forward(x, R.encoder_layers_from_params(leaves, prefix=""), heads, table)
    assert torch.allclose(y, T(g["y"]), atol=2e-6, rtol=1e-5)
    obj = (y * T(g["cot"])).sum()
    gx, = torch.autograd.grad(obj, x, retain_graph=True)
    assert torch.allclose(gx, T(g["gx"]), atol=1e-6, rtol=1e-4)
    for k, gr in grads_of(obj, leaves).items():
        want = T(g["g." + k])
        assert torch.allclose(gr, want, atol=1e-5 * max(1.0, float(want.abs().max())), rtol=1e-4), k


# ---------------------------------------------------------------- base model
@pytest.mark.parametrize("name", ["g1_base_tiny", "g2_base_aligned", "g2_base_d256"])
def test_base_model_forward_loss_grads(golden, name):
    g = golden(name)
    leaves = {k: v.requires_grad_(True) for k, v in params_of(g).items()}
    b = batch_of(g)
    uvw = T(g["uvw"])
    u = R.user_embedding(leaves, b[0], b[1], b[2], with_history=False)
    it = R.item_embeddings(leaves, b[3], b[4])
    assert torch.allclose(u, T(g["user_emb"]), atol=1e-5)
    assert torch.allclose(it, T(g["item_emb"]), atol=1e-5)
    assert torch.allclose(R.inbatch_logits(u, it), T(g["scores"]), atol=1e-4)
    assert torch.allclose(R.inbatch_rowwise_ce(u, it), T(g["ce_rows"]), atol=1e-4)
    loss = R.train_forward(leaves, b, uvw)
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    for k, gr in grads_of(loss, leaves).items():
        want = T(g["g." + k])
        assert torch.allclose(gr, want, atol=1e-6, rtol=1e-4), k
    if "loss_labels_1d" in g:  # train.py's 1-D label quirk
        b1 = batch_of(g, labels_key="labels_1d")
        assert abs(float(R.train_forward(leaves, b1, uvw)) - float(g["loss_labels_1d"])) < 1e-5


def test_adam_trajectory_matches_torch_optim(golden):
    """3 iterations of the ref:train/train.py:112-132 loop body."""
    g = golden("g2_base_aligned")
    # NB: the fixture's step loop starts from the initial weights p.* (the grads
    # computed before it do not touch the parameters).
    params = {k: v.clone() for k, v in params_of(g).items()}
    state = R.AdamState(params)
    uvw = T(g["uvw"])
    losses = []
    for s in range(3):
        losses.append(R.train_step(params, state, batch_of(g, prefix=f"step{s}.in."), uvw, lr=1e-3))
    assert np.allclose(losses, g["adam_losses"], atol=1e-5)
    after = params_of(g, prefix="after.")
    for k, v in params.items():
        # item_tower_arch.bias / item_features_arch.2.bias have an analytically ZERO
        # gradient (adding a constant vector to every item embedding shifts each
        # logit row by a constant, which softmax ignores): what reaches Adam is
        # ~1e-8 rounding noise that m/sqrt(v) normalises to O(lr) steps of
        # arbitrary sign.  Parity for them is bounded by steps*lr, not by ulps.
        noise_only = float(np.abs(g["g." + k]).max()) < 1e-6
        atol = 2 * 3 * 1e-3 * 1.05 if noise_only else 2e-6  # each run may step +-lr per step
        assert torch.allclose(v, after[k], atol=atol, rtol=1e-5), k
    # rows never looked up still moved?  (they must not: zero grad + zero state)
    touched = np.unique(np.concatenate([g[f"step{s}.in.item_id"] for s in range(3)]))
    untouched = np.setdiff1d(np.arange(params["item_id_embedding_arch.weight"].shape[0]), touched)
    if len(untouched):
        assert torch.equal(params["item_id_embedding_arch.weight"][untouched],
                           T(g["p.item_id_embedding_arch.weight"])[untouched])


# ---------------------------------------------------------------- history model
@pytest.mark.parametrize("name", ["g4_hist_d128", "g4_hist_tiny"])
def test_history_model(golden, name):
    g = golden(name)
    leaves = {k: v.requires_grad_(True) for k, v in params_of(g).items()}
    b = batch_of(g)
    kw = dict(with_history=True, heads=4, pos_table=T(g["pe_table"]))
    u = R.user_embedding(leaves, b[0], b[1], b[2], **kw)
    assert torch.allclose(u, T(g["user_emb"]), atol=1e-5)
    loss = R.train_forward(leaves, b, T(g["uvw"]), **kw)
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    for k, gr in grads_of(loss, leaves).items():
        want = T(g["g." + k])
        assert torch.allclose(gr, want, atol=1e-6, rtol=2e-4), k


def test_debias_model_loss_grads_and_topk(golden):
    g = golden("g6_debias_d128")
    # the oracle runs in float64 here: how a float32 evaluation of this model's gradients rounds depends on the host CPU's
    # BLAS kernels, and on some CPUs it lands outside the tolerance; a float64 one is the same everywhere
    f64 = lambda t: t.double() if t.is_floating_point() else t  # noqa: E731
    leaves = {k: f64(v).requires_grad_(True) for k, v in params_of(g).items()}
    b = [f64(t) for t in batch_of(g)]
    kw = dict(with_history=True, heads=4, pos_table=f64(T(g["pe_table"])))
    loss = R.train_forward(leaves, b, f64(T(g["uvw"])), debias=R.debias_combined, **kw)
    assert abs(float(loss) - float(g["loss"])) < 1e-4 * max(1.0, abs(float(g["loss"])))
    for k, gr in grads_of(loss, leaves).items():
        want = f64(T(g["g." + k]))
        assert torch.allclose(gr, want, atol=1e-5 * max(1.0, float(want.abs().max())), rtol=2e-4), k
    corpus = T(fg.bf16_round(fg.gaussianish((4096, 128), 901)))
    with torch.no_grad():
        u = R.user_embedding(leaves, b[0], b[1], b[2], **kw).float()
    idx, _, _ = R.mips_topk(u, corpus, 10)
    gate = g["topk_gap_min"] > 1e-3  # margin-gated rows must match exactly
    assert gate.sum() >= 32
    assert np.array_equal(idx.numpy()[gate], g["top_items"][gate])


@pytest.mark.parametrize("kind", ["position", "user"])
def test_single_term_debias_heads_loss_and_grads(golden, kind):
    """The two sibling heads of SURVEY 8f item 2 (ref:src/two_tower_with_position_debiased_weights.py:76-113, clamp 1e-3
    after the MSE; ref:src/two_tower_with_user_debiased_weights.py:102-135, clamp 1e-1 before it): loss and every
    gradient, including the head's own parameters, against fixtures produced by the reference classes."""
    g = golden(f"g8_debias_{kind}")
    leaves = {k: v.requires_grad_(True) for k, v in params_of(g).items()}
    kw = dict(with_history=True, heads=4, pos_table=T(g["pe_table"]))
    loss = R.train_forward(leaves, batch_of(g), T(g["uvw"]), debias=R.debias_position if kind == "position" else R.debias_user, **kw)
    assert abs(float(loss) - float(g["loss"])) < 1e-4 * max(1.0, abs(float(g["loss"])))
    for k, gr in grads_of(loss, leaves).items():
        want = T(g["g." + k])
        assert torch.allclose(gr, want, atol=1e-5 * max(1.0, float(want.abs().max())), rtol=2e-4), k


# ---------------------------------------------------------------- MIPS
@pytest.mark.parametrize("C", [4096, 65536])
@pytest.mark.parametrize("K", [10, 1000])
def test_mips_exact_corpus_bit_exact(golden, C, K):
    g = golden("g5_mips")
    corpus = T(fg.exact_mips_corpus(C, 128))
    q = T(fg.exact_mips_queries(16, 128))
    assert torch.equal(R.round_to_bf16(corpus), corpus) and torch.equal(R.round_to_bf16(q), q)
    idx, sc, rows = R.mips_topk(q, corpus, K)
    assert np.array_equal(idx.numpy(), g[f"exact_C{C}_K{K}.idx"].astype(np.int64))
    assert np.array_equal(sc.numpy(), g[f"exact_C{C}_K{K}.scores"])
    assert torch.equal(rows, corpus[idx])


@pytest.mark.parametrize("K", [10, 300])
def test_mips_exact_corpus_d256_bit_exact(golden, K):
    g = golden("g5_mips_d256")
    corpus, q = T(fg.exact_mips_corpus(4096, 256)), T(fg.exact_mips_queries(16, 256))
    idx, sc, _ = R.mips_topk(q, corpus, K)
    assert np.array_equal(idx.numpy(), g[f"exact_C4096_K{K}.idx"].astype(np.int64))
    assert np.array_equal(sc.numpy(), g[f"exact_C4096_K{K}.scores"])


@pytest.mark.parametrize("K", [10, 100])
def test_mips_random_corpus(golden, K):
    g = golden("g5_mips")
    corpus = T(fg.bf16_round(fg.gaussianish((4096, 128), 901)))
    q = T(fg.bf16_round(fg.gaussianish((16, 128), 902)))
    idx, sc, _ = R.mips_topk(q, corpus, K)
    want = g[f"rand_C4096_K{K}.idx"].astype(np.int64)
    gate = g[f"rand_gap_min_K{K}"] > 1e-4
    assert np.array_equal(idx.numpy()[gate], want[gate])
    # non-gated rows: same SET up to sub-margin neighbour swaps
    for r in np.nonzero(~gate)[0]:
        assert len(set(idx.numpy()[r]) ^ set(want[r])) <= 2
    assert np.allclose(sc.numpy(), g[f"rand_C4096_K{K}.scores"], atol=1e-4)
