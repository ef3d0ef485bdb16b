"""TwoTowerPlusLightRanker on MI355X (`pytest -m gpu`): loss, every gradient and a two-step Adam trajectory against
the reference class (fixtures g9_light_ranker_*, tests/golden/make_golden_light_ranker.py), reranked ids against the
reference's forward, the rerank kernel against a float64 restatement, the two candidate-row sources, the fused head
against the reference expressions, graph replay, and the error paths."""
import os

import numpy as np
import pytest
import torch

import fixture_gen as fg
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["g9_light_ranker_tiny", "g9_light_ranker_d128"]
BATCH = ("user_id", "user_features", "user_history", "item_id", "item_features", "position", "labels")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def golden_lr(name):
    g, k = load_golden(name), 1
    while os.path.exists(os.path.join(GOLDEN, f"{name}.p{k}.npz")):
        g.update(load_golden(f"{name}.p{k}"))
        k += 1
    return g


def cfg(g):
    return dict(zip(("n_users", "du", "iu", "n_items", "di", "ii", "T", "B", "H", "NU", "NI", "K", "C"),
                    (int(x) for x in g["cfg"])))


def corpus_of(g):
    c = cfg(g)
    return T(fg.bf16_round(fg.gaussianish((c["C"], c["di"]), 903)))


def make_lr(g, mips_cls=None):
    """The reference's seeded init, rebuilt (d128) or loaded (tiny), and the fixture's corpus."""
    import two_tower_models_amd as A
    c = cfg(g)
    torch.manual_seed(0)
    mips = (mips_cls or A.BaselineMIPSModule)(corpus_size=c["C"], embedding_dim=c["di"])
    m = A.TwoTowerPlusLightRanker(num_items=c["K"], num_mips_items=c["NI"], num_ranker_user_embeddings=c["NU"],
                                  user_id_hash_size=c["n_users"], user_id_embedding_dim=c["du"], user_features_size=c["iu"],
                                  user_history_seqlen=c["H"], item_id_hash_size=c["n_items"], item_id_embedding_dim=c["di"],
                                  item_features_size=c["ii"], user_value_weights=[float(x) for x in g["uvw"]],
                                  mips_module=mips)
    sd = m.state_dict()
    for i, k in enumerate(g["state_keys"]):
        v = sd[str(k)]
        if "p." + str(k) in g:
            assert torch.equal(v, T(g["p." + str(k)])), k
        assert v.double().sum().item() == float(g["init_sum"][i]), k
        assert v.double().abs().sum().item() == float(g["init_abs"][i]), k
    mips.corpus = corpus_of(g)
    return m.to(DEV)


def grad_scale(grads, name):
    """The size of the per-row terms a parameter's gradient sums.  A bias gradient is the column sum of the same rows
    whose outer products give its weight's gradient; where those rows cancel (the item tower's biases: the in-batch
    softmax part is analytically zero, and the MIPS weights reach 1 / 1e-3 through the debias hook's clamp) only the
    weight's scale says what rounding noise is."""
    scale = float(np.abs(grads[name]).max())
    if name.endswith(".bias") and name[:-5] + ".weight" in grads:
        scale = max(scale, float(np.abs(grads[name[:-5] + ".weight"]).max()))
    return scale


def check_grads(model, g, rtol=5e-4, atol_scale=4e-5):
    """test_gpu_models.check_grads's tolerances (the debias heads': rtol 5e-4, 4e-5 of the gradient's scale), the scale
    taken by grad_scale."""
    grads = {k[2:]: v for k, v in g.items() if k.startswith("g.")}
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        want = T(grads[name])
        tol = max(atol_scale * grad_scale(grads, name), 1e-7)
        got = p.grad.cpu()
        assert torch.allclose(got, want, atol=tol, rtol=rtol), (name, float((got - want).abs().max()), tol)


def assert_reference_trajectory(model, g, steps=2, lr=1e-3):
    """State after the fixture's Adam steps vs the reference's `after.*`: every element within the steps * 2 * lr bound
    (Adam's first update is lr * g / |g|: an element whose gradient is rounding noise may step either way), and all but
    0.1 % of the elements whose first gradient is at least 2 % of its tensor's scale within 5e-6."""
    grads = {k[2:]: v for k, v in g.items() if k.startswith("g.")}
    for k, v in model.state_dict().items():
        want = T(g["after." + k])
        err = (v.cpu() - want).abs() - 1e-5 * want.abs()
        assert float(err.max()) <= 2 * steps * lr * 1.05, (k, float(err.max()))
        if k in grads:
            big = torch.from_numpy(np.abs(grads[k])).reshape(err.shape) >= 2e-2 * grad_scale(grads, k)
            n_out = int((err[big] > 5e-6).sum())
            assert n_out <= max(1, int(1e-3 * int(big.sum()))), (k, n_out, float(err.max()))


def batch_of(g, prefix="in."):
    return [T(g[prefix + n]).to(DEV) for n in BATCH]


def values64(R, rows, score, W, b, uvw):
    """ref:src/two_tower_plus_light_ranker.py:165-199 in float64: R [B, NU, DI], rows [B, NI, DI], score [B, NI]."""
    R, rows, score, W, b, uvw = (x.double() for x in (R, rows, score, W, b, uvw))
    s = torch.bmm(R, rows.transpose(1, 2)).transpose(1, 2)  # [B, NI, NU]
    t = torch.bmm(torch.softmax(s, dim=2), R)
    z = torch.cat([rows, t, s, score.unsqueeze(2)], dim=2)
    return ((z @ W.t() + b) * uvw).sum(dim=2)


# ------------------------------------------------------------------ 1. golden parity: loss, gradients, Adam
@pytest.mark.parametrize("name", NAMES)
def test_loss_and_grads_match_reference(name):
    g = golden_lr(name)
    model = make_lr(g)
    loss = model.train_forward(*batch_of(g))
    assert abs(loss.item() - float(g["loss"])) < 1e-4 * max(1.0, abs(float(g["loss"])))
    loss.backward()
    assert model.ranker_user_tower.weight.grad is not None and model.light_ranker.bias.grad is not None
    check_grads(model, g)


@pytest.mark.parametrize("name", NAMES)
def test_dense_exact_adam_matches_reference_trajectory(name):
    import two_tower_models_amd as A
    g = golden_lr(name)
    model = make_lr(g)
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3)
    losses = []
    for s in range(2):
        loss = model.train_forward(*batch_of(g, prefix=f"step{s}.in."))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    opt.flush()
    assert np.allclose(losses, g["adam_losses"], atol=1e-4)
    assert_reference_trajectory(model, g)


# ------------------------------------------------------------------ 2. forward against the reference's top items
@pytest.mark.parametrize("name", NAMES)
def test_forward_matches_reference_top_items(name):
    g = golden_lr(name)
    c = cfg(g)
    model = make_lr(g)
    b = batch_of(g)
    top = model(b[0], b[1], b[2]).cpu()
    assert top.shape == (c["B"], c["K"]) and top.dtype == torch.int64
    want = T(g["top_items"])
    # float64 values of any corpus item for each query, from the reference's own user / ranker embeddings
    u, R = T(g["user_emb"]).double(), T(g["ranker_emb"]).double()
    corpus = corpus_of(g).double()
    lin = model.light_ranker
    W, bias, uvw = lin.weight.detach().cpu(), lin.bias.detach().cpu(), T(g["uvw"])
    for q in range(c["B"]):
        got_set, want_set = set(top[q].tolist()), set(want[q].tolist())
        assert len(got_set) == c["K"]
        if got_set == want_set:
            continue
        items = torch.tensor(sorted(got_set | want_set))
        rows = corpus[items].unsqueeze(0)
        val = values64(R[q:q + 1], rows, (rows[0] @ u[q]).unsqueeze(0), W, bias, uvw)[0]
        v_of = dict(zip(items.tolist(), val.tolist()))
        kth = min(v_of[i] for i in want_set)
        for i in got_set ^ want_set:
            assert abs(v_of[i] - kth) <= 1e-5 * abs(kth), (q, i, v_of[i], kth)


# ------------------------------------------------------------------ 3. rerank kernel against float64
def _rerank_case(B=256, NI=1000, K=100, C=1 << 20, NU=4, DI=128, T_=4, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    corpus = torch.randn(C, DI, device=DEV, generator=gen)
    R = torch.randn(B, NU, DI, device=DEV, generator=gen) * 0.2
    W = torch.randn(T_, 2 * DI + NU + 1, device=DEV, generator=gen) * 0.05
    b = torch.randn(T_, device=DEV, generator=gen)
    uvw = torch.rand(T_, device=DEV, generator=gen) + 0.1
    idx = torch.randint(0, C, (B, NI), device=DEV, generator=gen)
    scores = torch.randn(B, NI, device=DEV, generator=gen) * 5
    return corpus, R, W, b, uvw, idx, scores, K


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rerank_values_and_order_against_float64(dtype):
    from two_tower_models_amd import ops
    corpus, R, W, b, uvw, idx, scores, K = _rerank_case()
    corpus = corpus.to(dtype)
    ids, vals = ops.light_ranker_rerank(R, W, b, uvw, idx, scores, K, corpus=corpus, return_values=True)
    want = values64(R, corpus[idx].float(), scores, W, b, uvw)
    err = (vals.double() - want).abs()
    assert float(err.max()) <= 1e-4 * float(want.abs().max()), float(err.max())
    # the ids are the top K of the kernel's own values, ties to the lower candidate position
    order = torch.sort(vals, dim=1, descending=True, stable=True).indices[:, :K]
    assert torch.equal(ids, torch.gather(idx, 1, order))
    # ... and the top K of the float64 values up to near-ties at the K-th value
    srt = torch.sort(want, dim=1, descending=True).values
    kth = srt[:, K - 1:K]
    w_ids = torch.gather(idx, 1, torch.sort(want, dim=1, descending=True, stable=True).indices[:, :K])
    for q in range(idx.shape[0]):
        diff = set(ids[q].tolist()) ^ set(w_ids[q].tolist())
        if diff:
            pos = [int((idx[q] == i).nonzero()[0]) for i in diff]
            assert all(abs(float(want[q, p] - kth[q])) <= 1e-5 * abs(float(kth[q])) + 1e-6 for p in pos), q


def test_rerank_ties_go_to_the_lower_candidate_position():
    from two_tower_models_amd import ops
    corpus, R, W, b, uvw, idx, scores, K = _rerank_case(B=8, NI=300, K=50, C=4096)
    rows = corpus[7].expand(idx.shape[0], idx.shape[1], -1).contiguous()  # one row and one score for every candidate
    scores = torch.ones_like(scores)
    pos = torch.arange(idx.shape[1], device=DEV).expand_as(idx).contiguous()  # ids that show the positions chosen
    ids, vals = ops.light_ranker_rerank(R, W, b, uvw, pos, scores, K, rows=rows, return_values=True)
    assert bool((vals == vals[:, :1]).all())
    assert torch.equal(ids, pos[:, :K])


# ------------------------------------------------------------------ 4. index mode == dense-rows mode
def test_index_and_dense_row_sources_give_the_same_bits():
    import two_tower_models_amd as A
    from two_tower_models_amd import ops

    class OwnMIPS(A.BaselineMIPSModule):  # a caller's own module: the reference's 3-tuple call, dense rows
        def forward(self, query_embedding, num_items):
            return super().forward(query_embedding, num_items)

    g = golden_lr("g9_light_ranker_d128")
    b = batch_of(g)
    for bf16 in (False, True):
        m1, m2 = make_lr(g), make_lr(g, mips_cls=OwnMIPS)
        if bf16:
            m1.mips_module.use_bf16_storage()
            m2.mips_module.use_bf16_storage()
        assert torch.equal(m1(b[0], b[1], b[2]), m2(b[0], b[1], b[2]))
    corpus, R, W, bb, uvw, idx, scores, K = _rerank_case(B=64, NI=500, K=40, C=1 << 16)
    for c in (corpus, corpus.to(torch.bfloat16)):
        i1, v1 = ops.light_ranker_rerank(R, W, bb, uvw, idx, scores, K, corpus=c, return_values=True)
        i2, v2 = ops.light_ranker_rerank(R, W, bb, uvw, idx, scores, K, rows=ops.gather_corpus_rows(c, idx),
                                         return_values=True)
        assert torch.equal(v1, v2) and torch.equal(i1, i2)


# ------------------------------------------------------------------ 5. fused head == reference expressions; determinism
def _grads(model):
    return {k: p.grad.clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize("name", NAMES)
def test_fused_head_matches_reference_expressions_and_is_deterministic(name):
    g = golden_lr(name)
    b = batch_of(g)
    runs = []
    for fused in (True, True, False):
        model = make_lr(g)
        if not fused:
            model._fused_sizes = lambda: False  # the reference's tensor expressions on the GPU
        loss = model.train_forward(*b)
        loss.backward()
        runs.append((loss.detach(), _grads(model)))
        if not fused:  # same ranking from both rerank paths
            top_ref = model(b[0], b[1], b[2])
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    assert abs(runs[0][0].item() - runs[2][0].item()) <= 1e-5 * max(1.0, abs(runs[2][0].item()))
    general = {k: v.cpu().numpy() for k, v in runs[2][1].items()}
    for k, want in runs[2][1].items():
        tol = max(2e-5 * grad_scale(general, k), 1e-7)
        assert torch.allclose(runs[0][1][k], want, atol=tol, rtol=1e-4), (k, float((runs[0][1][k] - want).abs().max()))
    top = make_lr(g)(b[0], b[1], b[2])
    agree = (top.sort(dim=1).values == top_ref.sort(dim=1).values).float().mean().item()
    assert agree > 0.98, agree


# ------------------------------------------------------------------ 6. graph replay == eager
def test_graphed_train_step_is_bit_identical_to_eager():
    import two_tower_models_amd as A
    g = golden_lr("g9_light_ranker_d128")
    bs = [batch_of(g, prefix=p) for p in ("in.", "step0.in.", "step1.in.")]
    eager = make_lr(g)
    eopt = A.DenseExactAdam(eager.parameters(), lr=1e-3, overlap_sweep=False)
    elosses = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for b in bs:
            loss = eager.train_forward(*b)
            eopt.zero_grad()
            loss.backward()
            eopt.step()
            elosses.append(loss.item())
        eopt.flush()
    torch.cuda.current_stream().wait_stream(side)
    del loss
    model = make_lr(g)
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep=False)
    step = A.GraphedTrainStep(model, opt, bs[0], warmup=1)
    glosses = [step(*b).item() for b in bs[1:]]
    opt.flush()
    torch.cuda.synchronize()
    assert glosses == elosses[1:]
    for (k, a), (_, b) in zip(eager.state_dict().items(), model.state_dict().items()):
        assert torch.equal(a, b), k


# ------------------------------------------------------------------ 7. error paths
def test_out_of_range_candidate_raises_index_error():
    import two_tower_models_amd as A

    class BadSearch(A.BaselineMIPSModule):
        def search(self, query_embedding, num_items):
            idx, sc = super().search(query_embedding, num_items)
            idx[:, -1] = self.corpus.shape[0]  # one row past the corpus
            return idx, sc

    g = golden_lr("g9_light_ranker_tiny")
    model = make_lr(g, mips_cls=BadSearch)
    b = batch_of(g)
    with pytest.raises(IndexError):
        model(b[0], b[1], b[2])
    model.mips_module.__class__ = A.BaselineMIPSModule
    assert model(b[0], b[1], b[2]).shape == (cfg(g)["B"], cfg(g)["K"])  # the flag was consumed


def test_num_items_above_num_mips_items_raises():
    g = golden_lr("g9_light_ranker_tiny")
    model = make_lr(g)
    model.num_items = model.num_mips_items + 1
    b = batch_of(g)
    with pytest.raises(RuntimeError, match="selected index k out of range"):
        model(b[0], b[1], b[2])


# ------------------------------------------------------------------ 8. full-size head against float64
def test_head_full_size_against_float64():
    from two_tower_models_amd import ops
    B, DI, NU, T_ = 8192, 128, 4, 4
    gen = torch.Generator(device=DEV).manual_seed(3)
    R = (torch.randn(B, NU, DI, device=DEV, generator=gen) * 0.1).requires_grad_()
    u = (torch.randn(B, DI, device=DEV, generator=gen) * 0.1).requires_grad_()
    v = (torch.randn(B, DI, device=DEV, generator=gen) * 0.1).requires_grad_()
    W = (torch.randn(T_, 2 * DI + NU + 1, device=DEV, generator=gen) * 0.05).requires_grad_()
    bias = torch.randn(T_, device=DEV, generator=gen).requires_grad_()
    labels = (torch.rand(B, T_, device=DEV, generator=gen) > 0.5).float()
    loss = ops.LightRankerHead.apply(R, u, v, labels, W, bias)
    loss.backward()
    leaves = (R, u, v, W, bias)
    got = [x.grad.clone() for x in leaves]
    d = [x.detach().double().requires_grad_() for x in leaves]
    R6, u6, v6, W6, b6 = d
    s = torch.bmm(R6, v6.unsqueeze(2)).squeeze(2)
    t = torch.bmm(torch.softmax(s, dim=1).unsqueeze(1), R6).squeeze(1)
    z = torch.cat([v6, t, s, (u6 * v6).sum(1, keepdim=True)], dim=1)
    want = torch.nn.functional.binary_cross_entropy_with_logits(z @ W6.t() + b6, labels.double())
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-6 * max(1.0, abs(want.item()))
    for name, a, w in zip("R u v W b".split(), got, (x.grad for x in d)):
        err = float((a.double() - w).abs().max())
        assert err <= 1e-5 * float(w.abs().max()) + 1e-12, (name, err, float(w.abs().max()))
