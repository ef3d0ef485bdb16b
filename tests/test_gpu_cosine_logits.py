"""`use_cosine_logits` at the model level, on MI355X (`pytest -m gpu`): loss and every parameter gradient -- item-table rows
and `logit_log_scale` included -- against a float64 restatement (the oracle's towers in float64, F.normalize, / tau, then the
unchanged head), the optimiser's first step on the learned scale, a fixed scale that stays fixed, the launches a cosine step
adds, graph replay, serving, and the refusals.  Bounds: the project's model-level figures (loss 1e-4 relative, gradients
1e-5 max|g| + 2e-4 |g|)."""
import math
import warnings

import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref as R
from test_gpu_accidental_hits import CONFIGS, the_batch, the_extras
from test_gpu_logq import DEV, Tn_, batch_of, make_model, state_of

pytestmark = pytest.mark.gpu

VARIANTS = ("plain", "logq", "neg", "hits")
SCALES = ((0.05, True), (1.0, False), (1.0, True), (0.05, False))  # (temperature, learnable): each config meets all four


def log_scale_of(temperature):
    return torch.full((1,), -math.log(temperature), dtype=torch.float32)  # what use_cosine_logits registers


def restated_loss(params, log_scale, batch, uvw, extra, kind, gd, *, cosine=True, masked=False, debias=R.debias_identity,
                  head_sees_normalised=False, dtype=torch.float64):
    """float64: the oracle's towers; the logits' operands through F.normalize and exp(log_scale) (cosine) or as they are; log-Q
    term, accidental-hit mask, cross entropy; then the reference's head on the towers' OWN user embedding."""
    user_id, user_features, user_history, item_id, item_features, position, labels = batch
    fkw = dict(with_history=True, heads=4, pos_table=Tn_(gd["pe_table"]).to(dtype)) if kind != "base" else dict(with_history=False)
    u = R.user_embedding(params, user_id, user_features.to(dtype), user_history, **fkw)
    ids, feats = item_id, item_features.to(dtype)
    if "negative_item_id" in extra:
        ids = torch.cat([item_id, extra["negative_item_id"]])
        feats = torch.cat([feats, extra["negative_item_features"].to(dtype)])
    it = R.item_embeddings(params, ids, feats)
    lu, li = u, it
    if cosine:
        lu = torch.exp(log_scale.to(dtype)) * F.normalize(u, dim=1, eps=1e-12)
        li = F.normalize(it, dim=1, eps=1e-12)
    scores = lu @ li.t()
    if "item_log_q" in extra:
        log_q = torch.cat([extra["item_log_q"], extra["negative_log_q"]]) if "negative_log_q" in extra else extra["item_log_q"]
        scores = scores - log_q.to(dtype)[None, :]
    B = u.shape[0]
    target = torch.arange(B)
    if masked:
        hit = (ids[None, :] == ids[:B, None]) & (torch.arange(ids.shape[0])[None, :] != target[:, None])
        scores = scores.masked_fill(hit, float("-inf"))
    ce = F.cross_entropy(scores, target, reduction="none")
    nuv = R.net_user_value(labels.to(dtype), uvw.to(dtype))
    nuv, aux = debias(nuv, position, lu if head_sees_normalised else u, params)
    return torch.mean(ce * R.normalise_value_weights(nuv)) + aux


def extras_of(gd, B, variant, seed):
    return the_extras(gd, B, {"plain": "none", "hits": "none"}.get(variant, variant), seed)


def check_grads(model, grads, skip=()):
    worst = ("", 0.0)
    for pname, p in model.named_parameters():
        if pname in skip:
            continue
        w = grads[pname]
        w = torch.zeros_like(p, device="cpu", dtype=torch.float64) if w is None else w.double()
        assert p.grad is not None, pname
        got = p.grad.cpu().double()
        tol = max(1e-5 * float(w.abs().max()), 1e-7)  # floor: the analytically-zero gradients hold ~1e-8 of rounding noise
        rel = float(((got - w).abs() - 2e-4 * w.abs()).max()) / tol
        worst = max(worst, (pname, rel), key=lambda t: t[1])
        assert torch.allclose(got, w, atol=tol, rtol=2e-4), (pname, float((got - w).abs().max()), tol)
    return worst


def float64_side(gd, kind, cpu, extra, temperature, learnable, variant, debias=R.debias_identity, dot_condition=True):
    leaves = {k: v.double().requires_grad_(True) for k, v in state_of(gd).items()}
    ls = log_scale_of(temperature).double().requires_grad_(True)
    uvw = Tn_(gd["uvw"])
    want = restated_loss(leaves, ls, cpu, uvw, extra, kind, gd, masked=variant == "hits", debias=debias)
    dot = restated_loss(leaves, ls, cpu, uvw, extra, kind, gd, cosine=False, masked=variant == "hits", debias=debias)
    g = torch.autograd.grad(want, list(leaves.values()) + [ls], allow_unused=True)
    grads = dict(zip(list(leaves) + ["logit_log_scale"], g))
    # conditions of the fixture: cosine logits are another loss than dot-product logits, and the scale has a gradient
    want, dot = want.detach(), dot.detach()
    if dot_condition:
        assert abs(float(want) - float(dot)) > 100 * 1e-4 * max(1.0, abs(float(want))), (float(want), float(dot))
    g_ls = abs(float(grads["logit_log_scale"]))
    assert g_ls > 100 * (max(1e-5 * g_ls, 1e-7) + 2e-4 * g_ls), g_ls
    return want, dot, grads


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_cosine_train_forward_matches_float64(golden, config, variant):
    kind, name, repeat, fold = CONFIGS[config]
    temperature, learnable = SCALES[(list(CONFIGS).index(config) + VARIANTS.index(variant)) % 4]
    gd = golden(name)
    cpu = the_batch(gd, repeat, "cpu", fold)
    B = cpu[0].shape[0]
    extra = extras_of(gd, B, variant, seed=900 + B)
    want, dot, grads = float64_side(gd, kind, cpu, extra, temperature, learnable, variant)
    model = make_model(kind, gd).use_cosine_logits(temperature, learnable=learnable)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = model.train_forward(*the_batch(gd, repeat, DEV, fold), **{k: v.to(DEV) for k, v in extra.items()},
                                   remove_accidental_hits=variant == "hits")
    loss.backward()
    print(f"COSINE {config} {variant} tau={temperature} learnable={learnable}: loss {loss.item():.6f} float64 {float(want):.6f} "
          f"(dot product {float(dot):.6f}), d/dlog_scale float64 {float(grads['logit_log_scale']):.6e}")
    assert loss.dim() == 0 and abs(loss.item() - float(want)) < 1e-4 * max(1.0, abs(float(want)))
    assert ("logit_log_scale" in dict(model.named_parameters())) == learnable
    print("  worst", check_grads(model, grads))
    if not learnable:
        assert model.logit_log_scale.grad is None and not model.logit_log_scale.requires_grad


def test_debias_head_sees_the_towers_own_user_embedding(golden):
    """TwoTowerWithDebiasing: the head's Linear(DI + 1 -> 1) reads `user_embedding`.  Against float64 with the head on the
    un-normalised embedding; the same restatement with the head on the normalised one is far outside the bound.  (This
    model's loss is its two sum-MSE terms, ~3108 next to a cross entropy of ~3: no choice of logits moves it by 100 x its
    bound of 0.31, so the cosine-against-dot-product condition of the other cases is replaced by that one here; the
    condition on d loss / d log_scale holds as everywhere.)
    Loss and d loss / d log_scale against float64.  The other gradients against the float32 torch-CPU restatement, as
    tests/test_gpu_logq.py does for this model and for the reason it gives: the sum-MSE terms put float32 rounding of a loss
    of 3108 into the user-side gradients, and the float32 CPU restatement of these very expressions already sits 1.02 x the
    bound away from float64 on user_tower_arch.weight (0.90 x on user_features_arch.0.weight) before any kernel runs
    (profiles/l2norm_reference_tolerance.txt)."""
    gd = golden("g6_debias_d128")
    cpu = batch_of(gd, dev="cpu")
    cpu[3] = cpu[3] % 16
    want, dot, grads = float64_side(gd, "debias", cpu, {}, 0.05, True, "plain", debias=R.debias_combined,
                                     dot_condition=False)
    leaves = {k: v.double() for k, v in state_of(gd).items()}
    wrong = restated_loss(leaves, log_scale_of(0.05), cpu, Tn_(gd["uvw"]), {}, "debias", gd, debias=R.debias_combined,
                          head_sees_normalised=True)
    assert abs(float(wrong) - float(want)) > 100 * 1e-4 * abs(float(want))
    model = make_model("debias", gd).use_cosine_logits(0.05, learnable=True)
    dev = batch_of(gd)
    dev[3] = dev[3] % 16
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = model.train_forward(*dev)
    loss.backward()
    print(f"COSINE debias: loss {loss.item():.6f} float64 {float(want):.6f} (head on the normalised embedding {float(wrong):.6f})")
    assert abs(loss.item() - float(want)) < 1e-4 * max(1.0, abs(float(want)))
    g_ls = {"logit_log_scale": grads["logit_log_scale"]}
    check_grads(model, g_ls, skip=[n for n, _ in model.named_parameters() if n not in g_ls])
    l32 = {k: v.float().requires_grad_(True) for k, v in state_of(gd).items()}
    ls32 = log_scale_of(0.05).requires_grad_(True)
    w32 = restated_loss(l32, ls32, cpu, Tn_(gd["uvw"]), {}, "debias", gd, debias=R.debias_combined, dtype=torch.float32)
    grads32 = dict(zip(list(l32) + ["logit_log_scale"], torch.autograd.grad(w32, list(l32.values()) + [ls32], allow_unused=True)))
    print("  worst", check_grads(model, grads32, skip=["logit_log_scale"]))


def one_step(model, opt, batch, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = model.train_forward(*batch, **kw)
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss


@pytest.mark.parametrize("config", ["base-256x128", "hist-tiny"])
def test_first_adam_step_moves_the_learned_scale_by_lr(golden, config):
    """Adam's first step is lr * g / (|g| + 1e-8): the scale moves by -lr * sign(g_ref) to within 1e-3 lr."""
    import two_tower_models_amd as A
    kind, name, repeat, fold = CONFIGS[config]
    gd = golden(name)
    cpu = the_batch(gd, repeat, "cpu", fold)
    _, _, grads = float64_side(gd, kind, cpu, {}, 0.05, True, "plain")
    g_ref = float(grads["logit_log_scale"])
    lr = 1e-3
    model = make_model(kind, gd).use_cosine_logits(0.05, learnable=True)
    before = float(model.logit_log_scale.detach())
    opt = A.DenseExactAdam(model.parameters(), lr=lr)
    one_step(model, opt, the_batch(gd, repeat, DEV, fold))
    opt.flush()
    torch.cuda.synchronize()
    moved = float(model.logit_log_scale.detach()) - before
    print(f"COSINE adam {config}: g_ref {g_ref:.4e}, moved {moved:.6e}")
    assert abs(moved - (-lr * math.copysign(1.0, g_ref))) <= 1e-3 * lr
    assert abs(model.logit_temperature - math.exp(-float(model.logit_log_scale.detach()))) < 1e-9


def test_fixed_scale_has_no_grad_and_does_not_move(golden):
    import two_tower_models_amd as A
    kind, name, repeat, fold = CONFIGS["base-256x128"]
    gd = golden(name)
    model = make_model(kind, gd).use_cosine_logits(0.05)
    before = model.logit_log_scale.clone()
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3)
    w0 = model.user_tower_arch.weight.detach().clone()
    one_step(model, opt, the_batch(gd, repeat, DEV, fold))
    opt.flush()
    torch.cuda.synchronize()
    assert model.logit_log_scale.grad is None
    assert torch.equal(model.logit_log_scale.view(torch.int32), before.view(torch.int32))
    assert not torch.equal(model.user_tower_arch.weight.detach(), w0)  # (the step itself was taken)
    assert "logit_log_scale" in model.state_dict()


def traced_step(model, batch, **kw):
    from two_tower_models_amd import _native as N
    N.trace = []
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            loss = model.train_forward(*batch, **kw)
        loss.backward()
        calls = list(N.trace)
    finally:
        N.trace = None
    return calls, loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize("config,variant", [("base-256x128", "plain"), ("base-256x128", "hits"), ("hist-tiny", "logq"), ("base-tiny", "neg")])
def test_a_cosine_step_adds_one_launch_per_direction_and_a_plain_model_none(golden, config, variant):
    kind, name, repeat, fold = CONFIGS[config]
    gd = golden(name)
    B = the_batch(gd, repeat, "cpu", fold)[0].shape[0]
    extra = {k: v.to(DEV) for k, v in extras_of(gd, B, variant, seed=900 + B).items()}
    kw = dict(extra, remove_accidental_hits=variant == "hits")
    plain = [traced_step(make_model(kind, gd), the_batch(gd, repeat, DEV, fold), **kw) for _ in range(2)]
    assert not any(c.startswith("tt_l2norm") for c in plain[0][0])
    # a model without the switch: the same calls and the same bits as a second one
    assert plain[0][0] == plain[1][0] and torch.equal(plain[0][1].view(torch.int32), plain[1][1].view(torch.int32))
    for k in plain[0][2]:
        assert torch.equal(plain[0][2][k].view(torch.int32), plain[1][2][k].view(torch.int32)), k
    for learnable in (False, True):
        calls, _, _ = traced_step(make_model(kind, gd).use_cosine_logits(0.05, learnable=learnable),
                                  the_batch(gd, repeat, DEV, fold), **kw)
        assert calls.count("tt_l2norm_fwd") == 1 and calls.count("tt_l2norm_bwd") == 1
        assert [c for c in calls if not c.startswith("tt_l2norm")] == plain[0][0], (calls, plain[0][0])


def test_graphed_train_step_with_a_learned_scale_replays_the_eager_bits(golden):
    import two_tower_models_amd as A
    gd = golden("g2_base_aligned")
    full = batch_of(gd)
    W, n = 2, 3
    finals = []
    for graphed in (False, True):
        model = make_model("base", gd).use_cosine_logits(0.05, learnable=True)
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
                    loss = one_step(model, opt, full)
                    losses.append(loss.item())
            torch.cuda.current_stream().wait_stream(side)
            del loss
        opt.flush()
        torch.cuda.synchronize()
        assert opt.step_count == W + n
        finals.append(({k: v.detach().clone() for k, v in model.state_dict().items()}, losses))
    assert finals[1][1] == finals[0][1][W:]
    a, b = finals[0][0]["logit_log_scale"], finals[1][0]["logit_log_scale"]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and float(a) != -math.log(0.05)
    for k in finals[0][0]:
        assert torch.equal(finals[0][0][k], finals[1][0][k]), k


# ------------------------------------------------------------------ serving
def serving_model(gd, C=512, K=10):
    import two_tower_models_amd as A
    n_users, du, iu, n_items, di, ii, Tn, B, H = (int(v) for v in gd["cfg"])
    model = make_model("base", gd)
    model.mips_module = A.BaselineMIPSModule(corpus_size=C, embedding_dim=di).to(DEV)
    model.num_items = K
    g = torch.Generator().manual_seed(77)
    item_id = torch.randperm(n_items, generator=g)[:C].to(DEV) if n_items >= C else (torch.arange(C) % n_items).to(DEV)
    # item rows of very different lengths: the dot product prefers the long ones, the cosine does not
    item_features = (torch.randn(C, ii, generator=g) * torch.logspace(-1, 1, C)[torch.randperm(C, generator=g)][:, None]).to(DEV)
    return model, item_id, item_features


def test_serving_scores_are_cosines(golden):
    from two_tower_models_amd import ops
    gd = golden("g2_base_aligned")
    model, item_id, item_features = serving_model(gd)
    model.use_cosine_logits(0.05)
    batch = batch_of(gd)
    user_id, user_features, user_history = (t[:64] for t in batch[:3])
    K = model.num_items
    with torch.no_grad():
        v = model.compute_item_embeddings(item_id, item_features)
        u = model.compute_user_embedding(user_id, user_features, user_history)
    model.index_corpus(item_id, item_features)
    assert model.mips_module.corpus.dtype == torch.float32
    assert torch.equal(model.mips_module.corpus, ops.l2_normalize(v))
    top = model(user_id, user_features, user_history)
    want, _ = model.mips_module.search(ops.l2_normalize(u), K)
    assert torch.equal(top, want)
    # float64 cosines of the model's own fp32 embeddings: top-1 wherever float64 separates the first two by more than 1e-4
    cos = F.normalize(u.double().cpu(), dim=1) @ F.normalize(v.double().cpu(), dim=1).t()
    best2 = cos.topk(2, dim=1)
    clear = (best2.values[:, 0] - best2.values[:, 1]) > 1e-4
    assert int(clear.sum()) >= 0.9 * 64
    assert torch.equal(top[:, 0].cpu()[clear], best2.indices[:, 0][clear])
    dot_best = (u.double().cpu() @ v.double().cpu().t()).argmax(dim=1)
    assert bool((dot_best[clear] != best2.indices[:, 0][clear]).any()), "the fixture does not tell cosine from dot product"
    # exclusion is unchanged: no history item comes back
    model.mips_module.row_item_id = None
    hist = torch.randint(0, 512, (64, 6), generator=torch.Generator().manual_seed(5)).to(DEV)
    hist[:, 0] = top[:, 0]  # the best item is one the user has seen
    got = model(user_id, user_features, hist, exclude_history=True)
    assert not bool((got[:, :, None] == hist[:, None, :]).any())
    # bf16 corpus: normalised in fp32, then converted
    model.index_corpus(item_id, item_features, bf16=True)
    assert model.mips_module.corpus.dtype == torch.bfloat16
    ref = type(model.mips_module)(corpus_size=512, embedding_dim=v.shape[1]).to(DEV)
    ref.set_corpus(ops.l2_normalize(v), bf16=True)
    assert torch.equal(model.mips_module.corpus.view(torch.int16), ref.corpus.view(torch.int16))


def test_refusals(golden, monkeypatch):
    import two_tower_models_amd as A
    gd = golden("g1_base_tiny")
    model = make_model("base", gd).use_cosine_logits()
    from two_tower_models_amd import _native as N
    monkeypatch.setattr(type(model), "_sharded", lambda self: True)
    N.trace = []
    try:
        with pytest.raises(NotImplementedError, match="cosine"):
            model.train_forward(*batch_of(gd))
        with pytest.raises(NotImplementedError, match="cosine"):
            model.index_corpus(batch_of(gd)[3], batch_of(gd)[4])
        with pytest.raises(NotImplementedError, match="cosine"):
            make_model("base", gd).use_cosine_logits()
        assert N.trace == []  # refused before any kernel
    finally:
        N.trace = None
    monkeypatch.undo()
    mips = A.BaselineMIPSModule(16, 8)
    lr = A.TwoTowerPlusLightRanker(4, 8, 2, 10, 8, 4, 6, 10, 8, 4, [1.0], mips).to(DEV)
    with pytest.raises(NotImplementedError, match="cosine"):
        lr.use_cosine_logits(0.05, learnable=True)
