"""train_forward(..., remove_accidental_hits=True) at the model level, on MI355X (`pytest -m gpu`): the base and the history
model at B = 256, D = 128 and at the tiny golden dims, with and without log-Q terms and extra negatives, against a float64
torch restatement -- the oracle's towers in float64, then masked_fill(-inf) + F.cross_entropy + the reference's loss head
(ref:src/two_tower_base_retrieval.py:287-312, :322-345).  Loss and every parameter gradient, item-table rows included.
Bounds: the project's model-level figures (tests/test_gpu_logq.py: loss 1e-4 relative, gradients 1e-5 max|g| + 2e-4 |g|),
here against float64.  With the flag off the step is the call without the keyword, bit for bit, and launches none of the
masked entry points."""
import warnings

import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref as R
from test_gpu_logq import DEV, Tn_, batch_of, candidates, make_model, state_of

pytestmark = pytest.mark.gpu

# kind, golden fixture, how often the batch is repeated (the history fixture holds 64 rows: 4 x 64 = 256 rows), and the
# number of distinct item ids the batch is folded onto (id % fold: a head-heavy batch, every item many times -- with the
# fixtures' own ids an untrained model's loss moves by a few 1e-4 only, next to a bound of 1e-4)
CONFIGS = {"base-256x128": ("base", "g2_base_aligned", 1, 16), "hist-256x128": ("hist", "g4_hist_d128", 4, 16),
           "base-tiny": ("base", "g1_base_tiny", 1, 5), "hist-tiny": ("hist", "g4_hist_tiny", 1, 5)}


def the_batch(gd, repeat, dev, fold=None):
    batch = batch_of(gd, dev=dev)
    if fold:
        batch[3] = batch[3] % fold
    if repeat > 1:
        batch = [torch.cat([t] * repeat) for t in batch]
        # the copies of a sample differ in their features (and so in their embeddings), not in their item id
        for k in (1, 4):
            batch[k] = batch[k] * torch.linspace(0.8, 1.2, batch[k].shape[0], device=batch[k].device)[:, None]
    return batch


def the_extras(gd, B, variant, seed):
    """variant: none | logq | neg (37 extra negatives, a fifth of them batch items) | both | wide (3 B extra negatives with
    log q: N = 4 B, where InBatchSoftmaxCE keeps its logits by default and the fused loss head is not taken)."""
    if variant == "none":
        return {}
    Bn = 3 * B if variant == "wide" else 37 if variant in ("neg", "both") else 0
    kw = candidates(gd, Bn, seed, log_q=variant in ("logq", "both", "wide"), collide=Bn > 0)
    if "item_log_q" in kw and kw["item_log_q"].shape[0] != B:
        kw["item_log_q"] = torch.cat([kw["item_log_q"]] * (B // kw["item_log_q"].shape[0]))
    return kw


def restated_loss(params, batch, uvw, extra, kind, gd, masked=True):
    """float64: the oracle's towers, then the in-batch softmax with accidental hits removed and the reference's head."""
    user_id, user_features, user_history, item_id, item_features, position, labels = batch
    fkw = dict(with_history=True, heads=4, pos_table=Tn_(gd["pe_table"]).double()) if kind != "base" else dict(with_history=False)
    u = R.user_embedding(params, user_id, user_features.double(), user_history, **fkw)
    ids, feats = item_id, item_features.double()
    if "negative_item_id" in extra:
        ids = torch.cat([item_id, extra["negative_item_id"]])
        feats = torch.cat([feats, extra["negative_item_features"].double()])
    it = R.item_embeddings(params, ids, feats)
    scores = u @ it.t()
    if "item_log_q" in extra:
        log_q = torch.cat([extra["item_log_q"], extra["negative_log_q"]]) if "negative_log_q" in extra else extra["item_log_q"]
        scores = scores - log_q.double()[None, :]
    B = u.shape[0]
    target = torch.arange(B)
    if masked:
        hit = (ids[None, :] == ids[:B, None]) & (torch.arange(ids.shape[0])[None, :] != target[:, None])
        scores = scores.masked_fill(hit, float("-inf"))
    ce = F.cross_entropy(scores, target, reduction="none")
    nuv = torch.clamp(torch.sum(labels.double() * uvw.double(), dim=-1), min=0.000001)
    return torch.mean(ce * (nuv / torch.max(nuv)))


@pytest.mark.parametrize("variant", ["none", "logq", "neg", "both"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_train_forward_without_accidental_hits_matches_float64(golden, config, variant):
    check_against_float64(golden, config, variant, margin=50)


@pytest.mark.parametrize("config", ["base-256x128", "base-tiny"])
def test_train_forward_with_wide_negatives_matches_float64(golden, config):
    """3 B extra negatives (N = 4 B): no fused loss head, and at D = 128 the item side runs from the kept, masked logits.
    (Among 4 B candidates the hits weigh less: the loss moves by 20 x its bound at B = 256.)"""
    check_against_float64(golden, config, "wide", margin=10)


def check_against_float64(golden, config, variant, margin):
    kind, name, repeat, fold = CONFIGS[config]
    gd = golden(name)
    cpu = the_batch(gd, repeat, "cpu", fold)
    B = cpu[0].shape[0]
    extra = the_extras(gd, B, variant, seed=500 + B)
    ids = torch.cat([cpu[3], extra["negative_item_id"]]) if "negative_item_id" in extra else cpu[3]
    hits = (ids[None, :] == ids[:B, None]).sum() - B
    assert int(hits) > 0, "the batch holds no accidental hit"
    leaves = {k: v.double().requires_grad_(True) for k, v in state_of(gd).items()}
    uvw = Tn_(gd["uvw"])
    want = restated_loss(leaves, cpu, uvw, extra, kind, gd)
    plain = restated_loss(leaves, cpu, uvw, extra, kind, gd, masked=False)
    grads = dict(zip(leaves, torch.autograd.grad(want, list(leaves.values()), allow_unused=True)))
    model = make_model(kind, gd)
    from two_tower_models_amd import _native as N
    N.trace = []
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            loss = model.train_forward(*the_batch(gd, repeat, DEV, fold), **{k: v.to(DEV) for k, v in extra.items()},
                                       remove_accidental_hits=True)
        loss.backward()
        calls = list(N.trace)
    finally:
        N.trace = None
    print(f"HITS_MODEL {config} {variant}: {int(hits)} hits, loss {loss.item():.6f} float64 {float(want):.6f} (unmasked {float(plain):.6f})")
    if variant == "wide" and config.endswith("256x128"):  # D = 128, N = 4 B: the item side comes from the kept (masked) logits
        assert "tt_inbatch_ce_masked_fwd" in calls and "tt_inbatch_ce_bwd_kept" in calls, calls
    else:
        assert "tt_inbatch_ce_masked_fwd" in calls and "tt_inbatch_ce_masked_bwd" in calls, calls
    assert abs(float(want) - float(plain)) > margin * 1e-4 * max(1.0, abs(float(want)))  # the mask matters: margin x the loss bound
    assert loss.dim() == 0 and abs(loss.item() - float(want)) < 1e-4 * max(1.0, abs(float(want)))
    worst = ("", 0.0)
    for pname, p in model.named_parameters():
        w = grads[pname]
        w = torch.zeros_like(p, device="cpu", dtype=torch.float64) if w is None else w
        assert p.grad is not None, pname
        got = p.grad.cpu().double()
        tol = max(1e-5 * float(w.abs().max()), 1e-7)  # floor: the analytically-zero gradients hold ~1e-8 of rounding noise
        rel = float(((got - w).abs() - 2e-4 * w.abs()).max()) / tol
        worst = max(worst, (pname, rel), key=lambda t: t[1])
        assert torch.allclose(got, w, atol=tol, rtol=2e-4), (pname, float((got - w).abs().max()), tol)
    print("  worst", worst)


@pytest.mark.parametrize("config", ["base-256x128", "hist-tiny"])
def test_flag_off_is_the_call_without_the_keyword_bit_for_bit(golden, config):
    kind, name, repeat, fold = CONFIGS[config]
    gd = golden(name)
    from two_tower_models_amd import _native as N
    res = []
    for kw in ({}, {"remove_accidental_hits": False}):
        model = make_model(kind, gd)
        N.trace = []
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                loss = model.train_forward(*the_batch(gd, repeat, DEV, fold), **kw)
            loss.backward()
            calls = list(N.trace)
        finally:
            N.trace = None
        assert not any("masked" in c for c in calls), calls
        res.append((calls, loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}))
    assert res[0][0] == res[1][0]
    assert torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32))
    for k in res[0][2]:
        assert torch.equal(res[0][2][k].view(torch.int32), res[1][2][k].view(torch.int32)), k


def test_debias_model_takes_the_flag(golden):
    """A subclass that reaches the in-batch softmax through its own head: the flag changes the loss where the batch holds
    hits, and the masked entry points run."""
    from two_tower_models_amd import _native as N
    gd = golden("g6_debias_d128")
    model = make_model("debias", gd)
    batch = batch_of(gd)
    batch[3] = batch[3] % 7  # few distinct items: many hits
    out = []
    for flag in (False, True):
        N.trace = []
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                out.append(float(model.train_forward(*batch, remove_accidental_hits=flag)))
            calls = list(N.trace)
        finally:
            N.trace = None
        assert ("tt_inbatch_ce_masked_fwd" in calls) == flag, calls
    assert out[1] < out[0]  # every row lost negatives: its cross entropy can only fall


def test_refusals(golden):
    gd = golden("g1_base_tiny")
    model = make_model("base", gd)
    batch = batch_of(gd)
    model.item_id_embedding_arch.num_embeddings = 2 ** 31 + 1
    with pytest.raises(ValueError, match="32-bit"):
        model.train_forward(*batch, remove_accidental_hits=True)
    model.item_id_embedding_arch.num_embeddings = int(gd["cfg"][3])
    from two_tower_models_amd import ops
    U, I = torch.zeros(4, 8, device=DEV, requires_grad=True), torch.zeros(6, 8, device=DEV)
    with pytest.raises(TypeError):
        ops.InBatchSoftmaxCE.apply(U, I, 0, None, None, torch.zeros(6, device=DEV))
    with pytest.raises(RuntimeError):
        ops.InBatchSoftmaxCE.apply(U, I, 0, None, None, torch.zeros(6, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.InBatchSoftmaxWeightedLoss.apply(U, I, None, torch.ones(1, device=DEV), None, torch.zeros(5, dtype=torch.int32, device=DEV))


def test_row_sharded_model_refuses_the_flag(golden, monkeypatch):
    gd = golden("g1_base_tiny")
    model = make_model("base", gd)
    monkeypatch.setattr(type(model), "_sharded", lambda self: True)
    with pytest.raises(NotImplementedError, match="remove_accidental_hits"):
        model.train_forward(*batch_of(gd), remove_accidental_hits=True)
    u, v = torch.zeros(4, 8, device=DEV), torch.zeros(4, 8, device=DEV)
    with pytest.raises(NotImplementedError, match="remove_accidental_hits"):
        model.compute_training_loss(u, v, torch.zeros(4, device=DEV), torch.zeros(4, 1, device=DEV),
                                    item_id=torch.zeros(4, dtype=torch.int64, device=DEV))
