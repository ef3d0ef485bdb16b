"""Model-level parity on MI355X (`pytest -m gpu`): the nn.Module mirror of the reference
API, driven through libtt_hotpath.so, against the golden vectors the reference produced
(tests/golden/*.npz) -- embeddings, loss, every parameter gradient, Adam trajectories,
the reference's own known-answer test, and seeded-init identity."""
import numpy as np
import pytest
import torch

import fixture_gen as fg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def state_of(g, prefix="p."):
    return {k[len(prefix):]: T(v) for k, v in g.items() if k.startswith(prefix)}


def batch_of(g, prefix="in.", labels_key="labels", dev=DEV):
    names = ("user_id", "user_features", "user_history", "item_id", "item_features", "position")
    return [T(g[prefix + n]).to(dev) for n in names] + [T(g[prefix + labels_key]).to(dev)]


def make_model(kind, g, corpus=None, topk=10):
    import two_tower_models_amd as A
    n_users, du, iu, n_items, di, ii, Tn, B, H = (int(v) for v in g["cfg"])
    mips = A.BaselineMIPSModule(corpus_size=64 if corpus is None else corpus.shape[0], embedding_dim=di)
    if corpus is not None:
        mips.corpus = corpus
    common = dict(num_items=topk, user_id_hash_size=n_users, user_id_embedding_dim=du, user_features_size=iu,
                  item_id_hash_size=n_items, item_id_embedding_dim=di, item_features_size=ii,
                  user_value_weights=[float(v) for v in g["uvw"]], mips_module=mips)
    if kind == "base":
        m = A.TwoTowerBaseRetrieval(**common)
    elif kind == "hist":
        m = A.TwoTowerWithUserHistoryEncoder(user_history_seqlen=H, **common)
    elif kind == "position":
        m = A.TwoTowerWithPositionDebiasedWeights(user_history_seqlen=H, **common)
    elif kind == "user":
        m = A.TwoTowerWithUserDebiasedWeights(user_history_seqlen=H, **common)
    else:
        m = A.TwoTowerWithDebiasing(user_history_seqlen=H, **common)
    missing, unexpected = m.load_state_dict(state_of(g), strict=True) if True else (None, None)
    return m.to(DEV)


def check_grads(model, g, rtol=2e-4, atol_scale=1e-5):
    for name, p in model.named_parameters():
        want = T(g["g." + name])
        assert p.grad is not None, name
        got = p.grad.cpu()
        # floor 1e-7: item_tower_arch.bias / item_features_arch.2.bias have an analytically zero
        # gradient (softmax shift invariance); both sides hold ~1e-8 of rounding noise there
        tol = max(atol_scale * float(want.abs().max()), 1e-7)
        assert torch.allclose(got, want, atol=tol, rtol=rtol), (name, float((got - want).abs().max()), tol)


# ------------------------------------------------------------------ base model
@pytest.mark.parametrize("name", ["g1_base_tiny", "g2_base_aligned", "g2_base_d256"])
def test_base_model_matches_reference(golden, name):
    g = golden(name)
    model = make_model("base", g)
    b = batch_of(g)
    u = model.compute_user_embedding(b[0], b[1], b[2])
    it = model.compute_item_embeddings(b[3], b[4])
    assert torch.allclose(u.cpu(), T(g["user_emb"]), atol=1e-5)
    assert torch.allclose(it.cpu(), T(g["item_emb"]), atol=1e-5)
    loss = model.train_forward(*b)
    assert loss.dim() == 0 and abs(loss.item() - float(g["loss"])) < 1e-4
    loss.backward()  # no optimiser attached: dense embedding gradients, like the reference
    check_grads(model, g)
    if "loss_labels_1d" in g:  # train.py feeds 1-D labels
        b1 = batch_of(g, labels_key="labels_1d")
        assert abs(model.train_forward(*b1).item() - float(g["loss_labels_1d"])) < 1e-4


def test_base_model_seeded_init_is_reference_init(golden):
    """Same seed => same initial weights as the reference (same RNG draws, same order)."""
    import two_tower_models_amd as A
    g = golden("g1_base_tiny")
    n_users, du, iu, n_items, di, ii, Tn, B, H = (int(v) for v in g["cfg"])
    torch.manual_seed(0)
    mips = A.BaselineMIPSModule(corpus_size=64, embedding_dim=di)
    m = A.TwoTowerBaseRetrieval(10, n_users, du, iu, n_items, di, ii, [0.1, 0.2, 0.3], mips)
    for k, v in m.state_dict().items():
        assert torch.equal(v, T(g["p." + k])), k


def assert_reference_trajectory(model, g):
    """The model's state after the fixture's three Adam steps vs the reference's `after.*` arrays."""
    after = state_of(g, prefix="after.")
    for k, v in model.state_dict().items():
        noise_only = float(np.abs(g["g." + k]).max()) < 1e-6  # see tests/test_oracle_golden.py
        err = (v.cpu() - after[k]).abs() - 1e-5 * after[k].abs()
        # Adam's first updates are lr * g / (|g| + eps): an element whose gradient happens to be ~1e-4 of the typical size
        # turns a 1e-7 relative summation-order difference into a ~1e-5 step difference -- between ANY two fp32
        # implementations (torch CPU vs torch CPU with another reduction order included).  So: every element within the
        # 3-steps * 2 * lr bound, and all but <= 0.1 % of them within 5e-6.
        assert float(err.max()) <= 2 * 3 * 1e-3 * 1.05, (k, float(err.max()))
        if not noise_only:
            out = err > 5e-6
            n_out = int(out.sum())
            assert n_out <= max(1, int(1e-3 * err.numel())) and float(err.max()) <= 2e-4, (k, n_out, float(err.max()))
            if n_out:
                # ... and the elements outside ARE the small-gradient ones, not an arbitrary 0.1 % (a bug confined
                # to, say, the last row of a block would sit on typical gradients): their first-step |g| in the
                # reference is below 2 % of the tensor's largest, most far below
                g0 = torch.from_numpy(np.abs(g["g." + k])).reshape(err.shape)
                assert float(g0[out].max()) <= 2e-2 * float(g0.max()), (k, n_out, float(g0[out].max()), float(g0.max()))


@pytest.mark.parametrize("interleave", [False, True])
@pytest.mark.parametrize("schedule", [dict(), dict(overlap_sweep=False), dict(overlap_sweep="forward"), dict(lazy=True)])
def test_adam_trajectory_dense_exact(golden, schedule, interleave):
    """The ref:train/train.py:112-132 loop body x3 with DenseExactAdam vs torch.optim.Adam run in the
    REFERENCE (fixture g2): every schedule -- default overlapped, serial, forward-announced, deferred --
    against the reference trajectory, not against each other.  `interleave`: a no_grad eval forward and
    an index_corpus() of more than 4 chunks between the training steps must leave no lookups behind
    (needs_input_grad is True under no_grad)."""
    import two_tower_models_amd as A
    g = golden("g2_base_aligned")
    model = make_model("base", g)
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3, **schedule)
    losses = []
    n_items, ii = int(g["cfg"][3]), int(g["cfg"][5])
    cat_ids = torch.arange(n_items, device=DEV)
    cat_feats = torch.zeros(n_items, ii, device=DEV)
    for s in range(3):
        b = batch_of(g, prefix=f"step{s}.in.")
        if interleave:
            with torch.no_grad():
                model.train_forward(*b)
                model(b[0], b[1], b[2])
            model.index_corpus(cat_ids, cat_feats, chunk=max(n_items // 6, 1))
        loss = model.train_forward(*b)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert np.allclose(losses, g["adam_losses"], atol=1e-4)
    assert opt.step_count == 3
    opt.flush()
    assert_reference_trajectory(model, g)


@pytest.mark.parametrize("overlap", [False, "forward"])
def test_graphed_train_step_vs_reference_trajectory(golden, overlap):
    """GraphedTrainStep anchored on the REFERENCE (not on the eager HIP path): the warm-up step is the fixture's step 0,
    the two replays its steps 1 and 2; losses and the final state against torch.optim.Adam run in the reference."""
    import two_tower_models_amd as A
    g = golden("g2_base_aligned")
    model = make_model("base", g)
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep=overlap)
    batches = [batch_of(g, prefix=f"step{s}.in.") for s in range(3)]
    step = A.GraphedTrainStep(model, opt, batches[0], warmup=1, capture_overlap=overlap == "forward")
    losses = [step(*b).item() for b in batches[1:]]
    opt.flush()
    torch.cuda.synchronize()
    assert opt.step_count == 3
    assert np.allclose(losses, g["adam_losses"][1:], atol=1e-4)
    assert_reference_trajectory(model, g)


@pytest.mark.parametrize("lazy", [False, True])
def test_checkpoint_resume_vs_reference_trajectory(golden, lazy):
    """Checkpoint after the fixture's step 0 (model + optimiser state_dict through torch.save / torch.load), fresh objects,
    steps 1 and 2: the REFERENCE's uninterrupted three-step trajectory, losses included."""
    import io
    import two_tower_models_amd as A
    g = golden("g2_base_aligned")
    batches = [batch_of(g, prefix=f"step{s}.in.") for s in range(3)]
    losses = []

    def run(model, opt, bs):
        for b in bs:
            loss = model.train_forward(*b)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.item())

    m1 = make_model("base", g)
    o1 = A.DenseExactAdam(m1.parameters(), lr=1e-3, lazy=lazy)
    run(m1, o1, batches[:1])
    buf = io.BytesIO()
    torch.save({"opt": o1.state_dict(), "model": m1.state_dict()}, buf)  # optimiser first: it flushes
    ck = torch.load(io.BytesIO(buf.getvalue()))
    model = make_model("base", g)
    model.load_state_dict(ck["model"])
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3, lazy=lazy)
    opt.load_state_dict(ck["opt"])
    run(model, opt, batches[1:])
    opt.flush()
    assert opt.step_count == 3
    assert np.allclose(losses, g["adam_losses"], atol=1e-4)
    assert_reference_trajectory(model, g)


def test_label_and_id_dtypes_follow_the_reference(golden):
    """The reference type-promotes `labels * user_value_weights` and nn.Embedding takes int32 ids: integer /
    bool labels and int32 ids give the float32 / int64 result; float64 labels take the torch expressions."""
    g = golden("g2_base_aligned")
    model = make_model("base", g)
    b = batch_of(g)
    want = model.train_forward(*b).item()
    assert abs(want - float(g["loss"])) < 1e-4
    lab = b[6]
    if bool(((lab == 0) | (lab == 1)).all()):
        for dt in (torch.int64, torch.bool, torch.int32):
            assert abs(model.train_forward(*b[:6], lab.to(dt)).item() - want) < 1e-6
    b32 = [b[0].to(torch.int32), b[1], b[2].to(torch.int32), b[3].to(torch.int32), b[4], b[5], b[6]]
    assert abs(model.train_forward(*b32).item() - want) < 1e-6
    l64 = model.train_forward(*b[:6], lab.double())
    assert l64.dtype == torch.float64 and abs(l64.item() - want) < 1e-5
    from two_tower_models_amd import ops
    with pytest.raises(TypeError):
        ops.WeightedMeanLoss.apply(torch.zeros(4, device=DEV), torch.zeros(4, 1, device=DEV, dtype=torch.float64),
                                   torch.ones(1, device=DEV))


def test_torch_optim_adam_also_works_unchanged(golden):
    """A caller that keeps torch.optim.Adam (the reference train.py, unmodified) gets dense
    embedding gradients and the same trajectory."""
    g = golden("g2_base_aligned")
    model = make_model("base", g)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for s in range(3):
        loss = model.train_forward(*batch_of(g, prefix=f"step{s}.in."))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert np.allclose(losses, g["adam_losses"], atol=1e-4)


# ------------------------------------------------------------------ history encoder
def test_reference_known_answer_test_seed42():
    """ref:tests/test_user_history_enc.py:48-124 verbatim in spirit: seed 42, D=2, H=3."""
    import two_tower_models_amd as A
    x = torch.tensor([[[1, 2], [3, 4], [-1, 0]]], dtype=torch.float32, device=DEV)
    for pe, want in ((False, [[[0.8240, 0.7119], [1.0, 2.0]]]), (True, [[[1.4978, 1.2425], [1.0, 2.0]]])):
        torch.manual_seed(42)
        enc = A.UserHistoryEncoder(2, 3, 1, 1, pe).to(DEV)
        out = enc(x)
        assert out.shape == (1, 2, 2)
        assert torch.allclose(out.cpu(), torch.tensor(want), atol=1e-3)


def test_encoder_shape_case_from_reference_tests():
    """ref:tests/test_user_history_enc.py:21-46: D=64, H=128, 4 heads, 12 layers, B=32."""
    import two_tower_models_amd as A
    torch.manual_seed(42)
    enc = A.UserHistoryEncoder(64, 128, 4, 12, True).to(DEV)
    out = enc(torch.randn(32, 128, 64, device=DEV))
    assert out.shape == (32, 2, 64) and torch.isfinite(out).all()


@pytest.mark.parametrize("name", ["g3_encoder_d128", "g3_encoder_d128_nope", "g3_encoder_odd"])
def test_encoder_matches_reference(golden, name):
    import two_tower_models_amd as A
    g = golden(name)
    D, H, heads, L, B, pe = (int(v) for v in g["cfg"])
    enc = A.UserHistoryEncoder(D, H, heads, L, bool(pe))
    enc.load_state_dict(state_of(g))
    enc = enc.to(DEV)
    if pe:
        assert torch.equal(enc.positional_embeddings.cpu(), T(g["pe_table"]))
    x = T(g["x"]).to(DEV).requires_grad_(True)
    y = enc(x)
    assert torch.allclose(y.cpu(), T(g["y"]), atol=1e-5, rtol=1e-5)
    (y * T(g["cot"]).to(DEV)).sum().backward()
    assert torch.allclose(x.grad.cpu(), T(g["gx"]), atol=1e-5 * float(np.abs(g["gx"]).max()) + 1e-8, rtol=2e-4)
    check_grads(enc, g)


@pytest.mark.parametrize("name", ["g3_encoder_d128", "g3_encoder_odd"])
def test_encoder_plain_composition_matches_reference(golden, name, monkeypatch):
    """TT_ENC_GENERIC: every layer in full (in-projection, attention, out-projection; no folded out-projections, no
    collapsed last layer, no pool epilogue) -- the composition shapes outside the shortcut kernels' limits run -- against
    the same goldens as the default path."""
    from two_tower_models_amd import ops
    monkeypatch.setattr(ops, "_ENC_GENERIC", True)
    test_encoder_matches_reference(golden, name)


def _encoder_grads(g, main_only=False, hook=False, shared=False):
    """Weight gradients of the g3 encoder through loss.backward() (the side-stream deferral only arms inside a backward
    pass); `hook`: a tensor hook on one in_proj_bias; `shared`: the SAME encoder applied to two inputs in one graph."""
    import two_tower_models_amd as A
    from two_tower_models_amd import ops
    D, H, heads, L, B, pe = (int(v) for v in g["cfg"])
    enc = A.UserHistoryEncoder(D, H, heads, L, bool(pe))
    enc.load_state_dict(state_of(g))
    enc = enc.to(DEV)
    seen = []
    if hook:
        enc.multihead_attn_layers[1].in_proj_bias.register_hook(lambda gr: seen.append(gr.clone()))
    old = ops._SIDE_GRADS
    ops._SIDE_GRADS = not main_only
    try:
        x = T(g["x"]).to(DEV)
        y = enc(x)
        loss = (y * T(g["cot"]).to(DEV)).sum()
        if shared:
            loss = loss + (enc(x.flip(0)) * T(g["cot"]).to(DEV)).sum()
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops._SIDE_GRADS = old
    return {n: p.grad.clone() for n, p in enc.named_parameters()}, seen


def test_side_stream_weight_gradients_equal_inline_ones(golden):
    """ops.run_on_side: weight gradients queued on the third stream are the in-line ones bit for bit --
    including in_proj_bias of a folded layer, whose buffer must be STOLEN by AccumulateGrad (never held: a held output
    is cloned on the main stream before the side stream wrote it); a hooked Parameter and a Parameter that feeds two
    nodes of one backward pass get completed gradients (run in line)."""
    g = golden("g3_encoder_d128")
    want, _ = _encoder_grads(g, main_only=True)
    for kw in (dict(), dict(hook=True)):
        for _ in range(3):  # a race would not show every time
            got, seen = _encoder_grads(g, **kw)
            for n in want:
                assert torch.equal(got[n], want[n]), (n, kw)
            if kw.get("hook"):
                assert len(seen) == 1 and torch.equal(seen[0], want["multihead_attn_layers.1.in_proj_bias"])
    want2, _ = _encoder_grads(g, main_only=True, shared=True)
    for _ in range(3):
        got2, _ = _encoder_grads(g, shared=True)
        for n in want2:
            assert torch.equal(got2[n], want2[n]), (n, "shared")


_ENCODER_ENTRY_POINTS = ("tt_hist_embed_pool", "tt_gemm_f32", "tt_gemm_tn_colsum_f32", "tt_attn_fwd", "tt_attn_bwd",
                         "tt_enc_last_fwd", "tt_enc_last_bwd_data", "tt_enc_last_bwd_weights", "tt_hist_dx_pool_bwd",
                         "tt_hist_pool_bwd")


class _TracingLibrary:
    """The loaded library with every attribute forwarded; the encoder's entry points append (name, stream, dims) to `log`
    before they call through: stream = "side" if the call's stream argument (the last one) is the third stream, else "main";
    dims = (layout, M, N, K) of tt_gemm_f32, (M, N, K) of tt_gemm_tn_colsum_f32, () otherwise."""

    def __init__(self, lib, log, side_stream):
        self._lib, self._log, self._side_stream = lib, log, side_stream

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in _ENCODER_ENTRY_POINTS:
            return fn

        def traced(*args):
            dims = ()
            if name == "tt_gemm_f32":
                dims = (("NT", "NN", "TN")[args[0]], *args[1:4])
            elif name == "tt_gemm_tn_colsum_f32":
                dims = tuple(args[:3])
            self._log.append((name, "side" if args[-1] == self._side_stream else "main", dims))
            return fn(*args)

        return traced


class _HeldSweepStub:
    """What HistoryEncoder.forward asks of the table's optimiser: is the held sweep marked, and release it."""

    def __init__(self, log, marked):
        self.log, self.marked = log, marked

    def held_sweep_is_marked(self):
        return self.marked

    def release_sweep(self, after=None):
        self.log.append(("release", self.marked, after is not None))


def _encoder_trace(monkeypatch, D, H, heads, L, B, marked=None, generic=False, inline=False):
    """One forward + loss.backward() of a fresh encoder (every .grad None) -> the host-order list of its library calls.
    marked None: embedded history [B, H, D]; True / False: a [1000, D] table + ids whose optimiser holds a (marked) sweep."""
    import warnings
    import two_tower_models_amd as A
    from two_tower_models_amd import _native as N, ops
    assert (N.TT_GEMM_NT, N.TT_GEMM_NN, N.TT_GEMM_TN) == (0, 1, 2)
    log = []
    traced = _TracingLibrary(N.load(), log, N.aux_stream(torch.device(DEV)).cuda_stream)
    monkeypatch.setattr(N, "load", lambda: traced)
    monkeypatch.setattr(ops, "_ENC_GENERIC", generic)
    monkeypatch.setattr(ops, "_SIDE_GRADS", not inline)
    torch.manual_seed(0)
    enc = A.UserHistoryEncoder(D, H, heads, L, True).to(DEV)
    with warnings.catch_warnings():  # note_generic's once-per-process RuntimeWarning (odd widths): whoever meets it first
        warnings.simplefilter("ignore", RuntimeWarning)
        if marked is None:
            y = enc(torch.randn(B, H, D, device=DEV).requires_grad_(True))
        else:
            table = torch.randn(1000, D, device=DEV).requires_grad_(True)
            stub = _HeldSweepStub(log, marked)
            table._tt_optimizer = lambda: stub
            y = enc.encode_ids(table, torch.randint(0, 1000, (B, H), device=DEV))
        (y * torch.randn_like(y)).sum().backward()
    torch.cuda.synchronize()
    return log


def _k(name, stream="main"):
    return (name, stream, ())


def _g(stream, *dims):
    return ("tt_gemm_f32", stream, dims)


def _w(stream, *dims):
    return ("tt_gemm_tn_colsum_f32", stream, dims)


def _r(marked, after):
    return ("release", marked, after)


# case -> ((D, H, heads, L, B), options of _encoder_trace, the trace).  The traces are what the commit BEFORE the encoder's
# layer plan produced (dad9cd8), pasted: they pin the enqueue order, the stream of every launch and the sweep's release point
# that the measurements quoted in ops.py settled.
_ENCODER_TRACES = {
    "default": ((128, 50, 4, 3, 8), dict(), [
        _k("tt_hist_embed_pool"), _g("side", "NN", 384, 128, 128), _g("side", "NT", 1, 384, 128),
        _g("side", "NN", 384, 128, 128), _g("side", "NT", 1, 384, 128), _g("main", "NT", 400, 384, 128), _k("tt_attn_fwd"),
        _g("main", "NT", 400, 384, 128), _k("tt_attn_fwd"), _k("tt_enc_last_fwd"), _k("tt_enc_last_bwd_data"),
        _k("tt_enc_last_bwd_weights", "side"), _k("tt_attn_bwd"), _w("side", 384, 128, 400),
        _g("main", "NN", 400, 128, 384), _k("tt_attn_bwd"), _w("side", 384, 128, 400), _k("tt_hist_dx_pool_bwd"),
        _g("main", "NN", 400, 128, 384), _g("main", "NT", 384, 128, 128), _g("main", "NT", 384, 128, 1),
        _g("main", "TN", 128, 128, 384), _g("main", "NN", 1, 128, 384), _g("main", "NT", 384, 128, 128),
        _g("main", "NT", 384, 128, 1), _g("main", "TN", 128, 128, 384), _g("main", "NN", 1, 128, 384),
        _k("tt_hist_pool_bwd"),
    ]),
    "one layer": ((128, 50, 4, 1, 4), dict(), [
        _k("tt_hist_embed_pool"), _k("tt_enc_last_fwd"), _k("tt_enc_last_bwd_data"), _k("tt_enc_last_bwd_weights", "side"),
        _k("tt_hist_pool_bwd"),
    ]),
    "odd widths": ((40, 7, 4, 2, 5), dict(), [
        _k("tt_hist_embed_pool"), _g("side", "NN", 120, 40, 40), _g("side", "NT", 1, 120, 40),
        _g("main", "NT", 35, 120, 40), _k("tt_attn_fwd"), _g("main", "NT", 35, 120, 40), _k("tt_attn_fwd"),
        _g("main", "NT", 5, 40, 40), _w("main", 40, 40, 5), _g("main", "NN", 5, 40, 40), _k("tt_attn_bwd"),
        _w("side", 120, 40, 35), _g("main", "NN", 35, 40, 120), _k("tt_attn_bwd"), _w("side", 120, 40, 35),
        _k("tt_hist_dx_pool_bwd"), _g("main", "NN", 35, 40, 120), _g("main", "NT", 120, 40, 40),
        _g("main", "NT", 120, 40, 1), _g("main", "TN", 40, 40, 120), _g("main", "NN", 1, 40, 120), _k("tt_hist_pool_bwd"),
    ]),
    "plain": ((128, 50, 4, 3, 8), dict(generic=True), [
        _k("tt_hist_embed_pool"), _g("main", "NT", 400, 384, 128), _k("tt_attn_fwd"), _g("main", "NT", 400, 128, 128),
        _g("main", "NT", 400, 384, 128), _k("tt_attn_fwd"), _g("main", "NT", 400, 128, 128),
        _g("main", "NT", 400, 384, 128), _k("tt_attn_fwd"), _g("main", "NT", 8, 128, 128), _w("main", 128, 128, 8),
        _g("main", "NN", 8, 128, 128), _k("tt_attn_bwd"), _w("side", 384, 128, 400), _g("main", "NN", 400, 128, 384),
        _w("side", 128, 128, 400), _g("main", "NN", 400, 128, 128), _k("tt_attn_bwd"), _w("side", 384, 128, 400),
        _g("main", "NN", 400, 128, 384), _w("side", 128, 128, 400), _g("main", "NN", 400, 128, 128), _k("tt_attn_bwd"),
        _w("side", 384, 128, 400), _g("main", "NN", 400, 128, 384), _k("tt_hist_pool_bwd"),
    ]),
    "pool epilogue": ((128, 32, 4, 2, 512), dict(), [
        _k("tt_hist_embed_pool"), _g("side", "NN", 384, 128, 128), _g("side", "NT", 1, 384, 128),
        _g("main", "NT", 16384, 384, 128), _k("tt_attn_fwd"), _k("tt_enc_last_fwd"), _k("tt_enc_last_bwd_data"),
        _k("tt_enc_last_bwd_weights", "side"), _k("tt_attn_bwd"), _w("side", 384, 128, 16384), _k("tt_hist_dx_pool_bwd"),
        _g("main", "NT", 384, 128, 128), _g("main", "NT", 384, 128, 1), _g("main", "TN", 128, 128, 384),
        _g("main", "NN", 1, 128, 384),
    ]),
    "marked sweep": ((128, 50, 4, 3, 8), dict(marked=True), [
        _k("tt_hist_embed_pool"), _g("side", "NN", 384, 128, 128), _g("side", "NT", 1, 384, 128),
        _g("side", "NN", 384, 128, 128), _g("side", "NT", 1, 384, 128), _g("main", "NT", 400, 384, 128), _r(True, True),
        _k("tt_attn_fwd"), _g("main", "NT", 400, 384, 128), _k("tt_attn_fwd"), _k("tt_enc_last_fwd"),
        _k("tt_enc_last_bwd_data"), _k("tt_enc_last_bwd_weights", "side"), _k("tt_attn_bwd"), _w("side", 384, 128, 400),
        _g("main", "NN", 400, 128, 384), _k("tt_attn_bwd"), _w("side", 384, 128, 400), _k("tt_hist_dx_pool_bwd"),
        _g("main", "NN", 400, 128, 384), _g("main", "NT", 384, 128, 128), _g("main", "NT", 384, 128, 1),
        _g("main", "TN", 128, 128, 384), _g("main", "NN", 1, 128, 384), _g("main", "NT", 384, 128, 128),
        _g("main", "NT", 384, 128, 1), _g("main", "TN", 128, 128, 384), _g("main", "NN", 1, 128, 384),
        _k("tt_hist_pool_bwd"),
    ]),
    "unmarked sweep": ((128, 50, 4, 3, 8), dict(marked=False), [
        _k("tt_hist_embed_pool"), _r(False, False), _g("side", "NN", 384, 128, 128), _g("side", "NT", 1, 384, 128),
        _g("side", "NN", 384, 128, 128), _g("side", "NT", 1, 384, 128), _g("main", "NT", 400, 384, 128), _k("tt_attn_fwd"),
        _g("main", "NT", 400, 384, 128), _k("tt_attn_fwd"), _k("tt_enc_last_fwd"), _k("tt_enc_last_bwd_data"),
        _k("tt_enc_last_bwd_weights", "side"), _k("tt_attn_bwd"), _w("side", 384, 128, 400),
        _g("main", "NN", 400, 128, 384), _k("tt_attn_bwd"), _w("side", 384, 128, 400), _k("tt_hist_dx_pool_bwd"),
        _g("main", "NN", 400, 128, 384), _g("main", "NT", 384, 128, 128), _g("main", "NT", 384, 128, 1),
        _g("main", "TN", 128, 128, 384), _g("main", "NN", 1, 128, 384), _g("main", "NT", 384, 128, 128),
        _g("main", "NT", 384, 128, 1), _g("main", "TN", 128, 128, 384), _g("main", "NN", 1, 128, 384),
        _k("tt_hist_pool_bwd"),
    ]),
    "marked, one layer": ((128, 50, 4, 1, 4), dict(marked=True), [
        _k("tt_hist_embed_pool"), _k("tt_enc_last_fwd"), _r(True, False), _k("tt_enc_last_bwd_data"),
        _k("tt_enc_last_bwd_weights", "side"), _k("tt_hist_pool_bwd"),
    ]),
    "in line": ((128, 50, 4, 3, 8), dict(inline=True), [
        _k("tt_hist_embed_pool"), _g("side", "NN", 384, 128, 128), _g("side", "NT", 1, 384, 128),
        _g("side", "NN", 384, 128, 128), _g("side", "NT", 1, 384, 128), _g("main", "NT", 400, 384, 128), _k("tt_attn_fwd"),
        _g("main", "NT", 400, 384, 128), _k("tt_attn_fwd"), _k("tt_enc_last_fwd"), _k("tt_enc_last_bwd_data"),
        _k("tt_enc_last_bwd_weights"), _k("tt_attn_bwd"), _w("main", 384, 128, 400), _g("main", "NN", 400, 128, 384),
        _k("tt_attn_bwd"), _w("main", 384, 128, 400), _k("tt_hist_dx_pool_bwd"), _g("main", "NN", 400, 128, 384),
        _g("main", "NT", 384, 128, 128), _g("main", "NT", 384, 128, 1), _g("main", "TN", 128, 128, 384),
        _g("main", "NN", 1, 128, 384), _g("main", "NT", 384, 128, 128), _g("main", "NT", 384, 128, 1),
        _g("main", "TN", 128, 128, 384), _g("main", "NN", 1, 128, 384), _k("tt_hist_pool_bwd"),
    ]),
}


@pytest.mark.parametrize("case", list(_ENCODER_TRACES))
def test_encoder_call_trace(case, monkeypatch):
    """The sequence of library calls of one encoder forward + backward, with the stream each is queued on, the GEMM
    shapes and the point where a held table sweep is released, is the recorded one entry for entry."""
    shape, options, want = _ENCODER_TRACES[case]
    got = _encoder_trace(monkeypatch, *shape, **options)
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (case, "first difference at entry", first, got[first:first + 3], want[first:first + 3])


@pytest.mark.parametrize("kind,name", [("base", "g2_base_aligned"), ("hist", "g4_hist_d128")])
@pytest.mark.parametrize("schedule", ["forward", "zero_grad", "serial", "lazy", "torch"])
def test_item_tower_on_the_third_stream_is_bit_identical_to_one_stream(golden, monkeypatch, kind, name, schedule):
    """ops.AuxFork: the item tower's forward and (by autograd's stream rule) backward kernels run on the third stream next
    to the user tower's.  Same kernels, same operands -- so three steps end in the same bits as with one stream, under
    every optimiser schedule; the history model looks up the ITEM table from both towers (deferred schedule: the two
    catch-ups of one table are ordered, optim.py::_catch_up).  Repeated: a race would not show every time."""
    import two_tower_models_amd as A
    from two_tower_models_amd import ops
    g = golden(name)
    b = batch_of(g)
    monkeypatch.setattr(ops, "_FORK_MIN_ROWS", 1)

    def run(concurrent):
        monkeypatch.setattr(ops, "_CONCURRENT_TOWERS", concurrent)
        model = make_model(kind, g)
        if schedule == "torch":
            opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        else:
            kw = dict(forward=dict(overlap_sweep="forward"), zero_grad=dict(overlap_sweep=True), serial=dict(overlap_sweep=False),
                      lazy=dict(overlap_sweep=False, lazy=True))[schedule]
            opt = A.DenseExactAdam(model.parameters(), lr=1e-3, **kw)
        losses = []
        for _ in range(3):
            loss = model.train_forward(*b)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
        if schedule == "lazy":
            opt.flush()
        torch.cuda.synchronize()
        return losses, {k: v.clone() for k, v in model.state_dict().items()}

    want_l, want = run(False)
    for _ in range(3):
        got_l, got = run(True)
        assert all(torch.equal(a, c) for a, c in zip(got_l, want_l))
        for k in want:
            assert torch.equal(got[k], want[k]), k


def test_forked_item_tower_keeps_its_batch_tensors_from_the_allocator(golden, monkeypatch):
    """ops.AuxFork.uses: item_id / item_features are allocated on the caller's stream and read by the item tower's kernels
    on the third one -- in the backward pass too, after a training loop has dropped the batch.  Unrecorded, the block goes
    back to the caller's stream when autograd releases the saved tensor and the next allocation there overwrites it under
    the still-queued weight-gradient kernel (dW1 wrong once in ~1000 steps).  Checked structurally -- both inputs are
    recorded on the third stream -- and by use: batches that exist only for the duration of train_forward, memory churn on
    the main stream during the backward pass, gradients equal to the one-stream ones every time."""
    from two_tower_models_amd import _native as N
    from two_tower_models_amd import ops
    g = golden("g2_base_aligned")
    monkeypatch.setattr(ops, "_FORK_MIN_ROWS", 1)
    model = make_model("base", g)
    seen = []
    real = torch.Tensor.record_stream

    def spy(self, stream):
        seen.append((self.data_ptr(), stream))
        return real(self, stream)

    def grads(concurrent):
        monkeypatch.setattr(ops, "_CONCURRENT_TOWERS", concurrent)
        model.zero_grad(set_to_none=True)
        loss = model.train_forward(*[t.clone() for t in batch_of(g)])  # temporaries: gone when the call returns
        junk = [torch.full((1 << 16,), float("nan"), device=DEV) for _ in range(8)]  # what the freed blocks would be reused for
        loss.backward()
        del junk
        return {n: p.grad.clone() for n, p in model.named_parameters()}

    want = grads(False)
    monkeypatch.setattr(torch.Tensor, "record_stream", spy)
    for _ in range(5):
        seen.clear()
        got = grads(True)
        aux = N.aux_stream(torch.device(DEV))
        assert sum(1 for _, s in seen if s == aux) >= 2  # item_id and item_features
        for n in want:
            assert torch.equal(got[n], want[n]), n


def test_profile_filter_brackets_only_the_named_kernels(golden):
    """tt_profile_filter: a measurement puts HIP events around the kernel it reports and around nothing else (an event pair
    delays what follows it; bench.py's events once decided which of two streams' kernels reached the CUs first)."""
    import ctypes as C

    import two_tower_models_amd as A
    from two_tower_models_amd import _native as N
    lib = N.load()
    g = golden("g2_base_aligned")
    model = make_model("base", g)
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep="forward")

    def counts(filt):
        lib.tt_profile_filter(filt)
        lib.tt_profile_enable(1)
        loss = model.train_forward(*batch_of(g))
        opt.zero_grad()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        out = {}
        for k in (b"adam_sweep_kernel", b"ce_bwd_kernel"):
            ms, n = C.c_double(0.0), C.c_int64(0)
            N.check(lib.tt_profile_read(k, C.byref(ms), C.byref(n)), "tt_profile_read")
            out[k] = n.value
        lib.tt_profile_enable(0)
        lib.tt_profile_filter(None)
        return out

    only = counts(b"adam_sweep_kernel")
    assert only[b"adam_sweep_kernel"] == 1 and only[b"ce_bwd_kernel"] == 0
    both = counts(None)
    assert both[b"adam_sweep_kernel"] == 1 and both[b"ce_bwd_kernel"] >= 1
    # ... and the optimiser's OWN event pair around every sweep launch (what bench.py reports: no events added)
    opt.keep_sweep_events(True)
    for _ in range(3):
        loss = model.train_forward(*batch_of(g))
        opt.zero_grad()
        loss.backward()
        opt.step()
    total, n = opt.sweep_launch_ms()
    assert n == 3 and 0.0 < total < 100.0
    opt.keep_sweep_events(False)
    assert opt.sweep_launch_ms() == (0.0, 0)


@pytest.mark.parametrize("name", ["g4_hist_d128", "g4_hist_tiny"])
def test_history_model_matches_reference(golden, name):
    g = golden(name)
    model = make_model("hist", g)
    b = batch_of(g)
    u = model.compute_user_embedding(b[0], b[1], b[2])
    assert torch.allclose(u.cpu(), T(g["user_emb"]), atol=1e-5)
    loss = model.train_forward(*b)
    assert abs(loss.item() - float(g["loss"])) < 1e-4
    loss.backward()
    check_grads(model, g)  # item table grad = item_id rows + history rows


def test_history_model_dense_exact_adam_runs_and_matches_torch_adam(golden):
    import two_tower_models_amd as A
    g = golden("g4_hist_d128")
    m1, m2 = make_model("hist", g), make_model("hist", g)
    o1, o2 = A.DenseExactAdam(m1.parameters(), lr=1e-3), torch.optim.Adam(m2.parameters(), lr=1e-3)
    b = batch_of(g)
    for _ in range(2):
        for m, o in ((m1, o1), (m2, o2)):
            loss = m.train_forward(*b)
            o.zero_grad()
            loss.backward()
            o.step()
    for (k, v1), (_, v2) in zip(m1.state_dict().items(), m2.state_dict().items()):
        noise_only = k in ("item_tower_arch.bias", "item_features_arch.2.bias")
        assert torch.allclose(v1, v2, atol=4.4e-3 if noise_only else 5e-6, rtol=1e-5), k


@pytest.mark.parametrize("kind", ["position", "user"])
def test_single_term_debias_models_loss_and_grads(golden, kind):
    """TwoTowerWithPositionDebiasedWeights / TwoTowerWithUserDebiasedWeights (ref:src/two_tower_with_position_debiased_weights.py,
    ref:src/two_tower_with_user_debiased_weights.py): reference parameters loaded by name, loss 1e-4 and every gradient
    -- incl. the head's, which flow through the example weights and through the batch maximum -- vs the reference."""
    g = golden(f"g8_debias_{kind}")
    model = make_model(kind, g)
    loss = model.train_forward(*batch_of(g))
    assert abs(loss.item() - float(g["loss"])) < 1e-4 * max(1.0, abs(float(g["loss"]))), (loss.item(), float(g["loss"]))
    loss.backward()
    check_grads(model, g)
    # one optimiser step moves the head as torch.optim.Adam moves it: first step = -lr * sign(g) where g is not noise
    import two_tower_models_amd as A
    head = model.position_bias_net_user_value.weight if kind == "position" else model.user_debias_net_user_value[0].weight
    before, grad = head.detach().clone(), head.grad.detach().clone()
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3)
    loss2 = model.train_forward(*batch_of(g))
    opt.zero_grad()
    loss2.backward()
    opt.step()
    moved = (head.detach() - before)
    big = grad.abs() > 1e-4 * float(grad.abs().max())
    assert torch.allclose(moved[big], -1e-3 * torch.sign(grad[big]), atol=2e-6)
    assert float(moved[grad == 0].abs().max() if bool((grad == 0).any()) else 0.0) == 0.0


def test_debias_model_loss_and_grads(golden):
    g = golden("g6_debias_d128")
    corpus = T(fg.bf16_round(fg.gaussianish((4096, 128), 901)))
    model = make_model("debias", g, corpus=corpus)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = model.train_forward(*batch_of(g))
    assert abs(loss.item() - float(g["loss"])) < 1e-4 * max(1.0, abs(float(g["loss"])))
    loss.backward()
    # atol 4e-5 of max|g|: the sum-MSE debias terms put O(100) addends that cancel into d(user embedding); column 36 of
    # user_tower_arch.weight's gradient (max|g| 4.3) then differs from the float32 CPU reference by 1.0-1.3e-4 whichever
    # product path computes it (generic GEMM 1.06e-4, fused tower 1.24e-4: rounding order, not a defect)
    check_grads(model, g, rtol=5e-4, atol_scale=4e-5)


@pytest.mark.parametrize("kind,name", [("base", "g2_base_aligned"), ("hist", "g4_hist_d128")])
def test_overlapped_sweep_is_bit_identical_to_serial(golden, kind, name):
    """The side-stream schedule (zero_grad starts the sweep, step finishes from the stash) must
    leave exactly the bits of the serial schedule, for touched and untouched rows alike."""
    import two_tower_models_amd as A
    g = golden(name)
    finals = []
    for overlap in (True, False, "forward"):
        model = make_model(kind, g)
        opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep=overlap)
        b = batch_of(g)
        for _ in range(3):
            loss = model.train_forward(*b)
            assert (opt._begun is not None) == (overlap == "forward")  # sweep already running
            opt.zero_grad()
            assert (opt._begun is not None) == bool(overlap)
            loss.backward()
            opt.step()
            assert opt._begun is None and model.item_id_embedding_arch.weight._tt_active is None
        torch.cuda.synchronize()
        finals.append({k: v.clone() for k, v in model.state_dict().items()})
        assert opt.step_count == 3
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), k
        assert torch.equal(finals[2][k], finals[1][k]), k
    # inference between steps reads the (consistent) tables, and a no_grad loss does not start a step
    with torch.no_grad():
        model.train_forward(*b)
    assert opt._begun is None


@pytest.mark.parametrize("kind,name", [("base", "g2_base_aligned"), ("hist", "g4_hist_d128")])
def test_marked_sweep_is_bit_identical_to_parked_and_serial(golden, kind, name, monkeypatch):
    """Steps that look up many rows (>= optim._SPLIT_MIN_IDS: 65 536, lowered here) do not park them: the rows are marked,
    the sweep steps over them, the lookups read the table, the finish takes the rows' old p / m / v from the table
    (csrc/adam.hip, SweepTablesMarked).  Same bits as the parked forward schedule and as the serial one, and a lookup the
    optimiser was not told about is refused -- its rows could be mid-update."""
    import two_tower_models_amd as A
    from two_tower_models_amd import optim
    g = golden(name)
    monkeypatch.setattr(optim, "_SPLIT_MIN_IDS", 1)
    finals = []
    for mode in ("marked", "parked", "serial"):
        monkeypatch.setattr(optim, "_MARK_ROWS", mode == "marked")
        model = make_model(kind, g)
        opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep=False if mode == "serial" else "forward")
        b = batch_of(g)
        for _ in range(4):
            loss = model.train_forward(*b)
            if mode != "serial":
                assert all(ts.marked == (mode == "marked") for ts in opt._begun.values()) and opt._begun
                act = model.item_id_embedding_arch.weight._tt_active
                assert (act.p_plane is None) == (mode == "marked")
            opt.zero_grad()
            loss.backward()
            opt.step()
            assert opt._begun is None and model.item_id_embedding_arch.weight._tt_active is None
        torch.cuda.synchronize()
        finals.append({k: v.clone() for k, v in model.state_dict().items()})
        finals[-1].update({f"m{i}": opt.state[p]["exp_avg"].clone() for i, p in enumerate(opt._tables)})
        finals[-1].update({f"v{i}": opt.state[p]["exp_avg_sq"].clone() for i, p in enumerate(opt._tables)})
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), k
        assert torch.equal(finals[0][k], finals[2][k]), k
    # marked rows: a lookup that was not announced must not read the table
    monkeypatch.setattr(optim, "_MARK_ROWS", True)
    b = batch_of(g)
    from two_tower_models_amd import ops
    model = make_model(kind, g)
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep="forward")
    assert opt.begin_step(model._lookup_plan(b[0], b[2], b[3]))
    with pytest.raises(RuntimeError, match="not told about"):
        ops.EmbeddingLookup.apply(model.item_id_embedding_arch.weight, b[3][:3])
    opt.release_sweep()
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind,name", [("base", "g2_base_aligned"), ("hist", "g4_hist_d128"), ("base", "g1_base_tiny")])
def test_lazy_adam_is_bit_identical_to_dense(golden, kind, name):
    """DenseExactAdam(lazy=True) replays the zero-gradient steps of a row when the row is next
    needed instead of sweeping the table every step.  After flush() every table row, both Adam
    moments and every dense parameter must carry EXACTLY the bits of the dense schedule -- rows
    touched every step, rows touched after gaps of several steps, and rows never touched."""
    import two_tower_models_amd as A
    g = golden(name)
    n_users, n_items = int(g["cfg"][0]), int(g["cfg"][3])
    base = batch_of(g)
    Bsz = base[0].shape[0]
    gen = torch.Generator().manual_seed(77)
    steps = []
    for s in range(7):  # ids from a sliding window: rows recur after 1..6 idle steps
        b = [t.clone() for t in base]
        b[0] = ((torch.randint(0, 40, (Bsz,), generator=gen) + 13 * s) % n_users).to(DEV)
        b[3] = ((torch.randint(0, 50, (Bsz,), generator=gen) + 17 * s) % n_items).to(DEV)
        if kind == "hist":
            b[2] = ((torch.randint(0, 60, tuple(base[2].shape), generator=gen) + 11 * s) % n_items).to(DEV)
        steps.append(b)
    finals, moments = [], []
    for lazy in (False, True):
        model = make_model(kind, g)
        opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep=False, lazy=lazy)
        for s, b in enumerate(steps):
            loss = model.train_forward(*b)
            if lazy and s + 1 < len(steps) and s % 2 == 0:  # every other step: replay the next batch's rows early
                nb = steps[s + 1]
                opt.prefetch_rows(model._lookup_plan(nb[0], nb[2], nb[3]))
            opt.zero_grad()
            loss.backward()
            opt.step()
            if s == 3:  # inference between steps: its lookups must see up-to-date rows as well
                with torch.no_grad():
                    probe = model.train_forward(*steps[0])
                finals.append(probe.clone())
        if lazy:
            stale = model.item_id_embedding_arch.weight.detach().clone()
            opt.flush()
            assert not torch.equal(stale, model.item_id_embedding_arch.weight)  # something WAS deferred
        torch.cuda.synchronize()
        finals.append({k: v.clone() for k, v in model.state_dict().items()})
        moments.append([(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in opt._tables])
        assert opt.step_count == len(steps)
    assert torch.equal(finals[0], finals[2])  # the mid-run no_grad loss
    for k in finals[1]:
        assert torch.equal(finals[1][k], finals[3][k]), k
    for (m0, v0), (m1, v1) in zip(*moments):
        assert torch.equal(m0, m1) and torch.equal(v0, v1)


@pytest.mark.parametrize("lazy", [False, True])
def test_checkpoint_resume_is_bit_identical(golden, lazy):
    """model.state_dict() + optimizer.state_dict() after 3 steps, loaded into fresh objects, then 2
    more steps == 5 uninterrupted steps (tables, dense parameters, moments); the optimiser state
    uses torch.optim.Adam's keys (step, exp_avg, exp_avg_sq)."""
    import io
    import two_tower_models_amd as A
    g = golden("g2_base_aligned")
    batches = [batch_of(g, prefix=f"step{s}.in.") for s in range(3)]
    batches = batches + batches[:2]

    def run(model, opt, bs):
        for b in bs:
            loss = model.train_forward(*b)
            opt.zero_grad()
            loss.backward()
            opt.step()

    ref_model = make_model("base", g)
    ref_opt = A.DenseExactAdam(ref_model.parameters(), lr=1e-3, lazy=lazy)
    run(ref_model, ref_opt, batches)
    ref_opt.flush()

    m1 = make_model("base", g)
    o1 = A.DenseExactAdam(m1.parameters(), lr=1e-3, lazy=lazy)
    run(m1, o1, batches[:3])
    buf = io.BytesIO()
    torch.save({"opt": o1.state_dict(), "model": m1.state_dict()}, buf)  # optimiser first: it flushes
    ck = torch.load(io.BytesIO(buf.getvalue()))
    any_state = next(iter(ck["opt"]["state"].values()))
    assert set(any_state) == {"step", "exp_avg", "exp_avg_sq"} and float(any_state["step"]) == 3.0
    m2 = make_model("base", g)
    m2.load_state_dict(ck["model"])
    o2 = A.DenseExactAdam(m2.parameters(), lr=1e-3, lazy=lazy)
    o2.load_state_dict(ck["opt"])
    run(m2, o2, batches[3:])
    o2.flush()
    assert o2.step_count == 5
    for (k, a), (_, b) in zip(ref_model.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    for pa, pb in zip(ref_opt._params, o2._params):
        assert torch.equal(ref_opt.state[pa]["exp_avg"], o2.state[pb]["exp_avg"])
        assert torch.equal(ref_opt.state[pa]["exp_avg_sq"], o2.state[pb]["exp_avg_sq"])


@pytest.mark.parametrize("kind,name,lazy,overlap", [("base", "g2_base_aligned", True, False), ("base", "g2_base_aligned", False, False),
                                                    ("hist", "g4_hist_d128", True, False),
                                                    # multi-stream capture: the side-stream sweep is a branch of the graph
                                                    ("base", "g2_base_aligned", False, "forward"),
                                                    ("hist", "g4_hist_d128", False, "forward")])
def test_graphed_train_step_is_bit_identical_to_eager(golden, kind, name, lazy, overlap):
    """GraphedTrainStep (whole-step hipGraph: forward, zero_grad, backward, optimiser) replayed N
    times == N eager steps: the step count and bias corrections advance on the device, row plans
    are sized on the device, so nothing is baked into the captured graph but the shapes."""
    import two_tower_models_amd as A
    g = golden(name)
    base = batch_of(g)
    n_users, n_items = int(g["cfg"][0]), int(g["cfg"][3])
    gen = torch.Generator().manual_seed(5)
    bs = []
    for s in range(8):
        b = [t.clone() for t in base]
        b[0] = torch.randint(0, n_users, tuple(base[0].shape), generator=gen).to(DEV)
        b[3] = torch.randint(0, n_items, tuple(base[3].shape), generator=gen).to(DEV)
        bs.append(b)
    W = 2  # GraphedTrainStep's warm-up = W real steps on the example batch
    order = [bs[0]] * W + bs[1:]
    eager = make_model(kind, g)
    eopt = A.DenseExactAdam(eager.parameters(), lr=1e-3, overlap_sweep=False, lazy=lazy)
    elosses = []
    side = torch.cuda.Stream()  # eager reference on a side stream as well (same autograd stream rules)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for b in order:
            loss = eager.train_forward(*b)
            eopt.zero_grad()
            loss.backward()
            eopt.step()
            elosses.append(loss.item())
        eopt.flush()
    torch.cuda.current_stream().wait_stream(side)
    del loss
    model = make_model(kind, g)
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep=overlap, lazy=lazy)
    step = A.GraphedTrainStep(model, opt, bs[0], warmup=W, capture_overlap=overlap == "forward")
    assert opt.capture_overlap == (overlap == "forward")
    glosses = [step(*b).item() for b in bs[1:]]
    opt.flush()
    torch.cuda.synchronize()
    assert opt.step_count == len(order)
    assert glosses == elosses[W:]
    for (k, a), (_, b) in zip(eager.state_dict().items(), model.state_dict().items()):
        assert torch.equal(a, b), k


def test_zero_grad_before_forward_takes_serial_schedule(golden):
    import two_tower_models_amd as A
    g = golden("g2_base_aligned")
    model = make_model("base", g)
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3)
    losses = []
    for s in range(3):
        opt.zero_grad()  # the other common loop order
        loss = model.train_forward(*batch_of(g, prefix=f"step{s}.in."))
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert np.allclose(losses, g["adam_losses"], atol=1e-4)


# ------------------------------------------------------------------ edge cases
def _tiny(kind="base", H=3):
    import two_tower_models_amd as A
    torch.manual_seed(3)
    mips = A.BaselineMIPSModule(corpus_size=40, embedding_dim=16)
    kw = dict(num_items=5, user_id_hash_size=7, user_id_embedding_dim=16, user_features_size=3,
              item_id_hash_size=9, item_id_embedding_dim=16, item_features_size=2,
              user_value_weights=[1.0], mips_module=mips)
    m = A.TwoTowerBaseRetrieval(**kw) if kind == "base" else A.TwoTowerWithUserHistoryEncoder(user_history_seqlen=H, **kw)
    return m


def _oracle_step(model_cpu_state, batch, with_history, H, lr=1e-3, steps=1):
    from oracle import cpu_ref as R
    params = {k: v.clone() for k, v in model_cpu_state.items()}
    state = R.AdamState(params)
    kw = dict(with_history=with_history, heads=4, pos_table=R.positional_table(H, 16)) if with_history else {}
    losses = [R.train_step(params, state, batch, torch.tensor([1.0]), lr=lr, **kw) for _ in range(steps)]
    return losses, params


@pytest.mark.parametrize("kind,B,H", [("base", 1, 3), ("base", 5, 3), ("hist", 1, 1), ("hist", 4, 2)])
def test_tiny_batches_and_all_duplicate_ids(kind, B, H):
    """B = 1 (a 1x1 logit matrix: loss 0, zero logit gradient), H = 1, and a batch whose user and
    history ids are ALL the same row (maximal duplicate accumulation), two optimiser steps each.
    (Item ids stay distinct: identical item rows would add a common vector to every item
    embedding, whose gradient is analytically zero -- Adam would only see rounding noise.)"""
    import two_tower_models_amd as A
    model = _tiny(kind, H)
    state0 = {k: v.clone() for k, v in model.state_dict().items()}
    batch = [torch.full((B,), 2), torch.randn(B, 3), torch.full((B, H), 4), torch.arange(B) % 9,
             torch.randn(B, 2), torch.zeros(B, dtype=torch.long), torch.ones(B, 1)]
    want_losses, want = _oracle_step(state0, batch, kind == "hist", H, steps=2)
    model = model.to(DEV)
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3)
    got = []
    for _ in range(2):
        loss = model.train_forward(*[t.to(DEV) for t in batch])
        opt.zero_grad()
        loss.backward()
        opt.step()
        got.append(loss.item())
    assert np.allclose(got, want_losses, atol=1e-5)
    # With 1-5 samples many dense gradients are tiny (dead or barely-live ReLU units): Adam turns a
    # relative rounding difference in a ~1e-7 gradient into an O(lr) step difference, so the dense
    # parameters are bounded by steps*lr here; the loss trajectory (above) and the tables are tight.
    for k, v in model.state_dict().items():
        is_table = k.endswith("embedding_arch.weight")
        # item_tower_arch.bias / item_features_arch.2.bias: analytically ZERO gradient -- both sides
        # take +-lr steps of arbitrary sign on rounding noise, so two correct implementations can end 2 * steps * lr apart
        noise_only = k in ("item_tower_arch.bias", "item_features_arch.2.bias")
        atol = 1e-5 if is_table else (2 * 2 * 1.05e-3 if noise_only else 2 * 1.1e-3)
        assert torch.allclose(v.cpu(), want[k], atol=atol), k


def test_out_of_range_id_raises_index_error():
    model = _tiny().to(DEV)
    B = 4
    bad = [torch.tensor([0, 1, 99, 2], device=DEV), torch.randn(B, 3, device=DEV), torch.zeros(B, 3, dtype=torch.long, device=DEV)]
    with pytest.raises(IndexError):
        model(*bad)  # nn.Embedding would raise "index out of range in self"; inference checks eagerly
    ok = [torch.tensor([0, 1, 3, 2], device=DEV), bad[1], bad[2]]
    assert model(*ok).shape == (B, 5)


@pytest.mark.parametrize("D,kind", [(256, "hist"), (512, "hist"), (192, "base"), (96, "base"), (96, "hist")])
def test_wide_embeddings_train_step_vs_oracle(D, kind):
    """Embedding widths off the tuned set: the reference accepts any width; here D = 256 / 512 (history model: heads
    of 64 / 128, in-batch CE and MIPS through their generic-width forms), a ragged 192, and 96 (the
    fused tower and the matrix-core attention do not take it -- heads of 24 -- so the generic kernels run, and SAY so:
    `ops.generic_paths` names each path and the constraint, with a one-time RuntimeWarning).  One train step vs the
    oracle: loss 1e-4, updated tables and dense parameters; then forward() top-K vs the oracle's scores."""
    import two_tower_models_amd as A
    from two_tower_models_amd import ops
    from oracle import cpu_ref as R
    torch.manual_seed(11)
    B, H, NU, NI, F = 48, 6, 300, 500, 8
    mips = A.BaselineMIPSModule(corpus_size=700, embedding_dim=D)
    kw = dict(num_items=10, user_id_hash_size=NU, user_id_embedding_dim=D, user_features_size=F, item_id_hash_size=NI,
              item_id_embedding_dim=D, item_features_size=F, user_value_weights=[1.0], mips_module=mips)
    model = A.TwoTowerBaseRetrieval(**kw) if kind == "base" else A.TwoTowerWithUserHistoryEncoder(user_history_seqlen=H, **kw)
    with torch.no_grad():  # keep the logits O(1): D-wide towers with default init saturate the softmax
        for n, p in model.named_parameters():
            if n.endswith("tower_arch.weight"):
                p.mul_(0.2)
            if "embedding_arch" in n:
                p.mul_(0.3)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    corpus = mips.corpus.clone()
    model = model.to(DEV)
    g = torch.Generator().manual_seed(5)
    batch = [torch.randint(0, NU, (B,), generator=g), torch.randn(B, F, generator=g), torch.randint(0, NI, (B, H), generator=g),
             torch.randint(0, NI, (B,), generator=g), torch.randn(B, F, generator=g), torch.randint(0, 10, (B,), generator=g),
             torch.randint(0, 2, (B, 1), generator=g).float()]
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3)
    loss = model.train_forward(*[t.to(DEV) for t in batch])
    opt.zero_grad()
    loss.backward()
    opt.step()
    fkw = dict(with_history=True, heads=4, pos_table=R.positional_table(H, D)) if kind == "hist" else {}
    state = R.AdamState(params)
    want = R.train_step(params, state, batch, torch.tensor([1.0]), **fkw)
    assert abs(loss.item() - want) < 1e-4, (loss.item(), want)
    for k, v in model.state_dict().items():
        err = (v.cpu() - params[k]).abs()
        assert float(err.max()) <= 2 * 1e-3 * 1.05, (k, float(err.max()))  # one Adam step moves an element by <= lr
        noise_only = k in ("item_tower_arch.bias", "item_features_arch.2.bias") or k.endswith("in_proj_bias")
        if not noise_only:
            assert int((err > 5e-6).sum()) <= max(1, int(2e-3 * err.numel())), (k, int((err > 5e-6).sum()), err.numel())
    with torch.no_grad():
        top = model(*[t.to(DEV) for t in batch[:3]])
        u = R.user_embedding(params, *batch[:3], **fkw) if kind == "hist" else R.user_embedding(params, *batch[:3], with_history=False)
    full = u.double() @ corpus.double().t()
    picked = torch.gather(full, 1, top.cpu())
    kth = torch.topk(full, 10, dim=1).values[:, -1]
    assert bool((picked.min(1).values >= kth - 1e-4).all())
    # a fast path that was not taken is reported, with the constraint that ruled it out
    tower = [v for k, v in ops.generic_paths.items() if k.startswith("tower")]
    assert tower and "F <= 64" in tower[0]
    if D > 128:
        assert "in-batch softmax CE" in ops.generic_paths and "MIPS top-K" in ops.generic_paths
    if kind == "hist" and D in (96, 512):
        assert "head width" in ops.generic_paths["history-encoder attention"]


def test_sweep_throttle_does_not_change_results(golden):
    """The closed-loop sweep throttle (fewer persistent sweep workgroups when the step is much longer than the sweep)
    is a scheduling decision only: pinning the widest, a thin and the thinnest sweep gives bit-identical tables."""
    import os
    import two_tower_models_amd as A
    g = golden("g2_base_aligned")
    outs = []
    for wgs in (0, 128, 1):
        model = make_model("base", g)
        opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep="forward")
        opt._tune_sweep = lambda: None  # no controller: the width below stays
        opt._sweep_wgs = wgs
        for s in range(3):
            loss = model.train_forward(*batch_of(g, prefix=f"step{s}.in."))
            opt.zero_grad()
            loss.backward()
            opt.step()
        outs.append({k: v.clone() for k, v in model.state_dict().items()})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]) and torch.equal(outs[0][k], outs[2][k]), k


@pytest.mark.parametrize("kind,name", [("base", "g2_base_aligned"), ("hist", "g4_hist_d128")])
def test_inference_between_train_steps_leaves_training_alone(golden, kind, name):
    """model.forward() -- the reference's inference entry (ref:src/two_tower_base_retrieval.py:221-249), called WITHOUT
    torch.no_grad() like upstream's own tests do -- between two train steps of the forward-announced optimiser schedule: the
    training run is bit-identical to the one without the call (its lookups are not recorded for the table step)."""
    import two_tower_models_amd as A
    g = golden(name)

    def run(serve):
        model = make_model(kind, g)
        opt = A.DenseExactAdam(model.parameters(), lr=1e-3)
        b = batch_of(g)
        losses = []
        for _ in range(3):
            loss = model.train_forward(*b)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss))
            if serve:
                top = model(b[0], b[1], b[2])
                assert top.dtype == torch.int64 and top.shape[1] == 10 and not top.requires_grad
        return losses, {k: v.clone() for k, v in model.state_dict().items()}

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1 and all(torch.equal(s0[k], s1[k]) for k in s0)
