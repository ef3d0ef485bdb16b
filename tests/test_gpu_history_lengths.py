"""Variable-length histories on MI355X (`pytest -m gpu`): the `_len` kernels at the C ABI, ops.HistoryEncoder /
UserHistoryEncoder with `lengths`, and the history models with `user_history_lengths`, against the float64 CPU reference
of tests/history_lengths_ref.py (oracle.cpu_ref pieces, truncated per sample).

Tolerances are the project's own for the same quantities (tests/test_gpu_kernels.py, tests/test_gpu_models.py):
attention ctx 2e-6 / 1e-5; d_qkv 2e-6 max|.| + 1e-7 / 2e-4; collapsed layer output 4e-6, gradients 4e-6 max|.| + 1e-8 / 2e-4;
encoder output 1e-5, encoder / model gradients 1e-5 max|.| / 2e-4; model loss 1e-4."""
import numpy as np
import pytest
import torch

import fixture_gen as fg
import history_lengths_ref as HR
from oracle import cpu_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def rnd(shape, seed, scale=1.0):
    return T(fg.gaussianish(shape, seed)) * scale


def i32(lengths):
    return torch.tensor(lengths, dtype=torch.int32, device=DEV)


def pad_mask(lengths, H):
    """[B, H] bool, True on padded slots."""
    return torch.arange(H)[None, :] >= torch.tensor(lengths)[:, None]


def close(got, want, atol, rtol=0.0):
    got, want = got.detach().cpu().to(F64), want.detach().to(F64)
    err = (got - want).abs() - rtol * want.abs()
    return bool((err <= atol).all()), float(err.max())


def lib_and_native():
    from two_tower_models_amd import _native as N
    return N.load(), N


# ------------------------------------------------------------------ attention at the C ABI
ATTN = {"mfma_h50_wg_shape": (6, 50, 128, 4, [1, 2, 31, 32, 33, 50]),
        "mfma_h64": (5, 64, 64, 4, [1, 32, 33, 63, 64]),
        "valu_odd": (4, 7, 40, 4, [1, 3, 6, 7]),
        "valu_h128": (3, 128, 64, 4, [1, 65, 128])}


@pytest.mark.parametrize("case", sorted(ATTN))
def test_attention_len_forward_and_backward(case):
    """tt_attn_fwd_len / tt_attn_bwd_len on every implementation (matrix cores for H <= 64 -- at H = 50, D = 128, 4 heads the
    shape the workgroup backward takes without lengths --, the generic VALU pair otherwise): ctx and d_qkv match the
    reference on valid rows and are exactly zero on padded rows; padded rows of qkv hold NaN and padded rows of d_ctx
    NaN / 1e30 (never read)."""
    lib, N = lib_and_native()
    B, H, D, heads, lengths = ATTN[case]
    pad = pad_mask(lengths, H)
    qkv = rnd((B * H, 3 * D), 31, 0.5)
    d_ctx = rnd((B * H, D), 32)
    q64, g64 = qkv.to(F64).requires_grad_(True), d_ctx.to(F64)
    g64 = torch.where(pad.reshape(-1, 1), torch.zeros_like(g64), g64)
    ctx_ref = HR.attention_core(q64, B, H, D, heads, lengths)
    (dq_ref,) = torch.autograd.grad((ctx_ref * g64).sum(), [q64])
    qkv_g, dctx_g = qkv.clone(), d_ctx.clone()
    qkv_g[pad.reshape(-1)] = float("nan")
    garbage = torch.full((D,), 1e30)
    garbage[::2] = float("nan")
    dctx_g[pad.reshape(-1)] = garbage
    qkv_d, dctx_d, ln = qkv_g.to(DEV), dctx_g.to(DEV), i32(lengths)
    ctx = torch.full((B * H, D), 7.0, device=DEV)
    lse = torch.full((B, heads, H), 7.0, device=DEV)
    N.check(lib.tt_attn_fwd_len(qkv_d.data_ptr(), B, H, D, heads, ln.data_ptr(), ctx.data_ptr(), lse.data_ptr(), N.stream()),
            "tt_attn_fwd_len")
    d_qkv = torch.full((B * H, 3 * D), 7.0, device=DEV)
    N.check(lib.tt_attn_bwd_len(qkv_d.data_ptr(), ctx.data_ptr(), lse.data_ptr(), dctx_d.data_ptr(), B, H, D, heads,
                                ln.data_ptr(), d_qkv.data_ptr(), N.stream()), "tt_attn_bwd_len")
    torch.cuda.synchronize()
    ok, err = close(ctx, ctx_ref, 2e-6, 1e-5)
    print(f"{case}: ctx err {err:.3e}")
    assert ok, err
    ok, err = close(d_qkv, dq_ref, 2e-6 * float(dq_ref.abs().max()) + 1e-7, 2e-4)
    print(f"{case}: d_qkv err {err:.3e} (max|d_qkv| {float(dq_ref.abs().max()):.3e})")
    assert ok, err
    assert bool((ctx.cpu()[pad.reshape(-1)] == 0).all()) and bool((d_qkv.cpu()[pad.reshape(-1)] == 0).all())
    assert bool(torch.isfinite(lse).all())
    # lengths == NULL: exactly the call without `_len`
    full = rnd((B * H, 3 * D), 33, 0.5).to(DEV)
    c0, l0, c1, l1 = (torch.empty_like(ctx), torch.empty_like(lse), torch.empty_like(ctx), torch.empty_like(lse))
    N.check(lib.tt_attn_fwd(full.data_ptr(), B, H, D, heads, c0.data_ptr(), l0.data_ptr(), N.stream()), "tt_attn_fwd")
    N.check(lib.tt_attn_fwd_len(full.data_ptr(), B, H, D, heads, None, c1.data_ptr(), l1.data_ptr(), N.stream()), "tt_attn_fwd_len")
    g = d_ctx.to(DEV)
    d0, d1 = torch.empty_like(d_qkv), torch.empty_like(d_qkv)
    N.check(lib.tt_attn_bwd(full.data_ptr(), c0.data_ptr(), l0.data_ptr(), g.data_ptr(), B, H, D, heads, d0.data_ptr(), N.stream()),
            "tt_attn_bwd")
    N.check(lib.tt_attn_bwd_len(full.data_ptr(), c0.data_ptr(), l0.data_ptr(), g.data_ptr(), B, H, D, heads, None, d1.data_ptr(),
                                N.stream()), "tt_attn_bwd_len")
    assert torch.equal(c0, c1) and torch.equal(l0, l1) and torch.equal(d0, d1)


# ------------------------------------------------------------------ collapsed last layer at the C ABI
@pytest.mark.parametrize("B,H,D,heads", [(33, 50, 128, 4), (33, 10, 100, 5), (4, 3, 4, 1)])
def test_collapsed_last_layer_len(B, H, D, heads):
    """tt_enc_last_fwd_len, then the UNCHANGED backward (tt_enc_last_bwd): lengths cycle through 1 .. H (B = 33 crosses the
    32-sample partial-sum boundary of the weight-gradient kernel); output, dx (zero on padded rows) and the four parameter
    gradients.  Padded rows of x hold finite garbage: the backward halves see the padding through the saved probs alone."""
    lib, N = lib_and_native()
    assert lib.tt_enc_last_supported(H, D, heads)
    lengths = [(b % H) + 1 for b in range(B)]
    pad = pad_mask(lengths, H)
    x = rnd((B, H, D), 41)
    w_in, b_in = rnd((3 * D, D), 42, D ** -0.5), rnd((3 * D,), 43, 0.3)
    w_out, b_out = rnd((D, D), 44, D ** -0.5), rnd((D,), 45, 0.3)
    d_recent = rnd((B, D), 46)
    leaves = [t.to(F64).requires_grad_(True) for t in (x, w_in, b_in, w_out, b_out)]
    want = HR.last_layer_row0(*leaves[:1], lengths, *leaves[1:], heads)
    grads = torch.autograd.grad((want * d_recent.to(F64)).sum(), leaves)
    xg = x.clone()
    xg[pad] = rnd((int(pad.sum()), D), 47, 50.0)  # finite garbage
    dev = [t.to(DEV).contiguous() for t in (xg.reshape(B * H, D), w_in, b_in, w_out, b_out, d_recent)]
    xd, wi, bi, wo, bo, dr = dev
    ln = i32(lengths)
    recent, q0, ctx0 = (torch.empty(B, D, device=DEV) for _ in range(3))
    tq, xbar = (torch.empty(B, heads, D, device=DEV) for _ in range(2))
    probs = torch.full((B, heads, H), 7.0, device=DEV)
    N.check(lib.tt_enc_last_fwd_len(xd.data_ptr(), B, H, D, heads, ln.data_ptr(), wi.data_ptr(), bi.data_ptr(), wo.data_ptr(),
                                    bo.data_ptr(), recent.data_ptr(), D, q0.data_ptr(), tq.data_ptr(), probs.data_ptr(),
                                    xbar.data_ptr(), ctx0.data_ptr(), N.stream()), "tt_enc_last_fwd_len")
    dx = torch.full((B * H, D), 7.0, device=DEV)
    dW_in, db_in = torch.empty(3 * D, D, device=DEV), torch.empty(3 * D, device=DEV)
    dW_out, db_out = torch.empty(D, D, device=DEV), torch.empty(D, device=DEV)
    ws = torch.empty(max(int(lib.tt_enc_last_bwd_workspace_bytes(B, H, D, heads)), 16), dtype=torch.uint8, device=DEV)
    N.check(lib.tt_enc_last_bwd(xd.data_ptr(), B, H, D, heads, wi.data_ptr(), wo.data_ptr(), dr.data_ptr(), D, q0.data_ptr(),
                                tq.data_ptr(), probs.data_ptr(), xbar.data_ptr(), ctx0.data_ptr(), dx.data_ptr(),
                                dW_in.data_ptr(), db_in.data_ptr(), dW_out.data_ptr(), db_out.data_ptr(), ws.data_ptr(),
                                ws.numel(), N.stream()), "tt_enc_last_bwd")
    torch.cuda.synchronize()
    ok, err = close(recent, want, 4e-6)
    print(f"recent err {err:.3e}")
    assert ok, err
    assert bool((probs.cpu()[pad[:, None, :].expand(B, heads, H)] == 0).all())
    assert abs(float(probs.sum()) - B * heads) < 1e-3
    for name, got, ref in (("dx", dx.view(B, H, D), grads[0]), ("dW_in", dW_in, grads[1]), ("db_in", db_in, grads[2]),
                           ("dW_out", dW_out, grads[3]), ("db_out", db_out, grads[4])):
        ok, err = close(got, ref, 4e-6 * float(ref.abs().max()) + 1e-8, 2e-4)
        print(f"{name} err {err:.3e} (max {float(ref.abs().max()):.3e})")
        assert ok, (name, err)
    assert bool((dx.view(B, H, D).cpu()[pad] == 0).all())


# ------------------------------------------------------------------ gather + masked mean at the C ABI
POOL = {(128, 50, 9): [1, 2, 7, 8, 9, 25, 49, 50, 33], (50, 7, 4): [1, 3, 6, 7]}


@pytest.mark.parametrize("ids_form", [True, False])
@pytest.mark.parametrize("D,H,B", sorted(POOL))
def test_hist_embed_pool_len(D, H, B, ids_form):
    """x = row + pe on valid slots (the very fp32 add) and ZERO on padded slots, pooled = the masked mean; the embedded form's
    padded rows hold NaN.  Mean tolerance: recursive fp32 summation of n <= H terms errs by at most n u sum|x| / n
    <= H 2^-24 max|x|.  Then the pool's backward, tt_hist_pool_bwd_len: dx[b, h < len] += d_pooled[b] / len."""
    lib, N = lib_and_native()
    lengths = POOL[(D, H, B)]
    pad = pad_mask(lengths, H)
    n_rows = 97
    table, pe = rnd((n_rows, D), 51), rnd((H, D), 52)
    ids = T(fg.uniform_ids((B, H), n_rows, 53))
    emb = table[ids]  # [B, H, D]
    xv, pooled_ref = HR.masked_pool(emb.to(F64), lengths)
    x_ref = torch.where(pad[:, :, None], torch.zeros_like(emb), emb + pe[None])
    if ids_form:
        src, ids_d, rows = table.to(DEV), ids.to(DEV), n_rows
    else:
        e = emb.clone()
        e[pad] = float("nan")
        src, ids_d, rows = e.to(DEV), None, 0
    x = torch.full((B * H, D), 7.0, device=DEV)
    out = torch.full((B, 2, D), 7.0, device=DEV)
    pooled = out[:, 1, :]
    flag = N.oob.flag(torch.device(DEV))
    flag.zero_()
    ln, ped = i32(lengths), pe.to(DEV)
    N.check(lib.tt_hist_embed_pool_len(src.data_ptr(), rows, D, N.ptr(ids_d), B, H, ln.data_ptr(), ped.data_ptr(), x.data_ptr(),
                                       pooled.data_ptr(), 2 * D, flag.data_ptr(), N.stream()), "tt_hist_embed_pool_len")
    N.oob.poll(torch.device(DEV), blocking=True)  # nothing out of range
    assert torch.equal(x.view(B, H, D).cpu(), x_ref)
    ok, err = close(pooled, pooled_ref, H * 2.0 ** -24 * float(emb.abs().max()))
    print(f"pooled err {err:.3e}")
    assert ok, err
    # backward of the pool
    dx0 = rnd((B, H, D), 54)
    d_pooled = rnd((B, 2, D), 55).to(DEV)
    dx = dx0.to(DEV).contiguous()
    N.check(lib.tt_hist_pool_bwd_len(dx.data_ptr(), B, H, D, ln.data_ptr(), d_pooled[:, 1, :].data_ptr(), 2 * D, N.stream()),
            "tt_hist_pool_bwd_len")
    want = dx0.to(F64) + torch.where(pad[:, :, None], torch.zeros(1, dtype=F64),
                                     d_pooled[:, 1, :].cpu().to(F64)[:, None, :] / torch.tensor(lengths, dtype=F64)[:, None, None])
    ok, err = close(dx, want, 4 * 2.0 ** -24 * float(want.abs().max()))
    assert ok, err
    assert torch.equal(dx.cpu()[pad], dx0[pad])  # padded rows untouched
    # a length of 0 in place of a 1, and one of H + 1 in place of an H: the kernel completes with the value clamped into
    # [1, H] -- the same x and mean as before -- and the flag raises at the next poll
    for bad, acts_as in ((0, 1), (H + 1, H)):
        lb = list(lengths)
        lb[lengths.index(acts_as)] = bad
        x.fill_(7.0)
        out.fill_(7.0)
        N.check(lib.tt_hist_embed_pool_len(src.data_ptr(), rows, D, N.ptr(ids_d), B, H, i32(lb).data_ptr(), ped.data_ptr(),
                                           x.data_ptr(), pooled.data_ptr(), 2 * D, flag.data_ptr(), N.stream()),
                "tt_hist_embed_pool_len")
        torch.cuda.synchronize()
        with pytest.raises(IndexError):
            N.oob.poll(torch.device(DEV), blocking=True)
        N.oob.poll(torch.device(DEV), blocking=True)  # cleared
        assert torch.equal(x.view(B, H, D).cpu(), x_ref)
        ok, err = close(pooled, pooled_ref, H * 2.0 ** -24 * float(emb.abs().max()))
        assert ok, err


# ------------------------------------------------------------------ UserHistoryEncoder
ENC_LENGTHS = {"g3_encoder_d128": [1, 2, 31, 32, 33, 49, 50, 17], "g3_encoder_odd": [1, 3, 6, 7, 4]}
_enc_cache = {}


def encoder_case(golden, name):
    """(encoder on the device with L = 3 layers of golden weights, x, cot, lengths, float64 reference) -- the reference is
    computed once per fixture and shared.  g3_encoder_odd holds two layers: its third layer repeats the first one's weights."""
    import two_tower_models_amd as A
    g = golden(name)
    D, H, heads, L, B, pe = (int(v) for v in g["cfg"])
    sd = {k[2:]: T(v) for k, v in g.items() if k.startswith("p.")}
    for l in range(L, 3):
        for k in [k for k in sd if k.startswith("multihead_attn_layers.0.")]:
            sd[k.replace("layers.0.", f"layers.{l}.")] = sd[k].clone()
    enc = A.UserHistoryEncoder(D, H, heads, 3, True)
    enc.load_state_dict(sd)
    enc = enc.to(DEV)
    lengths = ENC_LENGTHS[name]
    if name not in _enc_cache:
        leaves = {k: v.to(F64).requires_grad_(True) for k, v in sd.items()}
        x64 = T(g["x"]).to(F64).requires_grad_(True)
        y = HR.encoder_truncated(x64, lengths, R.encoder_layers_from_params(leaves, prefix=""), heads, T(g["pe_table"]).to(F64))
        grads = torch.autograd.grad((y * T(g["cot"]).to(F64)).sum(), [x64] + list(leaves.values()))
        _enc_cache[name] = (y.detach(), grads[0], dict(zip(leaves, grads[1:])))
    return enc, T(g["x"]), T(g["cot"]), lengths, _enc_cache[name]


def check_encoder(enc, y, x, ref, label=""):
    y_ref, gx_ref, gp_ref = ref
    ok, err = close(y, y_ref, 1e-5)
    print(f"{label} y err {err:.3e}")
    assert ok, err
    ok, err = close(x.grad, gx_ref, 1e-5 * float(gx_ref.abs().max()), 2e-4)
    print(f"{label} gx err {err:.3e} (max {float(gx_ref.abs().max()):.3e})")
    assert ok, err
    for n, p in enc.named_parameters():
        ok, err = close(p.grad, gp_ref[n], max(1e-5 * float(gp_ref[n].abs().max()), 1e-7), 2e-4)
        print(f"{label} {n} err {err:.3e} (max {float(gp_ref[n].abs().max()):.3e})")
        assert ok, (n, err)


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("name", sorted(ENC_LENGTHS))
def test_encoder_with_lengths_matches_reference(golden, name, generic, monkeypatch):
    """Three layers, mixed lengths: output, input gradient (zero on padded rows) and every parameter gradient; once more with
    every layer in full (ops._ENC_GENERIC).  Lengths as int64 here, int32 in the other tests."""
    from two_tower_models_amd import ops
    monkeypatch.setattr(ops, "_ENC_GENERIC", generic)
    enc, x, cot, lengths, ref = encoder_case(golden, name)
    xd = x.to(DEV).requires_grad_(True)
    y = enc(xd, torch.tensor(lengths, dtype=torch.int64, device=DEV))
    (y * cot.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    check_encoder(enc, y, xd, ref, f"{name} generic={generic}")
    assert bool((xd.grad.cpu()[pad_mask(lengths, x.shape[1])] == 0).all())


def test_encoder_with_lengths_large_batch():
    """B * H >= 16384 at D = 128 (B = 328, H = 50): where the fixed-length path takes the fused pool-backward epilogue, the
    masked path's replacement (the product, then tt_hist_pool_bwd_len) runs.  Reference: the vectorised additive-mask form."""
    import two_tower_models_amd as A
    B, H, D, heads = 328, 50, 128, 4
    torch.manual_seed(3)
    enc = A.UserHistoryEncoder(D, H, heads, 3, True)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("bias"):
                p.copy_(rnd(tuple(p.shape), 61 + len(n), 0.2))
    lengths = [(b * 7) % H + 1 for b in range(B)]
    x, cot = rnd((B, H, D), 62), rnd((B, 2, D), 63)
    leaves = {k: v.detach().to(F64).requires_grad_(True) for k, v in enc.state_dict().items()}
    x64 = x.to(F64).requires_grad_(True)
    y_ref = HR.encoder_masked(x64, lengths, R.encoder_layers_from_params(leaves, prefix=""), heads,
                              enc.positional_embeddings.to(F64))
    grads = torch.autograd.grad((y_ref * cot.to(F64)).sum(), [x64] + list(leaves.values()))
    enc = enc.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    y = enc(xd, i32(lengths))
    (y * cot.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    check_encoder(enc, y, xd, (y_ref.detach(), grads[0], dict(zip(leaves, grads[1:]))), "large")
    assert bool((xd.grad.cpu()[pad_mask(lengths, H)] == 0).all())


def _run_encoder(enc, x, cot, lengths, table_ids=None):
    enc.zero_grad(set_to_none=True)
    if table_ids is not None:
        table, ids = table_ids
        table.grad = None
        y = enc.encode_ids(table, ids, lengths)
    else:
        x = x.clone().requires_grad_(True)
        y = enc(x, lengths)
    (y * cot).sum().backward()
    torch.cuda.synchronize()
    src_grad = table_ids[0].grad if table_ids is not None else x.grad
    return y.detach().clone(), src_grad.clone(), [p.grad.clone() for p in enc.parameters()]


@pytest.mark.parametrize("name", sorted(ENC_LENGTHS))
def test_padded_slots_do_not_matter(golden, name):
    """No reference involved: NaN, Inf and 1e30 in the padded rows of an embedded input, other valid ids in the padded
    slots of the id form -- output and every gradient are bit-identical to the clean run, padded-row gradients exactly 0.0
    (through the id entry: a row that only padded slots name gets exactly zero)."""
    enc, x, cot, lengths, _ = encoder_case(golden, name)
    B, H, D = x.shape
    pad = pad_mask(lengths, H)
    ln, cotd = i32(lengths), cot.to(DEV)
    clean = _run_encoder(enc, x.to(DEV), cotd, ln)
    dirty_x = x.clone()
    junk = torch.tensor([float("nan"), float("inf"), 1e30, float("-inf")]).repeat(D // 4 + 1)[:D]
    dirty_x[pad] = junk
    dirty = _run_encoder(enc, dirty_x.to(DEV), cotd, ln)
    assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1])
    assert all(torch.equal(a, b) for a, b in zip(clean[2], dirty[2]))
    assert bool(torch.isfinite(dirty[0]).all()) and bool((dirty[1].cpu()[pad] == 0).all())
    # the id form
    n_rows = 64
    table = torch.nn.Parameter(rnd((n_rows + 8, D), 71).to(DEV))
    ids = T(fg.uniform_ids((B, H), n_rows, 72))
    ids_a, ids_b = ids.clone(), ids.clone()
    ids_a[pad] = 0
    ids_b[pad] = n_rows + T(fg.uniform_ids((int(pad.sum()),), 8, 73))  # rows that ONLY padded slots name
    ra = _run_encoder(enc, None, cotd, ln, (table, ids_a.to(DEV)))
    rb = _run_encoder(enc, None, cotd, ln, (table, ids_b.to(DEV)))
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1]) and all(torch.equal(a, b) for a, b in zip(ra[2], rb[2]))
    assert bool((rb[1][n_rows:] == 0).all()) and float(rb[1][:n_rows].abs().max()) > 0


@pytest.mark.parametrize("name", sorted(ENC_LENGTHS))
def test_full_lengths_equal_no_lengths(golden, name):
    """All lengths = H against lengths = None: the same result within the encoder tolerances (whether it is bit-identical is
    recorded in DESIGN.md: the forward is, the backward takes another attention kernel at the workgroup kernel's shapes)."""
    enc, x, cot, _, _ = encoder_case(golden, name)
    B, H, D = x.shape
    cotd = cot.to(DEV)
    none = _run_encoder(enc, x.to(DEV), cotd, None)
    full = _run_encoder(enc, x.to(DEV), cotd, i32([H] * B))
    print(f"{name}: y bit-identical {torch.equal(none[0], full[0])}, gx {torch.equal(none[1], full[1])}, "
          f"params {all(torch.equal(a, b) for a, b in zip(none[2], full[2]))}")
    ok, err = close(full[0], none[0].cpu(), 1e-5)
    assert ok, err
    ok, err = close(full[1], none[1].cpu(), 1e-5 * float(none[1].abs().max()), 2e-4)
    assert ok, err
    for a, b in zip(none[2], full[2]):
        ok, err = close(b, a.cpu(), max(1e-5 * float(a.abs().max()), 1e-7), 2e-4)
        assert ok, err


def test_bad_length_raises_index_error_at_the_model_surface(golden):
    """A length outside [1, H] through the module: the kernels run (clamped), IndexError at the next blocking poll."""
    from two_tower_models_amd import _native as N
    enc, x, cot, lengths, _ = encoder_case(golden, "g3_encoder_odd")
    N.oob.flag(torch.device(DEV)).zero_()
    bad = list(lengths)
    bad[2] = x.shape[1] + 3
    y = enc(x.to(DEV), i32(bad))
    assert bool(torch.isfinite(y).all())
    with pytest.raises(IndexError):
        N.oob.poll(torch.device(DEV), blocking=True)
    with pytest.raises(TypeError):
        enc(x.to(DEV), torch.ones(x.shape[0], device=DEV))
    with pytest.raises(ValueError):
        enc(x.to(DEV), i32(lengths[:-1]))


# ------------------------------------------------------------------ models
def state_of(g, prefix="p."):
    return {k[len(prefix):]: T(v) for k, v in g.items() if k.startswith(prefix)}


def batch_of(g, dev=DEV):
    names = ("user_id", "user_features", "user_history", "item_id", "item_features", "position", "labels")
    return [T(g["in." + n]).to(dev) for n in names]


def make_model(kind, g, corpus=None, topk=10):
    import two_tower_models_amd as A
    n_users, du, iu, n_items, di, ii, Tn, B, H = (int(v) for v in g["cfg"])
    mips = A.BaselineMIPSModule(corpus_size=64 if corpus is None else corpus.shape[0], embedding_dim=di)
    if corpus is not None:
        mips.corpus = corpus
    cls = {"hist": A.TwoTowerWithUserHistoryEncoder, "user": A.TwoTowerWithUserDebiasedWeights}[kind]
    m = cls(num_items=topk, user_id_hash_size=n_users, user_id_embedding_dim=du, user_features_size=iu,
            user_history_seqlen=H, item_id_hash_size=n_items, item_id_embedding_dim=di, item_features_size=ii,
            user_value_weights=[float(v) for v in g["uvw"]], mips_module=mips)
    m.load_state_dict(state_of(g), strict=True)
    return m.to(DEV)


def model_lengths(g):
    B, H = int(g["cfg"][7]), int(g["cfg"][8])
    return [(b * 7) % H + 1 for b in range(B)]


_model_cache = {}


def model_reference(g, name, debias=R.debias_identity):
    if name not in _model_cache:
        H, di = int(g["cfg"][8]), int(g["cfg"][4])
        _model_cache[name] = HR.loss_and_grads(state_of(g), batch_of(g, "cpu"), model_lengths(g), T(g["uvw"]), 4,
                                               R.positional_table(H, di), debias)
    return _model_cache[name]


@pytest.mark.parametrize("name", ["g4_hist_d128", "g4_hist_tiny"])
def test_history_model_with_lengths_matches_reference(golden, name):
    """Loss 1e-4 and every parameter gradient -- the item table's rows (item ids + valid history slots; padded slots add
    exactly zero) included -- against the float64 reference; the padded ids are other valid ids (what the fixture drew)."""
    g = golden(name)
    model = make_model("hist", g)
    loss_ref, grads_ref = model_reference(g, name)
    loss = model.train_forward(*batch_of(g), user_history_lengths=i32(model_lengths(g)))
    print(f"{name}: loss {loss.item():.7f} ref {float(loss_ref):.7f}")
    assert abs(loss.item() - float(loss_ref)) < 1e-4
    assert model._tt_history_lengths is None
    loss.backward()
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        want = grads_ref[n]
        ok, err = close(p.grad, want, max(1e-5 * float(want.abs().max()), 1e-7), 2e-4)
        print(f"{name}: {n} err {err:.3e} (max {float(want.abs().max()):.3e})")
        assert ok, (n, err)


@pytest.mark.parametrize("lazy", [False, True])
def test_history_model_with_lengths_dense_exact_adam_step(golden, lazy):
    """One DenseExactAdam step (default schedule; lazy=True) against torch.optim.Adam on a second copy of the model, both
    with lengths -- the comparison and tolerances of test_history_model_dense_exact_adam_runs_and_matches_torch_adam."""
    import two_tower_models_amd as A
    g = golden("g4_hist_d128")
    m1, m2 = make_model("hist", g), make_model("hist", g)
    o1 = A.DenseExactAdam(m1.parameters(), lr=1e-3, **(dict(lazy=True) if lazy else {}))
    o2 = torch.optim.Adam(m2.parameters(), lr=1e-3)
    ln = i32(model_lengths(g))
    for m, o in ((m1, o1), (m2, o2)):
        loss = m.train_forward(*batch_of(g), user_history_lengths=ln)
        o.zero_grad()
        loss.backward()
        o.step()
    if lazy:
        o1.flush()
    torch.cuda.synchronize()
    for (k, v1), (_, v2) in zip(m1.state_dict().items(), m2.state_dict().items()):
        noise_only = k in ("item_tower_arch.bias", "item_features_arch.2.bias")
        assert torch.allclose(v1, v2, atol=4.4e-3 if noise_only else 5e-6, rtol=1e-5), k


@pytest.mark.parametrize("name", ["g4_hist_d128", "g4_hist_tiny"])
def test_forward_with_lengths_returns_the_reference_topk(golden, name):
    """forward(..., user_history_lengths=) on the g5 exact-arithmetic corpus: the top-K of the float64 reference query.  A row
    is decided where the reference's top K + 1 scores are further apart than the query tolerance allows to move them
    (|du| <= 1e-5 per element -> |d score| <= 1e-5 ||c||_1, twice for a pair); decided rows must match exactly, and most are."""
    g = golden(name)
    di, K = int(g["cfg"][4]), 10
    corpus = T(fg.exact_mips_corpus(4096, di))
    model = make_model("hist", g, corpus=corpus, topk=K)
    b, lengths = batch_of(g), model_lengths(g)
    top = model(*b[:3], user_history_lengths=i32(lengths))
    assert model._tt_history_lengths is None
    params = {k: v.to(F64) for k, v in state_of(g).items()}
    bc = batch_of(g, "cpu")
    u = HR.user_embedding(params, bc[0], bc[1].to(F64), bc[2], lengths, 4, R.positional_table(int(g["cfg"][8]), di).to(F64))
    scores = u @ corpus.to(F64).t()
    order = torch.sort(scores, dim=1, descending=True, stable=True)
    gaps = (order.values[:, :K] - order.values[:, 1:K + 1]).min(dim=1).values
    decided = gaps > 2 * 1e-5 * float(corpus.abs().sum(dim=1).max())
    print(f"{name}: {int(decided.sum())} of {len(decided)} rows decided")
    assert int(decided.sum()) >= len(decided) // 2
    assert torch.equal(top.cpu()[decided], order.indices[:, :K][decided])


def test_debias_subclass_with_lengths_loss(golden):
    """TwoTowerWithUserDebiasedWeights inherits the keyword: loss against the reference (1e-4)."""
    g = golden("g8_debias_user")
    model = make_model("user", g)
    loss_ref, _ = model_reference(g, "g8_debias_user", R.debias_user)
    loss = model.train_forward(*batch_of(g), user_history_lengths=i32(model_lengths(g)))
    print(f"loss {loss.item():.6f} ref {float(loss_ref):.6f}")
    assert abs(loss.item() - float(loss_ref)) < 1e-4
