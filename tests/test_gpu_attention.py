"""The attention kernels on MI355X (`pytest -m gpu`) against the float64 reference of tests/attention_ref.py: every
implementation behind tt_attn_fwd / tt_attn_bwd (the persistent one-sample-per-workgroup backward, the matrix-core pair,
the generic VALU pair) at the edges of its shape class and of the dispatcher, on flat, peaked (near one-hot rows) and
shifted (logits near +-200) inputs; then the fixed-length encoder and the history model at the batch sizes where the
kernels change.

Every C-ABI case asserts WHICH kernel ran, through the library's launch counters (tt_profile_*): attn_fwd_mfma_kernel,
attn_bwd_wg_kernel, attn_bwd_mfma_kernel; the VALU pair has no counter, so "all three zero" is the VALU pair.

Tolerances: attention_ref.tol (flat ctx / d_qkv: the project's figures; lse and the peaked / shifted classes: 4 x the
float32 CPU yardstick); encoder and model: the figures of tests/test_gpu_history_lengths.py and
test_history_model_matches_reference.  profiles/attention_reference_tolerance.txt records what a run printed."""
import ctypes as C

import pytest
import torch

import attention_ref as AR
import fixture_gen as fg
import history_lengths_ref as HR
from oracle import cpu_ref as R
from test_gpu_history_lengths import check_encoder, close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
FWD_MFMA, BWD_WG, BWD_MFMA = "attn_fwd_mfma_kernel", "attn_bwd_wg_kernel", "attn_bwd_mfma_kernel"
WG = {FWD_MFMA: 1, BWD_WG: 1, BWD_MFMA: 0}
MFMA = {FWD_MFMA: 1, BWD_WG: 0, BWD_MFMA: 1}
VALU = {FWD_MFMA: 0, BWD_WG: 0, BWD_MFMA: 0}


def lib_and_native():
    from two_tower_models_amd import _native as N
    return N.load(), N


class Launches:
    """with Launches(...) as n: ...  -> n[kernel] = launches the library counted inside the block."""

    def __init__(self, kernels=(FWD_MFMA, BWD_WG, BWD_MFMA)):
        self.kernels, self.n = kernels, {}

    def __enter__(self):
        lib, _ = lib_and_native()
        lib.tt_profile_filter(",".join(self.kernels).encode())
        lib.tt_profile_enable(1)
        return self.n

    def __exit__(self, *exc):
        lib, N = lib_and_native()
        torch.cuda.synchronize()
        try:
            for k in self.kernels:
                ms, cnt = C.c_double(0.0), C.c_int64(0)
                N.check(lib.tt_profile_read(k.encode(), C.byref(ms), C.byref(cnt)), "tt_profile_read")
                self.n[k] = cnt.value
        finally:
            lib.tt_profile_enable(0)
            lib.tt_profile_filter(None)
        return False


class Run:
    """One forward + backward at the C ABI.  Every operand is a view into a sentinel-filled buffer with 8 floats of margin on
    either side, 16-byte aligned -- or, for the names in `misalign`, one float further.  bwd_len: the backward through
    tt_attn_bwd_len with every length = H."""

    def __init__(self, case, misalign=(), bwd_len=False, data=None):
        lib, N = lib_and_native()
        B, H, D, heads, _ = case
        qkv, d_ctx = AR.case_inputs(case) if data is None else data
        self.bufs = {}

        def place(name, n, src=None):
            buf = torch.full((n + 16,), AR.SENTINEL, device=DEV)
            o = 8 + (1 if name in misalign else 0)
            assert (buf.data_ptr() + 4 * o) % 16 == (4 if name in misalign else 0)
            view = buf[o:o + n]
            if src is not None:
                view.copy_(src.reshape(-1))
            self.bufs[name] = (buf, o, n)
            return view

        q, g = place("qkv", qkv.numel(), qkv), place("d_ctx", d_ctx.numel(), d_ctx)
        ctx, lse, dq = place("ctx", B * H * D), place("lse", B * heads * H), place("d_qkv", B * H * 3 * D)
        with Launches() as self.launches:
            self.rc_fwd = lib.tt_attn_fwd(q.data_ptr(), B, H, D, heads, ctx.data_ptr(), lse.data_ptr(), N.stream())
            self.err_fwd = lib.tt_last_error_string() if self.rc_fwd else b""
            if bwd_len:
                ln = torch.full((B,), H, dtype=torch.int32, device=DEV)
                self.rc_bwd = lib.tt_attn_bwd_len(q.data_ptr(), ctx.data_ptr(), lse.data_ptr(), g.data_ptr(), B, H, D, heads,
                                                  ln.data_ptr(), dq.data_ptr(), N.stream())
            else:
                self.rc_bwd = lib.tt_attn_bwd(q.data_ptr(), ctx.data_ptr(), lse.data_ptr(), g.data_ptr(), B, H, D, heads,
                                              dq.data_ptr(), N.stream())
            self.err_bwd = lib.tt_last_error_string() if self.rc_bwd else b""
        self.got = {"ctx": ctx.cpu().reshape(B * H, D), "lse": lse.cpu().reshape(B, heads, H),
                    "dqkv": dq.cpu().reshape(B * H, 3 * D)}

    def margins_untouched(self):
        """The 8 (or 9 / 7) floats before and after every view still hold the sentinel."""
        return all(bool((buf[:o] == AR.SENTINEL).all()) and bool((buf[o + n:] == AR.SENTINEL).all())
                   for buf, o, n in self.bufs.values())

    def untouched(self, name):
        return bool((self.got[name] == AR.SENTINEL).all())


def check(group, case, run, expect, names=("ctx", "lse", "dqkv")):
    """Counters first, then every element of every output against float64; prints err / bound per quantity."""
    cls = case[4]
    assert run.rc_fwd == 0 and (run.rc_bwd == 0 or "dqkv" not in names), (run.rc_fwd, run.err_fwd, run.rc_bwd, run.err_bwd)
    assert run.launches == expect, (AR.case_id(case), run.launches, expect)
    ref = AR.case_reference(case)
    r = AR.ratios({n: run.got[n] for n in names}, ref, AR.family_of(case), cls)
    print(f"attn-ref {group} {AR.case_id(case)} err/bound " + " ".join(f"{n} {r[n]:.3f}" for n in names)
          + " launches " + "/".join(str(run.launches[k]) for k in (FWD_MFMA, BWD_WG, BWD_MFMA)))
    assert all(v <= 1.0 for v in r.values()), r
    assert run.margins_untouched()
    return r


# ------------------------------------------------------------------ 1, 2: the one-sample-per-workgroup backward
@pytest.mark.parametrize("case", AR.WG_EDGES, ids=AR.case_id)
def test_workgroup_backward_h_edges(case):
    """attn_bwd_wg_kernel at its own H edges (D = 128, 4 heads, B = 2): H = 48 leaves the loaders' remainder quad empty,
    49 half full, 50 full; 32 / 33 the key-tile edge; 8 exactly one staging round (32 H = 256 float4); 1 and 2 nearly
    nothing but padding rows."""
    check("wg-edges", case, Run(case), WG)


@pytest.mark.parametrize("case", AR.WG_TRIPS, ids=AR.case_id)
def test_workgroup_backward_persistent_loop_trips(case):
    """grid = 256 workgroups, B = 257 (workgroup 0 takes two samples, every other one and re-fetches its own), 512 (two
    each), 513 and 769 (three and four trips): the prefetched sample is consumed.  Every row of d_qkv against float64 (a
    stale or half-overwritten staged sample gives a plausible, wrong gradient), and no row keeps the sentinel."""
    run = Run(case)
    check("wg-trips", case, run, WG)
    kept = (run.got["dqkv"] == AR.SENTINEL).all(dim=1)
    assert int(kept.sum()) == 0, torch.nonzero(kept).flatten()[:8]


# ------------------------------------------------------------------ 3: alignment fallbacks
@pytest.mark.parametrize("name,expect", [(None, WG), ("d_qkv", {FWD_MFMA: 1, BWD_WG: 0, BWD_MFMA: 0}), ("qkv", VALU),
                                         ("d_ctx", {FWD_MFMA: 1, BWD_WG: 0, BWD_MFMA: 0}),
                                         ("ctx", {FWD_MFMA: 0, BWD_WG: 0, BWD_MFMA: 1})])
def test_alignment_fallbacks(name, expect):
    """(B, H, D, heads) = (2, 50, 128, 4) with one operand 4 bytes off 16-byte alignment: a misaligned d_qkv or d_ctx sends
    the backward from the workgroup kernel to the VALU kernel (the matrix-core backward needs both aligned), a misaligned
    qkv both directions to the VALU pair, a misaligned ctx the forward to the VALU kernel and the backward to the
    matrix-core kernel (which does not read ctx).  Same tolerance; the floats around every view keep their sentinel."""
    run = Run(AR.ALIGN, misalign=() if name is None else (name,))
    check(f"align-{name}", AR.ALIGN, run, expect)


# ------------------------------------------------------------------ 4: matrix-core pair
@pytest.mark.parametrize("case", AR.MFMA, ids=AR.case_id)
def test_mfma_pair(case):
    """dh in {64, 32, 16} with 3, 5 and 9 (sample, head) pairs -- a tail block of one wave for the 4-wave kernels and for the
    dh = 64 backward's 2-wave blocks -- at H = 1, the 32-row tile edges and the 64-row limit; 32 pairs of 16 heads."""
    check("mfma", case, Run(case), MFMA)


@pytest.mark.parametrize("case", AR.MFMA_EDGE_VALU, ids=AR.case_id)
def test_just_outside_the_mfma_class_runs_the_valu_pair(case):
    """H = 65 at dh = 32, and (2, 64, 128, 16): sixteen heads of dh = 8 -- not a matrix-core head width."""
    check("mfma-edge", case, Run(case), VALU)


# ------------------------------------------------------------------ 5: VALU pair
@pytest.mark.parametrize("case", AR.VALU_LONG, ids=AR.case_id)
def test_valu_pair_long_histories(case):
    """H >= 256: the block is capped at 256 threads and every thread loops over rows (255 / 256 / 257: the cap's edge);
    H = 300 at dh = 16: the backward's 79 200 B of LDS are the opt-in path above 64 KiB."""
    check("valu-long", case, Run(case), VALU)


@pytest.mark.parametrize("case", AR.VALU_WIDTH, ids=AR.case_id)
def test_valu_pair_head_widths(case):
    """H = 7; head widths 1, 4 | 5, 16 | 17 | 33 | 65, 128: the last of one padded-width class and the first of the next.
    dh = 16 at H = 7 is a matrix-core shape: its qkv sits 4 bytes off alignment, which is what hands it to the VALU pair."""
    dh = case[2] // case[3]
    check("valu-width", case, Run(case, misalign=("qkv",) if dh == 16 else ()), VALU)


def test_refusals_leave_the_outputs_alone():
    """dh = 129: TT_E_UNSUPPORTED both ways.  H = 700 at dh = 16: the forward's 89 600 B of LDS fit and it runs (checked
    against float64); the backward's 184 800 B exceed 160 KiB: TT_E_UNSUPPORTED.  A refused call writes nothing and
    tt_last_error_string names the reason."""
    _, N = lib_and_native()
    case = (2, 7, 129, 1, "flat")
    run = Run(case, data=AR.inputs(case))
    assert run.rc_fwd == N.TT_E_UNSUPPORTED and run.rc_bwd == N.TT_E_UNSUPPORTED
    assert b"head dim 129 > 128" in run.err_fwd and b"head dim 129 > 128" in run.err_bwd
    assert run.untouched("ctx") and run.untouched("lse") and run.untouched("dqkv") and run.margins_untouched()
    assert run.launches == VALU
    run = Run(AR.LDS_REFUSED)
    assert run.rc_bwd == N.TT_E_UNSUPPORTED and b"too large for LDS" in run.err_bwd
    check("valu-lds", AR.LDS_REFUSED, run, VALU, names=("ctx", "lse"))
    assert run.untouched("dqkv")


# ------------------------------------------------------------------ 6: same inputs, three kernels
def test_three_backward_kernels_on_the_same_inputs():
    """(9, 50, 128, 4): the workgroup backward (lengths = NULL), the matrix-core backward (tt_attn_bwd_len, every length = H),
    the VALU backward (qkv 4 bytes off alignment): each within tolerance of float64; their mutual differences are printed."""
    runs = {"wg": Run(AR.THREE), "mfma": Run(AR.THREE, bwd_len=True), "valu": Run(AR.THREE, misalign=("qkv",))}
    for name, expect in (("wg", WG), ("mfma", MFMA), ("valu", VALU)):
        check(f"three-{name}", AR.THREE, runs[name], expect)
    scale = float(AR.case_reference(AR.THREE)["dqkv"].abs().max())
    for a, b in (("wg", "mfma"), ("wg", "valu"), ("mfma", "valu")):
        d = float((runs[a].got["dqkv"].double() - runs[b].got["dqkv"].double()).abs().max())
        print(f"attn-ref three d_qkv {a} - {b}: max |diff| {d:.3e} = {d / scale:.3e} max|d_qkv|")


# ------------------------------------------------------------------ 7: the encoder without lengths where the kernels change
def rnd(shape, seed, scale=1.0):
    return AR.T(fg.gaussianish(shape, seed)) * scale


_enc_cache = {}


def encoder_case(B, L):
    """(CPU encoder with randomised biases, table [400, D], ids [B, H], cot, float64 reference of forward(table[ids])):
    one reference per (B, L), shared by the embedded and the id form -- the table's gradient is the scatter-add of dx."""
    import two_tower_models_amd as A
    H, D, heads, rows = 50, 128, 4, 400
    if (B, L) not in _enc_cache:
        torch.manual_seed(3)
        enc = A.UserHistoryEncoder(D, H, heads, L, True)
        with torch.no_grad():
            for n, p in enc.named_parameters():
                if n.endswith("bias"):
                    p.copy_(rnd(tuple(p.shape), 61 + len(n), 0.2))
        table, ids, cot = rnd((rows, D), 81), AR.T(fg.uniform_ids((B, H), rows, 82)), rnd((B, 2, D), 83)
        leaves = {k: v.detach().to(F64).requires_grad_(True) for k, v in enc.state_dict().items()}
        x64 = table[ids].to(F64).requires_grad_(True)
        y = R.history_encoder_forward(x64, R.encoder_layers_from_params(leaves, prefix=""), heads, enc.positional_embeddings.to(F64))
        grads = torch.autograd.grad((y * cot.to(F64)).sum(), [x64] + list(leaves.values()))
        gt = torch.zeros(rows, D, dtype=F64).index_add_(0, ids.reshape(-1), grads[0].reshape(-1, D))
        _enc_cache[(B, L)] = (enc.state_dict(), table, ids, cot, (y.detach(), grads[0], gt, dict(zip(leaves, grads[1:]))))
    sd, table, ids, cot, ref = _enc_cache[(B, L)]
    enc = A.UserHistoryEncoder(D, H, heads, L, True)
    enc.load_state_dict(sd)
    return enc.to(DEV), table, ids, cot, ref


ENC_CASES = [(257, 3, False), (328, 3, False), (600, 3, False), (328, 1, False), (328, 2, False), (328, 3, True)]


@pytest.mark.parametrize("B,L,generic", ENC_CASES)
def test_encoder_without_lengths_at_the_sizes_that_change_kernels(B, L, generic, monkeypatch):
    """UserHistoryEncoder(128, 50, 4, L, True) without lengths, B > 256 (the workgroup backward loops) and, from B = 328,
    B H >= 16384 (weights-stationary and streaming GEMMs, the fused pool-backward epilogue): output, dx / the table's
    gradient (400 rows: ids repeat) and all 4 L parameter gradients through forward(x) and through encode_ids(table, ids),
    against R.history_encoder_forward in float64 + autograd; once with every layer in full (ops._ENC_GENERIC).  The full
    layers' attention backward is the workgroup kernel: L - 1 launches beside the collapsed last layer, L in full."""
    from two_tower_models_amd import ops
    monkeypatch.setattr(ops, "_ENC_GENERIC", generic)
    enc, table, ids, cot, (y_ref, gx_ref, gt_ref, gp_ref) = encoder_case(B, L)
    cotd = cot.to(DEV)
    other = ("gemm_ws16_kernel", "gemm_ws_kernel", "tn_stream_kernel")
    for form in ("embedded", "ids"):
        enc.zero_grad(set_to_none=True)
        with Launches((BWD_WG, BWD_MFMA) + other) as n:
            if form == "ids":
                src = torch.nn.Parameter(table.to(DEV))
                y = enc.encode_ids(src, ids.to(DEV))
            else:
                src = table[ids].to(DEV).requires_grad_(True)
                y = enc(src)
            (y * cotd).sum().backward()
        print(f"attn-ref encoder B{B}-L{L}-generic{generic}-{form} launches " + " ".join(f"{k} {v}" for k, v in n.items()))
        assert n[BWD_WG] == (L if generic else L - 1) and n[BWD_MFMA] == 0, n
        check_encoder(enc, y, src, (y_ref, gt_ref if form == "ids" else gx_ref, gp_ref), f"B{B}-L{L}-generic{generic}-{form}")


# ------------------------------------------------------------------ 8: the history model's gradient VALUES at B > 256
def test_history_model_gradients_beyond_one_trip():
    """TwoTowerWithUserHistoryEncoder, D = 128, H = 50, B = 300 (the workgroup backward's second trip), 256 users and items:
    loss 1e-4 and every parameter gradient at max(1e-5 max|.|, 1e-7) / 2e-4 -- the figures of
    test_history_model_matches_reference -- against the float64 reference with full lengths in its vectorised masked form
    (HR.user_embedding(masked=True)).  A one-Adam-step comparison of parameters sees the gradient's sign only."""
    import two_tower_models_amd as A
    B, H, D, F, NU, NI, heads = 300, 50, 128, 8, 256, 256, 4
    torch.manual_seed(11)
    mips = A.BaselineMIPSModule(corpus_size=64, embedding_dim=D)
    model = A.TwoTowerWithUserHistoryEncoder(num_items=10, user_id_hash_size=NU, user_id_embedding_dim=D, user_features_size=F,
                                             user_history_seqlen=H, item_id_hash_size=NI, item_id_embedding_dim=D,
                                             item_features_size=F, user_value_weights=[1.0], mips_module=mips)
    with torch.no_grad():  # keep the logits O(1): D-wide towers with default init saturate the softmax
        for n, p in model.named_parameters():
            if n.endswith("tower_arch.weight"):
                p.mul_(0.2)
            if "embedding_arch" in n:
                p.mul_(0.3)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    batch = [AR.T(fg.uniform_ids((B,), NU, 91)), rnd((B, F), 92), AR.T(fg.uniform_ids((B, H), NI, 93)),
             AR.T(fg.uniform_ids((B,), NI, 94)), rnd((B, F), 95), AR.T(fg.uniform_ids((B,), 10, 96)),
             (AR.T(fg.uniform_ids((B, 1), 2, 97))).float()]
    leaves = {k: HR.f64(v).requires_grad_(True) for k, v in params.items()}
    u = HR.user_embedding(leaves, batch[0], HR.f64(batch[1]), batch[2], [H] * B, heads, HR.f64(R.positional_table(H, D)),
                          masked=True)
    it = R.item_embeddings(leaves, batch[3], HR.f64(batch[4]))
    loss_ref = R.training_loss(u, it, batch[5], HR.f64(batch[6]), torch.tensor([1.0], dtype=F64), leaves, R.debias_identity)
    grads = torch.autograd.grad(loss_ref, list(leaves.values()), allow_unused=True)
    loss_ref = loss_ref.detach()
    grads_ref = {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(leaves, grads)}
    model = model.to(DEV)
    with Launches() as n:
        loss = model.train_forward(*[t.to(DEV) for t in batch])
        loss.backward()
    print(f"attn-ref model loss {loss.item():.7f} ref {float(loss_ref):.7f} launches {n}")
    assert n[BWD_WG] >= 1 and n[BWD_MFMA] == 0, n
    assert abs(loss.item() - float(loss_ref)) < 1e-4
    for name, p in model.named_parameters():
        want = grads_ref[name]
        ok, err = close(p.grad, want, max(1e-5 * float(want.abs().max()), 1e-7), 2e-4)
        print(f"attn-ref model {name} err {err:.3e} (max {float(want.abs().max()):.3e})")
        assert ok, (name, err)
