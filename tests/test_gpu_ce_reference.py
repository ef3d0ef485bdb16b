"""The in-batch softmax cross entropy kernels (csrc/inbatch_ce.hip, ce_wide.hip, mfma_stream.hpp) against the float64
reference of tests/ce_ref.py, on MI355X (`pytest -m gpu`): every entry point through the C ABI, at every width class,
staging form, vector-load form, split plan, slab reduce and input class of ce_ref.CASES (test_ce_reference_cpu.py asserts
that the list reaches every cell), with operands laid out inside larger buffers whose slack is NaN (inputs) or the
sentinel 7.0 (outputs).  Every forward runs twice into NaN-filled outputs with the workspace filled with 0xA5 in between:
nothing may carry over, and the two runs must agree bit for bit.  Tolerances: ce_ref.tol (the project's figures for flat
inputs, 4 x the float32 CPU yardstick otherwise); profiles/ce_reference_tolerance.txt records what the GPU showed.

row_lse: for D <= 128 the vector is in the log2 domain (include/tt_hotpath.h) and row_lse ln 2 is compared with the float64
lse; for D > 128 the wide path writes natural-log units that only its own backward reads, and it is checked through ce
and the gradients."""
import pytest
import torch

import ce_ref as C
from test_gpu_logq import DEV, abi_bwd, abi_bwd_kept, abi_fwd, abi_workspace

pytestmark = pytest.mark.gpu
NAN = float("nan")
FORM = {"fwd": "plain", "fwd_du": "du", "keep": "keep", "loss": "loss", "bwd": "plain", "bwd_nodu": "plain",
        "bias_plain": "plain", "bias_du": "du", "bias_keep": "keep", "bias_loss": "loss"}
TAIL = 64  # floats behind the padded logits buffer that no call may touch


@pytest.fixture(scope="module")
def T():
    from two_tower_models_amd import _native as N
    from two_tower_models_amd import ops
    N.load()
    return ops, N


def bits(t):
    return t.contiguous().view(torch.int32)


def output(shape, lay):
    """A NaN-filled output view of layout `lay` inside a buffer whose slack holds the sentinel."""
    buf, view = C.place(shape, lay, C.SENTINEL, DEV)
    view.fill_(NAN)
    return buf, view


def forward(T, c, Uv, Iv, bd, lab, uvw):
    """The forward of case c, twice; -> (outputs of the second run, the logits buffer or None)."""
    form = FORM[c.entry]
    api = "bias" if c.entry in C.BIAS_ENTRIES else "plain"
    ws = abi_workspace(T, c.M, c.N, c.D)
    Mp, Np = -(-c.M // 128) * 128, -(-c.N // 128) * 128
    runs = []
    for _ in range(2):
        dubuf, duv = output((c.M, c.D), c.ldun) if form != "plain" else (None, None)
        zbuf = torch.full((Mp * Np + TAIL,), C.SENTINEL, device=DEV) if form == "keep" else None
        out = abi_fwd(T, Uv, Iv, c.off, bd, form, labels=lab, uvw=uvw, entry=api, du_unit=duv, logits=zbuf, fill=NAN)
        torch.cuda.synchronize()
        if duv is not None:
            assert C.slack_intact(dubuf, duv), "du_unit: a write outside the view"
        if zbuf is not None:
            assert bool((zbuf[Mp * Np:] == C.SENTINEL).all()), "logits: a write behind the padded buffer"
            # the forward stores whole 64-column tiles: with an odd number of them the last 64 columns of the padded
            # buffer stay unwritten (a tile loop one tile too far, or a wrong row stride, would land there)
            unwritten = zbuf[:Mp * Np].view(Mp, Np)[:, -(-c.N // 64) * 64:]
            assert bool((unwritten == C.SENTINEL).all()), "logits: a write into the unwritten columns of the padded buffer"
        runs.append(out)
        ws.fill_(0xA5)
    for k in runs[0]:
        assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), f"{k}: the second run differs from the first"
    return runs[1]


def run_case(T, c):
    """{quantity: worst err / bound} of every quantity case c's entry produces.  A HIP error ends the session: after a
    fault nothing more is started on the device."""
    try:
        return _run_case(T, c)
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"device error at {C.case_id(c)}: {e}", returncode=3)
        raise


def _run_case(T, c):
    ref = C.case_reference(c)
    U, I, b, coef, labels = C.inputs(C.math_key(c))
    _, Uv = C.place(U, c.lu, NAN, DEV)
    _, Iv = C.place(I, c.li, NAN, DEV)
    bd, cd = (None if b is None else b.to(DEV)), coef.to(DEV)
    out = forward(T, c, Uv, Iv, bd, labels.to(DEV), C.UVW.to(DEV))
    got = {"ce": out["ce"]}
    if c.D <= 128:
        got["lse"] = out["lse"].double() * C.LN2
    if "du_unit" in out:
        got["du_unit"] = out["du_unit"]
    if "logits" in out:
        Mp, Np = -(-c.M // 128) * 128, -(-c.N // 128) * 128
        got["logits"] = out["logits"][:Mp * Np].view(Mp, Np)[:c.M, :c.N]
    back = C.BACKWARD[c.entry]
    if back is not None:
        kind, with_du = back
        dibuf, div = output((c.N, c.D), c.ldi)
        if kind == "kept":
            abi_bwd_kept(T, Uv, c.N, c.off, out["lse"], cd, out["logits"], dI=div)
        else:
            dubuf, duv = output((c.M, c.D), c.ldu) if with_du else (None, None)
            abi_bwd(T, Uv, Iv, c.off, bd, out["lse"], cd, with_du, entry="bias" if c.entry in C.BIAS_ENTRIES else "plain",
                    dU=duv, dI=div)
            if with_du:
                assert C.slack_intact(dubuf, duv), "dU: a write outside the view"
                got["dU"] = duv
        torch.cuda.synchronize()
        assert C.slack_intact(dibuf, div), "dI: a write outside the view"
        got["dI"] = div
    assert set(got) == C.compared(c)  # (what the mutants of test_ce_reference_cpu.py are counted against)
    r = C.ratios(got, ref, c.cls)
    if "loss" in out:
        lt = C.loss_tolerances(ref, c.cls)
        r["w"] = C.ratio(out["w"], ref["w"], lt["w"])
        r["coef_w"] = C.ratio(out["coef"], ref["coef_w"], lt["coef_w"])
        r["loss"] = C.ratio(out["loss"], ref["loss"], lt["loss"])
    return r


LIGHT = [c for c in C.CASES if not C.heavy(C.math_key(c))]
HEAVY = [c for c in C.CASES if C.heavy(C.math_key(c))]


@pytest.mark.parametrize("c", LIGHT, ids=C.case_id)
def test_ce_matches_float64(T, c):
    r = run_case(T, c)
    p = C.case_plan(c)
    print(f"CE_REF {c.entry} dp8={p['dp8']} {C.staging_of(c)} di={p['stage_di']} {c.cls} {C.case_id(c)} "
          + " ".join(f"{q}={v:.3g}" for q, v in r.items()))
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("c", HEAVY, ids=C.case_id)
def test_wide_path_with_two_row_chunks_matches_float64(T, c):
    """M = 130, N = 524 352, D = 132: wide_chunk_rows = 128, a second chunk of two rows (r0 = 128 in U + r0 ldu,
    dU + r0 lddu, wide_sub_diag_kernel's row0, the accumulate flag of the TN product).  The float64 reference of its
    68 M logits is computed once per (shape, term) and shared."""
    assert C.case_plan(c)["chunks"] == [128, 2] and C.layout(c.lu, c.D)[0] != c.D
    r = run_case(T, c)
    print(f"CE_REF {c.entry} dp8=None gemm di=gemm {c.cls} {C.case_id(c)} " + " ".join(f"{q}={v:.3g}" for q, v in r.items()))
    assert max(r.values()) <= 1.0, r


# ------------------------------------------------------------------ the op on row-strided views
@pytest.mark.parametrize("bias", ["none", "zipf"])
@pytest.mark.parametrize("keep", [None, True, False])
@pytest.mark.parametrize("first_col", [4, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("D", [128, 50])
def test_op_on_column_slices_of_wider_tensors(T, D, first_col, keep, bias):
    """ops.InBatchSoftmaxCE on U = WU[:, a:a + D], I = WI[:, a:a + D] (row stride D + 8; a = 4: 16-byte aligned rows,
    a = 1: not), the other columns NaN: ce and both gradients against float64, and the kept-logits pair exactly where
    kept_logits_supported says so."""
    ops, N = T
    M, Nn, off = 130, 700, 200
    key = (M, Nn, D, off, "flat", bias)
    U, I, b, coef, _ = C.inputs(key)
    ref = C.key_reference(key)
    WU, WI = torch.full((M, D + 8), NAN, device=DEV), torch.full((Nn, D + 8), NAN, device=DEV)
    WU[:, first_col:first_col + D] = U.to(DEV)
    WI[:, first_col:first_col + D] = I.to(DEV)
    Uv = WU[:, first_col:first_col + D].detach().requires_grad_(True)
    Iv = WI[:, first_col:first_col + D].detach().requires_grad_(True)
    assert Uv.stride(0) == D + 8 and Uv.data_ptr() % 16 == (0 if first_col == 4 else 4)
    supported = ops.kept_logits_supported(Uv, Iv)
    assert supported == (D == 128 and first_col == 4)
    N.trace = []
    try:
        ce = ops.InBatchSoftmaxCE.apply(Uv, Iv, off, keep, None if b is None else b.to(DEV))
        (ce * coef.to(DEV)).sum().backward()
        calls = list(N.trace)
    finally:
        N.trace = None
    want_kept = supported and (keep is None or keep)  # N >= 4 M: kept by default
    assert ("tt_inbatch_ce_bwd_kept" in calls) == want_kept, calls
    assert ("tt_inbatch_ce_fwd_du_keep" in calls) == (want_kept and b is None), calls
    r = C.ratios({"ce": ce.detach(), "dU": Uv.grad, "dI": Iv.grad}, ref, "flat")
    print(f"CE_REF op D={D} col={first_col} keep={keep} bias={bias} " + " ".join(f"{q}={v:.3g}" for q, v in r.items()))
    assert max(r.values()) <= 1.0, r
    assert bool(torch.isnan(WU[:, :first_col]).all()) and bool(torch.isnan(WU[:, first_col + D:]).all())
