"""MIPS top-K on MI355X (`pytest -m gpu`) against the float64 reference of tests/mips_ref.py, on UNROUNDED inputs: every
dispatch path behind tt_mips_topk -- the shared-query x4 / x2 forms, the throughput form with one, two and three workgroups,
the three DMA widths, the generic pass 1 with the dense and with the sparse pass 2, the D > 128 form and its second slab,
every K regime, the corpus edges, two query batches with several selected-group slices, and every form of TT_F16X2 --
then the helper entry points tt_f32_to_bf16, tt_gather_rows_bf16, tt_mips_split_rows and tt_mips_unscale.

tt_mips_topk is called through the C ABI with idx_out pre-filled with -1 and score_out with NaN (ops.mips_topk allocates
with torch.empty, which would hide a slot that was never written).  Every case asserts WHICH pass 2 ran through the library's
launch counters (tt_profile_*): mips_sparse_kernel once per batch of 1024 queries, or not at all.

Bounds: mips_ref (E = 4 YARD 2^-24 A + 2^-24 |s64| per element; TT_F16X2 the fp32 E, plus the split's norm-wise term on the
range class).  profiles/mips_reference_tolerance.txt records what a run printed."""
import ctypes as C

import numpy as np
import pytest
import torch

import fixture_gen as fg
import mips_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPARSE = "mips_sparse_kernel"


def lib_and_native():
    from two_tower_models_amd import _native as N
    return N.load(), N


class Launches:
    """with Launches() as n: ...  -> n[SPARSE] = mips_sparse_kernel launches the library counted inside the block."""

    def __init__(self):
        self.n = {}

    def __enter__(self):
        lib, _ = lib_and_native()
        lib.tt_profile_filter(SPARSE.encode())
        lib.tt_profile_enable(1)
        return self.n

    def __exit__(self, *exc):
        lib, N = lib_and_native()
        torch.cuda.synchronize()
        try:
            ms, cnt = C.c_double(0.0), C.c_int64(0)
            N.check(lib.tt_profile_read(SPARSE.encode(), C.byref(ms), C.byref(cnt)), "tt_profile_read")
            self.n[SPARSE] = cnt.value
        finally:
            lib.tt_profile_enable(0)
            lib.tt_profile_filter(None)
        return False


def search(case, d):
    """One tt_mips_topk call at the C ABI -> (idx [B, K] int64, scores [B, K]) on the CPU and the sparse-kernel launches."""
    from two_tower_models_amd import ops
    lib, N = lib_and_native()
    B, Cn, D, K = case.B, case.C, case.D, case.K
    scales = None
    if case.dtype == "f16x2":
        (q, qs), (c, cs) = ops.mips_split_rows(d["q_raw"].to(DEV)), ops.mips_split_rows(d["c_raw"].to(DEV))
        dt, scales = N.TT_F16X2, (qs, cs)
    elif case.dtype == "bf16":
        q, c, dt = d["q"].to(DEV, torch.bfloat16).contiguous(), d["c"].to(DEV, torch.bfloat16).contiguous(), N.TT_BF16
    else:
        q, c, dt = d["q"].to(DEV).contiguous(), d["c"].to(DEV).contiguous(), N.TT_F32
    idx = torch.full((B, K), -1, dtype=torch.int64, device=DEV)
    sc = torch.full((B, K), float("nan"), dtype=torch.float32, device=DEV)
    wsn = lib.tt_mips_workspace_bytes(B, Cn, D, K, dt)
    ws = torch.empty(wsn, dtype=torch.uint8, device=DEV)
    with Launches() as n:
        N.check(lib.tt_mips_topk(q.data_ptr(), c.data_ptr(), dt, B, Cn, D, K, idx.data_ptr(), sc.data_ptr(), ws.data_ptr(), wsn,
                                 N.stream()), "tt_mips_topk")
    if scales is not None:
        N.check(lib.tt_mips_unscale(sc.data_ptr(), B * K, scales[0].data_ptr(), scales[1].data_ptr(), N.stream()), "tt_mips_unscale")
    return idx.cpu(), sc.cpu(), n[SPARSE]


def check(case):
    d = MR.case_data(case)
    idx, sc, launches = search(case, d)
    rep = MR.check_topk(idx, sc, d["q"], d["c"], case.K, d["E"], s64=d["s64"])
    print(f"mips-ref {MR.case_id(case)} err/E {rep.worst:.3f} undecided returned {rep.undecided} sparse launches {launches} {rep.fired()}")
    assert launches == MR.sparse_launches(case), (launches, MR.sparse_launches(case))
    assert rep.ok, rep
    return idx, sc, d


def ids(cases):
    return [MR.case_id(c) for c in cases]


@pytest.mark.parametrize("case", MR.FORMS, ids=ids(MR.FORMS))
def test_query_batch_forms(case):
    """C = 5197 (82 groups of 64, 42 of 128), K = 40, D = 128: B = 1, 32 the shared-query x4 form; 33, 64 x2; 65, 128 the
    throughput form with one workgroup (128-row groups); 129, 256 two; 257, 300 three (bf16: 2 and 4 query fragments per
    wave).  Flat, negative (empty-group coding, the runner-up bound for negative scores) and clustered data."""
    check(case)


@pytest.mark.parametrize("case", MR.WIDTHS, ids=ids(MR.WIDTHS))
def test_widths(case):
    """fp32 D = 32 / 64 / 128 the DMA forms; 48 and 16 D != dp: generic pass 1 and dense pass 2; 50 rows that are no 16-byte
    multiples.  bf16 D = 32: generic pass 1 feeding the sparse pass 2; 64 / 128 DMA forms; 40 generic."""
    check(case)


@pytest.mark.parametrize("case", MR.WIDE, ids=ids(MR.WIDE))
def test_wide_form(case):
    """D = 130 and 256 (library GEMM slabs + group epilogues), and C = 65536 + 300: the second slab."""
    check(case)


@pytest.mark.parametrize("case", MR.KS, ids=ids(MR.KS))
def test_k_regimes(case):
    """K = 1; 41 / 42 either side of the 128-row-group condition; 81 one group more than K; 82 = n_groups and K = C: every
    item a candidate, dense pass 2, the sort past SORT_LDS."""
    check(case)


@pytest.mark.parametrize("case", MR.EDGES, ids=ids(MR.EDGES))
def test_corpus_edges(case):
    """Rows 0, 63, 64, 127, 128, C - 1 and the one-row last group carry tripled rows: each is returned wherever float64
    says it certainly wins, and it wins for at least one query (test_mips_reference_cpu.py)."""
    idx, _, d = check(case)
    cin, _ = MR.membership(d["s64"], d["E"], case.K)
    for r in MR.plant_rows(case.C):
        assert bool(((idx == r).any(dim=1) | ~cin[:, r]).all()) and bool((idx == r).any()), r


@pytest.mark.parametrize("case", MR.BIG, ids=ids(MR.BIG))
def test_two_query_batches_and_selected_group_slices(case):
    """C = 20 077 (314 groups), K = 300 (> 256: several selected-group slices), B = 1089 = one batch of 1024 queries
    (2 chunks per split) and one of 65 that reuses the workspace."""
    check(case)


@pytest.mark.parametrize("case", MR.F16X2 + MR.TINY_F32, ids=ids(MR.F16X2 + MR.TINY_F32))
def test_split_fp16_forms(case):
    """TT_F16X2 through ops.mips_split_rows, tt_mips_topk and tt_mips_unscale: x4, x2, one and two workgroups, two query
    fragments per wave; held to the fp32 path's E (range: plus the split's norm-wise term).  The tiny class (operands near
    2^-52, scale_q scale_c = 2^130) is the one that needs tt_mips_unscale to divide without forming the product; the fp32
    path on the same inputs rides along."""
    check(case)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16x2"])
def test_same_queries_in_two_forms(dtype):
    """Queries 0 .. 15 in a B = 300 call (throughput form, 128-row groups) and in a B = 16 call (shared-query x4, 64-row
    groups) on the same corpus: the same certainly-in items, scores within 2 E of each other.  (Bit equality across forms is
    not claimed by the code.)"""
    big = next(c for c in MR.CASES if c.dtype == dtype and c.B == 300 and c.C == MR.C0 and c.cls == "flat")
    small = big._replace(B=16)
    i_b, s_b, d = check(big)
    i_s, s_s, _ = check(small)
    E = d["E"][:16]
    cin, _ = MR.membership(d["s64"][:16], E, big.K)
    for r in range(16):
        a = {int(i): float(s) for i, s in zip(i_b[r], s_b[r])}
        b = {int(i): float(s) for i, s in zip(i_s[r], s_s[r])}
        must = set(torch.nonzero(cin[r]).flatten().tolist())
        assert must & set(a) == must & set(b) == must
        for i in set(a) & set(b):
            assert abs(a[i] - b[i]) <= 2 * float(E[r, i]), (r, i, a[i], b[i])


# ------------------------------------------------------------------ helper entry points
def test_f32_to_bf16_bit_for_bit():
    """Every upper half x the lower halves 0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF: ties to even, the carry into the
    exponent, the largest finite value rounding to infinity, denormals, both zeros -- against torch's .to(torch.bfloat16).
    NaN inputs: NaN-ness only.  n = 1, 257 and 0."""
    lib, N = lib_and_native()
    hi = np.arange(65536, dtype=np.uint32)[:, None] << np.uint32(16)
    lo = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)[None, :]
    x = torch.from_numpy((hi | lo).reshape(-1).view(np.float32).copy())
    want = x.to(torch.bfloat16).view(torch.int16)
    for n in (x.numel(), 257, 1, 0):
        xin = x[:max(n, 1)].to(DEV)
        out = torch.full((max(n, 1) + 8,), 0x1234, dtype=torch.int16, device=DEV)
        assert lib.tt_f32_to_bf16(xin.data_ptr(), out.data_ptr(), n, N.stream()) == 0
        got = out.cpu()
        assert bool((got[n:] == 0x1234).all())
        nan = torch.isnan(x[:n])
        assert torch.equal(got[:n][~nan], want[:n][~nan])
        assert bool(((got[:n][nan].int() & 0x7FFF) > 0x7F80).all())
    assert int(torch.isnan(x).sum()) > 1000


@pytest.mark.parametrize("dim", [2, 50, 128, 130])
def test_gather_rows_bf16_strides_duplicates_and_out_of_range_ids(dim):
    """ld_out = dim + 4 with a sentinel in the padding columns; duplicate ids; ids -1 and n_rows give zero rows and set the
    flag -- and give zero rows with oob_flag = NULL (what parallel.py passes); valid ids leave the flag alone."""
    lib, N = lib_and_native()
    n_rows, ld = 37, dim + 4
    table = torch.from_numpy(fg.gaussianish((n_rows, dim), 610 + dim)).to(torch.bfloat16)
    for ids_l in ([5, 0, 36, 5, 5, -1, 17, n_rows, 36, 1, 2], [3, 3, 36, 0], [n_rows + 1000] * 9):
        ids_t = torch.tensor(ids_l, dtype=torch.int64)
        okr = (ids_t >= 0) & (ids_t < n_rows)
        want = table[ids_t.clamp(0, n_rows - 1)].float() * okr[:, None]
        table_d, ids_d = table.to(DEV), ids_t.to(DEV)
        for with_flag in (True, False):
            out = torch.full((len(ids_l), ld), 7.0, device=DEV)
            flag = torch.zeros(1, dtype=torch.int32, device=DEV)
            rc = lib.tt_gather_rows_bf16(table_d.data_ptr(), n_rows, dim, ids_d.data_ptr(), len(ids_l),
                                         out.data_ptr(), ld, flag.data_ptr() if with_flag else None, N.stream())
            assert rc == 0
            got = out.cpu()
            assert torch.equal(got[:, :dim], want)
            assert bool((got[:, dim:] == 7.0).all())
            assert int(flag.cpu()) == (1 if with_flag and not bool(okr.all()) else 0)


def _split(x, D):
    lib, N = lib_and_native()
    rows = x.shape[0]
    out = torch.full((rows, 2 * D), float("nan"), dtype=torch.float16, device=DEV)
    scale = torch.full((1,), float("nan"), device=DEV)
    ws = torch.empty(256, dtype=torch.uint8, device=DEV)
    x_d = x.to(DEV)
    rc = lib.tt_mips_split_rows(x_d.data_ptr(), rows, D, out.data_ptr(), scale.data_ptr(), ws.data_ptr(), 256, N.stream())
    return rc, out.cpu(), float(scale.cpu())


@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("mag", [2.0 ** -60, 1.0, 2.0 ** 60])
def test_split_rows_scale_and_representation(rows, mag):
    """scale is a power of two with absmax * scale in [2^14, 2^15); (h + l) / scale is the input within 2^-23 absmax."""
    D = 128
    x = torch.from_numpy(fg.gaussianish((rows, D), 77 + rows)).double()
    x = (x * (mag / float(x.abs().max()))).float()
    absmax = float(x.abs().max())
    rc, out, scale = _split(x, D)
    assert rc == 0
    assert scale > 0 and np.frexp(scale)[0] == 0.5
    assert 2.0 ** 14 <= absmax * scale < 2.0 ** 15
    back = (out[:, :D].double() + out[:, D:].double()) / scale
    assert float((back - x.double()).abs().max()) <= 2.0 ** -23 * absmax


def test_split_rows_zero_matrix_and_refusals():
    lib, N = lib_and_native()
    rc, out, scale = _split(torch.zeros(3, 128), 128)
    assert rc == 0 and scale == 1.0 and bool((out == 0).all())
    x = torch.ones(4, 16, device=DEV)
    out = torch.zeros(4, 32, dtype=torch.float16, device=DEV)
    sc = torch.zeros(1, device=DEV)
    ws = torch.empty(256, dtype=torch.uint8, device=DEV)
    assert lib.tt_mips_split_rows(x.data_ptr(), 4, 12, out.data_ptr(), sc.data_ptr(), ws.data_ptr(), 256, N.stream()) != 0  # D % 8
    assert lib.tt_mips_split_rows(x.data_ptr(), 4, 16, out.data_ptr(), sc.data_ptr(), ws.data_ptr(), 255, N.stream()) != 0  # workspace
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and float(sc.cpu()) == 0.0  # nothing was enqueued


@pytest.mark.parametrize("ea,eb", [(0, 0), (15, 15), (65, 65), (74, -46), (-46, -46), (-20, 0)])
def test_unscale_divides_exactly_by_powers_of_two(ea, eb):
    """s / (scale_a scale_b) exactly, also where the product of the scales is no fp32 number (2^65 * 2^65 = 2^130)."""
    lib, N = lib_and_native()
    n = 257
    s = torch.from_numpy(fg.gaussianish((n,), 88)) * 2.0 ** (30 + min(max(ea + eb, -60), 60))  # results well inside the normal range
    want = (s.double() / 2.0 ** ea / 2.0 ** eb).float()
    assert bool(torch.isfinite(want).all()) and float(want.abs().min()) > 2.0 ** -120
    buf = torch.full((n + 8,), 5.0, device=DEV)
    buf[:n] = s.to(DEV)
    sa, sb = torch.tensor([2.0 ** ea], device=DEV), torch.tensor([2.0 ** eb], device=DEV)
    assert lib.tt_mips_unscale(buf.data_ptr(), n, sa.data_ptr(), sb.data_ptr(), N.stream()) == 0
    got = buf.cpu()
    assert torch.equal(got[:n], want)
    assert bool((got[n:] == 5.0).all())
