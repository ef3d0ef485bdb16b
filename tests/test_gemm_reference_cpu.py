"""The yardstick of test_gpu_gemm_reference.py can fail: the float32 index-order evaluation stays within the recorded YARD
(and YARD is that measurement, not a chosen figure); the ReLU band is nearly empty at every case; the restated dispatch
sends every case where its table entry says, with the tiles / stages per workgroup it claims, and every path of the GEMM
family is named by some case; torch's float32 matmul plus the epilogue passes the checker at every case; and every way a
GEMM kernel could plausibly go wrong -- applied to that float32 result at the very cases the GPU tests run -- is rejected."""
import collections

import pytest

import gemm_ref as GR

IDS = [GR.case_id(c) for c in GR.CASES]


@pytest.mark.parametrize("cls,band", [(c, b) for c in GR.YARD for b in GR.YARD[c]])
def test_float32_evaluation_is_within_the_recorded_yardstick(cls, band):
    """One rounding per multiply and per add, index order, against float64 over the leading block of every shape of the
    (class, K band): the worst |s32 - s64| / (2^-24 Abs) is what YARD records, rounded up by at most 10 %."""
    worst, where = GR.measure(cls, band)
    y = GR.YARD[cls][band]
    print(f"gemm-yard {cls:<9} {GR.band_name(band):<10} {worst:.3f} (recorded {y}, at {where})")
    assert worst <= y, (worst, y, where)
    assert y <= 1.1 * worst, "YARD is the measurement rounded up, not a figure chosen to fit"


def test_every_class_and_band_in_use_has_a_yardstick():
    for c in GR.CASES:
        if c.cls != "exact":
            assert GR.band_of(GR.reduction(c)) in GR.YARD[c.cls], GR.case_id(c)  # (positive: K <= 8195 only)


@pytest.mark.parametrize("case", GR.CASES, ids=IDS)
def test_case_lands_where_its_table_entry_says(case):
    """The restated dispatch (plan_gemm, the tall-M and streaming predicates, the alignment rules) gives the path the case
    names, and the launch parameters it claims: split count and last split, gemm_ws store mode / staging / tiles per
    workgroup, gemm_ws16 and tn_stream stages per workgroup, ragged last rows."""
    r = GR.route(case)
    assert r["path"] == case.path, (r["path"], case.path)
    for what, said, got in GR.claims(case, r):
        assert said == got, (what, said, got)
    if case.entry in ("gemm", "tncs") and r.get("splits", 1) > 1 and not GR.tns_ws_floats(case.M, case.N, case.K, bool(case.env)):
        assert GR.workspace_bytes(case.layout, case.M, case.N, case.K, bool(case.env)) == r["ws_need"]


def test_every_path_is_named_by_some_case():
    """Every kernel, tile, FULL form and fall-through of the family, and inside the tall-M kernels every launch variant and
    every pipeline depth the loops have, is reached by a case whose route says so."""
    routes = [(c, GR.route(c)) for c in GR.CASES]
    paths = collections.Counter(r["path"] for _, r in routes)
    assert all(paths[p] for p in GR.PATHS), [p for p in GR.PATHS if not paths[p]]

    def some(pred):
        return any(pred(c, r) for c, r in routes)

    for L in (GR.NT, GR.NN, GR.TN):
        for path in ("t64", "t64f", "t64+sk", "t128+sk", "t128f+sk"):
            assert some(lambda c, r: c.layout == L and r["path"] == path), (L, path)
        for vec in ("a_vec", "b_vec"):  # scalar loads by ld % 4 != 0 and by a base pointer one float off
            assert some(lambda c, r: c.layout == L and r.get("tile") == 64 and not r[vec] and (c.padA % 4 or c.padB % 4))
            assert some(lambda c, r: c.layout == L and r.get("tile") == 64 and not r[vec] and (c.offA % 4 or c.offB % 4))
        # aligned rows whose width is no multiple of 4: the vector loads' scalar tail
        assert some(lambda c, r: c.layout == L and r.get("tile") == 64 and r["a_vec"] and r["b_vec"] and c.K % 4 and c.N % 4)
        for K in (0, 1, 31, 32, 33):
            assert some(lambda c, r: c.layout == L and c.K == K and c.entry == "gemm")
    for L in (GR.NT, GR.NN):
        for path in ("t128", "t128f", "ws", "ws2", "ws16"):
            assert some(lambda c, r: c.layout == L and r["path"] == path), (L, path)
        assert some(lambda c, r: c.layout == L and r["path"] == "t128" and not r["a_vec"] and not r["b_vec"])
        for tile in (64, 128):  # the reduce kernel's epilogue branches
            for bias, epi, acc in GR.EPIS:
                assert some(lambda c, r: c.layout == L and r.get("tile") == tile and r.get("splits", 1) > 1 and
                            (c.bias, c.epi, c.acc) == (bias, epi, acc)), (L, tile, bias, epi, acc)
        for dp8 in (4, 8, 16, 32):
            for dma in (True, False):
                for mode in ("PLAIN", "ACC", "GENERIC"):
                    assert some(lambda c, r: c.layout == L and r["path"] == "ws" and
                                (r["passes"][0]["dp8"], r["passes"][0]["dma"], r["passes"][0]["mode"]) == (dp8, dma, mode)), (L, dp8, dma, mode)
        assert some(lambda c, r: c.layout == L and r["path"] == "ws" and r["passes"][0]["dp8"] == 16 and not r["passes"][0]["dma"] and c.offA % 4)
        # WS_GENERIC: ragged columns, a misaligned C, a misaligned aux, every epilogue with and without accumulate
        gen = lambda c, r: c.layout == L and r["path"] == "ws" and r["passes"][0]["mode"] == "GENERIC"
        assert some(lambda c, r: gen(c, r) and c.N % 32) and some(lambda c, r: gen(c, r) and c.N % 32 == 0 and c.offC % 4)
        assert some(lambda c, r: gen(c, r) and c.epi == GR.EPI_MASK and c.offX % 4)
        for epi in (GR.EPI_RELU, GR.EPI_MASK):
            for acc in (0, 1):
                assert some(lambda c, r: gen(c, r) and c.epi == epi and c.acc == acc), (epi, acc)
        # the tile loop: 1, 2, 3 and >= 4 tiles in a workgroup, an odd count above one, both kinds of ragged last tile
        counts = set()
        for c, r in routes:
            if c.layout == L and r["path"] == "ws":
                counts.update(r["passes"][0]["tiles"])
        assert {1, 2, 3, 4, 5} <= counts, counts
        assert some(lambda c, r: c.layout == L and r["path"] == "ws" and 0 < r["last_rows"] <= 32)
        assert some(lambda c, r: c.layout == L and r["path"] == "ws" and 33 <= r["last_rows"] <= 63)
        # two passes: second pass by DMA (K2 = 128), by registers (44) and K2 = 1; WS_ACC in the second and in both
        for K in (384, 300, 257):
            assert some(lambda c, r: c.layout == L and r["path"] == "ws2" and c.K == K and r["passes"][1]["mode"] == "ACC" and c.bias)
            assert some(lambda c, r: c.layout == L and r["path"] == "ws2" and c.K == K and r["passes"][0]["mode"] == "ACC")
            for epi in (GR.EPI_RELU, GR.EPI_MASK):
                assert some(lambda c, r: c.layout == L and r["path"] == "ws2" and c.K == K and c.epi == epi)
        assert some(lambda c, r: c.layout == L and r["path"] == "ws2" and r["passes"][1]["dma"])
        # back to the generic kernel from the tall-M paths
        tall = lambda c, r: c.layout == L and c.M >= GR.WS_MIN_M and r.get("tile")
        assert some(lambda c, r: tall(c, r) and c.K > 512) and some(lambda c, r: tall(c, r) and 256 < c.K <= 512 and r["full"])
        assert some(lambda c, r: tall(c, r) and 256 < c.K <= 512 and c.acc and c.epi)
        for cfg in GR.WS16_CFGS:
            depth = set()
            for c, r in routes:
                if c.layout == L and r["path"] == "ws16" and r["cfg"] == cfg:
                    depth.update(r["stages"])
            assert {3, 4, 5} <= depth and min(depth) <= 2, (cfg, depth)
            assert some(lambda c, r: c.layout == L and r["path"] == "ws16" and r["cfg"] == cfg and max(r["stages"]) >= 4 and
                        r["last_rows"] < r["rows"])
        for K in (128, 384):  # what sends a ws16 shape on to gemm_ws
            sent = lambda c, r: c.layout == L and c.N == 128 and c.K == K and r["path"] in ("ws", "ws2")
            assert some(lambda c, r: sent(c, r) and c.bias == "mis") and some(lambda c, r: sent(c, r) and c.padA % 4)
            assert some(lambda c, r: sent(c, r) and c.acc)
    for H in (1, 29, 32):
        assert some(lambda c, r: r["path"] == "pool" and c.H == H)
    assert some(lambda c, r: r["path"] == "pool" and c.M == 16384) and some(lambda c, r: r["path"] == "pool" and max(r["stages"]) >= 4)
    assert some(lambda c, r: r["path"] == "pool" and c.padX) and some(lambda c, r: r["path"] == "pool" and c.H == 29 and r["rows"] % c.H)
    for cg in (1, 2, 3):
        tns = lambda c, r: r["path"] == "tns" and r["cg"] == cg
        for K in (8192, 8193):
            assert some(lambda c, r: tns(c, r) and c.K == K)
        assert some(lambda c, r: tns(c, r) and max(r["stages"]) >= 4 and r["last_rows"] < 2 * GR.tns_s(cg))
        for entry in ("gemm", "tncs"):
            for acc in (0, 1):
                assert some(lambda c, r: tns(c, r) and c.entry == entry and c.acc == acc), (cg, entry, acc)
        assert some(lambda c, r: tns(c, r) and c.padA == 0) and some(lambda c, r: tns(c, r) and c.padA)
        fell = lambda c, r: c.layout == GR.TN and c.M == 128 * cg and c.N == 128 and r.get("tile") and bool(c.env) == (cg < 3)
        assert some(lambda c, r: fell(c, r) and c.K == 8191) and some(lambda c, r: fell(c, r) and c.K == 8192 and (c.offA % 4 or c.offB % 4))
    # the default process sends the M = 128 / 256 shapes of the child process to the tiled kernel
    for c in GR.CHILD_CASES:
        if c.path == "tns":
            assert some(lambda d, r: not d.env and (d.M, d.N, d.K) == (c.M, c.N, c.K) and r.get("tile")), GR.case_id(c)
    assert some(lambda c, r: r["path"] == "colsum" and r["rows_per_part"] == 128)
    for M in (1, 63, 64, 65):
        assert some(lambda c, r: r["path"] == "colsum" and c.M == M)
    for N in (1, 63, 65):
        assert some(lambda c, r: r["path"] == "colsum" and c.N == N)
    assert some(lambda c, r: r["path"] == "none" and c.M == 0) and some(lambda c, r: r["path"] == "none" and c.N == 0)


def test_float32_is_accepted_and_every_mutant_is_rejected():
    """At every case: at most BAND_SHARE of the elements have their ReLU argument within E of zero (a condition, checked on
    the reference alone); torch's float32 matmul plus the float32 epilogue, written through the poisoned buffers, passes;
    and each mutant of gemm_ref.MUTANTS, wherever it changes a bit of that float32 result, is rejected."""
    ran, missed, worst32, worst_band = collections.Counter(), [], 0.0, 0.0
    for case in GR.CASES:
        d, s = GR.shape_data(case), GR.side_inputs(case)
        ref = GR.reference(case, d, s)
        bufs = GR.Buffers(case, d, s)
        n = ref["band"].numel()
        share = int(ref["band"].sum()) / n if n else 0.0
        worst_band = max(worst_band, share)
        assert share <= GR.BAND_SHARE, (GR.case_id(case), share)
        base = GR.run_f32(case, d, s, bufs)
        rep = GR.check(case, ref, bufs, *base)
        assert rep.ok, (GR.case_id(case), rep)
        assert rep.worst <= 0.5 and rep.db_worst <= 0.5, "BLAS float32 is another summation order of the same sum: inside the factor 4 by far"
        worst32 = max(worst32, rep.worst, rep.db_worst)
        for m in GR.MUTANTS:
            out = GR.run_f32(case, d, s, bufs, m)
            if out is None or (GR.same_bits(out[0], base[0]) and GR.same_bits(out[1], base[1])):
                continue  # nothing for this mutant to do at this case
            ran[m] += 1
            if GR.check(case, ref, bufs, *out).ok:
                missed.append((m, GR.case_id(case)))
    GR.drop_cache()
    print(f"gemm-f32 {len(GR.CASES)} cases: worst err / E of torch's float32 {worst32:.3f}, largest ReLU band share {100 * worst_band:.4f} %")
    for m in GR.MUTANTS:
        print(f"gemm-mutant {m:<18} rejected at {ran[m] - sum(1 for x, _ in missed if x == m)} of {ran[m]} cases where it differs")
    assert not missed, missed
    assert all(ran[m] > 0 for m in GR.MUTANTS), [m for m in GR.MUTANTS if not ran[m]]
