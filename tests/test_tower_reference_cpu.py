"""The yardstick of test_gpu_tower_reference.py can fail: the float32 index-order evaluation stays within the recorded YARD
(and YARD is that measurement, not a chosen figure); every reduction of the exact class stays a sum of multiples of 2^-2
below 2^22, so equality may be demanded of it; the ReLU band is nearly empty at every case; the restated dispatch names for
every case the template instantiation its table entry says, with the row tiles, LDS bytes, block counts and reduce trip
counts it claims, and every instantiation of tower.hip is named by some case; a float32 torch evaluation passes the checker
at every case; and every way a tower kernel could plausibly go wrong -- applied to that float32 result at the very cases the
GPU tests run -- is rejected."""
import collections

import pytest

import tower_ref as TR

IDS = [TR.case_id(c) for c in TR.CASES]


@pytest.mark.parametrize("cls", list(TR.YARD))
def test_float32_evaluation_is_within_the_recorded_yardstick(cls):
    """One rounding per multiply and per add, index order, against float64 over the leading block of every shape of the
    class: the worst |s32 - s64| / (2^-24 Abs) per band is what YARD records, rounded up by at most 10 %."""
    got = TR.measure(cls)
    for band in TR.BANDS:
        worst, where = got[band]
        y = TR.YARD[cls][band]
        print(f"tower-yard {cls:<6} {band:<4} {worst:.3f} (recorded {y}, at {where})")
        assert worst <= y, (band, worst, y, where)
        assert y <= 1.1 * worst, "YARD is the measurement rounded up, not a figure chosen to fit"


@pytest.mark.parametrize("case", TR.CASES, ids=IDS)
def test_case_lands_where_its_table_entry_says(case):
    """route() -- tower_row_tiles, the grids, the dynamic LDS, the workspace formula, the reduce loop -- gives the
    instantiation the case names and every launch parameter it claims."""
    r = TR.route(case)
    assert r["path"] == case.path, (r["path"], case.path)
    for what, said, got in TR.claims(case, r):
        assert said == got, (what, said, got)
    assert sum(r["launches"].values()) == (2 if case.entry == "wgrad" else 1)
    if case.entry == "wgrad":
        assert r["ws"] == [TR.workspace_bytes(case.B, case.D, TR.F_of(case, k), case.E) for k in range(case.sides)]
    assert r["lds"] <= 160 * 1024 and case.B <= 8257


def test_every_instantiation_and_edge_is_named_by_some_case():
    """All 12 tower_fwd_kernel, 12 tower_bwd_kernel, 6 + 6 pair, 6 tower_wgrad_kernel and 3 pair instantiations; both reduce
    kernels with every block count of the issue, a sixteenth that runs the unrolled loop and then the tail among them; and
    the edges of the forward / backward: every B and F, the 4096 / 4097 boundary, the largest LDS request, strided and
    misaligned operands, out-of-range ids with and without a flag."""
    routes = [(c, TR.route(c)) for c in TR.CASES]
    named = collections.Counter(r["path"] for _, r in routes)
    missing = [i for i in TR.instantiations() if not named[i]]
    assert len(TR.instantiations()) == 45 and not missing, missing

    def some(pred):
        return any(pred(c, r) for c, r in routes)

    for D in (32, 64, 128):
        for E in (0, 2 * D):
            for entry in ("fwd", "bwd"):
                for B, rt in TR.BS:
                    assert some(lambda c, r: (c.entry, c.sides, c.D, c.E, c.B) == (entry, 1, D, E, B) and r["rt"] == rt), (entry, D, E, B)
                for strided in (False, True):
                    for rt in (1, 2):
                        assert some(lambda c, r: (c.entry, c.sides, c.D, c.E, c.strided) == (entry, 1, D, E, strided) and r["rt"] == rt)
            for F in TR.FS:
                for rt in (1, 2):
                    assert some(lambda c, r: (c.entry, c.sides, c.D, c.E, c.F) == ("fwd", 1, D, E, F) and r["rt"] == rt), (D, E, F, rt)
                assert some(lambda c, r: (c.entry, c.sides, c.D, c.E, c.F, c.strided) == ("fwd", 1, D, E, F, True))
            for ids in ("oob", "oobnull"):
                for rt in (1, 2):
                    assert some(lambda c, r: (c.entry, c.D, c.E, c.ids) == ("fwd", D, E, ids) and r["rt"] == rt)
            for cls in ("flat", "exact"):
                assert some(lambda c, r: (c.entry, c.sides, c.D, c.E, c.cls) == ("wgrad", 1, D, E, cls))
        for entry in ("fwd", "bwd"):
            for rt in (1, 2):
                for cls in ("flat", "exact"):
                    assert some(lambda c, r: (c.entry, c.sides, c.D, c.cls) == (entry, 2, D, cls) and r["rt"] == rt), (entry, D, rt, cls)
        assert some(lambda c, r: c.entry == "fwd" and c.sides == 2 and c.D == D and c.F[0] != c.F[1] and c.F[0] < c.F[1])
        assert some(lambda c, r: c.entry == "fwd" and c.sides == 2 and c.D == D and c.F[0] > c.F[1])
        assert some(lambda c, r: c.entry == "wgrad" and c.sides == 2 and c.D == D and r["parts"][0] != r["parts"][1] and r["both"])
    for E in (0, 256):  # the 149 504-byte forward, its second 32-row tile wholly past B
        assert some(lambda c, r: (c.entry, c.D, c.E, c.B, c.F) == ("fwd", 128, E, 4097, 64) and r["lds"] == TR.LDS_MAX == 149504 and
                    r["last_rows"] == 1)
    for nb, trips in TR.NBS.items():
        for sides in (1, 2):
            if sides == 1 or nb in (1, 2, 17, 113, 129, 130):
                assert some(lambda c, r: c.entry == "wgrad" and c.sides == sides and r["nb"] == nb and r["trips"] == trips), (nb, sides)
    assert some(lambda c, r: c.entry == "wgrad" and c.B == 8257 and r["nb"] == 130 and r["last_rows"] == 1 and r["both"])
    assert not TR.route(next(c for c in TR.CASES if c.entry == "wgrad" and TR.route(c)["nb"] == 128))["both"]


def test_float32_is_accepted_and_every_mutant_is_rejected():
    """At every case: the exact class's reductions are sums of multiples of 2^-2 that stay below 2^22 (from the float64
    reference's Abs, not assumed); at most BAND_SHARE of h_out has its pre-activation within E of zero; the float32 torch
    evaluation, written through the poisoned buffers, passes; and each mutant of tower_ref.MUTANTS, wherever it changes a
    bit of that float32 result, is rejected."""
    ran, missed, worst32, worst_band, worst_abs = collections.Counter(), [], 0.0, 0.0, 0.0
    for case in TR.CASES:
        inp = TR.inputs(case)
        bufs = TR.Buffers(case, inp)
        if case.cls == "exact":
            a = TR.exact_abs(case, inp)
            worst_abs = max(worst_abs, a)
            assert a < TR.EXACT_LIMIT, (TR.case_id(case), a)
            for x in inp:
                for name, v in x.items():
                    if hasattr(v, "dtype") and v.dtype.is_floating_point and not name.startswith("_") and name != "h":
                        assert bool((v / TR.EXACT_QUANTUM == (v / TR.EXACT_QUANTUM).round()).all()), (TR.case_id(case), name)
        share = TR.band_share(case, inp)
        worst_band = max(worst_band, share)
        assert share <= TR.BAND_SHARE, (TR.case_id(case), share)
        base = TR.run_f32(case, inp, bufs)
        rep = TR.check(case, inp, bufs, *base)
        assert rep.ok, (TR.case_id(case), rep)
        assert rep.worst <= 1.0 and (case.cls != "exact" or rep.worst == 0.0)
        worst32 = max(worst32, rep.worst)
        for m in TR.MUTANTS:
            out = TR.run_f32(case, inp, bufs, m)
            if out is None or TR.same_outputs(out, base):
                continue  # nothing for this mutant to do at this case
            ran[m] += 1
            if TR.check(case, inp, bufs, *out).ok:
                missed.append((m, TR.case_id(case)))
    print(f"tower-f32 {len(TR.CASES)} cases: worst err / E of torch's float32 {worst32:.3f}, largest ReLU band share "
          f"{100 * worst_band:.4f} %, exact class: largest sum of |terms| {worst_abs:.0f}")
    for m in TR.MUTANTS:
        print(f"tower-mutant {m:<22} rejected at {ran[m] - sum(1 for x, _ in missed if x == m)} of {ran[m]} cases where it differs")
    assert not missed, missed
    assert all(ran[m] > 0 for m in TR.MUTANTS), [m for m in TR.MUTANTS if not ran[m]]
