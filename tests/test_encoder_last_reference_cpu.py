"""The yardstick of test_gpu_encoder_last_reference.py can fail: its float64 reference is the oracle's uncollapsed layer
(three pins); the float32 index-order evaluation of the kernels' algebra stays within the recorded YARD (and YARD is that
measurement, not a chosen figure) and inside every case's bound; the case table names every edge the kernels have; and every
way a kernel of csrc/encoder_last.hip could plausibly go wrong -- evaluated in float64 at the very cases the GPU tests run --
is rejected at every case where it can change a result."""
import math

import pytest
import torch

import encoder_last_ref as ER
import history_lengths_ref as HL
from oracle import cpu_ref as R

DISTINCT = ER.distinct_cases()
PIN = 1e-12
PIN_SHIFTED_DT = 5e-11  # dx and db_in of the shifted class: see the pin test
_f32 = {}


def f32_eval(c):
    k = ER._math_key(c)
    if k not in _f32:
        _f32[k] = ER.collapsed(ER.case_inputs(c), ER.F32)
    return _f32[k]


def _dist(a, b):
    return float((a.reshape(b.shape) - b).abs().max()) / float(b.abs().max())


@pytest.mark.parametrize("cls", ER.CLASSES)
def test_reference_is_the_oracle_layer_and_the_collapsed_algebra(cls):
    """Each within 1e-12 of max|ref|: (1) oracle.cpu_ref.self_attention_layer(...)[:, 0, :]; (2) history_lengths_ref.
    last_layer_row0 (with the case's lengths, or full ones); (3) the collapsed algebra in float64, all eleven quantities.
    dx and db_in of the shifted class are held to 5e-11 of max|ref| instead (1.2e-11 measured): rows 1 .. H-1 share a vector
    of up to 814 there, dt = sum_j ds_j x_j with sum_j ds_j = 0 cancels it, and BOTH float64 evaluations carry that
    cancellation's rounding (2^-53 * max|x| each, through two more products)."""
    worst = [0.0, 0.0, 0.0]
    for c in DISTINCT:
        if c.cls != cls:
            continue
        inp, ref = ER.case_inputs(c), ER.case_reference(c)
        x, w_in, b_in, w_out, b_out = (inp[k].double() for k in ("x_bwd", "w_in", "b_in", "w_out", "b_out"))
        lens = inp["lens"]
        if lens is None:
            worst[0] = max(worst[0], _dist(R.self_attention_layer(x, w_in, b_in, w_out, b_out, c.heads)[:, 0, :], ref["recent"]))
        worst[1] = max(worst[1], _dist(HL.last_layer_row0(x, lens if lens is not None else [c.H] * c.B, w_in, b_in, w_out, b_out, c.heads),
                                       ref["recent"]))
        col = ER.collapsed(inp)
        for n in ER.NAMES:
            d = _dist(col[n], ref[n])
            if cls == "shifted" and n in ("dx", "db_in"):
                assert d <= PIN_SHIFTED_DT, (ER.case_id(c), n, d)
                continue
            assert d <= PIN, (ER.case_id(c), n, d)
            worst[2] = max(worst[2], d)
    print(f"enc-last-pin {cls:<8} oracle {worst[0]:.1e} truncation {worst[1]:.1e} collapsed {worst[2]:.1e}")
    assert max(worst) <= PIN, worst


@pytest.mark.parametrize("cls", ER.CLASSES)
def test_float32_evaluation_is_within_the_recorded_yardstick_and_every_bound(cls):
    """One rounding per multiply and per add, index order, exp correctly rounded, against float64 at every case of the class:
    the worst normalised error per quantity is what YARD records (rounded up to two digits, floor 2^-24), and the same
    evaluation sits inside every case's bound."""
    worst = {n: (0.0, None) for n in ER.NAMES}
    for c in DISTINCT:
        if c.cls != cls:
            continue
        got, ref = f32_eval(c), ER.case_reference(c)
        for n in ER.NAMES:
            e = ER.normalised_error(got[n], ref[n], n)
            if e >= worst[n][0]:
                worst[n] = (e, ER.case_id(c))
        ratios, exact = ER.verdict(c, got, ref)
        assert not exact and max(ratios.values()) <= 1.0, (ER.case_id(c), ratios, exact)
    for n in ER.NAMES:
        y = ER.YARD[cls][n]
        print(f"enc-last-yard {cls:<8} {n:<7} {worst[n][0]:.3e} (recorded {y:.1e}, at {worst[n][1]})")
        assert worst[n][0] <= y, (n, worst[n], y)
        assert y <= 1.0001 * ER.round_up(worst[n][0]), "YARD is the measurement rounded up, not a figure chosen to fit"


@pytest.mark.parametrize("cls", ER.CLASSES)
def test_unmutated_float64_algebra_is_far_inside_the_tolerance(cls):
    for c in DISTINCT:
        if c.cls == cls:
            ratios, exact = ER.verdict(c, ER.collapsed(ER.case_inputs(c)), ER.case_reference(c))
            assert not exact and max(ratios.values()) <= 1e-3, (ER.case_id(c), ratios, exact)


@pytest.mark.parametrize("mut", ER.MUTANTS)
def test_mutant_is_rejected_at_every_case_where_it_changes_a_result(mut):
    """The wrong formula in float64 (no_max in float32: it is fp32's exp that overflows) against the case's own tolerance."""
    n_cases, missed = 0, []
    for c in DISTINCT:
        if not ER.applies(mut, c):
            continue
        n_cases += 1
        got = ER.collapsed(ER.case_inputs(c), ER.F32 if mut == "no_max" else ER.F64, mut)
        if not ER.rejected(c, got, ER.case_reference(c)):
            missed.append(ER.case_id(c))
    print(f"enc-last-mutant {mut:<18} rejected at {n_cases - len(missed)} of {n_cases} cases")
    assert n_cases > 0 and not missed, missed


def test_no_max_mutant_gives_inf_or_nan():
    c = next(c for c in ER.CASES if c.cls == "shifted" and c.H == 50)
    got = ER.collapsed(ER.case_inputs(c), ER.F32, "no_max")
    assert not bool(torch.isfinite(got["probs"]).all()) and not bool(torch.isfinite(got["recent"]).all())


def test_shifted_class_sits_where_it_says():
    """Every head's scores on rows 1 .. H-1 within 25 of +200 (even samples) or -200 (odd); exp(200) overflows fp32, and row
    0's probability underflows to zero (even) or takes all the mass (odd) in fp32."""
    for c in DISTINCT:
        if c.cls != "shifted":
            continue
        inp, ref = ER.case_inputs(c), ER.case_reference(c)
        s = torch.einsum("bhd,bjd->bhj", ref["t"], inp["x_bwd"].double()) / math.sqrt(c.D // c.heads)
        rel = s[:, :, 1:] - s[:, :, :1]  # against row 0, whose score is of the flat class's size
        sign = torch.where(torch.arange(c.B) % 2 == 0, 1.0, -1.0)[:, None, None]
        assert float((rel * sign - 200.0).abs().max()) < 25.0, ER.case_id(c)
        p0 = ref["probs"][:, :, 0].float()
        assert bool((p0[0::2] == 0).all()) and bool((p0[1::2] == 1).all()), ER.case_id(c)


def test_case_table_names_every_edge():
    """The 32-sample groups with 1, 31 and 32 samples in the last one; the reduce over 1, 2, 3, 4, 5, 8 and 9 partials; head
    width % 8 == 4; a tile of eight heads; a last tile of 4 and of 28 columns; D on both sides of 64; every H around the
    32-lane halves; lengths 1 .. H, the four out-of-contract ones; both placements; every case at most B = 257."""
    C = ER.CASES
    assert {len(ER.groups_of(c.B)) for c in C if c.group == "batch"} == {1, 2, 3, 4, 5, 8, 9}
    assert {c.B % 32 for c in C if c.group == "batch"} >= {0, 1, 31}
    widths = {(c.D, c.heads) for c in C if c.group == "width"}
    assert widths == set(ER.WIDTHS) and all({"flat", "peaked"} == {c.cls for c in C if c.group == "width" and (c.D, c.heads) == w} for w in widths)
    assert any((D // h) % 8 == 4 for D, h in widths) and (64, 16) in widths and any(D % 32 == 4 for D, _ in widths)
    assert any(D % 32 == 28 for D, _ in widths) and {64, 68} <= {D for D, _ in widths}
    for D, h in ((128, 4), (64, 16)):
        for H in ER.HISTORIES:
            want = set(ER.CLASSES) - ({"shifted"} if H == 1 else set())
            assert {c.cls for c in C if c.group == "history" and (c.H, c.D, c.heads) == (H, D, h)} == want
    for s in ER.LEN_SHAPES:
        kinds = {(c.cls, c.lens) for c in C if c.group == "lengths" and (c.B, c.H, c.D, c.heads) == s}
        assert kinds == {("flat", "cycle"), ("peaked", "cycle"), ("flat", "bad"), ("flat", "null")}
        raw, lens = ER.lengths_of(ER.Case("lengths", *s, "flat", "cycle"))
        assert raw == lens and {1, s[1]} <= set(lens)
        gaps = [b - a for a, b in zip(sorted(set(lens)), sorted(set(lens))[1:])]
        assert max(gaps, default=1) <= 2  # every length, or (B < H) no two neighbours more than 2 apart
        raw, lens = ER.lengths_of(ER.Case("lengths", *s, "flat", "bad"))
        assert raw[:4] == [0, -3, s[1] + 1, 2 ** 31 - 1] and lens[:4] == [1, 1, s[1], s[1]]
    assert {(c.B, c.H, c.D, c.heads, c.place) for c in C if c.group == "placement"} == {(33, 50, 128, 4, 1), (33, 50, 128, 4, 2),
                                                                                        (33, 10, 100, 5, 1), (33, 10, 100, 5, 2)}
    assert {(c.B, c.H, c.D, c.heads) for c in C if c.cls == "kbias" and c.group == "kbias"} == {(33, 50, 128, 4), (33, 7, 36, 3)}
    assert max(c.B for c in C) == 257 and all(c.H <= 64 and c.D <= 128 and c.D % c.heads == 0 and (c.D // c.heads) % 4 == 0 for c in C)


def test_workspace_formula_matches_the_library():
    from two_tower_models_amd import _native as N
    lib = N.load()
    for c in ER.CASES:
        assert lib.tt_enc_last_bwd_workspace_bytes(c.B, c.H, c.D, c.heads) == ER.workspace_bytes(c.B, c.H, c.D, c.heads)
