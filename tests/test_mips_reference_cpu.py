"""The yardstick of test_gpu_mips_reference.py can fail: the float32 index-order evaluation stays within the recorded
YARD at every case the GPU tests run; the conditions that keep the membership rule from hiding a failure hold at every
case; torch's float32 top-K passes the checker at every case; and every way a MIPS kernel could plausibly go wrong -- applied
to that float32 result at the very cases the GPU tests run -- is rejected, by the rule named."""
import numpy as np
import pytest
import torch

import mips_ref as MR

IDS = [MR.case_id(c) for c in MR.CASES]


@pytest.mark.parametrize("dtype,cls", [(d, c) for d in MR.YARD for c in MR.YARD[d]])
def test_float32_evaluation_is_within_the_recorded_yardstick(dtype, cls):
    """One rounding per multiply and per add, index order, against float64 over every reference of the (dtype, class): the
    worst |s32 - s64| / (2^-24 A) is what YARD records, rounded up to two digits -- the number every bound hangs on."""
    worst, where = MR.measure(dtype, cls)
    y = MR.YARD[dtype][cls]
    print(f"mips-yard {dtype:<5} {cls:<10} {worst:.3f} (recorded {y}, at {where})")
    assert worst <= y, (worst, y, where)
    assert y <= 1.25 * worst + 0.1, "YARD is the measurement rounded up, not a figure chosen to fit"


@pytest.mark.parametrize("case", MR.CASES, ids=IDS)
def test_conditions_hold_and_float32_topk_is_accepted(case):
    """Rule 5 (conditions, not measurements): enough (query, item) pairs are decided and enough of each query's float64
    top-K is certainly in that rule 4 cannot pass a wrong set.  And the reference alone stays inside: torch's float32
    top-K of the effective operands passes every rule."""
    d = MR.case_data(case)
    dec, inn = MR.conditions(d["s64"], d["E"], case.K)
    need = MR.CONDITIONS.get(case.cls, MR.CONDITIONS_DEFAULT)
    print(f"mips-cond {MR.case_id(case)} decided {100 * dec:.3f} % certainly-in {100 * inn:.2f} %")
    assert dec >= need[0] and inn >= need[1], (dec, inn, need)
    idx, sc = MR.topk32(d["q"], d["c"], case.K)
    rep = MR.check_topk(idx, sc, d["q"], d["c"], case.K, d["E"], s64=d["s64"])
    print(f"mips-f32topk {MR.case_id(case)} {rep}")
    assert rep.ok, rep
    assert rep.worst <= 0.5, "BLAS float32 is another summation order of the same sum: inside the factor 4 by far"
    if case.plant:  # every planted row must win somewhere, or the corpus-edge cases test nothing
        cin, _ = MR.membership(d["s64"], d["E"], case.K)
        rows = MR.plant_rows(case.C)
        assert bool(cin[:, rows].any(dim=0).all()), [r for r in rows if not bool(cin[:, r].any())]


@pytest.mark.parametrize("cls", ["flat", "negative", "clustered", "range", "tiny"])
def test_split_representation_alone_is_inside_its_bound(cls):
    """numpy float16 emulation of tt_mips_split_rows, float64 products of the three terms the kernel keeps: what the
    representation can express is within D 2^-21 max|Q| max|C| of float64 on every class (the range class's bound), and
    within the fp32 E on the classes held to it."""
    case = next(c for c in MR.F16X2 if c.cls == cls and c.B in (72, 300) and c.C == MR.C0)
    d = MR.case_data(case)
    err = (MR.split_scores(d["q_raw"], d["c_raw"]) - d["s64"]).abs()
    norm = MR.split_bound(d["q_raw"], d["c_raw"])
    print(f"mips-split {cls:<10} max err / norm-wise bound {float(err.max()) / norm:.3g}  max err / E {float((err / d['E']).max()):.3g}")
    assert float(err.max()) <= norm
    assert float((err / d["E"]).max()) <= 1.0


# ------------------------------------------------------------------ mutants
def _masked_topk(s32, K, cols):
    s = s32.clone()
    s[:, cols] = float("-inf")
    return MR.ordered_topk(s, K)


def _truncate_bf16(x):
    return torch.from_numpy((x.numpy().view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).copy())


def mutants_of(case, d):
    """(name, expected rule or None = any, idx, scores, s64, E, rows) of every mutant that can differ at this case; rows
    = the queries passed to the checker (None: all)."""
    B, C, K = case.B, case.C, case.K
    s32 = d["q"] @ d["c"].t()
    idx, sc = MR.ordered_topk(s32, K)
    cin, cout = MR.membership(d["s64"], d["E"], K)
    out = []
    r = B // 2
    if K < C:  # the tau item lost: the lowest-ranked returned item that is the best of its group and certainly in
        i1, s1 = MR.ordered_topk(s32, K + 1)
        pad = (-C) % MR.GROUP
        gbest = torch.nn.functional.pad(s32, (0, pad), value=float("-inf")).reshape(B, -1, MR.GROUP).argmax(dim=2)
        is_best = gbest.gather(1, idx // MR.GROUP) == idx % MR.GROUP
        ok = is_best & cin.gather(1, idx)
        rows = torch.nonzero(ok.any(dim=1)).flatten().tolist()
        if rows:
            rr = rows[len(rows) // 2]
            j = int(torch.nonzero(ok[rr]).flatten()[-1])
            keep = [k for k in range(K + 1) if k != j]
            mi, ms = idx.clone(), sc.clone()
            mi[rr], ms[rr] = i1[rr, keep], s1[rr, keep]
            out.append(("tau_item_dropped", 4, mi, ms, None))
    mi, ms = idx.clone(), sc.clone()
    mi[r, K // 2], ms[r, K // 2] = -1, float("nan")
    out.append(("sentinel_slot", 1, mi, ms, None))
    g0 = (C - 1) // MR.GROUP * MR.GROUP
    for name, cols in (("last_group_ignored", slice(g0, C)), ("last_row_ignored", slice(C - 1, C)),
                       ("rows_ge_65536_ignored", slice(MR.WIDE_ROWS, C))):
        if name == "last_row_ignored" and C % MR.CHUNK == 0:
            continue
        lo = cols.start
        if lo >= C or K > lo or not bool((idx >= lo).any()):
            continue
        mi, ms = _masked_topk(s32, K, cols)
        lost = cin[:, lo:].any()  # a certainly-in item among the ignored rows: otherwise the result is still a valid one
        if bool(lost):
            out.append((name, 4, mi, ms, None))
    j = K // 3
    nb = idx[r, j] + (1 if idx[r, j] + 1 < C else -1)
    ms = sc.clone()
    ms[r, j] = s32[r, nb]
    out.append(("neighbour_score", 2, idx, ms, None))
    if K >= 2:
        mi, ms = idx.clone(), sc.clone()
        mi[r, 1], ms[r, 1] = mi[r, 0], ms[r, 0]
        out.append(("duplicate_index", 1, mi, ms, None))
        # a real tie: the best row of query r copied to its neighbour; the pair must come out in ascending index order
        a = int(idx[r, 0])
        b = a + 1 if a + 1 < C else a - 1
        lo, hi = min(a, b), max(a, b)
        s64r, Er, s32r = d["s64"][r:r + 1].clone(), d["E"][r:r + 1].clone(), s32[r:r + 1].clone()
        s64r[0, b], Er[0, b], s32r[0, b] = s64r[0, a], Er[0, a], s32r[0, a]
        ti, ts = MR.ordered_topk(s32r, K)
        assert ti[0, 0] == lo and ti[0, 1] == hi and ts[0, 0] == ts[0, 1]
        assert MR.check_topk(ti, ts, None, None, K, Er, s64=s64r).ok
        ti = ti.clone()
        ti[0, 0], ti[0, 1] = hi, lo
        out.append(("tie_descending_index", 3, ti, ts, (s64r, Er)))
    if case.dtype == "bf16":
        qt, ct = _truncate_bf16(d["q_raw"]), _truncate_bf16(d["c_raw"])
        mi, ms = MR.topk32(qt, ct, K)
        out.append(("bf16_truncated", 2 if case.cls == "flat" else None, mi, ms, None))
    if B > MR.MIPS_QBATCH:
        # The second query batch against a tau the first one left behind -- the highest of them, the stale value that
        # hurts (a lower one than the query's own only adds candidates): fewer than K candidates, the slots after them are
        # emitted as -1 / 0, which is what the sort kernels write there.
        pad = (-C) % MR.GROUP
        gmax = torch.nn.functional.pad(s32, (0, pad), value=float("-inf")).reshape(B, -1, MR.GROUP).amax(dim=2)
        tau = torch.topk(gmax, K, dim=1).values[:, K - 1]
        stale = float(tau[:MR.MIPS_QBATCH].max())
        mi, ms = idx.clone(), sc.clone()
        short = 0
        for q in range(MR.MIPS_QBATCH, B):
            n = int((s32[q] >= stale).sum())
            if n < K:
                mi[q, n:], ms[q, n:] = -1, 0.0
                short += 1
        assert short > 0, "the stale tau leaves every query of the second batch K candidates: the mutant would be a no-op"
        out.append(("second_batch_stale_tau", 1, mi, ms, None))
    return out


MUTANTS = ("tau_item_dropped", "sentinel_slot", "last_group_ignored", "last_row_ignored", "rows_ge_65536_ignored",
           "neighbour_score", "duplicate_index", "tie_descending_index", "bf16_truncated", "second_batch_stale_tau")


def required_mutants(case):
    """The mutants that MUST be generated at a case, from its shape alone.  The ignored-rows mutants depend on where the
    winners lie: they are required where a winner is known to lie in the ignored rows (the planted last row; the wide corpus
    that reaches past 65536 rows) and are generated at many more cases."""
    need = {"sentinel_slot", "neighbour_score"}
    if case.K < case.C:
        need.add("tau_item_dropped")
    if case.K >= 2:
        need |= {"duplicate_index", "tie_descending_index"}
    if case.plant:
        need |= {"last_group_ignored", "last_row_ignored"}
    if case.C > MR.WIDE_ROWS:
        need.add("rows_ge_65536_ignored")
    if case.dtype == "bf16":
        need.add("bf16_truncated")
    if case.B > MR.MIPS_QBATCH:
        need.add("second_batch_stale_tau")
    return need


def test_every_named_mutant_is_required_at_some_case():
    """No mutant can vanish behind a guard: each is required at one case at least (and test_mutants_are_rejected asserts
    that every required one was generated), the stale tau at both B = 1089 cases."""
    assert set().union(*(required_mutants(c) for c in MR.CASES)) == set(MUTANTS)
    assert all("second_batch_stale_tau" in required_mutants(c) for c in MR.BIG) and len(MR.BIG) == 2


@pytest.mark.parametrize("case", MR.CASES, ids=IDS)
def test_mutants_are_rejected(case):
    """Each wrong result, built from the float32 top-K at every case where it can differ: the tau item dropped (what a
    pass-1 / pass-2 disagreement does), a slot left at the sentinel, the last group / the last row of a ragged final chunk /
    rows >= 65536 ignored, a score from the neighbouring row, a duplicated index, a tie in descending index order, bf16
    operands truncated instead of rounded (rule 2 in the flat class), the second 1024-batch against the first one's tau."""
    d = MR.case_data(case)
    built = mutants_of(case, d)
    names = {m[0] for m in built}
    assert required_mutants(case) <= names <= set(MUTANTS), (required_mutants(case) - names, names - set(MUTANTS))
    for name, rule, mi, ms, ref in built:
        s64, E = ref if ref is not None else (d["s64"], d["E"])
        rep = MR.check_topk(mi, ms, None, None, case.K, E, s64=s64)
        print(f"mips-mutant {name:<24} {MR.case_id(case)} fired {rep.fired()} worst err/E {rep.worst:.3g}")
        assert not rep.ok, name
        assert rule is None or rule in rep.fired(), (name, rule, rep)
