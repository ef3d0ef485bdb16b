"""The float64 yardstick of the in-batch softmax cross entropy, checked where no GPU is needed (tests/ce_ref.py):

  * the float32 index-order evaluation of the formulas stays within YARD of float64 at every case of
    test_gpu_ce_reference.py (the table the GPU tolerances are 4 x of);
  * ce_ref.plan, the Python statement of the host dispatch code, agrees with the built library's own workspace queries
    (they are functions of both split counts) at every case and at the shapes plan_ce's comments name;
  * the case list reaches every cell of the dispatch matrix;
  * the checker and tolerances the GPU test uses reject each deliberately wrong formula at every case where it can
    differ;
  * the input classes are what they claim to be (conditions on the float64 reference alone)."""
import collections

import pytest
import torch

import ce_ref as C

KEYS = C.yardstick_keys()
ALL_KEYS = sorted(set(C.math_key(c) for c in C.CASES), key=str)
HEAVY_KEYS = [k for k in ALL_KEYS if C.heavy(k)]


@pytest.fixture(scope="module")
def lib():
    from two_tower_models_amd import _native as N
    return N.load(), N


@pytest.fixture(scope="module")
def evaluated():
    """key -> (float64 reference, float32 evaluation, memo), each computed once."""
    cache = {}

    def get(key):
        if key not in cache:
            U, I, b, coef, _ = C.inputs(key)
            memo = {}
            cache[key] = (C.key_reference(key), C.evaluate(U, I, b, coef, key[3], C.F32, memo=memo), memo)
        return cache[key]

    return get


# ------------------------------------------------------------------ yardstick
def test_float32_evaluation_stays_within_the_yardstick(evaluated):
    worst = {cls: {q: 0.0 for q in C.QUANTITIES} for cls in C.CLASSES}
    for key in KEYS:
        ref, got, _ = evaluated(key)
        assert set(C.QUANTITIES) <= set(got) and set(C.QUANTITIES) <= set(ref)  # the cases skip no quantity
        for q in C.QUANTITIES:
            assert torch.isfinite(got[q]).all(), (key, q)
            worst[key[4]][q] = max(worst[key[4]][q], C.normalised_error(got[q], ref[q], q))
    for cls in C.CLASSES:
        print(cls, " ".join(f"{q} {worst[cls][q]:.2e} (YARD {C.YARD[cls][q]:.1e})" for q in C.QUANTITIES))
        for q in C.QUANTITIES:
            assert C.YARD[cls][q] >= C.FLOOR
            assert worst[cls][q] <= C.YARD[cls][q], (cls, q, worst[cls][q])
            assert worst[cls][q] >= 0.5 * C.YARD[cls][q] or C.YARD[cls][q] <= 6.0e-8, \
                (cls, q, worst[cls][q], "YARD is more than twice the measured worst case: re-measure it")


def test_the_float32_evaluation_passes_the_gpu_checker(evaluated):
    """The yardstick itself is within the tolerances the kernels are held to (a quarter of them, for the derived ones)."""
    for key in KEYS:
        ref, got, _ = evaluated(key)
        r = C.ratios(got, ref, key[4])
        assert max(r.values()) <= 1.0, (key, r)


# ------------------------------------------------------------------ plan mirror
def _gemm_ws(lib):
    lib, N = lib
    kinds = {"NT": N.TT_GEMM_NT, "NN": N.TT_GEMM_NN, "TN": N.TT_GEMM_TN}
    return lambda kind, m, n, k: lib.tt_gemm_workspace_bytes(kinds[kind], m, n, k)


NAMED_SHAPES = [(8192, 8192), (8192, 65536), (2048, 16384)]  # the shapes plan_ce's comments name


def test_plan_mirror_equals_the_library(lib):
    L, _ = lib
    gemm_ws = _gemm_ws(lib)
    shapes = sorted(set((c.M, c.N, c.D) for c in C.CASES)) + [(M, N, D) for M, N in NAMED_SHAPES for D in (32, 64, 128, 200)]
    for M, N, D in shapes:
        p = C.plan(M, N, D, gemm_ws=gemm_ws)
        assert p["ws"] == L.tt_inbatch_ce_workspace_bytes(M, N, D), (M, N, D)
        assert p["ws_bias"] == L.tt_inbatch_ce_bias_workspace_bytes(M, N, D), (M, N, D)
        assert p["logits_bytes"] == L.tt_inbatch_ce_logits_bytes(M, N), (M, N, D)


def test_plan_mirror_gives_the_split_plans_the_shapes_were_chosen_for():
    want = {(77, 203): ((1, [4]), (1, [2])), (130, 700): ((3, [4, 4, 3]), (1, [3])), (300, 300): ((2, [3, 2]), (2, [3, 2])),
            (321, 577): ((3, [4, 4, 2]), (2, [3, 3])), (385, 449): ((2, [4, 4]), (2, [4, 3])), (129, 1000): ((4, [4, 4, 4, 4]), (1, [3]))}
    for (M, N), ((su, tu), (si, ti)) in want.items():
        p = C.plan(M, N, 64)
        assert (p["user"][0], p["user"][2]) == (su, tu) and (p["item"][0], p["item"][2]) == (si, ti), (M, N, p)
    M, N, D, _ = C.TWO_CHUNK
    assert C.plan(M, N, D)["chunks"] == [128, 2]


# ------------------------------------------------------------------ coverage
def test_case_list_reaches_every_cell():
    missing = C.required_cells() - C.coverage(C.CASES)
    assert not missing, sorted(missing, key=str)
    assert len(set(C.case_id(c) for c in C.CASES)) == len(C.CASES)
    for c in C.CASES:
        assert 0 <= c.off and c.off + c.M <= c.N
        if c.entry not in C.BIAS_ENTRIES:
            assert c.bias == "none"
        if c.entry in C.KEEP_ENTRIES:  # the kept-logits pair is refused elsewhere
            p = C.case_plan(c)
            assert p["stage_fwd"] == "dma" and p["stage_di"] == "dma", c


# ------------------------------------------------------------------ mutants
def _strided_keys():
    return set(C.math_key(c) for c in C.CASES if c.lu != "dense" or c.li != "dense")


def _mutant_runs():
    strided = _strided_keys()
    runs = []
    for key in ALL_KEYS:
        pl = C.plan(*key[:3])
        for mut in C.MUTANTS:
            if C.applies(mut, key, pl) and (mut != "slack_read" or key in strided):
                runs.append((mut, key))
    return runs


def key3(k):
    return k[0], k[1], k[2]


def test_every_mutant_is_generated_wherever_it_can_differ():
    """The generated (mutant, key) set, pinned for all 16 mutants: the shape, plan and input conditions restated here, among
    the keys where some case compares a quantity the mutant stands for (ce_ref.watched), so that an edit of ce_ref.applies
    cannot drop cases unnoticed."""
    by = collections.defaultdict(set)
    for m, k in _mutant_runs():
        by[m].add(k)
    print({m: len(v) for m, v in by.items()})
    assert set(by) == set(C.MUTANTS)
    strided = _strided_keys()
    one_logit = ("slack_read", "bias_ln_units", "bias_fwd_only", "last_user_ignored")  # what can change p = 1's one logit

    def keys(mut, cond, heavy=False):
        return {k for k in ALL_KEYS if C.heavy(k) == heavy and C.watched(mut, k) and (k[1] > 1 or mut in one_logit) and cond(k)}

    ref = C.key_reference
    splits = lambda k: k[2] <= 128 and C.plan_ce(*key3(k))[1] > 1
    tps = lambda k: C.plan_ce(*key3(k))[2]
    assert by["ragged_tile_zero"] == keys("ragged_tile_zero", lambda k: k[1] % 64 and float(ref(k)["lse"].min()) < 11.5)
    assert {k[4] for k in by["ragged_tile_zero"]} >= {"flat", "shifted", "planted"}
    assert by["last_item_ignored"] == keys("last_item_ignored", lambda k: float(ref(k)["p_last"].max()) > 1e-3)
    assert by["last_user_ignored"] == keys("last_user_ignored", lambda k: True) | keys("last_user_ignored", lambda k: True, True)
    assert by["last_user_ignored"] == set(ALL_KEYS)
    assert by["no_diag_offset"] == keys("no_diag_offset", lambda k: k[3] != 0)
    assert by["diag_first_split"] == keys("diag_first_split", lambda k: splits(k) and k[3] + k[0] - 1 >= tps(k) * 64)
    assert by["no_max"] == keys("no_max", lambda k: k[4] == "shifted")
    assert by["merge_no_factor_lse"] == keys("merge_no_factor_lse", splits)
    assert by["merge_no_factor_du"] == keys("merge_no_factor_du", splits)
    assert by["bias_fwd_only"] == keys("bias_fwd_only", lambda k: k[5] != "none")
    assert by["bias_by_user_row"] == keys("bias_by_user_row", lambda k: k[5] != "none" and k[0] > 1)
    assert by["bias_ln_units"] == keys("bias_ln_units", lambda k: k[5] != "none")
    assert by["abs_coef"] == keys("abs_coef", lambda k: bool((C.inputs(k)[3] < 0).any()))
    assert by["zero_coef_neighbour"] == keys("zero_coef_neighbour", lambda k: k[0] >= 16)
    assert by["slack_read"] == keys("slack_read", lambda k: k in strided)
    assert by["chunk_overwrite_dI"] == keys("chunk_overwrite_dI", lambda k: True, True) and by["chunk_overwrite_dI"]
    assert by["chunk_diag_local"] == keys("chunk_diag_local", lambda k: True, True) and by["chunk_diag_local"]
    # every mutant is still run at the large majority of the keys whose shape allows it (the rest compare none of its quantities)
    for m in C.MUTANTS:
        unfiltered = {k for k in ALL_KEYS if C.MUTANTS[m](k, C.plan(*key3(k))) and (m in C.POSTHOC or not C.heavy(k))
                      and (k[1] > 1 or m in one_logit) and (m != "slack_read" or k in strided)}
        assert len(by[m]) >= 0.6 * len(unfiltered), (m, len(by[m]), len(unfiltered))


def _reject(mut, key, ref, base_memo):
    """-> (the watched quantity with the worst err / bound, {watched quantity: err / bound}).  Only the quantities that the
    mutant stands for AND that some case of the key compares on the GPU count."""
    U, I, b, coef, _ = C.inputs(key)
    got = C.evaluate(U, I, b, coef, key[3], C.F32, mut, C.plan(*key[:3]), memo=base_memo)
    r = C.ratios({q: got[q] for q in C.watched(mut, key)}, ref, key[4])
    return max(r, key=lambda q: r[q]), r


def test_mutants_are_rejected(evaluated):
    caught = collections.defaultdict(collections.Counter)
    for mut, key in _mutant_runs():
        if C.heavy(key):
            continue
        ref, _, memo = evaluated(key)
        q, r = _reject(mut, key, ref, memo)
        assert r[q] > 1.0, (mut, key, r)
        caught[mut][q] += 1
    for mut in C.MUTANTS:
        print(f"{mut:<22} {sum(caught[mut].values()):>3} cases, caught by " + ", ".join(f"{q} ({n})" for q, n in caught[mut].most_common()))


@pytest.mark.parametrize("key", HEAVY_KEYS, ids=str)
def test_two_chunk_mutants_are_rejected(key):
    """The two-chunk wide case: the POSTHOC mutants on the float64 reference rounded to float32 (see ce_ref.heavy), counted
    through the quantities its cases compare."""
    ref = C.key_reference(key)
    U, I, b, coef, _ = C.inputs(key)
    pl = C.plan(*key[:3])
    assert (coef[15::16] == 0).all() and (coef > 0).any() and (coef < 0).any()
    memo = {"base": {q: ref[q].float() for q in C.QUANTITIES}, "Sb": (ref["logits"] * C.LN2).float()}
    assert max(C.ratios(memo["base"], ref, key[4]).values()) <= 1.0
    ran = []
    for mut in C.POSTHOC:
        if not C.applies(mut, key, pl):
            continue
        q, r = _reject(mut, key, ref, memo)
        print(mut, {n: f"{v:.3g}" for n, v in r.items()})
        assert r[q] > 1.0, (mut, r)
        ran.append(mut)
    assert {"chunk_overwrite_dI", "chunk_diag_local", "last_user_ignored"} <= set(ran)


# ------------------------------------------------------------------ conditions
def test_the_input_classes_are_what_they_claim():
    seen = collections.Counter()
    for key in KEYS:
        M, N, D, off, cls, bias = key
        ref = C.key_reference(key)
        rows = torch.arange(M)
        U, I, b, coef, _ = C.inputs(key)
        assert (coef[15::16] == 0).all() and (M < 4 or ((coef > 0).any() and (coef < 0).any())), key
        if cls == "peaked":
            assert float((ref["p_max"] > 0.99).double().mean()) >= 0.9, key
        if cls == "shifted":
            assert float(ref["row_max"].abs().min()) > 60, key
            assert M < 2 or (float(ref["row_max"][0]) > 60 and float(ref["row_max"][1]) < -60)
        if cls == "planted":
            # 1 - p_pos without cancellation: the other columns' mass
            S = ref["logits"] * C.LN2
            others = S.clone()
            others[rows, rows + off] = -float("inf")
            one_minus = torch.exp(torch.logsumexp(others, dim=1) - ref["lse"]) if N > 1 else torch.zeros(M, dtype=C.F64)
            assert float(one_minus[rows % 4 == 0].max()) < 1e-6, key
            if M > 1:
                assert float(ref["p_pos"][rows % 4 == 1].max()) < 1e-12, key
        seen[cls] += 1
    assert all(seen[cls] > 0 for cls in C.CLASSES)
