"""tests/ce_hits_ref.py on the CPU: the float64 reference of the in-batch softmax with accidental hits masked, the key
patterns, the twin class's two conditions, the yardstick, the mutants through the GPU test's checker, and the interface
the feature adds (header, loader table, model arguments, command-line flag).  No GPU."""
import inspect
import os
import re

import pytest
import torch

import ce_hits_ref as H

C = H.C
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (M, N, off, D): the shapes at which the twin class's conditions are asserted
TWIN_SHAPES = ((77, 203, 126, 24), (77, 203, 126, 32), (130, 700, 200, 128), (300, 300, 0, 64), (129, 1000, 871, 128),
               (385, 449, 64, 40))


def test_patterns_are_what_they_are_chosen_for():
    for M, N, off in C.SHAPES:
        hit = {p: H.hit_matrix(H.keys(p, N), M, off) for p in H.PATTERNS}
        rows, pos = torch.arange(M), torch.arange(M) + off
        for p in H.PATTERNS:
            assert H.keys(p, N).dtype == torch.int32 and not bool(hit[p][rows, pos].any()), p  # the positive is never masked
        assert not bool(hit["none"].any())
        assert bool((hit["all_same"].sum(dim=1) == N - 1).all())
        assert bool((hit["pairs"].sum(dim=1) == 1).all()) or N % 2  # the partner, in the same register group of 4
        j = hit["pairs"].float().argmax(dim=1)
        assert bool(((j // 4 == pos // 4) | (hit["pairs"].sum(dim=1) == 0)).all())
        i, j = hit["stride64"].nonzero(as_tuple=True)
        assert bool(((j - pos[i]) % 64 == 0).all()) and bool(hit["stride64"].any())  # whole tiles away, same tile-local row
        i, j = hit["mod61"].nonzero(as_tuple=True)
        assert bool((j % 64 != pos[i] % 64).any())
        if off > 0:
            assert bool((j < off).any()), "mod61: a hit before diag_offset"
        if N > off + M:
            assert bool((j >= off + M).any()), "mod61: a hit among the extra negatives"
        tps = C.plan_ce(M, N, 64)[2] * 64
        if N > tps:
            assert bool((j // tps != pos[i] // tps).any()), "mod61: a hit in another split"
        free = float((hit["zipf"].sum(dim=1) == 0).float().mean())
        assert 0.15 <= free <= 0.35, (M, N, free)  # about a quarter of the rows has no hit


def test_cases_reach_every_form_width_staging_pattern_and_class():
    got = set()
    for c in H.CASES:
        st = H.staging_of(c)
        got |= {("form", c.entry), ("width", c.D), ("staging", st), ("pattern", c.pattern, c.cls), ("bias", c.entry, c.bias),
                ("shape", c.M, c.N, c.off), ("cell", c.entry, st), ("dp8", C.plan_ce(c.M, c.N, c.D) and C.plan_ce(c.M, c.N, c.D)[0]),
                ("stage_di", H.case_plan(c)["stage_di"]), ("layout_i", c.li), ("layout_u", c.lu)}
    need = {("form", e) for e in H.ENTRIES} | {("width", D) for D in H.WIDTHS} | {("staging", s) for s in ("dma", "reg", "gemm")}
    need |= {("pattern", p, cl) for p in H.PATTERNS for cl in H.CLASSES} | {("bias", e, b) for e in H.ENTRIES for b in ("none", "zipf")}
    need |= {("shape",) + s for s in H.SHAPES} | {("dp8", d) for d in (4, 8, 16, None)}
    need |= {("cell", e, s) for e in ("plain", "du", "loss") for s in ("dma", "reg", "gemm")} | {("cell", "keep", "dma")}
    need |= {("stage_di", s) for s in ("dma", "reg", "gemm")} | {("layout_i", l) for l in ("strided16", "misaligned", "odd_ld")}
    assert need <= got, sorted(need - got, key=str)
    assert all((c.cls, c.pattern) != ("flat", "x") and c.off + c.M <= c.N for c in H.CASES)


def test_reference_follows_the_semantics_element_by_element():
    """The float64 reference against loops over (i, j) written from the issue's formulas: small keys of both classes whose
    patterns have hits at N = 11 / 9, with and without a term."""
    for key in ((5, 11, 3, 4, "flat", "pairs", "zipf"), (5, 11, 3, 4, "flat", "zipf", "zipf"), (5, 11, 3, 6, "flat", "all_same", "none"),
                (6, 9, 4, 2, "twin", "pairs", "none"), (6, 9, 4, 3, "twin", "zipf", "zipf")):
        U, I, b, kv, coef, _ = H.inputs(key)
        M, N, D, off = key[:4]
        ref = H.reference(key)
        assert bool(ref["hit"].any())
        U, I = U.double(), I.double()
        dU, dI, ce = torch.zeros(M, D, dtype=H.F64), torch.zeros(N, D, dtype=H.F64), torch.zeros(M, dtype=H.F64)
        for i in range(M):
            s = [float(U[i] @ I[j]) + (float(b[j]) if b is not None else 0.0) for j in range(N)]
            keep = [j for j in range(N) if not (int(kv[j]) == int(kv[i + off]) and j != i + off)]
            assert [j for j in range(N) if not bool(ref["hit"][i, j])] == keep
            lse = torch.logsumexp(torch.tensor([s[j] for j in keep], dtype=H.F64), 0)
            ce[i] = lse - s[i + off]
            for j in keep:
                g = float(coef[i]) * (float(torch.exp(torch.tensor(s[j], dtype=H.F64) - lse)) - (1.0 if j == i + off else 0.0))
                dU[i] += g * I[j]
                dI[j] += g * U[i]
        for name, want in (("ce", ce), ("dU", dU), ("dI", dI)):
            assert torch.allclose(ref[name], want, rtol=1e-12, atol=1e-13), (key, name)
        assert bool((ref["logits"][ref["hit"]] == H.NEG_BIG).all())


def test_all_same_keys_leave_exact_zeros_in_float64():
    for key in [H.math_key(c) for c in H.CASES if c.pattern == "all_same"]:
        ref = H.key_reference(key)
        for q in ("ce", "du_unit", "dU", "dI"):
            assert float(ref[q].abs().max()) == 0.0, (key, q)


@pytest.mark.parametrize("shape", TWIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_twin_makes_every_hit_count(shape):
    """(a) at least 95 % of the rows that have a hit move by |ce_masked - ce_unmasked| >= 0.5; (b) leaving any single hit
    of a row unmasked moves that row's ce by more than 1000 x its bound.  On the float64 reference alone."""
    M, N, off, D = shape
    for pattern in ("pairs", "mod61", "zipf"):
        key = (M, N, D, off, "twin", pattern, "none")
        ref = H.reference(key)
        has = ref["hit"].any(dim=1)
        moved = (ref["ce"] - ref["ce_unmasked"]).abs() >= 0.5
        share = float(moved[has].float().mean())
        t = H.tol("twin", "ce", ref)
        bound = t[0] + t[1] * float(ref["ce"].abs().max()) + t[2] * ref["ce"].abs()
        # one more column j in row i's sum: ce_i grows by log(1 + exp(S'_ij - lse_i)); checked against reference(unmask=)
        U, I, b, kv, _, _ = H.inputs(key)
        S = U.double() @ I.double().t()
        step = torch.log1p(torch.exp(S - ref["lse"][:, None]))
        worst = float((step / bound[:, None])[ref["hit"]].min())
        i, j = [int(x[0]) for x in ref["hit"].nonzero(as_tuple=True)]
        one = H.reference(key, unmask=(i, j))
        assert abs(float(one["ce"][i] - ref["ce"][i]) - float(step[i, j])) <= 1e-9 * float(step[i, j]) + 1e-12
        print(f"CE_HITS twin {key}: (a) {100 * share:.1f} %  (b) {worst:.3g} x")
        assert share >= 0.95, (key, share)
        assert worst > 1000.0, (key, worst)


def test_yardstick_is_not_below_what_float32_gives():
    worst = H.measure()
    print("CE_HITS yardstick " + " ".join(f"{q}={worst[q][0]:.3e}" for q in H.QUANTITIES))
    for q in H.QUANTITIES:
        assert worst[q][0] <= H.YARD_TWIN[q], (q, worst[q])
        assert H.YARD_TWIN[q] <= 2.0 * max(worst[q][0], C.FLOOR), (q, "the recorded yardstick is stale")


def test_float32_evaluation_passes_and_every_mutant_fails_the_gpu_checker():
    """The index-order float32 evaluation of every key, flat and twin, through the checker of
    test_gpu_ce_hits_reference.py: as it is, within the bounds (twin: by the factor 4 of its yardstick); with a mutant,
    outside them wherever the mutant's mask differs from the true one in a compared quantity -- except at the pairs of
    ce_hits_ref.EXEMPT, which are accepted, each for the numerical reason written next to it."""
    seen = {(m, cls): 0 for m in H.MUTANTS for cls in H.CLASSES}
    accepted = set()
    for key in H.all_keys():
        U, I, b, kv, coef, _ = H.inputs(key)
        ref = H.key_reference(key)
        memo = {}
        got = H.evaluate(U, I, b, kv, coef, key[3], H.F32, None, memo)
        r = H.ratios({q: got[q] for q in H.key_compared(key)}, ref, key[4])
        assert max(r.values()) <= (1.0 / C.FACTOR + 1e-9 if key[4] == "twin" else 1.0), (key, r)
        for mut in H.MUTANTS:
            if not H.applies(mut, key):
                continue
            bad = H.evaluate(U, I, b, kv, coef, key[3], H.F32, mut, memo)
            rm = H.ratios({q: bad[q] for q in H.watched(mut, key)}, ref, key[4])
            if max(rm.values()) > 1.0:
                seen[(mut, key[4])] += 1
            else:
                accepted.add((mut, key))
    print("CE_HITS mutants rejected at " + " ".join(f"{m}/{c}={n}" for (m, c), n in seen.items()))
    assert accepted == H.EXEMPT, (sorted(accepted - H.EXEMPT, key=str), sorted(H.EXEMPT - accepted, key=str))
    assert all(n >= 3 for n in seen.values()), seen


# ------------------------------------------------------------------ the interface the feature adds
def test_header_loader_and_abi_version():
    from two_tower_models_amd import _native as N
    text = open(os.path.join(ROOT, "include", "tt_hotpath.h")).read()
    assert re.search(r"#define TT_ABI_VERSION 6\b", text)
    for name in ("tt_inbatch_ce_masked_workspace_bytes", "tt_inbatch_ce_masked_fwd", "tt_inbatch_ce_masked_bwd"):
        assert re.search(r"\b" + name + r"\(", text), name
        assert name in N.SIGNATURES, name
    assert "const int32_t* item_key /* [N], may be NULL */" in text
    # the masked calls are the _bias_ calls plus one pointer
    for kind in ("fwd", "bwd"):
        assert len(N.SIGNATURES[f"tt_inbatch_ce_masked_{kind}"][1]) == len(N.SIGNATURES[f"tt_inbatch_ce_bias_{kind}"][1]) + 1


def test_model_and_op_arguments_exist():
    """The new arguments are plain parameters of the methods and of the autograd forwards; only `user_history_lengths`
    still rides on a wrapper (`takes_history_lengths`)."""
    import two_tower_models_amd as A
    from two_tower_models_amd import ops
    own = lambda f: inspect.signature(f).parameters
    base = A.TwoTowerBaseRetrieval
    assert own(base.train_forward)["remove_accidental_hits"].default is False
    assert own(base.compute_training_loss)["item_id"].default is None
    assert own(ops.InBatchSoftmaxCE.forward)["item_key"].default is None
    assert own(ops.InBatchSoftmaxWeightedLoss.forward)["item_key"].default is None
    assert not hasattr(base.compute_training_loss, "__wrapped__") and not hasattr(ops.InBatchSoftmaxCE.forward, "__wrapped__")
    assert not hasattr(base.train_forward.__wrapped__, "__wrapped__")  # takes_history_lengths, and nothing inside it
    for cls in (A.TwoTowerWithUserHistoryEncoder, A.TwoTowerWithDebiasing, A.TwoTowerWithPositionDebiasedWeights,
                A.TwoTowerWithUserDebiasedWeights, A.TwoTowerPlusLightRanker):
        assert "remove_accidental_hits" in own(cls.train_forward), cls
    with pytest.raises(TypeError):
        ops.InBatchSoftmaxCE.forward(None, 1, 2, 3, 4, 5, 6, 7)


def test_remove_accidental_hits_is_bound_per_call_and_not_inherited():
    """train_forward hands the candidate block's ids to compute_training_loss exactly when THIS call asks for the mask: a
    call without the keyword, or with False, passes no `item_id`, whatever the call before it did."""
    import two_tower_models_amd as A
    from two_tower_models_amd import two_tower_base_retrieval as B
    seen = []
    u, v = torch.arange(24.0).reshape(3, 8), torch.ones(5, 8)

    class M(A.TwoTowerBaseRetrieval):
        def compute_user_embedding(self, user_id, user_features, user_history):
            return u

        def compute_item_embeddings(self, item_id, item_features):
            return v

        def compute_training_loss(self, user_embedding, item_embeddings, position, labels, **kw):
            assert user_embedding is u and item_embeddings is v
            seen.append(kw)
            return torch.zeros(())

    m = M(4, 10, 8, 4, 12, 8, 4, [1.0], A.BaselineMIPSModule(corpus_size=16, embedding_dim=8))
    z = torch.zeros(3, dtype=torch.int64)
    item_id, neg_id = torch.tensor([7, 3, 7]), torch.tensor([3, 11])
    batch = (z, torch.zeros(3, 4), torch.zeros(3, 6, dtype=torch.int64), item_id, torch.zeros(3, 4), z, torch.zeros(3, 1))
    neg = dict(negative_item_id=neg_id, negative_item_features=torch.zeros(2, 4))
    assert float(m.train_forward(*batch, **neg, remove_accidental_hits=True)) == 0.0
    assert list(seen[0]) == ["item_id"] and torch.equal(seen[0]["item_id"], torch.tensor([7, 3, 7, 3, 11]))
    m.train_forward(*batch, **neg)
    m.train_forward(*batch, **neg, remove_accidental_hits=False)
    assert seen[1:] == [{}, {}]
    m.train_forward(*batch, remove_accidental_hits=True)
    assert list(seen[3]) == ["item_id"] and seen[3]["item_id"] is item_id
    for name in ("_REMOVE_HITS", "_HIT_ITEM_ID", "takes_item_id", "takes_remove_accidental_hits"):
        assert not hasattr(B, name), name


def test_item_key_is_validated_before_any_device_work():
    from two_tower_models_amd import ops
    I = torch.zeros(4, 8)
    assert ops._item_key(None, I, "x") is None
    with pytest.raises(TypeError):
        ops._item_key(torch.zeros(4), I, "x")
    with pytest.raises(TypeError):
        ops._item_key([1, 2, 3, 4], I, "x")
    with pytest.raises(ValueError):
        ops._item_key(torch.zeros(5, dtype=torch.int64), I, "x")
    with pytest.raises(ValueError):
        ops._item_key(torch.zeros(4, 1, dtype=torch.int32), I, "x")
    with pytest.raises(RuntimeError):
        ops._item_key(torch.zeros(4, dtype=torch.int32, device="meta"), I, "x")
    k = ops._item_key(torch.tensor([1, 2, 2 ** 31 - 1, 0]), I, "x")
    assert k.dtype == torch.int32 and k.tolist() == [1, 2, 2 ** 31 - 1, 0]


def test_hash_size_beyond_32_bits_is_refused_before_any_device_work():
    import two_tower_models_amd as A
    mips = A.BaselineMIPSModule(corpus_size=16, embedding_dim=8)
    m = A.TwoTowerBaseRetrieval(4, 10, 8, 4, 12, 8, 4, [1.0], mips)
    m.item_id_embedding_arch.num_embeddings = 2 ** 31 + 1  # (a table of that size cannot be allocated here)
    z = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="32-bit"):
        m.train_forward(z, torch.zeros(3, 4), torch.zeros(3, 6, dtype=torch.int64), z, torch.zeros(3, 4), z, torch.zeros(3, 1),
                        remove_accidental_hits=True)


def test_command_line_flag_is_refused_with_row_sharding():
    from two_tower_models_amd import train
    args = train.build_parser().parse_args(["--remove_accidental_hits", "--world_size", "2"])
    assert args.remove_accidental_hits is True
    assert train.build_parser().parse_args([]).remove_accidental_hits is False
    text = inspect.getsource(train.main)
    assert "--remove_accidental_hits is not implemented with --world_size > 1" in text
