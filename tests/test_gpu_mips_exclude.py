"""MIPS exclusion on the GPU: tt_mips_exclude at the C ABI against the integer reference (exact equality, scores by bit
pattern), BaselineMIPSModule.search / forward with `exclude` against the float64 masked top-K on exact-arithmetic corpora,
the models' `exclude_history` / `exclude_item_id` keywords, and the row-sharded module (two gloo ranks on one device)."""
import os
import tempfile

import numpy as np
import pytest
import torch

import fixture_gen as fg
import mips_exclude_ref as XR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def lib_and_native():
    from two_tower_models_amd import _native as N
    return N.load(), N


# ------------------------------------------------------------------ 1. the kernel at the C ABI
SENT_IDX, SENT_BITS = -7, 0x7FC00ABC  # what the outputs hold before the call: neither can come out of the filter
KINDS = ("none", "absent", "pad", "dup", "exact_k", "k_minus_1", "all", "oob", "upper32")
ROWS = 5000  # corpus rows of the mapped cases: [0, 1000) may be excluded, [1000, 4000) never are, [4000, 5000) are never candidates
SPECIAL = np.array([0x80000000, 0x00000000, 0x7FC00123, 0x7F800000, 0xFF800000, 0x00000001], dtype=np.uint32)


def make_keys(mapped, rng):
    """(row_key or None, C): a permutation of the rows with bits 32..34 in use, or no map and 2^40 rows."""
    if not mapped:
        return None, 1 << 40
    return rng.permutation(ROWS).astype(np.int64) + ((np.arange(ROWS, dtype=np.int64) % 5) << 32), ROWS


def make_row(kind, n, K, E, row_key, C, rng):
    """One query: (idx [n], exclude [E], survivors expected).  Candidates may repeat a row: the filter does not care."""
    key = (lambda r: r) if row_key is None else (lambda r: row_key[r])
    pool = rng.choice(1000, min(E, 40), replace=False).astype(np.int64)
    s = {"none": n, "absent": n, "pad": n, "exact_k": K, "k_minus_1": K - 1, "all": 0}.get(kind)
    if s is None:
        s = int(rng.integers(0, n + 1))
    live = np.zeros(n, dtype=bool)
    live[rng.choice(n, s, replace=False)] = True
    rows_live = rng.integers(1000, 4000, n).astype(np.int64)
    if kind == "upper32" and row_key is None:  # an index that differs from an excluded one only above bit 31: kept
        rows_live[::2] = pool[rng.integers(0, len(pool), len(rows_live[::2]))] + (1 << 33)
    idx = np.where(live, rows_live, pool[rng.integers(0, len(pool), n)])
    if kind == "oob":  # -1 and C among the excluded AND the surviving positions: dropped, never read through row_key
        out = rng.random(n) < 0.3
        idx[out] = np.where(rng.random(int(out.sum())) < 0.5, -1, C)
        live &= ~out
    bites = kind not in ("none", "absent", "pad")
    ex = list(key(pool)) if bites else []
    absent = lambda m: list(key(rng.integers(4000, 5000, m).astype(np.int64)))  # noqa: E731
    decoys = lambda m: list(key(rows_live[rng.integers(0, n, m)]) ^ (1 << 35))  # noqa: E731 -- differ only above bit 31
    room = E - len(ex)
    if kind == "pad":
        ex += [-1] * room
    elif kind == "absent":
        ex += absent(room)
    elif kind == "dup":
        ex += [ex[int(j)] for j in rng.integers(0, len(ex), room)]
    elif kind == "upper32":
        ex += decoys(room)
    else:
        a, b = room // 3, room // 3
        ex += absent(a) + decoys(b) + [-(1 + int(j)) for j in rng.integers(0, 9, room - a - b)]
    ex = np.array(ex, dtype=np.int64)
    rng.shuffle(ex)
    return idx, ex, int(live.sum())


def make_case(B, n, K, E, mapped, shift, seed):
    rng = np.random.default_rng(seed)
    row_key, C = make_keys(mapped, rng)
    rows = [make_row(KINDS[(b + shift) % len(KINDS)], n, K, E, row_key, C, rng) for b in range(B)]
    idx, ex = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    sc = rng.standard_normal((B, n)).astype(np.float32)
    odd = rng.random((B, n)) < 0.05  # -0.0, NaN with a payload, infinities, a denormal: copied like any other bits
    sc.view(np.uint32)[odd] = SPECIAL[rng.integers(0, len(SPECIAL), int(odd.sum()))]
    return idx, sc, ex, row_key, C, np.array([r[2] for r in rows])


def run_exclude(idx, sc, K, ex, row_key, C, expect_rc=0, null=()):
    """One tt_mips_exclude call on sentinel-filled outputs -> (rc, idx_out, score bits, flag) on the CPU."""
    lib, N = lib_and_native()
    B, n = idx.shape
    t = {"idx": T(idx).to(DEV), "sc": T(sc).to(DEV), "ex": T(ex).to(DEV),
         "oi": torch.full((B, max(K, 1)), SENT_IDX, dtype=torch.int64, device=DEV),
         "os": torch.full((B, max(K, 1)), SENT_BITS, dtype=torch.int32, device=DEV),
         "flag": torch.zeros(1, dtype=torch.int32, device=DEV)}
    key = None if row_key is None else T(row_key).to(DEV)
    p = {k: (None if k in null else v.data_ptr()) for k, v in t.items()}
    rc = lib.tt_mips_exclude(p["idx"], p["sc"], B, n, K, p["ex"], ex.shape[1], N.ptr(key), C, p["oi"], p["os"], p["flag"],
                             N.stream())
    torch.cuda.synchronize()
    assert (rc == 0) == (expect_rc == 0), (rc, lib.tt_last_error_string())
    return rc, t["oi"].cpu().numpy(), t["os"].cpu().numpy().view(np.uint32), int(t["flag"].item())


def check_case(B, n, K, E, mapped, shift, seed):
    idx, sc, ex, row_key, C, survivors = make_case(B, n, K, E, mapped, shift, seed)
    want_i, want_s, short = XR.filter_candidates(idx, sc, K, ex, row_key, C)
    assert np.array_equal(short, survivors < K)  # the case is what it was built to be
    _, got_i, got_bits, flag = run_exclude(idx, sc, K, ex, row_key, C)
    assert not (got_i == SENT_IDX).any() and not (got_bits == SENT_BITS).any()  # every slot written
    assert np.array_equal(got_i, want_i), (B, n, K, E, mapped, np.nonzero((got_i != want_i).any(axis=1))[0][:5])
    assert np.array_equal(got_bits, XR.bits(want_s))
    assert flag == int(short.any())
    return short


@pytest.mark.parametrize("E", [1, 50, 64, 65, 1000, 4096])
@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 300, 1100])
def test_kernel_equals_the_integer_reference(n_cand, E):
    """n_cand crosses the 64-lane tile and the 256-thread workgroup, E both membership forms (list up to 64, hash set
    above); B = 1, 3, 1100; row_key NULL and a permutation.  The rows of a batch cycle through KINDS: nothing excluded,
    every exclusion absent, all -1, duplicated exclusions, exactly K survivors (flag 0), K - 1 (flag 1, tail -1 / -inf), every
    candidate excluded, candidates -1 and C, keys that differ only in the upper 32 bits."""
    seen_short = seen_full = False
    ks = sorted({1, max(1, 2 * n_cand // 3), n_cand})
    for mapped in (False, True):
        for B in (1, 3, 1100):
            for j, K in enumerate(ks if B < 1100 else ks[len(ks) // 2:len(ks) // 2 + 1]):
                for shift in (range(0, len(KINDS), B) if B < 1100 else (0,)):
                    short = check_case(B, n_cand, K, E, mapped, shift, seed=7 * n_cand + E + 13 * B + j + 100 * shift)
                    seen_short |= bool(short.any())
                    seen_full |= bool((~short).all())
    assert seen_short and seen_full


def test_kernel_flag_stays_zero_when_exactly_k_survive():
    """A whole batch of `exact_k` rows: no tail, the flag untouched; one `k_minus_1` row among them sets it."""
    for E, mapped in ((50, True), (1000, False)):
        rng = np.random.default_rng(E)
        row_key, C = make_keys(mapped, rng)
        n, K = 300, 200
        rows = [make_row("exact_k", n, K, E, row_key, C, rng) for _ in range(5)]
        idx, ex = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
        sc = rng.standard_normal((5, n)).astype(np.float32)
        _, got_i, _, flag = run_exclude(idx, sc, K, ex, row_key, C)
        assert flag == 0 and (got_i >= 0).all()
        idx[3], ex[3], _ = make_row("k_minus_1", n, K, E, row_key, C, rng)
        _, got_i, got_bits, flag = run_exclude(idx, sc, K, ex, row_key, C)
        assert flag == 1 and got_i[3, -1] == -1 and got_bits[3, -1] == 0xFF800000 and (got_i[3, :-1] >= 0).all()
        assert (np.delete(got_i, 3, axis=0) >= 0).all()


def test_kernel_bad_arguments_leave_the_outputs_untouched():
    rng = np.random.default_rng(3)
    B, n, K, E = 3, 60, 10, 50
    idx, sc = rng.integers(0, 100, (B, n)).astype(np.int64), rng.standard_normal((B, n)).astype(np.float32)
    ex = rng.integers(0, 100, (B, E)).astype(np.int64)
    _, N = lib_and_native()

    def refused(K=K, ex=ex, C=100, idx=idx, sc=sc, null=()):
        rc, oi, ob, flag = run_exclude(idx, sc, K, ex, None, C, expect_rc=N.TT_E_BADARG, null=null)
        assert rc == N.TT_E_BADARG and (oi == SENT_IDX).all() and (ob == SENT_BITS).all() and flag == 0

    refused(K=0)
    refused(K=n + 1)
    refused(K=-1)
    refused(ex=ex[:, :0])  # E = 0
    refused(ex=np.zeros((B, 4097), dtype=np.int64))
    refused(C=0)
    refused(idx=idx[:, :0], sc=sc[:, :0], K=1)  # n_cand = 0
    for name in ("idx", "sc", "ex", "oi", "os", "flag"):
        refused(null=(name,))
    lib, _ = lib_and_native()
    x = torch.zeros(8, dtype=torch.int64, device=DEV).data_ptr()  # n_cand = 2^31: refused by size, nothing is read
    assert lib.tt_mips_exclude(x, x, 1, 1 << 31, 1, x, 1, None, 1, x, x, x, N.stream()) == N.TT_E_BADARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. the module, bit-exact
_exact = {}


def exact_case(C=4096, D=128, B=40, E=50):
    """Shared by the module tests (leave unchanged): fixture_gen's exact corpus / queries -- distinct, exactly representable
    scores --, the float64 scores, and per query an exclusion list of every other row of its own unmasked top-E plus
    random rows: the exclusions bite, differently per query."""
    k = (C, D, B, E)
    if k not in _exact:
        corpus, q = fg.exact_mips_corpus(C, D), fg.exact_mips_queries(B, D)
        s64 = q.astype(np.float64) @ corpus.astype(np.float64).T
        top = XR.ordered_topk(s64, E)[0]
        rng = np.random.default_rng(17)
        ex = np.concatenate([top[:, ::2], rng.integers(0, C, (B, E - top[:, ::2].shape[1]))], axis=1).astype(np.int64)
        ex = ex[:, rng.permutation(E)]
        _exact[k] = {"corpus": corpus, "q": q, "s64": s64, "ex": ex}
    return _exact[k]


def module_of(corpus, how):
    import two_tower_models_amd as A
    m = A.BaselineMIPSModule(corpus.shape[0], corpus.shape[1])
    m.set_corpus(T(corpus).to(DEV), bf16=(how == "bf16"))
    if how == "split16":
        m.use_split_fp16_scoring()
    return m


@pytest.mark.parametrize("how,K", [("fp32", 10), ("fp32", 1000), ("bf16", 10), ("bf16", 1000), ("split16", 10)])
def test_module_search_and_forward_equal_the_masked_float64_topk(how, K):
    d = exact_case()
    m = module_of(d["corpus"], how)
    q, ex = T(d["q"]).to(DEV), T(d["ex"]).to(DEV)
    want_i, want_s, short = XR.masked_topk(d["s64"], K, d["ex"])
    assert not short.any()
    plain_i = XR.ordered_topk(d["s64"], K)[0]
    assert (plain_i != want_i).any(axis=1).all()  # the exclusions bite for every query
    idx, sc = m.search(q, K, ex)
    assert idx.dtype == torch.int64 and sc.dtype == torch.float32
    assert np.array_equal(idx.cpu().numpy(), want_i)
    assert np.array_equal(sc.cpu().numpy().astype(np.float64), want_s)
    fi, fs, rows = m(query_embedding=q, num_items=K, exclude=ex)
    assert torch.equal(fi, idx) and torch.equal(fs, sc)
    assert rows.dtype == torch.float32 and torch.equal(rows.cpu(), T(d["corpus"])[idx.cpu()])
    # exclude=None: what search returns today
    from two_tower_models_amd import ops
    ni, ns = m.search(q, K)
    assert np.array_equal(ni.cpu().numpy(), plain_i)
    if how != "split16":
        oi, os_ = ops.mips_topk(q, m.corpus, K)
        assert torch.equal(ni, oi) and torch.equal(ns, os_)


def test_module_through_a_row_item_id_map():
    """Keys are item ids: the same search, the exclusion list translated through a permutation with ids above 2^32."""
    d = exact_case()
    m = module_of(d["corpus"], "fp32")
    C = d["corpus"].shape[0]
    item_of_row = np.random.default_rng(4).permutation(C).astype(np.int64) + (np.int64(1) << 40)
    m.row_item_id = T(item_of_row).to(DEV)
    K = 10
    ex_items = item_of_row[d["ex"]]
    want_i, want_s, _ = XR.masked_topk(d["s64"], K, d["ex"])
    idx, sc = m.search(T(d["q"]).to(DEV), K, T(ex_items).to(DEV))
    assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(sc.cpu().numpy().astype(np.float64), want_s)
    # row NUMBERS are not keys any more, and the low 32 bits of an id are not the id
    for other in (d["ex"], ex_items & 0xFFFFFFFF):
        idx, _ = m.search(T(d["q"]).to(DEV), K, T(other).to(DEV))
        assert np.array_equal(idx.cpu().numpy(), XR.ordered_topk(d["s64"], K)[0])


def test_module_all_equal_scores_return_the_lowest_surviving_indices():
    C, D, B, K = 700, 128, 5, 10
    m = module_of(np.ones((C, D), dtype=np.float32), "fp32")
    ex = np.full((B, 6), -1, dtype=np.int64)
    ex[1, :4] = [0, 1, 2, 5]
    ex[2, :] = [9, 9, 3, 3, 699, 11]
    ex[3, :] = np.arange(6)
    idx, sc = m.search(torch.ones(B, D, device=DEV), K, T(ex).to(DEV))
    for b in range(B):
        S = XR.exclusion_set(ex[b])
        assert idx[b].tolist() == [r for r in range(C) if r not in S][:K]
    assert (sc == float(D)).all()


def test_module_clamp_to_the_corpus_size():
    """C = 129, K = 120, E = 20: the search is clamped to 129 candidates.  5 effective exclusions leave 124 rows: fine;
    15 leave 114 < K: `selected index k out of range`."""
    C, D, B, K, E = 129, 128, 4, 120, 20
    corpus, q = fg.exact_mips_corpus(C, D), fg.exact_mips_queries(B, D)
    s64 = q.astype(np.float64) @ corpus.astype(np.float64).T
    m = module_of(corpus, "fp32")
    rng = np.random.default_rng(2)
    ex = np.full((B, E), -1, dtype=np.int64)
    for b in range(B):
        ex[b, rng.choice(E, 5, replace=False)] = rng.choice(C, 5, replace=False)
    idx, sc = m.search(T(q).to(DEV), K, T(ex).to(DEV))
    want_i, want_s, short = XR.masked_topk(s64, K, ex)
    assert not short.any() and np.array_equal(idx.cpu().numpy(), want_i)
    assert np.array_equal(sc.cpu().numpy().astype(np.float64), want_s)
    ex[2, :15] = rng.choice(C, 15, replace=False)
    for call in (lambda: m.search(T(q).to(DEV), K, T(ex).to(DEV)), lambda: m(T(q).to(DEV), K, T(ex).to(DEV))):
        with pytest.raises(RuntimeError, match="selected index k out of range"):
            call()
    idx, _ = m.search(T(q).to(DEV), K, T(ex[[0, 1, 3, 0]]).to(DEV))
    assert (idx >= 0).all()  # the flag of the refused call does not leak into the next one


# ------------------------------------------------------------------ 3. the models
def identity_model(cls_name, C, D, n_users, H, K, **extra):
    """The identity-tower trick of test_gpu_parallel._serve_model on BOTH towers: user tower = the user table's row, item
    tower = the item table's row (x * 1 + 0 * anything), the tables = fixture_gen's exact queries / corpus.  forward()'s
    queries and index_corpus()'s rows are then exact, and the top-K has one right answer."""
    import two_tower_models_amd as A
    torch.manual_seed(0)
    mips = A.BaselineMIPSModule(corpus_size=C, embedding_dim=D)
    model = getattr(A, cls_name)(num_items=K, user_id_hash_size=n_users, user_id_embedding_dim=D, user_features_size=8,
                                 user_history_seqlen=H, item_id_hash_size=C, item_id_embedding_dim=D, item_features_size=8,
                                 user_value_weights=[1.0], mips_module=mips, **extra)
    queries, table = T(fg.exact_mips_queries(n_users, D)), T(fg.exact_mips_corpus(C, D))
    sd = model.state_dict()
    sd["user_id_embedding_arch.weight"], sd["item_id_embedding_arch.weight"] = queries, table
    for name in ("user_tower_arch", "item_tower_arch"):
        w = torch.zeros_like(sd[name + ".weight"])
        w[:, :D] = torch.eye(D)
        sd[name + ".weight"], sd[name + ".bias"] = w, torch.zeros(D)
    model.load_state_dict(sd)
    return model.to(DEV), queries, table


def biting_history(s64, row_item, H, rng, n_top=3):
    """[B, H] item ids: n_top of each user's best rows (as item ids) and random items, shuffled."""
    B, C = s64.shape
    top = XR.ordered_topk(s64, 8)[0]
    hist = rng.integers(0, C, (B, H)).astype(np.int64)
    for b in range(B):
        hist[b, rng.choice(H, n_top, replace=False)] = row_item[top[b, rng.choice(8, n_top, replace=False)]]
    return hist


@pytest.mark.parametrize("catalogue", ["identity", "permuted"])
def test_history_model_excludes_the_history(catalogue):
    C, D, n_users, H, K, B = 1000, 128, 64, 6, 20, 16
    model, queries, table = identity_model("TwoTowerWithUserHistoryEncoder", C, D, n_users, H, K)
    rng = np.random.default_rng(11)
    item_id = np.arange(C, dtype=np.int64) if catalogue == "identity" else rng.permutation(C).astype(np.int64)
    model.index_corpus(T(item_id).to(DEV), torch.randn(C, 8, device=DEV))
    mips = model.mips_module
    assert torch.equal(mips.corpus.cpu(), table[T(item_id)])  # the identity item tower: rows are the table's, exactly
    if catalogue == "identity":
        assert mips.row_item_id is None
    else:
        assert torch.equal(mips.row_item_id.cpu(), T(item_id)) and mips.row_item_id.is_cuda
    uid = rng.integers(0, n_users, B)
    s64 = queries[T(uid)].double().numpy() @ table[T(item_id)].double().numpy().T  # [B, rows]
    hist = biting_history(s64, item_id, H, rng)
    batch = (T(uid).to(DEV), torch.randn(B, 8, device=DEV), T(hist).to(DEV))
    want, _, short = XR.masked_topk(s64, K, hist, item_id)
    assert not short.any() and (want != XR.ordered_topk(s64, K)[0]).any(axis=1).all()
    top = model(*batch, exclude_history=True)
    assert top.dtype == torch.int64 and np.array_equal(top.cpu().numpy(), want)
    for b in range(B):  # no returned row holds an item of the user's history
        assert not (set(item_id[top[b].cpu().numpy()].tolist()) & set(hist[b].tolist()))
    assert np.array_equal(model(*batch).cpu().numpy(), XR.ordered_topk(s64, K)[0])  # the default is untouched
    # the caller's own list, alone and on top of the history
    own = np.full((B, 9), -1, dtype=np.int64)
    own[:, :5] = item_id[XR.ordered_topk(s64, 12)[0][:, 7:12]]
    own[3, :] = -1
    got = model(*batch, exclude_item_id=T(own).to(DEV))
    assert np.array_equal(got.cpu().numpy(), XR.masked_topk(s64, K, own, item_id)[0])
    got = model(*batch, exclude_history=True, exclude_item_id=T(own).to(DEV))
    assert np.array_equal(got.cpu().numpy(), XR.masked_topk(s64, K, np.concatenate([hist, own], axis=1), item_id)[0])


def test_history_lengths_padding_id_zero_never_excludes_item_zero():
    """Item 0 is planted as the certain winner of one user, who appears twice in the batch: once with item 0 only in the
    PADDED slots of its history (id 0 is the documented pad) -- item 0 is returned, first --, once with item 0 inside the
    valid prefix -- item 0 is not returned."""
    C, D, n_users, H, K, B = 1000, 128, 64, 6, 20, 8
    model, queries, table = identity_model("TwoTowerWithUserHistoryEncoder", C, D, n_users, H, K)
    rng = np.random.default_rng(12)
    uid = rng.integers(0, n_users, B)
    uid[1] = uid[0]
    best = int(np.argmax(queries[int(uid[0])].double().numpy() @ table[1:].double().numpy().T)) + 1
    table = table.clone()
    table[0] = 2.0 * table[best]  # exact, and above every other score of that user (its best score is positive)
    with torch.no_grad():
        model.item_id_embedding_arch.weight.copy_(table.to(DEV))
    model.index_corpus(torch.arange(C, device=DEV), torch.randn(C, 8, device=DEV))
    assert model.mips_module.row_item_id is None and torch.equal(model.mips_module.corpus.cpu(), table)
    s64 = queries[T(uid)].double().numpy() @ table.double().numpy().T
    assert s64[0, best] > 0 and int(np.argmax(s64[0])) == 0
    hist = rng.integers(1, C, (B, H)).astype(np.int64)
    lengths = rng.integers(1, H + 1, B).astype(np.int64)
    lengths[0] = lengths[1] = 2
    hist[0, 2:] = 0  # padding
    hist[1, 0], hist[1, 2:] = 0, 0  # item 0 in the valid prefix (and in the padding)
    for b in range(2, B):
        hist[b, lengths[b]:] = 0
    masked = np.where(np.arange(H)[None, :] < lengths[:, None], hist, -1)
    want = XR.masked_topk(s64, K, masked)[0]
    batch = (T(uid).to(DEV), torch.randn(B, 8, device=DEV), T(hist).to(DEV))
    top = model(*batch, exclude_history=True, user_history_lengths=T(lengths).to(DEV)).cpu().numpy()
    assert np.array_equal(top, want)
    assert top[0, 0] == 0 and 0 not in top[1].tolist()
    # without the lengths every slot counts: item 0 goes for both
    top = model(*batch, exclude_history=True).cpu().numpy()
    assert np.array_equal(top, XR.masked_topk(s64, K, hist)[0]) and 0 not in top[0].tolist()


@pytest.mark.parametrize("NU", [4, 33])
def test_light_ranker_reranks_the_filtered_candidates(NU):
    """NU = 4: the fused rerank kernel; NU = 33 (outside its sizes): the module's own `_rerank_reference` IS the path.
    Either way forward(exclude_history=True) is that rerank run on the candidates BaselineMIPSModule.search returns with the
    history excluded -- and no history item comes back."""
    import two_tower_models_amd as A
    from two_tower_models_amd import ops
    C, D, n_users, H, K, NI, B = 2000, 128, 50, 6, 10, 40, 12
    torch.manual_seed(1)
    mips = A.BaselineMIPSModule(corpus_size=C, embedding_dim=D)
    model = A.TwoTowerPlusLightRanker(num_items=K, num_mips_items=NI, num_ranker_user_embeddings=NU, user_id_hash_size=n_users,
                                      user_id_embedding_dim=D, user_features_size=8, user_history_seqlen=H,
                                      item_id_hash_size=C, item_id_embedding_dim=D, item_features_size=8,
                                      user_value_weights=[1.0, 0.5], mips_module=mips).to(DEV)
    g = torch.Generator().manual_seed(5)
    uid, uf = torch.randint(0, n_users, (B,), generator=g).to(DEV), torch.randn(B, 8, generator=g).to(DEV)
    hist = torch.randint(0, C, (B, H), generator=g).to(DEV)
    with torch.no_grad():
        u, R = model.compute_user_embedding(uid, uf, hist)
        plain_idx, _ = mips.search(u, NI)
        hist[:, :3] = plain_idx[:, [0, 5, 17]]  # (the user embedding moves with the history: the list is rebuilt below)
        u, R = model.compute_user_embedding(uid, uf, hist)
        idx, sc = mips.search(u, NI, hist)
        assert not (idx.unsqueeze(2) == hist.unsqueeze(1)).any()
        if NU == 4:
            lin = model.light_ranker
            want = ops.light_ranker_rerank(R, lin.weight, lin.bias, model.user_value_weights, idx, sc, K, corpus=mips.corpus)
        else:
            want = model._rerank_reference(R, ops.gather_corpus_rows(mips.corpus, idx), sc, idx)
    top = model(uid, uf, hist, exclude_history=True)
    assert top.shape == (B, K) and torch.equal(top, want)
    assert not (top.unsqueeze(2) == hist.unsqueeze(1)).any()
    plain = model(uid, uf, hist)
    assert (plain.unsqueeze(2) == hist.unsqueeze(1)).any() or not torch.equal(plain, top)


# ------------------------------------------------------------------ 4. row-sharded
def _sharded_worker(rank, world, port, outdir, C, K, D):
    import test_gpu_parallel as P
    P._paths()
    import torch.distributed as dist
    from two_tower_models_amd import parallel
    dev = P.init_pg("gloo", rank, world, port)
    try:
        n_users, B, E2 = 64, 6, 46
        model, queries = P._serve_model(C, D, n_users, "born", dev)
        m = model.mips_module
        corpus = P._serve_corpus(C, D)
        _, lo, hi = parallel.block_range(C, rank, world)
        m.set_corpus(corpus[lo:hi].to(dev))
        assert m.is_sharded() and m.corpus_size == C and m.row_item_id is None
        model.num_items = K
        g = torch.Generator().manual_seed(200 + rank)
        uid = torch.randint(0, n_users, (B,), generator=g)
        hist = torch.randint(0, 50, (B, 4), generator=g)
        s64 = queries[uid].double().numpy() @ corpus.double().numpy().T
        own = XR.ordered_topk(s64, 2 * E2)[0][:, ::2].astype(np.int64)  # every other row of the user's own top 92
        batch = (uid.to(dev), torch.randn(B, 8, generator=g).to(dev), hist.to(dev))
        plain = model(*batch)
        tags_plain = dict(parallel.comm_bytes)
        top = model(*batch, exclude_history=True, exclude_item_id=torch.from_numpy(own).to(dev))
        comm = dict(parallel.comm_bytes)
        with torch.no_grad():
            q = model.compute_user_embedding(*batch)
            ex = torch.cat([hist, torch.from_numpy(own)], dim=1).to(dev)
            idx, sc, rows = m(query_embedding=q, num_items=K, exclude=ex)
        torch.save({"uid": uid, "hist": hist, "own": own, "plain": plain.cpu(), "top": top.cpu(), "idx": idx.cpu(),
                    "sc": sc.cpu(), "rows": rows.cpu(), "comm": comm, "tags_plain": tags_plain},
                   os.path.join(outdir, f"excl{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_sharded_model_excludes_on_global_row_numbers():
    """W = 2 (gloo, both ranks on cuda:0), C = 9000, K = 100, E = 4 + 46: the row-sharded TwoTowerWithDebiasing.forward
    with both exclusion keywords equals the float64 masked top-K over the WHOLE corpus on every rank, bit for bit; the list
    exchange is sized for K + E and no exchange is added."""
    import torch.multiprocessing as mp
    import test_gpu_parallel as P
    from two_tower_models_amd import parallel
    world, C, K, D, B, E = 2, 9000, 100, 128, 6, 50
    outdir = tempfile.mkdtemp()
    mp.spawn(_sharded_worker, args=(world, P._free_port(), outdir, C, K, D), nprocs=world, join=True)
    corpus = P._serve_corpus(C, D)
    queries = T(fg.exact_mips_queries(64, D))
    for r in range(world):
        got = torch.load(os.path.join(outdir, f"excl{r}.pt"), weights_only=False)
        s64 = queries[got["uid"]].double().numpy() @ corpus.double().numpy().T
        ex = np.concatenate([got["hist"].numpy(), got["own"]], axis=1)
        want_i, want_s, short = XR.masked_topk(s64, K, ex)
        assert not short.any()
        assert np.array_equal(got["plain"].numpy(), XR.ordered_topk(s64, K)[0])
        assert np.array_equal(got["top"].numpy(), want_i) and (want_i != got["plain"].numpy()).any(axis=1).all()
        assert np.array_equal(got["idx"].numpy(), want_i)
        assert np.array_equal(got["sc"].numpy().astype(np.float64), want_s)
        assert torch.equal(got["rows"], corpus[got["idx"]])  # fetched from their owners after the filter
        assert set(got["comm"]) == set(got["tags_plain"]) == {"mips_queries_allgather", "mips_lists_alltoall"}
        assert got["comm"]["mips_lists_alltoall"] == (world - 1) * B * 12 * parallel.first_try_k(K + E, world)
        assert got["tags_plain"]["mips_lists_alltoall"] == (world - 1) * B * 12 * parallel.first_try_k(K, world)
