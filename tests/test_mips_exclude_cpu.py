"""CPU-side checks of MIPS exclusion: the lemma on the integer reference alone, the refusals that come before any kernel,
the public keywords, the train.py flag and the `row_item_id` bookkeeping."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mips_exclude_ref as XR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the lemma, on the reference alone
def _scores(kind, B, C, rng):
    if kind == "random":
        return rng.standard_normal((B, C)).astype(np.float32)
    if kind == "ties":  # few distinct scores: the index order decides nearly everything
        return rng.integers(0, 3, (B, C)).astype(np.float32)
    return np.full((B, C), 0.25, dtype=np.float32)  # all equal


def _exclusions(B, C, E, rng):
    """[B, E]: row numbers of the corpus, absent ones (>= C), duplicates and -1 padding, a different mix per query."""
    ex = rng.integers(0, C + 10, (B, E)).astype(np.int64)
    ex[0, :] = -1  # nothing excluded
    if B > 1:
        ex[1, :] = ex[1, 0]  # one key, E times
    if B > 2:
        ex[2, :] = np.arange(C, C + E)  # every exclusion absent from the corpus
    if B > 3 and E > 1:
        ex[3, ::2] = -1
    return ex


@pytest.mark.parametrize("kind", ["random", "ties", "equal"])
@pytest.mark.parametrize("C", [5, 129, 1000])
@pytest.mark.parametrize("E", [1, 5, 50])
def test_lemma_filter_of_topk_k_plus_e_is_the_masked_topk(kind, C, E):
    """filter(topk(min(K + E, C))) == masked topk(K), indices, score bits and the short marks, for K in {1, 7, C - E}."""
    rng = np.random.default_rng(1000 * C + 10 * E + len(kind))
    B = 6
    s = _scores(kind, B, C, rng)
    ex = _exclusions(B, C, E, rng)
    for K in sorted({k for k in (1, 7, C - E) if 1 <= k <= C}):
        want_i, want_s, want_short = XR.masked_topk(s, K, ex)
        ci, cs = XR.ordered_topk(s, min(K + E, C))
        got_i, got_s, got_short = XR.filter_candidates(ci, cs, K, ex, C=C)
        assert np.array_equal(got_i, want_i), (K, kind)
        assert np.array_equal(XR.bits(got_s), XR.bits(want_s))
        assert np.array_equal(got_short, want_short)
        if K + E <= C:
            assert not want_short.any()  # at most E rows went: K always survive
        if kind == "equal":  # the lowest non-excluded indices, in order
            for b in range(B):
                S = XR.exclusion_set(ex[b])
                assert want_i[b].tolist() == ([r for r in range(C) if r not in S] + [-1] * K)[:K]


def test_lemma_through_a_row_key_map():
    """Keys are item ids: row r holds item row_key[r] (a permutation with ids far above 2^32)."""
    rng = np.random.default_rng(5)
    B, C, E, K = 5, 129, 5, 7
    s = _scores("ties", B, C, rng)
    row_key = rng.permutation(C).astype(np.int64) + ((np.arange(C, dtype=np.int64) % 3 + 1) << 33)
    ex = row_key[rng.integers(0, C, (B, E))]
    ex[0, 1] = ex[0, 0]
    ex[1, :] = -1
    want = XR.masked_topk(s, K, ex, row_key)
    ci, cs = XR.ordered_topk(s, K + E)
    got = XR.filter_candidates(ci, cs, K, ex, row_key)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    for b in range(B):  # nothing returned is excluded, and it differs from the unmasked answer where an exclusion bit
        assert not (set(row_key[got[0][b]].tolist()) & XR.exclusion_set(ex[b]))
    # ids that differ only above bit 31 are different keys
    low = XR.filter_candidates(ci, cs, K, ex & 0xFFFFFFFF, row_key)
    assert np.array_equal(low[0], XR.ordered_topk(s, K)[0])


def test_filter_drops_out_of_range_candidates_and_pads_the_tail():
    idx = np.array([[4, -1, 7, 9, 2, 5]], dtype=np.int64)
    sc = np.array([[6., 5., 4., 3., 2., 1.]], dtype=np.float32)
    ex = np.array([[2, -1, 2]], dtype=np.int64)
    gi, gs, short = XR.filter_candidates(idx, sc, 4, ex, C=9)
    assert gi.tolist() == [[4, 7, 5, -1]] and gs.tolist() == [[6., 4., 1., -np.inf]] and short.tolist() == [True]
    gi, gs, short = XR.filter_candidates(idx, sc, 3, ex, C=9)
    assert gi.tolist() == [[4, 7, 5]] and short.tolist() == [False]


# ------------------------------------------------------------------ the C ABI without a GPU
def test_entry_point_exists_in_header_library_and_bindings():
    from two_tower_models_amd import _native as N
    lib = N.load()
    header = open(os.path.join(ROOT, "include", "tt_hotpath.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "tt_mips_exclude" in N.SIGNATURES and hasattr(lib, "tt_mips_exclude")
    assert re.search(r"\btt_mips_exclude\s*\(", code)
    assert len(N.SIGNATURES["tt_mips_exclude"][1]) == 13
    assert "ref:src/two_tower_base_retrieval.py:221-249" in header


def test_entry_point_validates_arguments_without_a_gpu():
    """Null pointers and bad sizes: TT_E_BADARG before any HIP call (there is no device here)."""
    from two_tower_models_amd import _native as N
    lib = N.load()
    x = 0x1000  # never dereferenced: every call below is refused by the argument checks

    def call(idx=x, sc=x, B=4, n=60, K=10, ex=x, E=50, key=None, C=100, oi=x, os_=x, flag=x):
        return lib.tt_mips_exclude(idx, sc, B, n, K, ex, E, key, C, oi, os_, flag, None)

    for kw in (dict(idx=None), dict(sc=None), dict(ex=None), dict(oi=None), dict(os_=None), dict(flag=None)):
        assert call(**kw) == N.TT_E_BADARG
        assert b"null pointer" in lib.tt_last_error_string()
    for kw in (dict(K=0), dict(K=61), dict(K=-1), dict(E=0), dict(E=4097), dict(n=0), dict(n=1 << 31, K=10), dict(B=0),
               dict(B=-2), dict(C=0)):
        assert call(**kw) == N.TT_E_BADARG, kw
        assert b"sizes" in lib.tt_last_error_string()


# ------------------------------------------------------------------ refusals before any kernel
def _module(C=16, D=8):
    import two_tower_models_amd as A
    return A.BaselineMIPSModule(C, D)


def test_exclude_type_shape_and_size_are_checked_before_the_device():
    from two_tower_models_amd import ops
    m = _module()
    q = torch.zeros(4, 8)
    for call in (lambda e: m.search(q, 3, e), lambda e: m(q, 3, e), lambda e: m(query_embedding=q, num_items=3, exclude=e)):
        with pytest.raises(TypeError):
            call(torch.zeros(4, 2, dtype=torch.int32))
        with pytest.raises(TypeError):
            call(torch.zeros(4, 2))
        with pytest.raises(TypeError):
            call([[1, 2]] * 4)
        with pytest.raises(ValueError):
            call(torch.zeros(4, dtype=torch.int64))  # not [B, E]
        with pytest.raises(ValueError):
            call(torch.zeros(3, 2, dtype=torch.int64))  # B mismatch
        with pytest.raises(ValueError):
            call(torch.zeros(4, 0, dtype=torch.int64))
        with pytest.raises(ValueError, match="4096"):
            call(torch.zeros(4, 4097, dtype=torch.int64))
        with pytest.raises(RuntimeError, match="no CPU path"):  # a well-formed list gets as far as the search
            call(torch.zeros(4, 2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="selected index k out of range"):
        m.search(q, 17, torch.zeros(4, 2, dtype=torch.int64))
    # ops.mips_exclude itself
    idx, sc, ex = torch.zeros(4, 6, dtype=torch.int64), torch.zeros(4, 6), torch.zeros(4, 2, dtype=torch.int64)
    with pytest.raises(TypeError):
        ops.mips_exclude(idx.int(), sc, 3, ex)
    with pytest.raises(ValueError):
        ops.mips_exclude(idx, sc, 3, ex[:3])
    with pytest.raises(ValueError, match="4096"):
        ops.mips_exclude(idx, sc, 3, torch.zeros(4, 4097, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="selected index k out of range"):
        ops.mips_exclude(idx, sc, 7, ex)
    with pytest.raises(TypeError):
        ops.mips_exclude(idx, sc, 3, ex, row_key=torch.zeros(9))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mips_exclude(idx, sc, 3, ex)


def test_sharded_module_with_a_row_item_id_map_refuses_before_any_collective():
    """No process group exists here: reaching a collective would raise something else."""
    from two_tower_models_amd import parallel
    m = _module()
    m._shard = parallel.RowShard(16, 8, 2, 0)
    m.row_item_id = torch.arange(16) + 100
    q, ex = torch.zeros(4, 8), torch.zeros(4, 2, dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        m.search(q, 3, ex)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        m(q, 3, ex)


def _model(cls_name="TwoTowerWithUserHistoryEncoder", mips=None, **extra):
    import two_tower_models_amd as A
    mips = mips if mips is not None else A.BaselineMIPSModule(16, 8)
    cls = getattr(A, cls_name)
    if cls is A.TwoTowerBaseRetrieval:
        return cls(4, 10, 8, 4, 10, 8, 4, [1.0], mips)
    if cls is A.TwoTowerPlusLightRanker:
        return cls(num_items=2, num_mips_items=4, num_ranker_user_embeddings=2, user_id_hash_size=10,
                   user_id_embedding_dim=8, user_features_size=4, user_history_seqlen=2, item_id_hash_size=10,
                   item_id_embedding_dim=8, item_features_size=4, user_value_weights=[1.0], mips_module=mips)
    return cls(4, 10, 8, 4, 2, 10, 8, 4, [1.0], mips)


ARGS = (torch.zeros(4, dtype=torch.long), torch.zeros(4, 4), torch.zeros(4, 2, dtype=torch.long))


@pytest.mark.parametrize("cls_name", ["TwoTowerBaseRetrieval", "TwoTowerWithUserHistoryEncoder", "TwoTowerWithDebiasing",
                                      "TwoTowerPlusLightRanker"])
def test_models_refuse_exclusion_with_a_foreign_mips_module_and_bad_lists(cls_name):
    import two_tower_models_amd as A
    from two_tower_models_amd import parallel

    class Foreign(A.BaselineMIPSModule):  # any class whose forward is not BaselineMIPSModule.forward
        def forward(self, query_embedding, num_items):
            raise AssertionError("never reached")

    m = _model(cls_name, Foreign(16, 8))
    own = torch.zeros(4, 3, dtype=torch.int64)
    for kw in (dict(exclude_history=True), dict(exclude_item_id=own), dict(exclude_history=True, exclude_item_id=own)):
        with pytest.raises(NotImplementedError, match="BaselineMIPSModule"):
            m(*ARGS, **kw)
    m = _model(cls_name)
    with pytest.raises(TypeError):
        m(*ARGS, exclude_item_id=own.int())
    with pytest.raises(ValueError):
        m(*ARGS, exclude_item_id=own[:3])
    with pytest.raises(ValueError, match="4096"):
        m(*ARGS, exclude_history=True, exclude_item_id=torch.zeros(4, 4095, dtype=torch.int64))  # 2 + 4095
    with pytest.raises(TypeError):
        m(ARGS[0], ARGS[1], ARGS[2].int(), exclude_history=True)
    with pytest.raises(TypeError):
        m(*ARGS, True)  # keyword-only
    with pytest.raises(RuntimeError, match="no CPU path"):  # well-formed: stops at the CPU tensors, like forward() itself
        m(*ARGS, exclude_history=True, exclude_item_id=own)
    # a row-sharded corpus with an item-id map: refused by the model too, before anything else runs
    m.mips_module._shard = parallel.RowShard(16, 8, 2, 0)
    m.mips_module.row_item_id = torch.arange(16) + 100
    if cls_name != "TwoTowerPlusLightRanker":
        with pytest.raises(NotImplementedError, match="row-sharded"):
            m(*ARGS, exclude_history=True)


def test_light_ranker_exclusion_stays_refused_on_a_sharded_model():
    from two_tower_models_amd import parallel
    m = _model("TwoTowerPlusLightRanker")
    m.item_id_embedding_arch.weight._tt_shard = parallel.RowShard(20, 8, 2, 0)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        m(*ARGS, exclude_history=True)


# ------------------------------------------------------------------ signatures
def test_new_keywords_are_keyword_only_with_defaults():
    import two_tower_models_amd as A
    for cls in (A.TwoTowerBaseRetrieval, A.TwoTowerWithUserHistoryEncoder, A.TwoTowerWithDebiasing,
                A.TwoTowerWithPositionDebiasedWeights, A.TwoTowerWithUserDebiasedWeights, A.TwoTowerPlusLightRanker):
        p = inspect.signature(cls.forward).parameters  # the method's own signature (behind takes_history_lengths)
        assert list(p) == ["self", "user_id", "user_features", "user_history", "exclude_history", "exclude_item_id"], cls
        assert p["exclude_history"].kind is inspect.Parameter.KEYWORD_ONLY and p["exclude_history"].default is False
        assert p["exclude_item_id"].kind is inspect.Parameter.KEYWORD_ONLY and p["exclude_item_id"].default is None
        assert "exclude_history" not in inspect.signature(cls.train_forward).parameters
    for meth in (A.BaselineMIPSModule.search, A.BaselineMIPSModule.forward):
        p = inspect.signature(meth).parameters
        assert list(p) == ["self", "query_embedding", "num_items", "exclude"] and p["exclude"].default is None
    from two_tower_models_amd import ops
    p = inspect.signature(ops.mips_exclude).parameters
    assert list(p)[:5] == ["idx", "scores", "k", "exclude", "row_key"] and p["row_key"].default is None


def test_train_parser_exclude_history_is_off_by_default():
    from two_tower_models_amd import train
    p = train.build_parser()
    assert p.parse_args([]).exclude_history is False
    a = p.parse_args(["--retrieve", "--exclude_history"])
    assert a.exclude_history is True and a.retrieve is True
    assert "--retrieve" in p.format_help().rsplit("--exclude_history", 1)[1][:400]  # the help says where it applies


# ------------------------------------------------------------------ row_item_id lifecycle
def test_every_corpus_assignment_resets_row_item_id_and_a_move_keeps_it():
    m = _module(16, 128)
    assert m.row_item_id is None and m.state_dict() == {}
    for assign in (lambda: setattr(m, "corpus", torch.zeros(16, 128)), lambda: m.set_corpus(torch.ones(8, 128)),
                   lambda: m.use_bf16_storage()):
        m.row_item_id = torch.arange(m.corpus.shape[0]) + 7
        assign()
        assert m.row_item_id is None
    # .to() moves the SAME corpus: its map travels with it, stays int64 and is not part of the state_dict
    m.row_item_id = torch.arange(8) + 7
    m.to(torch.device("cpu"))
    m.to(torch.float64)
    assert m.row_item_id.dtype == torch.int64 and m.row_item_id.tolist() == list(range(7, 15))
    assert m.corpus.dtype == torch.bfloat16 and m.state_dict() == {}
    # a map of the wrong length is refused, not read out of bounds
    m.row_item_id = torch.arange(5)
    with pytest.raises(ValueError, match="row_item_id"):
        m.search(torch.zeros(2, 128), 3, torch.zeros(2, 2, dtype=torch.int64))


def test_index_corpus_records_the_catalogue(monkeypatch):
    """index_corpus on CPU tensors, the item tower replaced by a table lookup (the product tower needs the GPU):
    an `arange` catalogue leaves row_item_id None, any other one stores a clone of the ids."""
    m = _model("TwoTowerWithUserHistoryEncoder", _module(16, 8))
    monkeypatch.setattr(type(m), "compute_item_embeddings",
                        lambda self, item_id, item_features: self.item_id_embedding_arch.weight.detach()[item_id])
    feats = torch.zeros(10, 4)
    m.mips_module.row_item_id = torch.arange(16)
    m.index_corpus(torch.arange(10), feats)
    assert m.mips_module.row_item_id is None and m.mips_module.corpus_size == 10
    ids = torch.tensor([3, 1, 4, 1, 5, 9, 2, 6, 5, 3])
    m.index_corpus(ids, feats, chunk=4)
    got = m.mips_module.row_item_id
    assert got.dtype == torch.int64 and torch.equal(got, ids) and got.data_ptr() != ids.data_ptr()
    assert torch.equal(m.mips_module.corpus, m.item_id_embedding_arch.weight.detach()[ids])
    m.index_corpus(torch.arange(1, 11) % 10, feats)  # a rotation is not the identity
    assert m.mips_module.row_item_id is not None
    m.index_corpus(torch.arange(10), feats)
    assert m.mips_module.row_item_id is None
