"""Integer / float64 yardstick for MIPS exclusion (csrc/mips_exclude.hip: tt_mips_exclude; BaselineMIPSModule.search with
`exclude`).  A helper, not a test: imported by test_mips_exclude_cpu.py and test_gpu_mips_exclude.py; the product never
imports it.  numpy only.

  masked_topk        the definition: leave out every row whose key is in the query's exclusion set, stable sort of the rest
                     by (score desc, index asc), the first K -- what masking those rows to -inf before the top-K gives.
  ordered_topk       the same without exclusions: the candidate list a search at K' returns.
  filter_candidates  tt_mips_exclude's contract on a given candidate list: the first K candidates, in input order, whose
                     index lies in [0, C) and whose key is not excluded; the tail -1 / -inf and a `short` mark per query.
The lemma (DESIGN.md "Exclusion"): filter_candidates(ordered_topk(s, min(K + E, C))) == masked_topk(s, K) whenever every
query excludes at most E ROWS.  Scores keep their dtype (and bits) everywhere: nothing is computed with them but the sort."""
import numpy as np

NEG_INF = -np.inf


def exclusion_keys(row):
    """The keys >= 0 of one query's exclusion list, each once (negative entries are padding), as an int64 array."""
    row = np.asarray(row, dtype=np.int64).reshape(-1)
    return np.unique(row[row >= 0])


def exclusion_set(row):
    return set(exclusion_keys(row).tolist())


def _order(s):
    """Row indices of one score vector under (score desc, index asc)."""
    return np.argsort(-s.astype(np.float64), kind="stable")


def _pad(idx, sc, K, dtype):
    n = len(idx)
    oi = np.full(K, -1, dtype=np.int64)
    osc = np.full(K, NEG_INF, dtype=dtype)
    oi[:n], osc[:n] = idx, sc
    return oi, osc


def ordered_topk(scores, K):
    """(idx int64 [B, K], scores [B, K]) of the K best per query under (score desc, index asc)."""
    scores = np.asarray(scores)
    idx = np.stack([_order(s)[:K] for s in scores]).astype(np.int64)
    return idx, np.take_along_axis(scores, idx, axis=1)


def masked_topk(scores, K, exclude, row_key=None):
    """scores [B, C], exclude int64 [B, E], row_key int64 [C] or None (the key of row r is r) ->
    (idx int64 [B, K], scores [B, K], short bool [B]): the top-K of the rows whose key is not excluded."""
    scores = np.asarray(scores)
    B, C = scores.shape
    keys = np.arange(C, dtype=np.int64) if row_key is None else np.asarray(row_key, dtype=np.int64)
    out_i, out_s, short = [], [], np.zeros(B, dtype=bool)
    for b in range(B):
        keep = ~np.isin(keys, exclusion_keys(exclude[b]))
        order = _order(scores[b])
        order = order[keep[order]][:K]
        short[b] = len(order) < K
        oi, osc = _pad(order, scores[b][order], K, scores.dtype)
        out_i.append(oi), out_s.append(osc)
    return np.stack(out_i), np.stack(out_s), short


def filter_candidates(idx, scores, K, exclude, row_key=None, C=None):
    """idx int64 [B, n_cand], scores [B, n_cand] -> (idx [B, K], scores [B, K], short bool [B]); C: the number of corpus
    rows (default: row_key's length, else no upper limit)."""
    idx, scores = np.asarray(idx, dtype=np.int64), np.asarray(scores)
    B = idx.shape[0]
    if C is None:
        C = len(row_key) if row_key is not None else np.iinfo(np.int64).max
    out_i, out_s, short = [], [], np.zeros(B, dtype=bool)
    for b in range(B):
        valid = (idx[b] >= 0) & (idx[b] < C)
        keys = idx[b].copy()
        if row_key is not None:
            keys[valid] = np.asarray(row_key, dtype=np.int64)[idx[b][valid]]
        keep = valid & ~np.isin(keys, exclusion_keys(exclude[b]))
        pos = np.nonzero(keep)[0][:K]
        short[b] = len(pos) < K
        oi, osc = _pad(idx[b][pos], scores[b][pos], K, scores.dtype)
        out_i.append(oi), out_s.append(osc)
    return np.stack(out_i), np.stack(out_s), short


def bits(x):
    """The bit patterns of a float32 array (scores are compared by these: -0.0, NaN payloads and all)."""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32
    return x.view(np.uint32)
