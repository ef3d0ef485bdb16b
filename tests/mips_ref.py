"""Float64 yardstick for MIPS top-K (csrc/mips.hip: tt_mips_topk, tt_mips_split_rows, tt_mips_unscale).  A helper, not a
test: imported by test_mips_reference_cpu.py and test_gpu_mips_reference.py the way attention_ref.py is imported by its
tests; the product never imports it.

  inputs      five classes, all from fixture_gen.gaussianish and never bf16_round (every mantissa bit in use):
                flat       plain
                negative   q = |q|, c = -|c|: every score negative
                clustered  base + 2^-8 noise for corpus and queries: adjacent scores a few tens of ulps apart
                range      corpus rows scaled by 2^(4 g), g gaussianish per row
                tiny       flat times 2^-52 on both operands: scores near 2^-100, still normal fp32 numbers
              `plant` overwrites the rows plant_rows(C) of the corpus with 3 x the row that query 0, 1, .. likes best
              (the corpus-edge cases): each must win for its query.
              The seeds leave B out and the values are a hash of the element index, so the queries of a smaller batch
              are a PREFIX of a larger one's: one reference per (dtype, C, D, class, plant), sliced.
  effective   what the kernel is given: fp32 and TT_F16X2 the inputs themselves, bf16 both operands through torch's
              .to(torch.bfloat16).float().
  reference   s64 = the float64 matmul of the effective operands, A = |q| @ |c|^T in float64.
  YARD        the worst |s32 - s64| / (2^-24 A) of a float32 index-order evaluation (one rounding per multiply and per
              add, no BLAS) over the cases of a (dtype, class): `python tests/mips_ref.py` prints the table,
              test_mips_reference_cpu.py re-measures it.
  bound       per element  E = 4 YARD 2^-24 A + 2^-24 |s64|.  The factor 4 is the project's (attention_ref.py,
              profiles/adam_reference_tolerance.txt): another summation order (matrix cores); the last term is the
              result's own rounding.  TT_F16X2 uses the fp32 E (the header claims the fp32 path's contract), except on
              the range class: there h + l represents x * scale to 2^-23 of the MATRIX maximum and the dropped l * l
              term is at most 2^-24 of the product of the two maxima, so E + D 2^-21 max|Q| max|C| (norm-wise).
  check_topk  the five rules of a result (idx, scores) against (s64, E); see its docstring.
  CASES       every shape test_gpu_mips_reference.py runs, with whether the sparse pass 2 is expected -- shared with the
              CPU tests, which check the conditions and run the mutants at the very same cases.

profiles/mips_reference_tolerance.txt records the tables and what the GPU showed."""
import collections
import os
import sys

import numpy as np
import torch

try:
    import fixture_gen as fg
except ImportError:  # run as a script: pytest's conftest.py is what puts tests/golden on the path
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import fixture_gen as fg

EPS = 2.0 ** -24
FACTOR = 4.0
CLASSES = ("flat", "negative", "clustered", "range", "tiny")
# constants of csrc/mips.hip the cases rest on
GROUP, CHUNK, QB_WG, MIPS_QBATCH, WIDE_ROWS, SORT_LDS = 64, 128, 128, 1024, 65536, 2048
CLUSTER_SPREAD = 2.0 ** -8

# worst |s32 - s64| / (2^-24 A) of the float32 index-order evaluation per (effective dtype, class): see main().
# bf16 operands have exact fp32 products, so only the adds round.
YARD = {
    "f32": {"flat": 7.3, "negative": 15.0, "clustered": 1.9, "range": 6.9, "tiny": 6.6},
    "bf16": {"flat": 4.2, "negative": 8.3, "clustered": 0.38, "range": 2.9},
}
# rule 5: (share of (query, item) pairs decided, share of each query's float64 top-K that is certainly in)
CONDITIONS = {"clustered": (0.99, 0.80)}
CONDITIONS_DEFAULT = (0.999, 0.95)

Case = collections.namedtuple("Case", "group dtype B C D K cls plant sparse")


def _c(group, dtype, B, C, D, K, cls="flat", plant=False, sparse=True):
    return Case(group, dtype, B, C, D, K, cls, plant, sparse)


C0 = CHUNK * 40 + 77  # 5197 rows: 82 groups of 64, 42 of 128
FORM_B = (1, 32, 33, 64, 65, 128, 129, 256, 257, 300)
# query-batch forms: shared-query x4 (B <= 32), x2 (<= 64), throughput form with one, two and three workgroups
FORMS = [_c("forms", dt, B, C0, 128, 40, cls) for dt in ("f32", "bf16") for cls in ("flat", "negative", "clustered")
         for B in FORM_B]
FORMS += [_c("forms", dt, B, C0, 128, 40, "range") for dt in ("f32", "bf16") for B in (72, 300)]
# widths: fp32 32 / 64 / 128 the three DMA forms, 48 / 16 D != dp (generic pass 1, dense pass 2), 50 rows not 16-byte
# multiples; bf16 32 generic pass 1 with the sparse pass 2, 64 / 128 DMA forms, 40 generic
WIDTHS = [_c("widths", "f32", B, C0, D, 40, sparse=D in (32, 64, 128)) for D in (32, 64, 128, 48, 16, 50) for B in (72, 16)]
WIDTHS += [_c("widths", "bf16", B, C0, D, 40, sparse=D != 40) for D in (32, 64, 128, 40) for B in (72, 16)]
# D > 128: library GEMM slabs + group epilogues; C = 65536 + 300 reaches the second slab
WIDE = [_c("wide", dt, 40, C0, D, 40, sparse=False) for dt in ("f32", "bf16") for D in (130, 256)]
WIDE += [_c("wide", dt, 40, WIDE_ROWS + 300, 130, 40, sparse=False) for dt in ("f32", "bf16")]
# K: 1; 41 / 42 around the 128-row-group count 2 ceil(C / 256) = 42 (128-row groups need more groups than K); 81 one group
# more than K; 82 = n_groups (every item a candidate, dense pass 2); K == C
KS = [_c("k", dt, 72, C0, 128, K, sparse=K < 82) for dt in ("f32", "bf16") for K in (1, 41, 42, 81, 82, C0)]
# corpus edges: planted rows (x3) at 0, 63, 64, 127, 128, C - 1 and the first row of the last 64- / 128-row group;
# C ends one row into a 128-row chunk, one row into its second half, one row into the second half of a 256-row chunk
EDGE_C = (CHUNK * 40 + 1, CHUNK * 40 + 65, 2 * CHUNK * 20 + 129)
EDGES = [_c("edges", dt, B, C, 128, 40, plant=True) for dt in ("f32", "bf16") for C in EDGE_C for B in (16, 72)]
# 314 groups > K = 300 > 256: several selected-group slices; B = 1024 + 65: two query batches, 2 chunks per split
BIG = [_c("big", dt, 1089, 20077, 128, 300) for dt in ("f32", "bf16")]
# TT_F16X2: x4, x2, one workgroup, two, and two query fragments per wave (B > 256)
F16X2 = [_c("f16x2", "f16x2", B, C0, 128, 40, cls) for cls in ("flat", "negative", "clustered") for B in (16, 48, 72, 200, 300)]
F16X2 += [_c("f16x2", "f16x2", B, C0, 128, 40, cls) for cls in ("range", "tiny") for B in (72, 300)]
F16X2 += [_c("f16x2", "f16x2", 300, 20077, 128, 300)]
TINY_F32 = [_c("tiny-f32", "f32", B, C0, 128, 40, "tiny") for B in (72, 300)]
CASES = FORMS + WIDTHS + WIDE + KS + EDGES + BIG + F16X2 + TINY_F32


def case_id(c):
    return f"{c.group}-{c.dtype}-B{c.B}-C{c.C}-D{c.D}-K{c.K}-{c.cls}" + ("-plant" if c.plant else "")


def sparse_launches(c):
    """mips_sparse_kernel launches expected: one per batch of MIPS_QBATCH queries where the sparse pass 2 runs, else none."""
    return -(-c.B // MIPS_QBATCH) if c.sparse else 0


def plant_rows(C):
    """Rows that carry a planted winner: the first and last rows of the first 64- and 128-row groups, the last row, and the
    first row of the last 64-row and of the last 128-row group.  For EDGE_C the last row is the ONLY row of the last 64-row
    group (128 * 40 + 1, 128 * 40 + 65) or of the last 128-row group (256 * 20 + 129)."""
    return sorted({0, 63, 64, 127, 128, C - 1, (C - 1) // GROUP * GROUP, (C - 1) // (2 * GROUP) * (2 * GROUP)})


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def inputs(B, C, D, cls, plant=False):
    """fp32 (q [B, D], c [C, D])."""
    sq, sc = 52000 + 7 * D, 51000 + 13 * D + C
    q, c = fg.gaussianish((B, D), sq), fg.gaussianish((C, D), sc)
    if cls == "negative":
        q, c = np.abs(q), -np.abs(c)
    elif cls == "clustered":
        q = fg.gaussianish((1, D), sq + 1) + np.float32(CLUSTER_SPREAD) * q
        c = fg.gaussianish((1, D), sc + 1) + np.float32(CLUSTER_SPREAD) * c
    elif cls == "range":
        c = c * np.exp2(4.0 * fg.gaussianish((C, 1), sc + 2).astype(np.float64)).astype(np.float32)
    elif cls == "tiny":
        q, c = q * np.float32(2.0 ** -52), c * np.float32(2.0 ** -52)
    elif cls != "flat":
        raise KeyError(cls)
    if plant:  # the k-th planted row is 3 x the row that query k likes best: it must win for query k
        rows = plant_rows(C)
        assert B >= len(rows)
        best = np.argmax(q[:len(rows)].astype(np.float64) @ c.astype(np.float64).T, axis=1)
        planted = np.float32(3.0) * c[best]
        c = c.copy()
        c[rows] = planted
    return T(q.astype(np.float32)).contiguous(), T(c.astype(np.float32)).contiguous()


def effective(x, dtype):
    return x.to(torch.bfloat16).float() if dtype == "bf16" else x


def eff_name(dtype):
    return "bf16" if dtype == "bf16" else "f32"


def e_bound(s64, A, yard):
    return (FACTOR * yard * EPS) * A + EPS * s64.abs()


def split_bound(q, c):
    """The TT_F16X2 representation's norm-wise term: D 2^-21 max|Q| max|C|."""
    return q.shape[1] * 2.0 ** -21 * float(q.abs().max()) * float(c.abs().max())


_cache = {}


def _key(c):
    return (eff_name(c.dtype), c.C, c.D, c.cls, c.plant)


def case_data(c):
    """{"q", "c" (effective, fp32), "q_raw", "c_raw", "s64", "A", "E"} of a case, computed once per (dtype, C, D, class,
    plant) at the largest batch any case runs it with and sliced.  Leave it unchanged.  A reference of more than 2^22
    (query, item) pairs (the B = 1089 cases: 0.5 GB each) is dropped again when the next reference is computed."""
    k = _key(c)
    if k not in _cache or _cache[k]["q"].shape[0] < c.B:
        for big in [x for x, v in _cache.items() if v["s64"].numel() > 1 << 22]:
            del _cache[big]
        Bmax = max([x.B for x in CASES if _key(x) == k] + [c.B])
        q_raw, c_raw = inputs(Bmax, c.C, c.D, c.cls, c.plant)
        q, cm = effective(q_raw, k[0]), effective(c_raw, k[0])
        s64 = q.double() @ cm.double().t()
        A = q.double().abs() @ cm.double().abs().t()
        _cache[k] = {"q": q, "c": cm, "q_raw": q_raw, "c_raw": c_raw, "s64": s64, "A": A,
                     "E": e_bound(s64, A, YARD[k[0]][c.cls])}
    d = _cache[k]
    out = {n: (v if n in ("c", "c_raw") else v[:c.B]) for n, v in d.items()}
    if c.dtype == "f16x2" and c.cls == "range":
        out["E"] = out["E"] + split_bound(d["q_raw"][:c.B], d["c_raw"])
    return out


def drop_cache():
    _cache.clear()


# ------------------------------------------------------------------ float32 evaluations
def index_order_f32(q, c, rows=64):
    """q @ c^T in float32, one rounding per multiply and per add, summed in index order (numpy ufuncs: no BLAS, no fma)."""
    qn, cn = q.numpy(), np.ascontiguousarray(c.numpy().T)  # [D, C]
    out = np.empty((qn.shape[0], cn.shape[1]), dtype=np.float32)
    for r0 in range(0, qn.shape[0], rows):
        qq = qn[r0:r0 + rows]
        acc = np.zeros((qq.shape[0], cn.shape[1]), dtype=np.float32)
        tmp = np.empty_like(acc)
        for d in range(qn.shape[1]):
            np.multiply(qq[:, d, None], cn[d][None, :], out=tmp)
            np.add(acc, tmp, out=acc)
        out[r0:r0 + rows] = acc
    return T(out)


def ordered_topk(s, K):
    """(idx int64, scores) of the K best per row under (score desc, index asc)."""
    v, i = torch.sort(s, dim=1, descending=True, stable=True)
    return i[:, :K].contiguous(), v[:, :K].contiguous()


def topk32(q, c, K):
    """torch.topk(q @ c.T, K) in float32, ties in ascending index order."""
    return ordered_topk(q @ c.t(), K)


def yard_cases(dtype, cls):
    """One case per reference of (effective dtype, class) -- the largest batch; the smaller ones are prefixes of it."""
    best = {}
    for c in CASES:
        if eff_name(c.dtype) == dtype and c.cls == cls and (_key(c) not in best or best[_key(c)].B < c.B):
            best[_key(c)] = c
    return list(best.values())


def measure(dtype, cls):
    """(worst |s32 - s64| / (2^-24 A), case id) of the index-order float32 evaluation over yard_cases."""
    worst = (0.0, None)
    for c in yard_cases(dtype, cls):
        d = case_data(c)
        r = float(((index_order_f32(d["q"], d["c"]).double() - d["s64"]).abs() / (EPS * d["A"])).max())
        if r >= worst[0]:
            worst = (r, case_id(c))
    return worst


# ------------------------------------------------------------------ the checker
def membership(s64, E, K):
    """(certainly_in, certainly_out) [B, C] bool.  U = s64 + E, L = s64 - E.  Item i is certainly in if fewer than K OTHER
    items j have U_j >= L_i: U_i >= L_i always, so at most K items in all, i.e. the (K+1)-th largest U is below L_i.
    It is certainly out if at least K items j have L_j > U_i: the K-th largest L is above U_i."""
    U, L = s64 + E, s64 - E
    C = s64.shape[1]
    if K < C:
        u = torch.topk(U, K + 1, dim=1).values[:, K:K + 1]
        cin = L > u
    else:
        cin = torch.ones_like(s64, dtype=torch.bool)
    lk = torch.topk(L, K, dim=1).values[:, K - 1:K]
    return cin, lk > U


def conditions(s64, E, K):
    """Rule 5's two shares: (decided pairs / all pairs, the smallest share over the queries of the float64 top-K that is
    certainly in)."""
    cin, cout = membership(s64, E, K)
    top = torch.topk(s64, K, dim=1).indices
    return float((cin | cout).double().mean()), float(cin.gather(1, top).double().mean(dim=1).min())


class Report:
    """What check_topk found: rules[r] = the queries that break rule r (1 .. 4); worst = the largest |score - s64| / E over
    the slots with a valid index; undecided = returned items that are neither certainly in nor certainly out."""

    def __init__(self):
        self.rules, self.worst, self.undecided = {1: [], 2: [], 3: [], 4: []}, 0.0, 0

    @property
    def ok(self):
        return not any(self.rules.values())

    def fired(self):
        return [r for r, qs in self.rules.items() if qs]

    def __repr__(self):
        broken = {r: (len(qs), qs[:4]) for r, qs in self.rules.items() if qs}
        return f"Report(worst err/E {self.worst:.3g}, undecided returned {self.undecided}, broken rules {broken})"


def check_topk(idx, scores, q_eff, c_eff, K, E, s64=None):
    """A top-K result idx [B, K] int64, scores [B, K] fp32 against float64, every rule per query:
      1  every slot was written: no sentinel (-1 / NaN) survives, indices lie in [0, C) and are pairwise distinct, scores
         are finite;
      2  |score - s64[idx]| <= E[idx];
      3  the output's own order: scores non-increasing, equal scores in ascending index order (-0.0 equals +0.0);
      4  every certainly-in item is returned and no certainly-out item is (membership); the undecided band is left alone.
    s64: the float64 scores if the caller has them already.  -> Report."""
    idx, scores = idx.detach().cpu(), scores.detach().cpu().double()
    if s64 is None:
        s64 = q_eff.double() @ c_eff.double().t()
    B, C = s64.shape
    assert idx.shape == (B, K) and scores.shape == (B, K) and E.shape == s64.shape
    rep = Report()
    valid = (idx >= 0) & (idx < C)
    srt = torch.sort(idx, dim=1).values
    dup = (srt[:, 1:] == srt[:, :-1]).any(dim=1) if K > 1 else torch.zeros(B, dtype=torch.bool)
    bad1 = ~valid.all(dim=1) | dup | ~torch.isfinite(scores).all(dim=1)
    safe = idx.clamp(0, C - 1)
    ratio = (scores - s64.gather(1, safe)).abs() / E.gather(1, safe)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    bad2 = ((ratio > 1.0) & valid).any(dim=1)
    rep.worst = float(torch.where(valid, ratio, torch.zeros_like(ratio)).max())
    if K > 1:
        a, b = scores[:, :-1], scores[:, 1:]
        bad3 = ((b > a) | ((b == a) & (idx[:, 1:] <= idx[:, :-1])) | torch.isnan(a) | torch.isnan(b)).any(dim=1)
    else:
        bad3 = torch.isnan(scores).any(dim=1)
    cin, cout = membership(s64, E, K)
    got = torch.zeros(B, C, dtype=torch.bool)
    got[torch.arange(B)[:, None].expand(B, K)[valid], idx[valid]] = True  # the valid slots only
    bad4 = (cin & ~got).any(dim=1) | (cout & got).any(dim=1)
    rep.undecided = int((got & ~cin & ~cout).sum())
    for r, bad in ((1, bad1), (2, bad2), (3, bad3), (4, bad4)):
        rep.rules[r] = torch.nonzero(bad).flatten().tolist()
    return rep


# ------------------------------------------------------------------ the TT_F16X2 operand split, emulated
def split_emulate(x):
    """tt_mips_split_rows in numpy: (h, l float16, scale) with x * scale = h + l up to the split's own error; scale = the
    power of two that brings max|x| into [2^14, 2^15) (1 for an all-zero matrix)."""
    x = x.numpy().astype(np.float32)
    mx = float(np.abs(x).max())
    scale = np.float32(1.0)
    if 0.0 < mx < 3.0e38:
        scale = np.float32(np.ldexp(1.0, 15 - int(np.frexp(mx)[1])))
    v = x * scale
    h = v.astype(np.float16)
    l = (v - h.astype(np.float32)).astype(np.float16)
    return h, l, float(scale)


def split_scores(q, c):
    """What the three-product scheme represents, in float64: (hq hc + hq lc + lq hc) / (scale_q scale_c)."""
    hq, lq, sq = split_emulate(q)
    hc, lc, sc = split_emulate(c)
    hq, lq, hc, lc = (T(a.astype(np.float64)) for a in (hq, lq, hc, lc))
    return (hq @ hc.t() + hq @ lc.t() + lq @ hc.t()) / sq / sc


def main():
    print("float32 index-order evaluation against float64: worst |s32 - s64| / (2^-24 A) per effective dtype and class")
    print(f"{'dtype':<5} {'class':<10} {'measured':>9} {'YARD':>6}   worst case")
    ok = True
    for dt in YARD:
        for cls in YARD[dt]:
            w = measure(dt, cls)
            print(f"{dt:<5} {cls:<10} {w[0]:9.3f} {YARD[dt][cls]:6.1f}   {w[1]}")
            ok = ok and w[0] <= YARD[dt][cls]
        drop_cache()
    print("\nrule 5: decided pairs / certainly-in share of the float64 top-K (the smallest over the queries), worst per group and class")
    worst = {}
    for c in CASES:
        d = case_data(c)
        dec, inn = conditions(d["s64"], d["E"], c.K)
        k = (c.group, c.dtype, c.cls)
        worst[k] = (min(dec, worst.get(k, (1.0, 1.0))[0]), min(inn, worst.get(k, (1.0, 1.0))[1]))
        need = CONDITIONS.get(c.cls, CONDITIONS_DEFAULT)
        if dec < need[0] or inn < need[1]:
            ok = False
            print("MISSED", case_id(c), dec, inn)
    for k, (dec, inn) in worst.items():
        print(f"{k[0]:<9} {k[1]:<6} {k[2]:<10} {100 * dec:8.3f} % {100 * inn:7.2f} %")
    assert ok, "YARD is below the measured worst case, or a case misses a rule-5 condition"


if __name__ == "__main__":
    main()
