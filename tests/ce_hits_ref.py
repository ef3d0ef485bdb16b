"""Float64 yardstick for the in-batch softmax cross entropy with accidental hits masked (tt_inbatch_ce_masked_fwd / _bwd:
the MASK forms of csrc/inbatch_ce.hip and the key argument of ce_wide.hip).  A helper, not a test: imported by
test_ce_hits_reference_cpu.py and test_gpu_ce_hits_reference.py; it builds on ce_ref.py (operands, layouts, plans, the
index-order float32 primitives, the tolerance arithmetic) and the product never imports it.

  semantics   pos(i) = i + off,  hit[i, j] = key[j] == key[pos(i)] and j != pos(i),  S' = U I^T (+ b[None, :]),
              ce_i = logsumexp_{j : not hit} S'[i, j] - S'[i, pos(i)],  G = coef (.) (softmax over the unmasked columns -
              onehot), 0 where hit,  dU = G I,  dI = G^T U,  du_unit = P I - I[pos];  kept logits = S' log2 e, NEG_BIG for a
              hit.  No gradient to the keys or to b.
  reference   float64: masked_fill(-inf) + logsumexp, gradients by torch autograd through sum(coef ce); written from the
              semantics above (the reference's in-batch softmax is ref:src/two_tower_base_retrieval.py:287-312, which has
              no mask); the float32 oracle is not called.
  evaluate    the same formulas in float64 or in index-order float32 (ce_ref's primitives: one rounding per operation),
              `mut` a deliberately wrong mask (MUTANTS).
  keys        PATTERNS, each chosen for what it can catch:
                none      all distinct: the mask must never fire
                pairs     j // 2: a hit inside one register group of 4
                stride64  j % 64: every hit whole tiles away at the same tile-local row (tile-relative indices)
                mod61     j % 61: hits across sub-tiles, tiles, splits, before `off` and among the extra negatives
                zipf      a popularity draw (id = floor(N^u)): about a quarter of the rows has no hit
                all_same  one key: every row keeps its positive only; ce, du_unit, dU, dI are exactly 0
  classes     flat  ce_ref's flat operands and its flat bounds: magnitudes.
              twin  items of equal key share one embedding row w_g (what the item tower yields for equal id and features);
                    the user whose positive has key g is U[i] = t w_g / |w_g|^2 + n_i with n_i orthogonal to w_g, t = 24:
                    a hit's logit equals the positive's, so every hit left unmasked at least doubles the row's mass.
              With a term the Zipf -log q is taken per KEY (equal keys = same item = same q).
  bounds      flat: ce_ref.tol("flat", .) unchanged.
              twin: |got - ref| <= 4 x YARD_TWIN[q] x scale[q] + r |ref|, r = ce_ref.RTOL.  A twin result is what a
              cancellation leaves (ce = lse - S[pos] with both near t = 24 and ce down to 1e-5; du_unit = E - I[pos] with E
              almost I[pos]), so its error is set by the operands of the difference, not by the result, and max|ref| -- ce_ref's
              unit -- says nothing here.  scale: ce, lse max|lse|; logits max|S' log2 e|; du_unit max|I|; dU max|coef| max|I|;
              dI max|coef| max|U|.  YARD_TWIN is the worst ((|fp32 - f64| - r |f64|)+) / scale of the float32 index-order
              evaluation over the twin cases (measured by `python tests/ce_hits_ref.py`, rounded up to two digits, re-measured
              by test_ce_hits_reference_cpu.py), never below 2^-24; the factor 4 is profiles/ce_reference_tolerance.txt's.
              The yardstick is never measured against a kernel.
              profiles/ce_hits_reference_tolerance.txt records the table and what the GPU showed."""
import collections
import functools
import math
import os
import sys

import numpy as np
import torch

import ce_ref as C

try:
    import fixture_gen as fg
except ImportError:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import fixture_gen as fg

F64, F32 = torch.float64, torch.float32
NEG_BIG = -3.0e38
TWIN_T = 24.0
TWIN_NOISE = 1.0  # n_i at the flat scale
PATTERNS = ("none", "pairs", "stride64", "mod61", "zipf", "all_same")
CLASSES = ("flat", "twin")
QUANTITIES = C.QUANTITIES
WIDTHS = (24, 32, 50, 64, 100, 128, 200)
SHAPES = C.SHAPES + ((1, 1, 0),)
# forward form -> (the backward that follows, with dU): the four forward forms and the three backwards
ENTRIES = {"plain": ("bwd", True), "du": ("bwd", False), "keep": ("kept", False), "loss": ("bwd", False)}

# worst normalised error of the float32 CPU evaluation against float64 over the twin cases: see main()
YARD_TWIN = {"ce": 1.2e-07, "lse": 6.8e-07, "logits": 7.1e-07, "du_unit": 3.0e-06, "dU": 2.4e-06, "dI": 1.8e-06}


# ------------------------------------------------------------------ keys
@functools.lru_cache(maxsize=None)
def keys(pattern, N):
    """int32 [N] item keys of a pattern."""
    j = torch.arange(N, dtype=torch.int64)
    if pattern == "none":
        k = 1000 + 3 * j
    elif pattern == "pairs":
        k = j // 2
    elif pattern == "stride64":
        k = j % 64
    elif pattern == "mod61":
        k = j % 61
    elif pattern == "zipf":
        u = torch.from_numpy(fg.uniform_ids((N,), 1 << 20, 4242 + N).astype(np.float64)) / float(1 << 20)
        k = torch.floor(torch.pow(torch.tensor(float(N), dtype=F64), u)).long()
    elif pattern == "all_same":
        k = torch.full((N,), 5, dtype=torch.int64)
    else:
        raise KeyError(pattern)
    return k.to(torch.int32)


def hit_matrix(key, M, off, mut=None):
    """bool [M, N]: the columns masked for each user row (mut: a wrong mask of MUTANTS)."""
    N = key.shape[0]
    rows, cols = torch.arange(M), torch.arange(N)
    pos = rows + off
    pk = key[rows] if mut == "key_by_row_index" else key[pos]
    hit = (key[None, :] == pk[:, None]) & (cols[None, :] != pos[:, None])
    if mut == "mask_positive_too":
        hit = key[None, :] == key[pos][:, None]
    if mut == "mask_within_tile":
        hit = hit & ((cols[None, :] // 64) == (pos[:, None] // 64))
    if mut == "mask_batch_only":
        hit = hit & (cols[None, :] < M)
    return hit


def transposed_hits(hit, off):
    """hit_T[i, j] = hit[j - off, i + off] where that element exists (the positives' block), else no hit: the mask a dI
    kernel forms when it swaps the roles of its two keys.  Equal keys are symmetric, so inside the block it IS the mask;
    the hits among the columns outside the block are lost."""
    M, N = hit.shape
    out = torch.zeros_like(hit)
    out[:, off:off + M] = hit[:, off:off + M].t()
    return out


# ------------------------------------------------------------------ cases
Case = collections.namedtuple("Case", "entry M N D off cls pattern bias lu li ldu ldi ldun")


def dma_width(D):
    return D in (32, 64, 128)


def _cases():
    """One case per (forward form, width, pattern); class, term, shape and layouts rotate with the indices.  The kept-logits
    pair exists in the LDS-DMA form only (D in {32, 64, 128}, aligned rows)."""
    cases = []
    n = 0
    for ie, entry in enumerate(ENTRIES):
        for iD, D in enumerate(WIDTHS):
            if entry == "keep" and not dma_width(D):
                continue
            for ip, pattern in enumerate(PATTERNS):
                n += 1
                cls = CLASSES[(ie + iD + ip) % 2]
                bias = ("none", "zipf")[(ie + iD // 2 + ip // 2) % 2]
                M, N, off = C.SHAPES[(iD + ip + 2 * ie) % len(C.SHAPES)]
                if entry == "keep":
                    li = ("dense", "strided16")[(ip + iD) % 2]
                    lu = ("strided16", "dense")[(ip + ie) % 2]
                else:  # items: LDS-DMA where the width allows it and the layout is aligned, registers otherwise
                    li = ("dense", "misaligned", "strided16", "odd_ld")[(ip + iD + ie) % 4]
                    lu = ("strided16", "dense", "misaligned", "odd_ld")[(ip + 2 * iD + ie) % 4]
                rot = lambda k: C.LAYOUTS[(n + k) % len(C.LAYOUTS)]
                cases.append(Case(entry, M, N, D, off, cls, pattern, bias, lu, li, rot(0), rot(2), rot(4)))
    for ie, entry in enumerate(ENTRIES):  # one row, one item: nothing to mask
        for D in ((32, 128) if entry == "keep" else (24, 64, 200)):
            cases.append(Case(entry, 1, 1, D, 0, "twin", "all_same", "zipf" if ie % 2 else "none", "dense", "dense",
                              C.LAYOUTS[ie % 5], C.LAYOUTS[(ie + 1) % 5], C.LAYOUTS[(ie + 2) % 5]))
    return cases


CASES = _cases()


def case_id(c):
    return (f"{c.entry}-{c.M}x{c.N}x{c.D}+{c.off}-{c.cls}-{c.pattern}-{c.bias}-U.{c.lu}-I.{c.li}-dU.{c.ldu}-dI.{c.ldi}"
            f"-du.{c.ldun}")


def math_key(c):
    """What the reference of a case depends on."""
    return (c.M, c.N, c.D, c.off, c.cls, c.pattern, c.bias)


def case_plan(c):
    return C.plan(c.M, c.N, c.D, c.lu, c.li, c.ldu if ENTRIES[c.entry] == ("bwd", True) else "dense", c.ldi)


def staging_of(c):
    p = case_plan(c)
    return "gemm" if p["dp8"] is None else p["stage_fwd"]


def compared(c):
    q = {"ce"} | ({"lse"} if c.D <= 128 else set())
    if c.entry != "plain":
        q.add("du_unit")
    if c.entry == "keep":
        q.add("logits")
    q.add("dI")
    if ENTRIES[c.entry][1]:
        q.add("dU")
    return frozenset(q)


@functools.lru_cache(maxsize=None)
def key_compared(key):
    return frozenset().union(*[compared(c) for c in CASES if math_key(c) == key])


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def inputs(key):
    """fp32 (U, I, b or None, item keys int32 [N], coef, labels [M, 3]) of a math_key."""
    M, N, D, off, cls, pattern, bias = key
    kv = keys(pattern, N)
    uniq, inv = torch.unique(kv.long(), return_inverse=True)
    if cls == "flat":
        U, I, coef, labels = C._operands(M, N, D, off, "flat")
    else:
        seed = 9100 + 7 * M + 13 * N + 131 * D
        k = 0.5 * (128.0 / D) ** 0.25
        W = C.T(fg.gaussianish((len(uniq), D), seed)).double() * k
        I = W[inv]
        w = W[inv[torch.arange(M) + off]]
        n = C.T(fg.gaussianish((M, D), seed + 1)).double() * k * TWIN_NOISE
        ww = (w * w).sum(dim=1, keepdim=True)
        n = n - (n * w).sum(dim=1, keepdim=True) / ww * w
        U = TWIN_T * w / ww + n
        coef = C.T(fg.gaussianish((M,), seed + 2)).double() / M
        coef[15::16] = 0.0
        labels = (C.T(fg.gaussianish((M, 3), seed + 3)) > 0.3).float()
        U, I, coef = U.float().contiguous(), I.float().contiguous(), coef.float().contiguous()
    b = None
    if bias == "zipf":  # one q per item: the term of a key's first occurrence
        first = torch.full((len(uniq),), N, dtype=torch.int64).scatter_reduce(0, inv, torch.arange(N), "amin")
        b = C.zipf_bias(N)[first[inv]].contiguous()
    return U, I, b, kv, coef, labels


# ------------------------------------------------------------------ the formulas
MUTANTS = ("mask_positive_too", "mask_fwd_only", "key_by_row_index", "mask_within_tile", "mask_batch_only",
           "dI_mask_transposed", "kept_logits_unmasked")
_ALL = frozenset(QUANTITIES)
# the quantities a mutant stands for in the kernels
AFFECTS = {
    "mask_positive_too": _ALL, "mask_fwd_only": frozenset({"dU", "dI"}), "key_by_row_index": _ALL,
    "mask_within_tile": _ALL, "mask_batch_only": _ALL, "dI_mask_transposed": frozenset({"dI"}),
    "kept_logits_unmasked": frozenset({"logits", "dI"}),
}


def masks(key_vec, M, off, mut):
    """(forward, dU, dI, kept-logits) masks of a mutant; None: the true ones."""
    true = hit_matrix(key_vec, M, off)
    if mut in ("mask_positive_too", "key_by_row_index", "mask_within_tile", "mask_batch_only"):
        h = hit_matrix(key_vec, M, off, mut)
        return h, h, h, h
    none = torch.zeros_like(true)
    if mut == "mask_fwd_only":
        return true, none, none, true
    if mut == "dI_mask_transposed":
        return true, true, transposed_hits(true, off), true
    if mut == "kept_logits_unmasked":
        return true, true, none, none  # (the kept backward forms dI from what was stored)
    return true, true, true, true


# (mutant, math key) pairs at which the mutant's mask differs from the true one and the checker still accepts the result, each
# for a numerical reason that profiles/ce_hits_reference_tolerance.txt states by name.  test_ce_hits_reference_cpu.py holds
# this list to what the checker does: every pair listed is accepted, every other differing pair is rejected.
EXEMPT = frozenset({
    # twin inputs with all keys distinct: key[i] instead of key[i + off] hides column i, an ordinary negative ~20 below the
    # positive's logit of 24 (a part of e^-20 of the row's mass); no true hit exists that it could leave in
    ("key_by_row_index", (129, 1000, 128, 871, "twin", "none", "none")),
    ("key_by_row_index", (130, 700, 32, 200, "twin", "none", "none")),
    ("key_by_row_index", (321, 577, 64, 256, "twin", "none", "zipf")),
    ("key_by_row_index", (385, 449, 50, 64, "twin", "none", "none")),
    ("key_by_row_index", (77, 203, 100, 126, "twin", "none", "zipf")),
    ("key_by_row_index", (77, 203, 200, 126, "twin", "none", "none")),
    # flat, pairs, off = 871 (odd): the transposed mask differs in ONE element, row 0's partner column 870 just outside the
    # positives' block; p ~ 1 / N times coef ~ 1 / M moves one row of dI by a third of the flat bound
    ("dI_mask_transposed", (129, 1000, 100, 871, "flat", "pairs", "zipf")),
})


def watched(mut, key):
    """The quantities through which a mutant at a key can be seen by the GPU test: those it stands for, that some case of
    the key compares, and whose mask (or the forward's, which they all inherit lse from) differs from the true one."""
    M, N, D, off, cls, pattern, bias = key
    kv = keys(pattern, N)
    (tf, tu, ti, tk), (mf, mu, mi, mk) = masks(kv, M, off, None), masks(kv, M, off, mut)
    fwd = not torch.equal(tf, mf)
    moved = set()
    if fwd:
        moved |= {"ce", "lse", "du_unit"}
    if fwd or not torch.equal(tu, mu):
        moved.add("dU")
    if fwd or not torch.equal(ti, mi):
        moved.add("dI")
    if not torch.equal(tk, mk):
        moved.add("logits")
    if mut == "kept_logits_unmasked" and not any(c.entry == "keep" for c in CASES if math_key(c) == key):
        return frozenset()
    return frozenset(moved) & AFFECTS[mut] & key_compared(key)


def applies(mut, key):
    """Wherever the mutant can differ: its mask differs from the true one in a quantity that some case of the key compares."""
    return key[1] > 1 and bool(watched(mut, key))


def all_keys():
    return sorted(set(math_key(c) for c in CASES), key=str)


def evaluate(U, I, b, key_vec, coef, off, dtype, mut=None, memo=None):
    """{"ce", "lse", "logits", "du_unit", "dU", "dI"} in `dtype` (lse in natural-log units).  float32: index order, one
    rounding per operation (ce_ref's primitives).  memo carries the logits from one call to the next."""
    memo = {} if memo is None else memo
    U, I, coef = U.to(dtype), I.to(dtype), coef.to(dtype)
    M, N = U.shape[0], I.shape[0]
    rows = torch.arange(M)
    pos = rows + off
    if "Sb" not in memo:
        S = C._nt(U, I)
        memo["Sb"] = S if b is None else S + b.to(dtype)[None, :]
    Sb = memo["Sb"]
    h_f, h_u, h_i, h_k = masks(key_vec, M, off, mut)
    ninf = torch.tensor(float("-inf"), dtype=dtype)
    Sm = torch.where(h_f, ninf, Sb)
    mx = Sm.max(dim=1).values
    e = C._exp(Sm - mx[:, None])
    l = C._sum(e)
    lse = mx + C._log(l)
    ce = lse - Sb[rows, pos]
    P = e / l[:, None]
    du_unit = C._nn(P, I) - I[pos]
    if torch.equal(h_u, h_f):
        dU = coef[:, None] * du_unit
    else:
        dU = coef[:, None] * (C._nn(C._exp(torch.where(h_u, ninf, Sb) - lse[:, None]), I) - I[pos])
    G = P.clone() if torch.equal(h_i, h_f) else C._exp(torch.where(h_i, ninf, Sb) - lse[:, None])
    G[rows, pos] -= 1.0
    dI = C._tn(G * coef[:, None], U)
    logits = torch.where(h_k, torch.tensor(NEG_BIG, dtype=dtype), Sb * C.LOG2E)
    return {"ce": ce, "lse": lse, "logits": logits, "du_unit": du_unit, "dU": dU, "dI": dI}


def reference(key, unmask=None):
    """float64 quantities of a math_key: masked_fill(-inf) + logsumexp, torch autograd through sum(coef ce), the weighted
    mean loss of the fused loss form.  unmask = (i, j): that one hit is left in (condition (b) of the twin class)."""
    U32, I32, b, kv, coef, labels = inputs(key)
    M, off = key[0], key[3]
    U, I = U32.double().requires_grad_(True), I32.double().requires_grad_(True)
    S = U @ I.t()
    if b is not None:
        S = S + b.double()[None, :]
    hit = hit_matrix(kv, M, off)
    if unmask is not None:
        hit = hit.clone()
        hit[unmask] = False
    rows = torch.arange(M)
    Sm = S.masked_fill(hit, float("-inf"))
    lse = torch.logsumexp(Sm, dim=1)
    ce = lse - S[rows, rows + off]
    dU, dI = torch.autograd.grad((ce * coef.double()).sum(), [U, I])
    with torch.no_grad():
        P = torch.exp(Sm - lse[:, None])
        du_unit = P @ I - I[rows + off]
        w, coef_w, loss = C.weighted_loss(ce, labels)
        logits = (S * C.LOG2E).masked_fill(hit, NEG_BIG)
        ce_unmasked = torch.logsumexp(S, dim=1) - S[rows, rows + off]
        cmax, imax, umax = float(coef.abs().max()), float(I.detach().abs().max()), float(U.detach().abs().max())
        top = float(lse.detach().abs().max())
        scale = {"ce": top, "lse": top, "logits": float((S.detach() * C.LOG2E).abs().max()), "du_unit": imax, "dU": cmax * imax,
                 "dI": cmax * umax}
        return {"ce": ce.detach(), "lse": lse.detach(), "logits": logits.detach(), "du_unit": du_unit, "dU": dU, "dI": dI,
                "w": w, "coef_w": coef_w, "loss": loss, "hit": hit, "ce_unmasked": ce_unmasked.detach(), "scale": scale}


_ref_cache = {}


def key_reference(key):
    """reference(key), computed once per key.  Leave it unchanged."""
    if key not in _ref_cache:
        _ref_cache[key] = reference(key)
    return _ref_cache[key]


def case_reference(c):
    return key_reference(math_key(c))


# ------------------------------------------------------------------ tolerances
def tol(cls, name, ref):
    """(a, m, r) of |got - ref| <= a + m max|ref| + r |ref| (twin: a = 4 x yardstick x the quantity's scale, m = 0)."""
    if cls == "flat":
        return C.tol("flat", name)
    return (C.FACTOR * max(YARD_TWIN[name], C.FLOOR) * ref["scale"][name], 0.0, C.RTOL[name])


def ratios(got, ref, cls):
    """{quantity: worst err / bound}.  A kept logit of a hit must BE NEG_BIG (it is compared exactly: inf otherwise)."""
    out = {}
    for n in got:
        if n not in QUANTITIES:
            continue
        g, r = got[n], ref[n]
        if n == "logits":
            hit = ref["hit"].to(g.device)
            if not bool((g[hit] == NEG_BIG).all()):
                out[n] = float("inf")
                continue
            g = torch.where(hit, torch.zeros_like(g), g)
            r = torch.where(ref["hit"], torch.zeros_like(r), r)
        out[n] = C.ratio(g, r, tol(cls, n, ref))
    return out


def loss_tolerances(ref, cls):
    """ce_ref.loss_tolerances with this module's ce bound."""
    ce_t = tol(cls, "ce", ref)
    ce_bound = ce_t[0] + ce_t[1] * float(ref["ce"].abs().max()) + ce_t[2] * ref["ce"].abs()
    M = ref["ce"].shape[0]
    adds = M / 1024 + 6 + 16 + 2
    loss_bound = float((ce_bound * ref["w"]).sum()) / M + (adds + 8) * C.FLOOR * float((ref["ce"].abs() * ref["w"]).sum()) / M
    return {"w": (0.0, 8 * C.FLOOR, 0.0), "coef_w": (0.0, 8 * C.FLOOR, 0.0), "loss": (loss_bound, 0.0, 0.0)}


def twin_keys():
    return sorted(set(math_key(c) for c in CASES if c.cls == "twin"), key=str)


def measure(keys_=None):
    """Worst normalised error of the float32 evaluation per quantity over the twin cases' math keys, and where."""
    worst = {q: (0.0, None) for q in QUANTITIES}
    for key in (twin_keys() if keys_ is None else keys_):
        U, I, b, kv, coef, _ = inputs(key)
        ref = key_reference(key)
        got = evaluate(U, I, b, kv, coef, key[3], F32)
        for q in QUANTITIES:
            g, r = got[q], ref[q]
            if q == "logits":
                g, r = torch.where(ref["hit"], torch.zeros_like(g), g), torch.where(ref["hit"], torch.zeros_like(r), r)
            e = float(((g.double() - r).abs() - C.RTOL[q] * r.abs()).clamp_min(0.0).max()) / ref["scale"][q]
            if e >= worst[q][0]:
                worst[q] = (e, key)
    return worst


def main():
    print("twin: float32 CPU evaluation against float64, worst max((|err| - r |ref|)+) / scale")
    worst = measure()
    print("measured " + " ".join(f"{q} {worst[q][0]:.3e}" for q in QUANTITIES))
    print("recorded " + " ".join(f"{q} {YARD_TWIN[q]:.1e}" for q in QUANTITIES))
    for q in QUANTITIES:
        print(f"  worst {q} at {worst[q][1]}")
    assert all(worst[q][0] <= YARD_TWIN[q] for q in QUANTITIES), "YARD_TWIN is below the measured worst case"


if __name__ == "__main__":
    main()
