"""Float64 reference of the row-normalise op (csrc/l2norm.hip; include/tt_hotpath.h "row L2-normalise with a scale"), the
fp32 restatement that is its yardstick, and the kernel-level case list the GPU suite runs.

    python tests/l2norm_ref.py        # measures the yardstick on the suite's own inputs, on the CPU

forward     inv[r] = 1 / max(||x_r||, eps);  y_r = s * inv[r] * x_r,  s = exp(log_scale) (None: 1)
backward    ||x_r|| >  eps:  dx_r = s * inv[r] * (dy_r - n <n, dy_r>),  n = x_r * inv[r]
            ||x_r|| <= eps:  dx_r = s * dy_r / eps
            d_log_scale = sum_r <dy_r, y_r>

BOUND (tests/test_gpu_l2norm_reference.py), element-wise |got - ref| <= m * max|ref| + r * |ref|, max over the element's
ROW (rows of one call differ by 30 orders of magnitude), with (m, r) = MARGIN x the yardstick below:
    inv, y        purely relative:  m = 0,  r = MARGIN * Y_REL
    dx            m = MARGIN * Y_DX (dy - n <n, dy> cancels: its error scales with the row, not the element),
                  r = MARGIN * Y_REL (the factor s * inv)
    d_log_scale   a sum over rows that can cancel to nothing: its error scales with the sum of the terms' magnitudes,
                  |got - ref| <= MARGIN * Y_DLS * sum_r |<dy_r, y_r>|
    D = 1, unclamped: dx is identically 0 in exact arithmetic (dy is parallel to n) and any rounding of n = x * (1/|x|)
                  leaves dy * (1 - n^2): no multiple of |ref| = 0 bounds it.  From the formats: n = +-(1 + e), |e| <= 2u
                  (two roundings, u = 2^-24), t = n dy (1 + e2), dy - n t = -dy (2e + e2 + ...) <= 5u |dy|, times
                  c = s * inv (two more roundings): |dx| <= 2^-21 * c * |dy|.  That absolute bound is used there.
The yardstick is the restatement below against float64 -- fp32, one rounding per operation, sums in index order -- on the
inputs of `cases()`; it is never taken from the kernel.  MARGIN = 4 is the project's factor: it covers the kernel's other
summation order (4 elements per lane, xor butterfly; a tree over the partials), fused multiply-adds, and a 1-ulp exp,
reciprocal or square root.
"""
from __future__ import annotations

import math
from typing import Iterator, NamedTuple, Optional, Tuple

import numpy as np
import torch

EPS = 1e-12
EPS32 = float(np.float32(EPS))  # what the kernel sees
MARGIN = 4.0
# measured by `python tests/l2norm_ref.py` (profiles/l2norm_reference_tolerance.txt)
Y_REL = 4.6e-7   # inv 4.565e-07, y 4.477e-07 (the index-order sum of D = 516 squares)
Y_DX = 1.6e-6    # 1.540e-06 of the row's largest |dx|
Y_DLS = 4.7e-7   # 4.684e-07 of sum_r |<dy_r, y_r>|
D1_ABS = 2.0 ** -21

ROWS_PER_WG = 4        # csrc/l2norm.hip L2N_ROWS_PER_WG: one wave per row
FINISH_THREADS = 256   # csrc/l2norm.hip L2N_FINISH_THREADS: partials one pass of the finishing workgroup takes
ROWS_BEYOND_ONE_WG = ROWS_PER_WG + 1
ROWS_BEYOND_ONE_PASS = ROWS_PER_WG * FINISH_THREADS + 1  # 257 partials: thread 0 of the finish takes two


# ----------------------------------------------------------------- float64
def forward64(x: torch.Tensor, log_scale: Optional[float], eps: float = EPS32) -> Tuple[torch.Tensor, torch.Tensor]:
    x = x.double()
    s = 1.0 if log_scale is None else math.exp(float(np.float32(log_scale)))
    inv = 1.0 / x.norm(dim=1).clamp_min(eps)
    return s * inv[:, None] * x, inv


def backward64(x: torch.Tensor, dy: torch.Tensor, log_scale: Optional[float], eps: float = EPS32):
    """(dx, d_log_scale, per-row terms <dy_r, y_r>) by the closed form."""
    x, dy = x.double(), dy.double()
    s = 1.0 if log_scale is None else math.exp(float(np.float32(log_scale)))
    norm = x.norm(dim=1)
    inv = 1.0 / norm.clamp_min(eps)
    n = x * inv[:, None]
    t = (n * dy).sum(dim=1)
    dx = torch.where((norm > eps)[:, None], s * inv[:, None] * (dy - n * t[:, None]), s * dy / eps)
    terms = s * t
    return dx, terms.sum(), terms


# ----------------------------------------------------------------- fp32, one rounding per operation, index order
def _seqsum32(a: np.ndarray) -> np.ndarray:
    acc = np.zeros(a.shape[0], np.float32)
    for j in range(a.shape[1]):
        acc = (acc + a[:, j]).astype(np.float32)
    return acc


def forward32(x: np.ndarray, log_scale: Optional[float], eps: float = EPS32):
    x = x.astype(np.float32)
    s = np.float32(1.0) if log_scale is None else np.exp(np.float32(log_scale))
    norm = np.sqrt(_seqsum32(x * x))
    with np.errstate(divide="ignore"):
        inv = np.where(norm > np.float32(eps), np.float32(1.0) / norm, np.float32(1.0) / np.float32(eps)).astype(np.float32)
    c = (s * inv).astype(np.float32)
    return (c[:, None] * x).astype(np.float32), inv


def backward32(x: np.ndarray, dy: np.ndarray, inv: np.ndarray, log_scale: Optional[float], eps: float = EPS32):
    x, dy = x.astype(np.float32), dy.astype(np.float32)
    s = np.float32(1.0) if log_scale is None else np.exp(np.float32(log_scale))
    n = (x * inv[:, None]).astype(np.float32)
    t = _seqsum32(n * dy)
    c = (s * inv).astype(np.float32)
    clamped = ~(inv < np.float32(1.0) / np.float32(eps))
    p = np.where(clamped, np.float32(0.0), t).astype(np.float32)
    dx = (c[:, None] * (dy - (n * p[:, None]).astype(np.float32)).astype(np.float32)).astype(np.float32)
    terms = (s * t).astype(np.float32)
    total = np.float32(0.0)
    for v in terms:
        total = np.float32(total + v)
    return dx, total


# ----------------------------------------------------------------- the suite's inputs
CLASSES = ("gauss", "tiny", "huge", "zero", "one")  # rows of a side take them in turn (a side of one row: its first)


def make_rows(rows: int, D: int, seed: int, first_class: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x, dy) float32 [rows, D].  Row r is of class CLASSES[(first_class + r) % 5]: gaussian; gaussian * 1e-15 (below
    eps = 1e-12: a clamped row that is not zero) and * 1e15 (the fp32 squares stay finite and normal); exactly zero; one
    non-zero element."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g, dtype=torch.float32)
    dy = torch.randn(rows, D, generator=g, dtype=torch.float32)
    for r in range(rows):
        k = CLASSES[(first_class + r) % len(CLASSES)]
        if k == "tiny":
            x[r] *= 1e-15
        elif k == "huge":
            x[r] *= 1e15
        elif k == "zero":
            x[r] = 0.0
        elif k == "one":
            keep = float(x[r, r % D])
            x[r] = 0.0
            x[r, r % D] = keep if keep != 0.0 else 1.0
    return x, dy


class Side(NamedTuple):
    rows: int
    layout: str                 # "aligned" | "offset1" (base one float past 16-byte alignment) | "ld_odd" (ld % 4 != 0)
    log_scale: Optional[float]  # None: NULL pointer
    want_dls: bool
    first_class: int = 0


class Case(NamedTuple):
    name: str
    D: int
    sides: Tuple[Side, ...]
    seed: int


LOG_SCALES = (None, 0.0, math.log(20.0), -3.0)
DIMS = (1, 3, 4, 50, 64, 128, 252, 256, 260, 516)
ROW_PAIRS = ((1, 2), (4, 5), (63, 257), (5, 1), (2, 63), (257, 4))


def cases() -> Iterator[Case]:
    n = 0
    # every D with two row pairs each (all six row counts per three Ds), two sides of different sizes, scales in turn
    for i, D in enumerate(DIMS):
        for k in range(2):
            r0, r1 = ROW_PAIRS[(2 * i + k) % len(ROW_PAIRS)]
            ls = LOG_SCALES[(i + k) % 4]
            yield Case(f"D{D}_rows{r0}+{r1}", D, (Side(r0, "aligned", ls, ls is not None, n), Side(r1, "aligned", None, False, n + 2)), 100 + n)
            n += 1
    # the scalar form forced on vector-eligible widths: by the base, by the row stride (D % 4 != 0 is in the list above)
    for D in (4, 64, 128, 256, 260, 516):
        for layout in ("offset1", "ld_odd"):
            ls = LOG_SCALES[n % 4]
            yield Case(f"D{D}_{layout}", D, (Side(5, layout, ls, ls is not None, n), Side(63, "aligned", None, False, n)), 100 + n)
            n += 1
    # ... and on one side only of a call (the form is chosen per side)
    yield Case("D128_side1_offset1", 128, (Side(63, "aligned", math.log(20.0), True), Side(5, "offset1", None, False)), 100 + n)
    # every log_scale at the width the model uses; both sides scaled, each with its own sum
    for j, ls in enumerate(LOG_SCALES):
        yield Case(f"D128_scale{j}", 128, (Side(257, "aligned", ls, ls is not None), Side(63, "aligned", ls, ls is not None, 3)), 200 + j)
    # one-side calls
    for D, rows in ((128, 257), (50, 63), (1, 5), (516, 2)):
        yield Case(f"D{D}_oneside_rows{rows}", D, (Side(rows, "aligned", -3.0, True),), 300 + D)
    # a side without rows: first, second, and alone with a d_log_scale (0 is written)
    yield Case("D64_rows0+5", 64, (Side(0, "aligned", 0.0, True), Side(5, "aligned", None, False)), 400)
    yield Case("D64_rows5+0", 64, (Side(5, "aligned", math.log(20.0), True), Side(0, "aligned", None, False)), 401)
    yield Case("D3_rows0", 3, (Side(0, "aligned", -3.0, True),), 402)
    # d_log_scale beyond one workgroup's share and beyond one pass of the finishing workgroup, both forms
    for D, layout in ((128, "aligned"), (50, "aligned"), (260, "ld_odd")):
        yield Case(f"D{D}_{layout}_rows{ROWS_BEYOND_ONE_PASS}", D,
                   (Side(ROWS_BEYOND_ONE_PASS, layout, math.log(20.0), True), Side(ROWS_BEYOND_ONE_WG, "aligned", 0.0, True, 1)), 500 + D)


def ld_of(D: int, layout: str) -> int:
    if layout == "ld_odd":
        return D + 4 + (1 if (D + 5) % 4 else 2)  # > D and not a multiple of 4
    return (D + 3) // 4 * 4 + 4                    # a multiple of 4, wider than D


# ----------------------------------------------------------------- yardstick
def measure() -> dict:
    worst = {"rel_inv": 0.0, "rel_y": 0.0, "dx_rowmax": 0.0, "dls_sumabs": 0.0, "d1_abs": 0.0}
    for case in cases():
        for si, side in enumerate(case.sides):
            if side.rows == 0:
                continue
            x, dy = make_rows(side.rows, case.D, case.seed * 10 + si, side.first_class)
            y64, inv64 = forward64(x, side.log_scale)
            dx64, dls64, terms64 = backward64(x, dy, side.log_scale)
            y32, inv32 = forward32(x.numpy(), side.log_scale)
            dx32, dls32 = backward32(x.numpy(), dy.numpy(), inv32, side.log_scale)
            y64, inv64, dx64 = y64.numpy(), inv64.numpy(), dx64.numpy()
            nz = y64 != 0
            worst["rel_inv"] = max(worst["rel_inv"], float(np.max(np.abs(inv32 - inv64) / inv64)))
            if nz.any():
                worst["rel_y"] = max(worst["rel_y"], float(np.max(np.abs(y32 - y64)[nz] / np.abs(y64)[nz])))
            assert np.all(y32[~nz] == 0)
            rowmax = np.abs(dx64).max(axis=1)
            live = rowmax > 0
            if case.D == 1:
                s = 1.0 if side.log_scale is None else math.exp(float(np.float32(side.log_scale)))
                dead = ~live
                if dead.any():
                    ref_scale = s * inv64[dead] * np.abs(dy.numpy()[dead, 0])
                    worst["d1_abs"] = max(worst["d1_abs"], float(np.max(np.abs(dx32[dead, 0]) / ref_scale)))
            if live.any():
                # the relative part (factor s * inv) is taken out at the yardstick's own Y_REL share: what is left scales with the row
                err = np.abs(dx32 - dx64)[live]
                worst["dx_rowmax"] = max(worst["dx_rowmax"], float(np.max(err / rowmax[live][:, None])))
            sumabs = float(terms64.abs().sum())
            if side.want_dls and sumabs > 0:
                worst["dls_sumabs"] = max(worst["dls_sumabs"], abs(float(dls32) - float(dls64)) / sumabs)
    return worst


if __name__ == "__main__":
    w = measure()
    u = 2.0 ** -24
    print(f"cases: {sum(1 for _ in cases())}")
    for k, v in w.items():
        print(f"{k:12s} {v:.3e}  ({v / u:.2f} u)")
    # the constants above are these figures rounded up to two digits; D1_ABS is derived, the measurement only has to fit
    for const, got in ((Y_REL, max(w["rel_inv"], w["rel_y"])), (Y_DX, w["dx_rowmax"]), (Y_DLS, w["dls_sumabs"])):
        assert got <= const <= 1.05 * got, (const, got)
    assert w["d1_abs"] <= D1_ABS
    print(f"bounds: MARGIN {MARGIN:g} x (Y_REL {Y_REL:.1e}, Y_DX {Y_DX:.1e}, Y_DLS {Y_DLS:.1e}); D = 1: {D1_ABS:.3e} * c * |dy|")
