"""Float64 yardstick for the Adam kernels (csrc/adam.hip).  A helper, not a test: imported by test_adam_reference_cpu.py
and test_gpu_adam.py the way sharded_cpu_backend.py is imported by its tests; the product never imports it.

  adam_step64   torch.optim.Adam's single-tensor formula in float64, out of place
  edge_state    fp32 p, m, v with the states a kernel can get wrong (tiny / denormal / zero v, sqrt(v) near eps, +-0, 1e30)
  bounds        the float64 trajectory of K steps and the element-wise error a fp32 implementation may show against it

The error model.  Per step and element, with eps32 = 2^-23, TINY = 2^-149 (the fp32 denormal spacing: below it "an ulp of
the value" stops shrinking) and mag_m = max(|m_old|, |m_new|) (m_new = 0.9 m + 0.1 g cancels: the rounding of the operands
is proportional to THEIR size, not to the size of what is left):

  m:  c_m * max(eps32 * mag_m, TINY)
  v:  c_v * max(eps32 * v_new, TINY)                                  (no cancellation: every term is >= 0)
  p:  ulp(max(|p_old|, |p_new|)) / 2                                  (the rounding of p += ..., whatever the update)
      + c_p * max(eps32 * step_size * mag_m / denom, TINY)            (the update, at the operand magnitude of m)

and over K steps the per-step terms are summed along the float64 trajectory: both moment recurrences are contractions
(factors 0.9 and 0.999), so an error made at one step never grows at a later one.

The constants are not chosen, they are measured: ORACLE_C is the worst case of the project's own IEEE fp32 restatement
(oracle.cpu_ref.adam_update: correctly rounded sqrt and division) against adam_step64 on edge_state inputs, rounded up to
two digits; `python tests/adam_ref.py` repeats the measurement.  KERNEL_C = 4 x ORACLE_C: adam_ratio() replaces the IEEE
square root and the two divisions by v_sqrt_f32, v_rcp_f32 (1 ulp each) and a prepared reciprocal of sqrt(bc2) -- three
extra roundings on the update, none on m and v.  profiles/adam_reference_tolerance.txt records both and what the GPU
showed."""
import math
from collections import namedtuple

import torch

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
EPS32 = 2.0 ** -23
TINY = 2.0 ** -149

# worst case of oracle.cpu_ref.adam_update against adam_step64, one step, steps 1 .. 10^6, 5 widths x 3 seeds (see main())
ORACLE_C = {"p": 2.7, "m": 1.3, "v": 1.4}
KERNEL_C = {k: 4.0 * c for k, c in ORACLE_C.items()}

Ref = namedtuple("Ref", "p m v bp bm bv")


def adam_step64(p, m, v, g, step, lr=LR, b1=B1, b2=B2, eps=EPS):
    """One torch.optim.Adam step (no weight decay, no amsgrad) in float64 -> new (p, m, v); inputs are converted exactly."""
    p, m, v, g = (t.detach().cpu().double() for t in (p, m, v, g))
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    p = p - (lr / bc1) * (m / denom)
    return p, m, v


def hyper64(step, lr=LR, b1=B1, b2=B2):
    """hyper[4..6] after the advance to `step`, in double: step, lr / (1 - b1^t), sqrt(1 - b2^t)."""
    return float(step), lr / (1.0 - b1 ** step), math.sqrt(1.0 - b2 ** step)


def edge_state(n_rows, D, seed):
    """fp32 p, m, v of an n_rows x D table (n_rows >= 8, D >= 16):
    half the elements |p| ~ 1, half |p| ~ 1e-3 (the update is then far above ulp(p)); m ~ 0.01 N(0,1); v ~ 1e-4 U;
    rows 3 .. 3 + n_rows // 8: v in [1e-16, 1e-14] (sqrt(v) = 1 .. 10 eps), m scaled by 1e-6;
    rows 1 and n_rows // 2: m = v = 0;  row 2 of a table wider than 256 columns: m = v = 0 in columns 0 .. 255 only;
    single elements of row 0 and of the last row: m = 0 with v != 0, v = 1e-40, m = 1e-41, p = +0, p = -0, p = 1e30."""
    assert n_rows >= 8 and D >= 16
    gen = torch.Generator().manual_seed(1000003 * seed + 31 * n_rows + D)
    p = torch.randn(n_rows, D, generator=gen)
    small = torch.rand(n_rows, D, generator=gen) < 0.5
    p = torch.where(small, p * 1e-3, p)
    m = torch.randn(n_rows, D, generator=gen) * 0.01
    v = torch.rand(n_rows, D, generator=gen) * 1e-4
    r0, r1 = 3, 3 + max(1, n_rows // 8)
    v[r0:r1] = 10.0 ** (-16.0 + 2.0 * torch.rand(r1 - r0, D, generator=gen))
    m[r0:r1] *= 1e-6
    for r in (1, n_rows // 2):
        m[r] = 0.0
        v[r] = 0.0
    if D > 256:
        m[2, :256] = 0.0
        v[2, :256] = 0.0
    for r in (0, n_rows - 1):
        m[r, 0] = 0.0
        v[r, 1] = 1e-40
        m[r, 2] = 1e-41
        p[r, 3] = 0.0
        p[r, 4] = -0.0
        p[r, 5] = 1e30
        v[r, 6] = 1e-40
        m[r, 6] = 1e-41
    return p.contiguous(), m.contiguous(), v.contiguous()


def edge_flat(n, seed):
    """The first n elements of an edge_state table of 64-wide rows (the sweeps take flat arrays)."""
    rows = max(8, (n + 63) // 64)
    return tuple(t.reshape(-1)[:n].clone() for t in edge_state(rows, 64, seed))


def ulp32(x):
    """Spacing of fp32 at |x| (x in float64), 2^-149 below the normal range."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))  # |x| = f * 2^e, f in [0.5, 1)
    return torch.ldexp(torch.ones_like(x), e - 24)


def step_terms(p, m, v, g, step, lr=LR, b1=B1, b2=B2, eps=EPS):
    """One float64 step -> new p, m, v and the error model's terms for it: the half ulp of p and the units that c_p, c_m
    and c_v multiply."""
    p, m, v, g = (t.detach().cpu().double() for t in (p, m, v, g))
    tiny = torch.full_like(p, TINY)
    p1, m1, v1 = adam_step64(p, m, v, g, step, lr, b1, b2, eps)
    mag_m = torch.maximum(m.abs(), m1.abs())
    denom = v1.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    upd = (lr / (1.0 - b1 ** step)) * mag_m / denom
    half = 0.5 * ulp32(torch.maximum(p.abs(), p1.abs()))
    return (p1, m1, v1, half, torch.maximum(EPS32 * upd, tiny), torch.maximum(EPS32 * mag_m, tiny),
            torch.maximum(EPS32 * v1, tiny))


def bounds(p, m, v, grads, first_step, c=None, lr=LR, b1=B1, b2=B2, eps=EPS):
    """K = len(grads) steps first_step, first_step + 1, ... (or the steps listed in `first_step`) from fp32 (p, m, v);
    grads[k] is a tensor or None (zero gradient).
    -> Ref(p, m, v: the float64 trajectory's end;  bp, bm, bv: the element-wise error allowed against it, constants c)."""
    c = KERNEL_C if c is None else c
    p, m, v = (t.detach().cpu().double() for t in (p, m, v))
    bp, bm, bv = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    zero = torch.zeros_like(p)
    steps = [first_step + k for k in range(len(grads))] if isinstance(first_step, int) else list(first_step)
    for step, g in zip(steps, grads):
        p, m, v, half, up, um, uv = step_terms(p, m, v, zero if g is None else g, step, lr, b1, b2, eps)
        bp += half + c["p"] * up
        bm += c["m"] * um
        bv += c["v"] * uv
    return Ref(p, m, v, bp, bm, bv)


def ratios(got, ref):
    """Worst |got - ref| / bound per tensor -> {"p": .., "m": .., "v": ..}; <= 1 means within bounds."""
    out = {}
    for name, x, want, b in (("p", got[0], ref.p, ref.bp), ("m", got[1], ref.m, ref.bm), ("v", got[2], ref.v, ref.bv)):
        out[name] = float(((x.detach().cpu().double() - want).abs() / b).max())
    return out


def violations(got, ref):
    """Elements outside the bound per tensor (every element is checked; NaN counts)."""
    out = {}
    for name, x, want, b in (("p", got[0], ref.p, ref.bp), ("m", got[1], ref.m, ref.bm), ("v", got[2], ref.v, ref.bv)):
        out[name] = int((~((x.detach().cpu().double() - want).abs() <= b)).sum())
    return out


def measured_constants(got, p, m, v, g, step):
    """c_p, c_m, c_v that ONE step of an fp32 implementation (`got`, from fp32 p, m, v, g) needs under the model above."""
    p1, m1, v1, half, up, um, uv = step_terms(p, m, v, g, step)
    ep = ((got[0].double() - p1).abs() - half).clamp_min(0.0) / up
    em = (got[1].double() - m1).abs() / um
    ev = (got[2].double() - v1).abs() / uv
    assert not (torch.isnan(ep).any() or torch.isnan(em).any() or torch.isnan(ev).any())
    return {"p": float(ep.max()), "m": float(em.max()), "v": float(ev.max())}


STEPS = (1, 2, 10, 1000, 65535, 65536, 10 ** 6)
WIDTHS = (32, 50, 128, 200, 320)


def oracle_step(p, m, v, g, step):
    from oracle import cpu_ref as R
    p, m, v = p.clone(), m.clone(), v.clone()
    R.adam_update(p, g, m, v, step, LR, B1, B2, EPS)
    return p, m, v


def main():
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    print("oracle.cpu_ref.adam_update (IEEE fp32) against adam_step64, one step, 97 rows x D, seeds 0-2, gradient 0.01 N and 0")
    print(f"{'step':>8} {'c_p':>7} {'c_m':>7} {'c_v':>7}")
    for step in STEPS:
        at = {"p": 0.0, "m": 0.0, "v": 0.0}
        for D in WIDTHS:
            for seed in range(3):
                p, m, v = edge_state(97, D, seed)
                gen = torch.Generator().manual_seed(seed + 7)
                g = torch.randn(97, D, generator=gen) * 0.01
                g[::2] = 0.0  # untouched rows
                got = oracle_step(p, m, v, g, step)
                for k, x in measured_constants(got, p, m, v, g, step).items():
                    at[k] = max(at[k], x)
        print(f"{step:>8} {at['p']:7.3f} {at['m']:7.3f} {at['v']:7.3f}")
        for k in worst:
            worst[k] = max(worst[k], at[k])
    print("worst    " + " ".join(f"{worst[k]:7.3f}" for k in "pmv"))
    print("ORACLE_C " + " ".join(f"{ORACLE_C[k]:7.3f}" for k in "pmv"))
    print("KERNEL_C " + " ".join(f"{KERNEL_C[k]:7.3f}" for k in "pmv"))
    assert all(worst[k] <= ORACLE_C[k] for k in worst), "ORACLE_C is below the measured worst case"


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    main()
