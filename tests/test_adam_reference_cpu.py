"""The yardstick of test_gpu_adam.py can fail: adam_ref.bounds holds for the IEEE fp32 oracle at every step count the GPU
tests use, adam_step64 IS torch.optim.Adam, and every mutated formula a kernel could plausibly implement is outside the
bounds the kernels are held to (KERNEL_C)."""
import math

import pytest
import torch

import adam_ref as AR

ROWS = 97


def _inputs(D, seed):
    p, m, v = AR.edge_state(ROWS, D, seed)
    gen = torch.Generator().manual_seed(seed + 7)
    g = torch.randn(ROWS, D, generator=gen) * 0.01
    g[::2] = 0.0  # untouched rows: zero gradient
    return p, m, v, g


@pytest.mark.parametrize("step", AR.STEPS)
def test_oracle_adam_is_within_bounds_of_float64(step):
    """oracle.cpu_ref.adam_update (fp32, correctly rounded operations) against adam_step64 under the constants measured
    for it (ORACLE_C, x 1): every element, every width, three seeds."""
    for D in AR.WIDTHS:
        for seed in range(3):
            p, m, v, g = _inputs(D, seed)
            ref = AR.bounds(p, m, v, [g], step, c=AR.ORACLE_C)
            got = AR.oracle_step(p, m, v, g, step)
            assert AR.violations(got, ref) == {"p": 0, "m": 0, "v": 0}, (D, seed, AR.ratios(got, ref))


@pytest.mark.parametrize("K,rows,D,idle", [(40, 257, 200, False), (1200, 64, 128, True)])
def test_oracle_adam_stays_within_bounds_over_many_steps(K, rows, D, idle):
    """The K-step form (per-step terms summed along the float64 trajectory) at the lengths the GPU tests run: 40 steps
    with sparse gradients, 1200 idle steps.  The idle run also shows the fixed point the deferred schedule must reproduce:
    fp32 m <- fma(0.1, -m, m) does not reach zero, it sticks at a few denormal units."""
    p, m, v = AR.edge_state(rows, D, 0)
    gen = torch.Generator().manual_seed(1)
    grads = [None if idle else torch.randn(rows, D, generator=gen) * 0.01 * (torch.rand(rows, 1, generator=gen) < 0.2)
             for _ in range(K)]
    ref = AR.bounds(p, m, v, grads, 7, c=AR.ORACLE_C)
    got = (p, m, v)
    for k, g in enumerate(grads):
        got = AR.oracle_step(*got, torch.zeros_like(p) if g is None else g, 7 + k)
    assert AR.violations(got, ref) == {"p": 0, "m": 0, "v": 0}, AR.ratios(got, ref)
    if idle:
        stuck = (got[1] != 0) & (got[1].abs() < 2.0 ** -126)
        assert int(stuck.sum()) > 0 and float(got[1].abs().max()) < 1e-43


def test_adam_step64_is_torch_optim_adam_in_float64():
    gen = torch.Generator().manual_seed(3)
    w = torch.nn.Parameter(torch.randn(33, 20, generator=gen, dtype=torch.float64))
    opt = torch.optim.Adam([w], lr=AR.LR, betas=(AR.B1, AR.B2), eps=AR.EPS)
    p, m, v = w.detach().clone(), torch.zeros_like(w), torch.zeros_like(w)
    for step in range(1, 6):
        g = torch.randn(33, 20, generator=gen, dtype=torch.float64) * 0.01
        g[::3] = 0.0
        w.grad = g.clone()
        opt.step()
        p, m, v = AR.adam_step64(p, m, v, g, step)
        st = opt.state[w]
        assert torch.allclose(w.detach(), p, rtol=1e-13, atol=0.0), step
        assert torch.allclose(st["exp_avg"], m, rtol=1e-13, atol=1e-300) and torch.allclose(st["exp_avg_sq"], v, rtol=1e-13, atol=1e-300)
    # ... and from a non-trivial state at a late step: edge_state moments injected as the optimiser's state
    p0, m0, v0 = (t.double() for t in AR.edge_state(ROWS, 50, 1))
    g = torch.randn(ROWS, 50, generator=gen, dtype=torch.float64) * 0.01
    w = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([w], lr=AR.LR, betas=(AR.B1, AR.B2), eps=AR.EPS)
    opt.state[w] = {"step": torch.tensor(999.0), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    w.grad = g.clone()
    opt.step()
    p, m, v = AR.adam_step64(p0, m0, v0, g, 1000)
    assert torch.allclose(w.detach(), p, rtol=1e-13, atol=1e-300)
    assert torch.allclose(opt.state[w]["exp_avg"], m, rtol=1e-13, atol=1e-300)


def _mutant(kind, p, m, v, g, step):
    lr, b1, b2, eps = AR.LR, AR.B1, AR.B2, AR.EPS
    p, m, v, g = (t.double() for t in (p, m, v, g))
    m1 = m + (g - m) * (1.0 - b1)
    v1 = v * b2 + (1.0 - b2) * g * g
    t = step
    if kind == "step-1":
        t = step - 1
    elif kind == "step+1":
        t = step + 1
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    if kind == "no-bc2":
        bc2 = 1.0
    if kind == "no-bc1":
        bc1 = 1.0
    if kind == "eps/sqrt(bc2)":
        denom = (v1.sqrt() + eps) / math.sqrt(bc2)
    elif kind == "eps-in-sqrt":
        denom = (v1 / bc2 + eps).sqrt()
    else:
        denom = v1.sqrt() / math.sqrt(bc2) + eps
    if kind == "v-kept-where-g=0":
        v1 = torch.where(g == 0, v, v1)
    return p - (lr / bc1) * (m1 / denom), m1, v1


TINY_V_ROWS = slice(3, 3 + ROWS // 8)  # edge_state's block with sqrt(v) = 1 .. 10 eps


@pytest.mark.parametrize("kind,step,tensor,rows", [
    ("step-1", 2, "p", None), ("step-1", 10, "p", None), ("step+1", 2, "p", None), ("step+1", 10, "p", None),
    ("no-bc2", 1000, "p", None), ("no-bc1", 2, "p", None), ("eps/sqrt(bc2)", 10, "p", TINY_V_ROWS),
    ("eps-in-sqrt", 1, "p", None), ("eps-in-sqrt", 1000, "p", None), ("eps-in-sqrt", 10 ** 6, "p", None),
    ("v-kept-where-g=0", 10, "v", None)])
def test_mutated_formulas_violate_the_kernel_bounds(kind, step, tensor, rows):
    """A float64 (i.e. otherwise exact) implementation of each wrong formula is outside KERNEL_C's bounds on a non-zero
    number of elements at the steps where it differs -- and the unmutated formula on none.  Shares observed with these
    constants (printed): the bias-correction mutants 97-99 % of p, eps / sqrt(bc2) 86 % of the tiny-v block, eps inside the
    root 14 % (step 1) to 89 % (step 10^6), v kept where g = 0 49 % of v (every element of the zero-gradient rows with
    v != 0)."""
    p, m, v, g = _inputs(128, 0)
    ref = AR.bounds(p, m, v, [g], step)  # KERNEL_C
    i = "pmv".index(tensor)
    sel = slice(None) if rows is None else rows
    bad = _mutant(kind, p, m, v, g, step)
    err = (bad[i] - ref[i]).abs()[sel]
    n_bad = int((~(err <= ref[3 + i][sel])).sum())
    print(f"{kind} @ {step}: {n_bad} of {err.numel()} elements of {tensor} outside the bounds ({100.0 * n_bad / err.numel():.1f} %)")
    assert n_bad > 0
    good = _mutant("none", p, m, v, g, step)
    assert AR.violations(good, ref) == {"p": 0, "m": 0, "v": 0}
