"""tt_l2norm_fwd / tt_l2norm_bwd against float64 through the C ABI: every case of l2norm_ref.cases() -- widths on both
sides of the float4 form's 256 columns, row counts around the 4 rows of a workgroup, one and two sides, the scalar form
forced by base, row stride and width, clamped rows, every log_scale -- with the operands inside NaN-filled buffers.
Bounds and their derivation: l2norm_ref's docstring (the yardstick is measured on the CPU, never against the kernel)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import l2norm_ref as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 4  # floats in front of an "aligned" operand (torch allocations are 256-byte aligned: 16 bytes in is still aligned)


@pytest.fixture(scope="module")
def T():
    from two_tower_models_amd import _native as N
    N.load()
    return N


class Buf:
    """A [rows, D] operand with row stride ld inside a NaN-filled flat buffer."""

    def __init__(self, rows, D, layout, value=None):
        self.rows, self.D, self.ld = rows, D, L.ld_of(D, layout)
        self.off = PAD + (1 if layout == "offset1" else 0)
        self.flat = torch.full((self.off + max(rows, 1) * self.ld + PAD,), float("nan"), dtype=torch.float32, device=DEV)
        self.ptr = self.flat.data_ptr() + 4 * self.off
        assert (self.ptr % 16 != 0) == (layout == "offset1") and (self.ld % 4 != 0) == (layout == "ld_odd")
        if value is not None and rows:
            self.view().copy_(value)

    def view(self):
        return self.flat[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.D]

    def check_outside_untouched(self):
        mask = torch.ones_like(self.flat, dtype=torch.bool)
        if self.rows:
            mask[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.D] = False
        assert bool(torch.isnan(self.flat[mask]).all()), "wrote outside its rows"
        assert not bool(torch.isnan(self.flat[~mask]).any()), "left a row element unwritten"


class SideRun:
    def __init__(self, case, si):
        side = case.sides[si]
        self.side, self.D = side, case.D
        self.x, self.dy = L.make_rows(side.rows, case.D, case.seed * 10 + si, side.first_class)
        self.bx = Buf(side.rows, case.D, side.layout, self.x)
        self.bdy = Buf(side.rows, case.D, side.layout, self.dy)
        self.by = Buf(side.rows, case.D, side.layout)
        self.bdx = Buf(side.rows, case.D, side.layout)
        self.inv = torch.full((PAD + side.rows + PAD,), float("nan"), dtype=torch.float32, device=DEV)
        self.ls = None if side.log_scale is None else torch.tensor([side.log_scale], dtype=torch.float32, device=DEV)
        self.dls = torch.full((3,), float("nan"), dtype=torch.float32, device=DEV)  # [guard, value, guard]

    def fwd_side(self, N):
        return N.L2NormFwdSide(self.bx.ptr, self.bx.ld, self.by.ptr, self.by.ld, self.inv.data_ptr() + 4 * PAD, self.side.rows, N.ptr(self.ls))

    def bwd_side(self, N, want_dls=None):
        want = self.side.want_dls if want_dls is None else want_dls
        return N.L2NormBwdSide(self.bx.ptr, self.bx.ld, self.bdy.ptr, self.bdy.ld, self.inv.data_ptr() + 4 * PAD, self.bdx.ptr,
                               self.bdx.ld, self.side.rows, N.ptr(self.ls), self.dls.data_ptr() + 4 if want else None)


def run(N, case, want_dls=None, ws_fill=None):
    lib = N.load()
    sides = [SideRun(case, i) for i in range(len(case.sides))]
    n = len(sides)
    fs = (N.L2NormFwdSide * n)(*[s.fwd_side(N) for s in sides])
    N.check(lib.tt_l2norm_fwd(fs, n, case.D, L.EPS, None), "tt_l2norm_fwd")
    bs = (N.L2NormBwdSide * n)(*[s.bwd_side(N, want_dls) for s in sides])
    need = sum(lib.tt_l2norm_bwd_workspace_bytes(s.side.rows) for s, b in zip(sides, bs) if b.d_log_scale)
    ws = torch.full((max(need, 256) // 4 + PAD,), float("nan") if ws_fill is None else ws_fill, dtype=torch.float32, device=DEV)
    N.check(lib.tt_l2norm_bwd(bs, n, case.D, L.EPS, ws.data_ptr(), need, None), "tt_l2norm_bwd")
    torch.cuda.synchronize()
    return sides, ws, need


ALL = list(L.cases())


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_kernel_matches_float64(T, case):
    sides, ws, need = run(T, case)
    again, _, _ = run(T, case)
    for s, s2 in zip(sides, again):
        side, rows, D = s.side, s.side.rows, s.D
        for b in (s.bx, s.bdy):  # inputs untouched
            b.check_outside_untouched()
        s.by.check_outside_untouched()
        s.bdx.check_outside_untouched()
        assert bool(torch.isnan(s.inv[:PAD]).all()) and bool(torch.isnan(s.inv[PAD + rows:]).all())
        assert bool(torch.isnan(s.dls[0])) and bool(torch.isnan(s.dls[2])) and bool(torch.isnan(s.dls[1])) == (not side.want_dls)
        # determinism: a second call on the same inputs, bit for bit (NaN padding included)
        for a, b in ((s.by.flat, s2.by.flat), (s.bdx.flat, s2.bdx.flat), (s.inv, s2.inv), (s.dls, s2.dls)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        if rows == 0:
            if side.want_dls:
                assert float(s.dls[1]) == 0.0
            continue
        y64, inv64 = L.forward64(s.x, side.log_scale)
        dx64, dls64, terms = L.backward64(s.x, s.dy, side.log_scale)
        inv = s.inv[PAD:PAD + rows].double().cpu()
        y, dx = s.by.view().double().cpu(), s.bdx.view().double().cpu()
        r = L.MARGIN * L.Y_REL
        e_inv = float(((inv - inv64).abs() / inv64).max())
        e_y = float(((y - y64).abs() - r * y64.abs()).max())
        print(f"{case.name} side {sides.index(s)}: inv rel {e_inv:.2e} (bound {r:.2e})", end="")
        assert e_inv <= r
        assert e_y <= 0, e_y
        zero = (s.x == 0).all(dim=1)
        assert torch.equal(y[zero], torch.zeros_like(y[zero]))  # an exactly zero row: y = 0 exactly
        rowmax = dx64.abs().amax(dim=1, keepdim=True)
        bound = L.MARGIN * L.Y_DX * rowmax + r * dx64.abs()
        if D == 1:  # identically zero gradient on unclamped rows: the absolute bound from the formats (l2norm_ref docstring)
            sc = 1.0 if side.log_scale is None else math.exp(float(np.float32(side.log_scale)))
            bound = torch.where(rowmax > 0, bound, L.D1_ABS * sc * inv64[:, None] * s.dy.double().abs())
        err = (dx - dx64).abs()
        live = rowmax.squeeze(1) > 0
        if bool(live.any()):
            print(f"; dx / rowmax {float((err[live] / rowmax[live]).max()):.2e} (yardstick {L.Y_DX:.1e})", end="")
        assert bool((err <= bound).all()), float((err - bound).max())
        clamped = s.x.double().norm(dim=1) <= L.EPS32
        want = (1.0 if side.log_scale is None else math.exp(float(np.float32(side.log_scale)))) * s.dy.double()[clamped] / L.EPS32
        assert bool(((dx[clamped] - want).abs() <= r * want.abs()).all())  # dx = s dy / eps on clamped rows
        if side.want_dls:
            sumabs = float(terms.abs().sum())
            e = abs(float(s.dls[1]) - float(dls64))
            print(f"; d_log_scale / sum|terms| {e / max(sumabs, 1e-300):.2e} (bound {L.MARGIN * L.Y_DLS:.2e})", end="")
            assert e <= L.MARGIN * L.Y_DLS * sumabs
        print()


def test_a_row_with_one_non_zero_element_is_a_signed_unit_vector(T):
    case = L.Case("one", 128, (L.Side(5, "aligned", None, False, 4),), 7)  # first row's class: "one"
    sides, _, _ = run(T, case)
    y = sides[0].by.view().cpu()[0]
    k = int(y.abs().argmax())
    assert k == 0 and int((y != 0).sum()) == 1 and torch.sign(y[0]) == torch.sign(sides[0].x[0, 0])
    assert abs(abs(float(y[0])) - 1.0) <= 2.0 ** -23  # sqrt(x * x) == |x| exactly; x * fl(1 / |x|) is within two roundings of 1


@pytest.mark.parametrize("D,layout", [(128, "aligned"), (50, "aligned")])
def test_fixed_temperature_call_forms_no_sum(T, D, layout):
    """d_log_scale == NULL on every side: the finishing kernel is not launched (the library's own launch record), no
    partial reaches the workspace, the would-be output word keeps its NaN; asking for it makes exactly one such launch."""
    lib = T.load()
    case = L.Case("fixed", D, (L.Side(L.ROWS_BEYOND_ONE_PASS, layout, math.log(20.0), True), L.Side(63, "aligned", None, False)), 9)

    def launches(name):
        ms, n = C.c_double(), C.c_int64()
        assert lib.tt_profile_read(name.encode(), C.byref(ms), C.byref(n)) == 0
        return n.value

    try:
        lib.tt_profile_enable(1)
        sides, ws, _ = run(T, case, want_dls=False)
        assert launches("l2norm_bwd_kernel") == 1 and launches("l2norm_finish_kernel") == 0 and launches("l2norm_fwd_kernel") == 1
        assert bool(torch.isnan(ws).all()) and bool(torch.isnan(sides[0].dls).all())
        fixed_dx = sides[0].bdx.flat.clone()
        lib.tt_profile_enable(1)  # (clears the record)
        sides, ws, need = run(T, case)
        assert launches("l2norm_bwd_kernel") == 1 and launches("l2norm_finish_kernel") == 1
        assert bool(torch.isnan(ws[need // 4:]).all()) and not bool(torch.isnan(sides[0].dls[1]))
        assert torch.equal(fixed_dx.view(torch.int32), sides[0].bdx.flat.view(torch.int32))  # dx does not depend on it
    finally:
        lib.tt_profile_enable(0)


def test_d_log_scale_is_written_not_accumulated_and_ignores_the_workspace_contents(T):
    case = L.Case("written", 128, (L.Side(L.ROWS_BEYOND_ONE_PASS, "aligned", -3.0, True),), 11)
    a, _, _ = run(T, case, ws_fill=0.0)
    b, _, _ = run(T, case, ws_fill=1.0e30)
    assert torch.equal(a[0].dls.view(torch.int32), b[0].dls.view(torch.int32))


def test_ops_take_strided_views_as_they_are(T):
    """ops.L2NormalizePair / ops.l2_normalize on column slices of wider tensors (row stride > D, base off 16 bytes: the
    scalar form) and on contiguous copies (the float4 form): one launch per direction, each within the kernel bounds of
    float64, autograd's gradients in the right rows."""
    from two_tower_models_amd import ops
    g = torch.Generator().manual_seed(3)
    wide_u = torch.randn(37, 70, generator=g).to(DEV)
    wide_v = torch.randn(50, 70, generator=g).to(DEV)
    wu, wv = torch.randn(37, 64, generator=g), torch.randn(50, 64, generator=g)  # d loss / d outputs, exactly
    ls = torch.tensor([math.log(20.0)], device=DEV, requires_grad=True)
    xu, xv = wide_u[:, 1:65].cpu(), wide_v[:, 3:67].cpu()
    r = L.MARGIN * L.Y_REL
    for u, v in ((wide_u[:, 1:65], wide_v[:, 3:67]), (wide_u[:, 1:65].contiguous(), wide_v[:, 3:67].contiguous())):
        u, v = u.detach().requires_grad_(True), v.detach().requires_grad_(True)
        T.trace = []
        try:
            yu, yv = ops.L2NormalizePair.apply(u, v, ls)
            ((yu * wu.to(DEV)).sum() + (yv * wv.to(DEV)).sum()).backward()
            calls = [c for c in T.trace if c.startswith("tt_l2norm")]
        finally:
            T.trace = None
        assert calls == ["tt_l2norm_fwd", "tt_l2norm_bwd"]
        for x, w, y, dx, scale in ((xu, wu, yu, u.grad, math.log(20.0)), (xv, wv, yv, v.grad, None)):
            y64, _ = L.forward64(x, scale)
            dx64, dls64, terms = L.backward64(x, w, scale)
            assert bool(((y.detach().double().cpu() - y64).abs() <= r * y64.abs()).all())
            bound = L.MARGIN * L.Y_DX * dx64.abs().amax(dim=1, keepdim=True) + r * dx64.abs()
            assert bool(((dx.double().cpu() - dx64).abs() <= bound).all())
            if scale is not None:
                assert abs(float(ls.grad) - float(dls64)) <= L.MARGIN * L.Y_DLS * float(terms.abs().sum())
        assert torch.equal(ops.l2_normalize(v.detach()), yv.detach())  # the serving form: the same kernel, the same bits
        ls.grad = None
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.l2_normalize(torch.zeros(2, 4))
