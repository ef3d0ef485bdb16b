"""Float64 yardstick for the fused tower (csrc/tower.hip behind tt_tower_fwd, tt_tower_bwd_data and tt_tower_bwd_weights).  A
helper, not a test: imported by test_tower_reference_cpu.py and test_gpu_tower_reference.py the way gemm_ref.py is imported
by its tests; the product never imports it.

  entries     fwd, bwd, wgrad, each called with inputs of its own: tt_tower_bwd_data takes h, dy, W2, W3 and
              tt_tower_bwd_weights dy, tin, d_f, h, dh, feats, extra as independent operands.  Only the forward is a chain,
              and it exposes its intermediates (h_out, tin_out).
  inputs      from fixture_gen, one flat stream per operand kind and side, hashed by ELEMENT INDEX: a smaller B is a prefix
              of a larger one.
                exact   fg.trits everywhere; batch rows (feats / dy) times 2^((m % 5) - 2).  Every product and partial sum
                        of every stage is a multiple of 2^-2 below 2^22 (test_tower_reference_cpu.py asserts it from the
                        reference's Abs), so ANY summation order gives the float64 result and the checker demands equality,
                        the forward end to end from its inputs.  wgrad: trits directly (sums over B <= 8257).
                flat    fg.gaussianish, never rounded
                range   batch rows (fwd: feats and extra; bwd: dy; wgrad: dy, d_f, dh) scaled by 2^(4 g), g gaussianish
  reference   float64, stage by stage.  Forward: h from feats, W1, b1; tin_out[:, :D] must be the table rows BIT FOR BIT
              (zero rows for out-of-range ids); tin_out[:, D:] from the kernel's own h_out; y from the kernel's own tin_out
              (and extra) -- a ReLU decision within the bound of zero does not propagate.  Backward: d_tin = dy W3 split
              into d_emb | d_f | d_extra; dh = (d_f W2) [h > 0] from the kernel's own d_f, the mask on h, not on the value;
              h carries -0.0, +0.0, 2^-126, -2^-126 at h_plants(): only 2^-126 passes.  Wgrad: the six tensors
              dW3 [D, 2D + E] = dy^T [tin | extra], dW2 = d_f^T h, dW1 = dh^T feats, db3, db2, db1.
              The forward's fmaxf(NaN, 0) = 0 differs from torch's ReLU on a NaN input (torch gives NaN): no input here is
              NaN and neither behaviour is asserted.
  YARD        the worst |s32 - s64| / (2^-24 Abs) of a float32 index-order evaluation (gemm_ref.index_order_f32) of the
              reference's own operands per (class, reduction-length band): "F" (F + 1), "hid" (256 + 1), "2D" / "4D" (the
              tower input without / with the third block, + 1), "D" (the backward's two products) and "B" (wgrad).  `python tests/tower_ref.py` prints the table,
              test_tower_reference_cpu.py re-measures it.  Never calibrated against a kernel.
  bound       per element E = 4 YARD 2^-24 Abs + 2^-24 |result| (the factor 4 is the project's).  h_out elements whose
              pre-activation is within E of zero accept either branch; they are counted, at most BAND_SHARE of a case.
  buffers     every operand and output is a view into a larger NaN-filled buffer; outputs are NaN-prefilled.  check() wants
              every logical element finite and within E, every byte outside each output view unchanged (ld padding columns,
              rows before and after, the floats past the reported workspace size) and the out-of-range flag right.
  CASES       every call test_gpu_tower_reference.py makes, each naming the template instantiation it must land on;
              route() restates tower_row_tiles, the grids, the dynamic LDS of both launchers, the workspace size and the
              reduce loop's trip counts.

profiles/tower_reference_tolerance.txt records the tables and what the GPU showed."""
import collections

import numpy as np
import torch

import gemm_ref as GR
from gemm_ref import BAND_SHARE, EPS, FACTOR, Launches, T, ceil_div, fg, index_order_f32, index_order_sum_f32, round_up, same_bits

HID, WG_ROWS = 256, 64
E_BADARG, E_WORKSPACE, E_UNSUPPORTED = GR.E_BADARG, GR.E_WORKSPACE, GR.E_UNSUPPORTED
KERNELS = ("tower_fwd_kernel_r1", "tower_fwd_kernel_r2", "tower_fwd_pair_kernel_r1", "tower_fwd_pair_kernel_r2",
           "tower_bwd_kernel_r1", "tower_bwd_kernel_r2", "tower_bwd_pair_kernel_r1", "tower_bwd_pair_kernel_r2",
           "tower_wgrad_kernel", "tower_wgrad_pair_kernel", "tower_wgrad_reduce_kernel", "tower_wgrad_reduce_pair_kernel")

# worst |s32 - s64| / (2^-24 Abs) of the float32 index-order evaluation per (class, band): see main()
BANDS = ("F", "hid", "2D", "4D", "D", "B")
YARD = {
    "flat": {"F": 4.4, "hid": 4.7, "2D": 5.2, "4D": 10.2, "D": 4.5, "B": 4.9},
    "range": {"F": 3.9, "hid": 4.5, "2D": 4.1, "4D": 9.2, "D": 4.2, "B": 19.0},
}
YARD_ROWS, YARD_COLS = 64, 64
EXACT_QUANTUM, EXACT_LIMIT = 2.0 ** -2, 2.0 ** 22

Case = collections.namedtuple("Case", "group entry sides D E B F cls strided ids path need")
OUTPUTS = {"fwd": ("y", "h_out", "tin_out"), "bwd": ("d_emb", "d_f", "dh", "d_extra"),
           "wgrad": ("dW1", "db1", "dW2", "db2", "dW3", "db3", "ws")}


def _c(group, entry, sides, D, E, B, F, cls, strided, path, ids="in", **need):
    return Case(group, entry, sides, D, E, B, F, cls, bool(strided), ids, path, tuple(sorted(need.items())))


def case_id(c):
    f = "" if c.entry == "bwd" else ("-F" + (str(c.F) if c.sides == 1 else "%d.%d" % c.F))
    return (f"{c.group}-{c.entry}{c.sides}-D{c.D}-E{c.E}-B{c.B}{f}-{c.cls}" + ("-strided" if c.strided else "") +
            ("" if c.ids == "in" else "-" + c.ids))


def F_of(c, k):
    return c.F if c.sides == 1 else c.F[k]


def n_rows_of(k):
    return 50 + 37 * k


# ------------------------------------------------------------------ the dispatch, restated
def row_tiles(B):
    """tower.hip tower_row_tiles."""
    return 1 if B <= 4096 else 2


def part_floats(D, F, E):
    """One 64-row block's partial: dW3 [D][2D + E] | dW2 [D][256] | dW1 [256][F] | db3 [D] | db2 [D] | db1 [256]."""
    return D * (2 * D + E) + D * HID + HID * F + 2 * D + HID


def workspace_bytes(B, D, F, E):
    """tt_tower_bwd_weights_workspace_bytes."""
    return round_up(ceil_div(B, WG_ROWS) * part_floats(D, F, E) * 4, 256)


def reduce_trips(n_blocks):
    """Per sixteenth q of tower_wgrad_reduce_body: (trips of the 8-way unrolled loop, trips of the 16-stride tail)."""
    out = []
    for q in range(16):
        w, u, t = q, 0, 0
        while w + 112 < n_blocks:
            w, u = w + 128, u + 1
        while w < n_blocks:
            w, t = w + 16, t + 1
        out.append((u, t))
    return out


def route(c):
    """The launches a case must produce: {"path" (the template instantiation), "launches" {name: count}, and the launch
    parameters}."""
    none = {k: 0 for k in KERNELS}
    Fmax = max(F_of(c, k) for k in range(c.sides)) if c.entry != "bwd" else 0
    x = "true" if c.E else "false"
    pair = "_pair" if c.sides == 2 else ""
    if c.entry in ("fwd", "bwd"):
        rt = row_tiles(c.B)
        rows = 32 * rt
        grid = ceil_div(c.B, rows)
        fam = f"tower_{c.entry}{pair}_kernel"
        path = f"{fam}<{c.D // 8},{rt}>" if pair else f"{fam}<{c.D // 8},{x},{rt}>"
        none[f"{fam}_r{rt}"] = 1
        lds = 4 * (rows * (HID + 4) + rows * (2 * c.D + 4) + rows * Fmax) if c.entry == "fwd" else 0
        return dict(path=path, launches=none, rt=rt, rows=rows, grid=(grid, c.sides), lds=lds,
                    static_lds=0 if c.entry == "fwd" else 2 * rows * (c.D + 4) * 4, last_rows=c.B - (grid - 1) * rows)
    nb = ceil_div(c.B, WG_ROWS)
    fam = f"tower_wgrad{pair}_kernel"
    path = f"{fam}<{c.D // 8}>" if pair else f"{fam}<{c.D // 8},{x}>"
    none[fam] = 1
    none[f"tower_wgrad_reduce{pair}_kernel"] = 1
    parts = [part_floats(c.D, F_of(c, k), c.E) for k in range(c.sides)]
    trips = reduce_trips(nb)
    return dict(path=path, launches=none, nb=nb, grid=(nb, c.sides), lds=4 * (WG_ROWS * c.D + WG_ROWS * HID + WG_ROWS * Fmax),
                parts=parts, ws=[round_up(nb * p * 4, 256) for p in parts], reduce_grid=(ceil_div(max(parts), 64), c.sides),
                trips=(max(u for u, _ in trips), max(t for _, t in trips)), both=any(u and t for u, t in trips),
                last_rows=c.B - (nb - 1) * WG_ROWS)


def claims(c, r):
    """[(claim, what the case table says, what route() gives)]."""
    return [(k, v, r.get(k)) for k, v in c.need]


def instantiations():
    """Every template instantiation of tower.hip's dispatch functions, by the name route() gives."""
    out = []
    for e8 in (4, 8, 16):
        for fam in ("tower_fwd_kernel", "tower_bwd_kernel"):
            out += [f"{fam}<{e8},{x},{rt}>" for x in ("false", "true") for rt in (1, 2)]
        for fam in ("tower_fwd_pair_kernel", "tower_bwd_pair_kernel"):
            out += [f"{fam}<{e8},{rt}>" for rt in (1, 2)]
        out += [f"tower_wgrad_kernel<{e8},{x}>" for x in ("false", "true")] + [f"tower_wgrad_pair_kernel<{e8}>"]
    return out


# ------------------------------------------------------------------ inputs
_SEED = {"table": 72001, "ids": 72002, "feats": 72003, "W1": 72004, "b1": 72005, "W2": 72006, "b2": 72007, "W3": 72008,
         "b3": 72009, "extra": 72010, "dy": 72011, "h": 72012, "tin": 72013, "d_f": 72014, "dh": 72015, "g": 72016}
OOB_IDS = (-1, None, 1 << 40, -(1 << 63))  # None: n_rows itself


def stream(kind, side, trit, shape):
    """The operand kind's flat stream (a hash of the element index), reshaped: float32 torch."""
    n = int(np.prod(shape))
    v = (fg.trits if trit else fg.gaussianish)((n,), _SEED[kind] + 100 * side + (50 if trit else 0))
    return T(v.reshape(shape))


def row_scale(c):
    if c.cls == "exact":
        return T(np.exp2((np.arange(c.B) % 5) - 2.0).astype(np.float32))[:, None]
    if c.cls == "range":
        return T(np.exp2(4.0 * fg.gaussianish((c.B,), _SEED["g"]).astype(np.float64)).astype(np.float32))[:, None]
    if c.cls == "flat":
        return None
    raise KeyError(c.cls)


def h_plants(B):
    """[(m, j, value)]: -0.0, +0.0, 2^-126 and -2^-126 in the backward's h; only 2^-126 passes the mask."""
    n = B * HID
    return [(f // HID, f % HID, v) for f, v in zip((0, n // 3, n // 2, n - 1), (-0.0, 0.0, 2.0 ** -126, -(2.0 ** -126)))]


def oob_plants(B, n_rows):
    """[(m, id)]: -1, n_rows, 2^40 and -2^63 among the ids."""
    pos = sorted({0, B // 3, B // 2, B - 1})
    return [(m, n_rows if v is None else v) for m, v in zip(pos, OOB_IDS)] if len(pos) == 4 else []


def side_inputs(c, k):
    """The logical operands of side k of a case: float32 torch tensors, ids int64."""
    trit = c.cls == "exact"
    D, E, B = c.D, c.E, c.B
    sc = row_scale(c)
    s = lambda kind, *shape: stream(kind, k, trit, shape)
    x = {}
    if c.entry == "fwd":
        F, n_rows = F_of(c, k), n_rows_of(k)
        ids = T(fg.uniform_ids((B,), n_rows, _SEED["ids"] + 100 * k).copy())
        if B > 1:
            ids[B - 1] = ids[0]  # a duplicate whatever the hash gives
        if c.ids != "in":
            for m, v in oob_plants(B, n_rows):
                ids[m] = v
        x.update(F=F, n_rows=n_rows, ids=ids, table=s("table", n_rows, D), feats=s("feats", B, F), W1=s("W1", HID, F),
                 b1=s("b1", HID), W2=s("W2", D, HID), b2=s("b2", D), W3=s("W3", D, 2 * D + E), b3=s("b3", D))
        if sc is not None:
            x["feats"] = x["feats"] * sc
        if E:
            x["extra"] = s("extra", B, E) * (sc if c.cls == "range" else 1.0)
    elif c.entry == "bwd":
        h = s("h", B, HID).clone()
        for m, j, v in h_plants(B):
            h[m, j] = v
        x.update(dy=s("dy", B, D), W2=s("W2", D, HID), W3=s("W3", D, 2 * D + E), h=h)
        if sc is not None:
            x["dy"] = x["dy"] * sc
    else:
        F = F_of(c, k)
        x.update(F=F, dy=s("dy", B, D), tin=s("tin", B, 2 * D), d_f=s("d_f", B, D), h=s("h", B, HID), dh=s("dh", B, HID),
                 feats=s("feats", B, F))
        if E:
            x["extra"] = s("extra", B, E)
        if c.cls == "range":
            for n in ("dy", "d_f", "dh"):
                x[n] = x[n] * sc
    return {n: (v.contiguous() if torch.is_tensor(v) else v) for n, v in x.items()}


def inputs(c):
    return [side_inputs(c, k) for k in range(c.sides)]


def yard(c, band):
    return FACTOR * YARD[c.cls][band] * EPS


def _bound(c, band, Abs, ref):
    return None if c.cls == "exact" else yard(c, band) * Abs + EPS * ref.abs()


def _d(x, name):
    """float64 copy of an operand, kept with the inputs."""
    k = "_64" + name
    if k not in x:
        x[k] = x[name].double()
    return x[k]


def table_rows(x):
    """[B, D] float32: the table row of every id, zeros where the id is out of range."""
    ids, n = x["ids"], x["n_rows"]
    ok = (ids >= 0) & (ids < n)
    return torch.where(ok[:, None], x["table"][ids.clamp(0, n - 1)], torch.zeros(1, dtype=torch.float32))


def fwd_layer1(c, x):
    """(pre1, Abs1, band) of h = ReLU(feats W1^T + b1) from the inputs alone; band: |pre1| within its bound of zero."""
    if "_l1" not in x:
        f, w, b = _d(x, "feats"), _d(x, "W1"), _d(x, "b1")
        pre = f @ w.t() + b
        Abs = f.abs() @ w.abs().t() + b.abs()
        band = torch.zeros_like(pre, dtype=torch.bool)
        if c.cls != "exact":
            band = (pre.abs() <= yard(c, "F") * Abs + EPS * pre.abs()) & (pre != 0)
        x["_l1"] = (pre, Abs, band)
    return x["_l1"]


def fwd_chain(c, x):
    """The forward end to end in float64 from the inputs: {"h", "tin", "y"} and the largest Abs of any stage."""
    if "_chain" not in x:
        pre, Abs1, _ = fwd_layer1(c, x)
        h = pre.clamp(min=0.0)
        w2, b2, w3, b3 = _d(x, "W2"), _d(x, "b2"), _d(x, "W3"), _d(x, "b3")
        f = h @ w2.t() + b2
        tin = torch.cat([table_rows(x).double(), f], 1)
        K3 = 2 * c.D
        y = tin @ w3[:, :K3].t() + b3
        Abs3 = tin.abs() @ w3[:, :K3].abs().t() + b3.abs()
        if c.E:
            y = y + _d(x, "extra") @ w3[:, K3:].t()
            Abs3 = Abs3 + _d(x, "extra").abs() @ w3[:, K3:].abs().t()
        Abs2 = h @ w2.abs().t() + b2.abs()
        x["_chain"] = {"h": h, "tin": tin, "y": y, "Abs": max(float(Abs1.max()), float(Abs2.max()), float(Abs3.max()))}
    return x["_chain"]


def bwd_dtin(c, x):
    if "_dtin" not in x:
        dy, w3 = _d(x, "dy"), _d(x, "W3")
        x["_dtin"] = (dy @ w3, dy.abs() @ w3.abs())
    return x["_dtin"]


def wgrad_ref(c, x):
    """{name: (ref, Abs)} of the six gradients, float64."""
    if "_wg" not in x:
        dy, d_f, dh = _d(x, "dy"), _d(x, "d_f"), _d(x, "dh")
        X = torch.cat([_d(x, "tin")] + ([_d(x, "extra")] if c.E else []), 1)
        h, ft = _d(x, "h"), _d(x, "feats")
        x["_wg"] = {"dW3": (dy.t() @ X, dy.abs().t() @ X.abs()), "db3": (dy.sum(0)[None], dy.abs().sum(0)[None]),
                    "dW2": (d_f.t() @ h, d_f.abs().t() @ h.abs()), "db2": (d_f.sum(0)[None], d_f.abs().sum(0)[None]),
                    "dW1": (dh.t() @ ft, dh.abs().t() @ ft.abs()), "db1": (dh.sum(0)[None], dh.abs().sum(0)[None])}
    return x["_wg"]


def exact_abs(c, inp):
    """The largest sum of |terms| of any reduction of an exact-class case (every term is a multiple of EXACT_QUANTUM)."""
    worst = 0.0
    for x in inp:
        if c.entry == "fwd":
            worst = max(worst, fwd_chain(c, x)["Abs"])
        elif c.entry == "bwd":
            d_tin, Abs = bwd_dtin(c, x)
            worst = max(worst, float(Abs.max()), float((d_tin[:, c.D:2 * c.D].abs() @ _d(x, "W2").abs()).max()))
        else:
            worst = max(worst, max(float(a.max()) for _, a in wgrad_ref(c, x).values()))
    return worst


def band_share(c, inp):
    """The largest share of h_out elements of a side whose pre-activation is within the bound of zero."""
    return max(float(fwd_layer1(c, x)[2].double().mean()) for x in inp) if c.entry == "fwd" else 0.0


# ------------------------------------------------------------------ buffers
SLICE = ((8, 4), (12, 8))    # (pad, offset) of a 16-byte aligned column slice of a wider buffer, per side
FEATS = ((3, 1), (5, 3))     # ldf > F, the base one / three floats off a 16-byte boundary


class Buffers(GR.Buffers):
    """The operands and outputs of a case as views into larger NaN-filled float32 buffers (CPU), named <operand><side>.
    Side 0 of a strided case and side 1 of every two-sided case are strided (so the two sides differ in strides); the
    out-of-range flag is element FLAG_AT of a small int32 buffer."""
    FLAG_AT = 3

    def __init__(self, c, inp):
        self.c, self.buf, self.geom = c, {}, {}
        self.flag = torch.full((8,), 7, dtype=torch.int32)
        self.flag[self.FLAG_AT] = 0
        D, E, B = c.D, c.E, c.B
        nan = lambda *s: torch.full(s, float("nan"))
        for k, x in enumerate(inp):
            strided = c.strided if k == 0 else True
            sl = SLICE[k] if strided else (0, 0)
            ft = FEATS[k] if strided else (0, 0)
            a = lambda name, t, g=(0, 0): self._add(name + str(k), t if t.dim() == 2 else t[None, :], g[0], g[1])
            if c.entry == "fwd":
                a("table", x["table"]), a("feats", x["feats"], ft), a("W1", x["W1"], (0, 1 if strided else 0))
                a("b1", x["b1"], (0, 1 if strided else 0)), a("W2", x["W2"]), a("b2", x["b2"]), a("W3", x["W3"]), a("b3", x["b3"])
                if E:
                    a("extra", x["extra"], sl)
                a("y", nan(B, D), sl), a("h_out", nan(B, HID)), a("tin_out", nan(B, 2 * D))
            elif c.entry == "bwd":
                a("dy", x["dy"], sl), a("W2", x["W2"]), a("W3", x["W3"]), a("h", x["h"])
                a("d_emb", nan(B, D), sl), a("d_f", nan(B, D)), a("dh", nan(B, HID))
                if E:
                    a("d_extra", nan(B, E), sl)
            else:
                F = x["F"]
                a("dy", x["dy"], sl), a("tin", x["tin"]), a("d_f", x["d_f"]), a("h", x["h"]), a("dh", x["dh"]), a("feats", x["feats"], ft)
                if E:
                    a("extra", x["extra"], sl)
                a("dW1", nan(HID, F)), a("db1", nan(1, HID)), a("dW2", nan(D, HID)), a("db2", nan(1, D))
                a("dW3", nan(D, 2 * D + E)), a("db3", nan(1, D)), a("ws", nan(1, workspace_bytes(B, D, F, E) // 4))

    def _add(self, name, x, pad, off):
        rows, w = x.shape
        ld = w + pad
        guard = (round_up(2 * ld, 4) if ld <= 4096 else 0) + 64  # (the workspace: 64 floats each way)
        buf = torch.full((guard + off + rows * ld + guard,), float("nan"), dtype=torch.float32)
        self.buf[name], self.geom[name] = buf, (rows, w, ld, guard + off)
        self.view(name).copy_(x)

    def outputs(self, k=None):
        """Names of the output buffers (of side k)."""
        return [n for n in self.buf if n[:-1] in OUTPUTS[self.c.entry] and (k is None or n[-1] == str(k))]


# ------------------------------------------------------------------ the checker
class Report(GR.Report):
    """gemm_ref.Report plus: rows = elements of tin_out[:, :D] that are not the table row's bits; flag = the out-of-range
    flag (and its neighbours) is what it must be; per = the worst err / E of each output."""

    def __init__(self):
        super().__init__()
        self.rows, self.flag, self.per = 0, True, {}

    @property
    def ok(self):
        return self.bad == 0 and self.nonfinite == 0 and self.clean and self.rows == 0 and self.flag

    def __repr__(self):
        return (f"Report(worst err/E {self.worst:.3g}, band {self.band}, outside E {self.bad}, non-finite {self.nonfinite}, "
                f"id rows off {self.rows}, surroundings {'clean' if self.clean else 'CHANGED'}, flag {'ok' if self.flag else 'WRONG'})")


def _cmp(rep, what, got, ref, E, band=None, alt=None):
    before, rep.worst = rep.worst, 0.0
    _cmp1(rep, got, ref, E, band, alt)
    rep.per[what] = max(rep.per.get(what, 0.0), rep.worst)
    rep.worst = max(rep.worst, before)


def _cmp1(rep, got, ref, E, band, alt):
    rep.nonfinite += int((~torch.isfinite(got)).sum())
    if E is None:  # the exact class: equality, in float32 (the reference is representable)
        bad = int((~(got == ref.float())).sum())
        rep.bad += bad
        rep.worst = float("inf") if bad else rep.worst
        return
    err = (got.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    ratio = GR._ratio(err, E)
    if band is not None and bool(band.any()):
        err2 = (got.double() - alt).abs()
        err2 = torch.where(torch.isnan(err2), torch.full_like(err2, float("inf")), err2)
        ratio = torch.where(band, torch.minimum(ratio, GR._ratio(err2, E)), ratio)
        rep.band += int(band.sum())
    rep.bad += int((ratio > 1.0).sum())
    if ratio.numel():
        rep.worst = max(rep.worst, float(ratio.max()))


def want_flag(c):
    return 1 if c.ids == "oob" else 0


def check(c, inp, bufs, after, flag=None):
    """The output buffers after a call ({name: whole buffer, CPU float32}; flag: the int32 flag buffer) against the
    reference -> Report."""
    rep = Report()
    D, K3, exact = c.D, 2 * c.D, c.cls == "exact"
    for k, x in enumerate(inp):
        v = lambda name: bufs.view(name + str(k), after[name + str(k)])
        if c.entry == "fwd":
            h, tin, y = v("h_out"), v("tin_out"), v("y")
            rep.rows += int((tin[:, :D].contiguous().view(torch.int32) != table_rows(x).view(torch.int32)).sum())
            rep.nonfinite += int((~torch.isfinite(tin[:, :D])).sum())
            if exact:
                ch = fwd_chain(c, x)
                _cmp(rep, "h_out", h, ch["h"], None), _cmp(rep, "tin_out", tin[:, D:], ch["tin"][:, D:], None), _cmp(rep, "y", y, ch["y"], None)
                continue
            pre, Abs1, band = fwd_layer1(c, x)
            ref = pre.clamp(min=0.0)
            _cmp(rep, "h_out", h, ref, _bound(c, "F", Abs1, ref), band, torch.where(pre > 0, torch.zeros_like(pre), pre))
            hg, w2, b2 = h.double(), _d(x, "W2"), _d(x, "b2")
            ref = hg @ w2.t() + b2
            _cmp(rep, "tin_out", tin[:, D:], ref, _bound(c, "hid", hg.abs() @ w2.abs().t() + b2.abs(), ref))
            tg, w3, b3 = tin.double(), _d(x, "W3"), _d(x, "b3")
            ref = tg @ w3[:, :K3].t() + b3
            Abs = tg.abs() @ w3[:, :K3].abs().t() + b3.abs()
            if c.E:
                ref = ref + _d(x, "extra") @ w3[:, K3:].t()
                Abs = Abs + _d(x, "extra").abs() @ w3[:, K3:].abs().t()
            _cmp(rep, "y", y, ref, _bound(c, "4D" if c.E else "2D", Abs, ref))
        elif c.entry == "bwd":
            d_tin, Abs = bwd_dtin(c, x)
            d_f = v("d_f")
            _cmp(rep, "d_emb", v("d_emb"), d_tin[:, :D], _bound(c, "D", Abs[:, :D], d_tin[:, :D]))
            _cmp(rep, "d_f", d_f, d_tin[:, D:K3], _bound(c, "D", Abs[:, D:K3], d_tin[:, D:K3]))
            if c.E:
                _cmp(rep, "d_extra", v("d_extra"), d_tin[:, K3:], _bound(c, "D", Abs[:, K3:], d_tin[:, K3:]))
            dfg, w2 = d_f.double(), _d(x, "W2")
            val = dfg @ w2
            ref = torch.where(x["h"] > 0, val, torch.zeros_like(val))
            _cmp(rep, "dh", v("dh"), ref, _bound(c, "D", dfg.abs() @ w2.abs(), ref))
        else:
            for name, (ref, Abs) in wgrad_ref(c, x).items():
                _cmp(rep, name, v(name), ref, _bound(c, "B", Abs, ref))
    for name in bufs.outputs():
        if after[name] is not bufs.buf[name]:
            rep.clean = rep.clean and GR.outside_unchanged(bufs, name, after[name])
    if flag is not None:
        want = bufs.flag.clone()
        want[bufs.FLAG_AT] = want_flag(c)
        rep.flag = bool(torch.equal(flag, want))
    return rep


# ------------------------------------------------------------------ float32 evaluation and the mutants
MUTANTS = ("id_neighbour", "oob_row0", "b2_omitted", "b3_omitted", "feats_ge16_dropped", "relu_dropped", "mask_ge0",
           "mask_from_value", "extra_omitted", "extra_w3_again", "tin_swapped", "second_tile_unwritten", "ragged_row",
           "row_past_B", "swap_cols", "last_block_dropped", "blocks_ge128_dropped", "db1_from_h", "dW3_extra_omitted",
           "pair_side1_F0")
_BY_ENTRY = {"fwd": {"id_neighbour", "oob_row0", "b2_omitted", "b3_omitted", "feats_ge16_dropped", "relu_dropped", "extra_omitted",
                     "extra_w3_again", "tin_swapped", "second_tile_unwritten", "ragged_row", "row_past_B", "swap_cols",
                     "pair_side1_F0"},
             "bwd": {"mask_ge0", "mask_from_value", "second_tile_unwritten", "ragged_row", "row_past_B", "swap_cols"},
             "wgrad": {"swap_cols", "last_block_dropped", "blocks_ge128_dropped", "db1_from_h", "dW3_extra_omitted", "pair_side1_F0"}}


def _swap(t):
    """Columns n0 and n0 + 4 of every 32-column block exchanged."""
    perm = torch.arange(t.shape[1])
    for n0 in range(0, t.shape[1] - 4, 32):
        perm[n0], perm[n0 + 4] = n0 + 4, n0
    return t[:, perm]


def run_f32(c, inp, bufs, mutant=None):
    """A float32 torch evaluation of the entry written through the output views of a copy of the buffers ->
    ({name: buffer}, flag buffer); with a mutant, that way of going wrong (None where the case gives it nothing to do)."""
    if mutant is not None and mutant not in _BY_ENTRY[c.entry]:
        return None
    r = route(c)
    D, E, B, K3 = c.D, c.E, c.B, 2 * c.D
    out = {n: (bufs.buf[n] if n.startswith("ws") else bufs.buf[n].clone()) for n in bufs.outputs()}  # (the workspace: untouched)
    flag = bufs.flag.clone()
    did = mutant is None
    for k, x in enumerate(inp):
        res = {}
        if c.entry == "fwd":
            feats, W1, F = x["feats"], x["W1"], x["F"]
            if mutant == "pair_side1_F0" and c.sides == 2 and k == 1 and c.F[0] < F:  # side 1 walks its operands with side 0's F
                F0 = c.F[0]
                feats, W1, did = feats[:, :F0], W1.flatten()[:HID * F0].reshape(HID, F0), True
            if mutant == "feats_ge16_dropped" and F > 16:
                feats, W1, did = feats[:, :16], W1[:, :16], True
            pre = feats @ W1.t() + x["b1"]
            h = pre if mutant == "relu_dropped" else pre.clamp(min=0.0)
            ids, n_rows = x["ids"], x["n_rows"]
            valid = (ids >= 0) & (ids < n_rows)
            if mutant == "id_neighbour" and B > 1:
                ids, did = torch.roll(ids, -1), True
                valid = (ids >= 0) & (ids < n_rows)
            rows = torch.where(valid[:, None], x["table"][ids.clamp(0, n_rows - 1)], torch.zeros(1))
            if mutant == "oob_row0" and not bool(valid.all()):
                rows, did = torch.where(valid[:, None], rows, x["table"][0][None, :]), True
            if not bool(valid.all()) and c.ids == "oob":
                flag[bufs.FLAG_AT] = 1
            f = h @ x["W2"].t() + (0.0 if mutant == "b2_omitted" else x["b2"])
            tin = torch.cat([f, rows], 1) if mutant == "tin_swapped" else torch.cat([rows, f], 1)
            y = tin @ x["W3"][:, :K3].t() + (0.0 if mutant == "b3_omitted" else x["b3"])
            if E and mutant != "extra_omitted":
                y = y + x["extra"] @ (x["W3"][:, :K3] if mutant == "extra_w3_again" else x["W3"][:, K3:]).t()
            did = did or mutant in ("relu_dropped", "b2_omitted", "b3_omitted", "tin_swapped") or (E and mutant in ("extra_omitted", "extra_w3_again"))
            res, primary = {"y": y, "h_out": h, "tin_out": tin}, "y"
        elif c.entry == "bwd":
            d_tin = x["dy"] @ x["W3"]
            d_f = d_tin[:, D:K3]
            val = d_f @ x["W2"]
            mask = val > 0 if mutant == "mask_from_value" else x["h"] >= 0 if mutant == "mask_ge0" else x["h"] > 0
            did = did or mutant in ("mask_from_value", "mask_ge0")
            res, primary = {"d_emb": d_tin[:, :D], "d_f": d_f, "dh": torch.where(mask, val, torch.zeros_like(val))}, "d_emb"
            if E:
                res["d_extra"] = d_tin[:, K3:]
        else:
            n = B
            if mutant == "last_block_dropped":
                n, did = WG_ROWS * (r["nb"] - 1), True
            if mutant == "blocks_ge128_dropped" and r["nb"] > 128:
                n, did = WG_ROWS * 128, True
            dy, d_f, dh = x["dy"][:n], x["d_f"][:n], x["dh"][:n]
            X = torch.cat([x["tin"]] + ([x["extra"]] if E else []), 1)[:n]
            dW1 = dh.t() @ x["feats"][:n]
            if mutant == "pair_side1_F0" and c.sides == 2 and k == 1 and c.F[0] < x["F"]:
                F0 = c.F[0]
                flat = torch.full((HID * x["F"],), float("nan"))
                flat[:HID * F0] = dW1[:, :F0].flatten()
                dW1, did = flat.reshape(HID, x["F"]), True
            dW3 = dy.t() @ X
            if mutant == "dW3_extra_omitted" and E:
                dW3, did = dW3.clone(), True
                dW3[:, K3:] = 0.0
            db1 = (x["h"][:n] if mutant == "db1_from_h" else dh).sum(0)[None]
            did = did or mutant == "db1_from_h"
            res, primary = {"dW3": dW3, "db3": dy.sum(0)[None], "dW2": d_f.t() @ x["h"][:n], "db2": d_f.sum(0)[None], "dW1": dW1,
                            "db1": db1}, "dW2"
        if mutant == "swap_cols":
            res[primary], did = _swap(res[primary]), True
        for name, val in res.items():
            view = bufs.view(name + str(k), out[name + str(k)])
            keep = view.clone()
            view.copy_(val)
            if c.entry == "wgrad":
                continue
            if mutant == "second_tile_unwritten" and r["rt"] == 2 and r["last_rows"] > 32:
                lo = (r["grid"][0] - 1) * 64 + 32
                view[lo:] = keep[lo:]
                did = True
            if mutant == "ragged_row" and B % r["rows"]:
                view[B - 1] = keep[B - 1]
                did = True
            if mutant == "row_past_B" and name == primary:  # one more row of the same stride: the first row past the view
                rows_, w, ld, start = bufs.geom[name + str(k)]
                torch.as_strided(out[name + str(k)], (1, w), (ld, 1), start + rows_ * ld).copy_(val[:1])
                did = True
    return (out, flag) if did else None


def same_outputs(a, b):
    return a is b or (a is not None and b is not None and all(same_bits(a[0][n], b[0][n]) for n in a[0]) and torch.equal(a[1], b[1]))


# ------------------------------------------------------------------ the yardstick
def _rel(s32, s64, Abs):
    r = (s32.double() - s64).abs() / (EPS * Abs)
    return float(torch.where(Abs > 0, r, torch.zeros_like(r)).max())


def _prod(oa, ob):
    """max |index-order float32 - float64| / (2^-24 Abs) of oa ob, and the float32 product."""
    oa, ob = oa.contiguous(), ob.contiguous()
    s32 = index_order_f32(oa, ob)
    return _rel(s32, oa.double() @ ob.double(), oa.double().abs() @ ob.double().abs()), s32


def yard_shapes(cls):
    """One (case, side) per distinct (entry, D, E, F) -- wgrad: and B -- of the class: the yardstick reads leading blocks."""
    best = {}
    for c in CASES:
        if c.cls != cls:
            continue
        for k in range(c.sides):
            key = (c.entry, k, c.D, c.E, 0 if c.entry == "bwd" else F_of(c, k), c.B if c.entry == "wgrad" else 0, c.ids != "in")
            if key not in best or best[key][0].B < c.B:
                best[key] = (c, k)
    return list(best.values())


def measure(cls):
    """{band: (worst, case id)} of the float32 index-order evaluation over yard_shapes(cls)."""
    worst = {b: (0.0, None) for b in BANDS}

    def put(band, r, c):
        if r >= worst[band][0]:
            worst[band] = (r, case_id(c))

    for c, k in yard_shapes(cls):
        x = side_inputs(c, k)
        D, K3, R = c.D, 2 * c.D, YARD_ROWS
        ones = torch.ones(min(R, c.B), 1)
        if c.entry == "fwd":
            r1, pre = _prod(torch.cat([x["feats"][:R], ones], 1), torch.cat([x["W1"].t(), x["b1"][None]], 0))
            r2, f = _prod(torch.cat([pre.clamp(min=0.0), ones], 1), torch.cat([x["W2"].t(), x["b2"][None]], 0))
            tin = [table_rows(x)[:R], f] + ([x["extra"][:R]] if c.E else [])
            r3, _ = _prod(torch.cat(tin + [ones], 1), torch.cat([x["W3"].t(), x["b3"][None]], 0))
            put("F", r1, c), put("hid", r2, c), put("4D" if c.E else "2D", r3, c)
        elif c.entry == "bwd":
            r1, d_tin = _prod(x["dy"][:R], x["W3"])
            r2, _ = _prod(d_tin[:, D:K3], x["W2"])
            put("D", max(r1, r2), c)
        else:
            X = torch.cat([x["tin"]] + ([x["extra"]] if c.E else []), 1)
            rs = [_prod(x["dy"][:, :32].t(), X[:, :YARD_COLS])[0], _prod(x["d_f"][:, :32].t(), x["h"][:, :YARD_COLS])[0],
                  _prod(x["dh"][:, :32].t(), x["feats"])[0]]
            for n in ("dy", "d_f", "dh"):
                v = x[n][:, :32].contiguous()
                rs.append(_rel(index_order_sum_f32(v), v.double().sum(0), v.double().abs().sum(0)))
            put("B", max(rs), c)
    return worst


# ------------------------------------------------------------------ the GPU call (test_gpu_tower_reference.py)
def run_gpu(c, inp, bufs, dev="cuda:0", only=None, ws_short=0):
    """One call of the case's entry point at the C ABI with explicit pointers and leading dimensions (only: that side
    alone, as a one-sided call) -> {"rc", "after" {name: whole buffer, CPU}, "flag", "launches", "ws_bytes"}."""
    import ctypes as C
    from two_tower_models_amd import _native as N
    lib = N.load()
    ks = list(range(c.sides)) if only is None else [only]
    g = {n: v.to(dev) for n, v in bufs.buf.items() if int(n[-1]) in ks}
    ids = {k: inp[k]["ids"].to(dev) for k in ks if c.entry == "fwd"}
    flag = bufs.flag.to(dev)
    D, E, B = c.D, c.E, c.B

    def p(name, k):
        t = g[name + str(k)]
        assert t.data_ptr() % 16 == 0
        return t.data_ptr() + 4 * bufs.geom[name + str(k)][3]

    ld = lambda name, k: bufs.ld(name + str(k))
    wsn = []
    if c.entry == "fwd":
        arr = (N.TowerFwdSide * len(ks))()
        for i, k in enumerate(ks):
            arr[i] = N.TowerFwdSide(p("table", k), inp[k]["n_rows"], ids[k].data_ptr(), p("feats", k), ld("feats", k), inp[k]["F"],
                                    p("W1", k), p("b1", k), p("W2", k), p("b2", k), p("W3", k), p("b3", k), p("y", k), ld("y", k),
                                    p("h_out", k), p("tin_out", k), p("extra", k) if E else None, ld("extra", k) if E else 0)
        fp = None if c.ids == "oobnull" else flag.data_ptr() + 4 * bufs.FLAG_AT
        with Launches(KERNELS) as n:
            rc = lib.tt_tower_fwd(arr, len(ks), B, D, HID, E, fp, N.stream())
    elif c.entry == "bwd":
        arr = (N.TowerBwdSide * len(ks))()
        for i, k in enumerate(ks):
            arr[i] = N.TowerBwdSide(p("dy", k), ld("dy", k), p("W2", k), p("W3", k), p("h", k), p("d_emb", k), ld("d_emb", k), p("d_f", k),
                                    p("dh", k), p("d_extra", k) if E else None, ld("d_extra", k) if E else 0)
        with Launches(KERNELS) as n:
            rc = lib.tt_tower_bwd_data(arr, len(ks), B, D, HID, E, N.stream())
    else:
        arr = (N.TowerWgradSide * len(ks))()
        for i, k in enumerate(ks):
            wsn.append(lib.tt_tower_bwd_weights_workspace_bytes(B, D, inp[k]["F"], HID, E))
            arr[i] = N.TowerWgradSide(p("dy", k), ld("dy", k), p("tin", k), p("d_f", k), p("h", k), p("dh", k), p("feats", k), ld("feats", k),
                                      inp[k]["F"], p("dW1", k), p("db1", k), p("dW2", k), p("db2", k), p("dW3", k), p("db3", k),
                                      p("ws", k), 4 * bufs.geom["ws" + str(k)][1] - ws_short, p("extra", k) if E else None,
                                      ld("extra", k) if E else 0)
        with Launches(KERNELS) as n:
            rc = lib.tt_tower_bwd_weights(arr, len(ks), B, D, HID, E, N.stream())
    torch.cuda.synchronize()
    return {"rc": rc, "after": {name: g[name].cpu() for name in bufs.outputs() if int(name[-1]) in ks}, "flag": flag.cpu(),
            "launches": dict(n), "ws_bytes": wsn}


def _same(a, b, names):
    return all(same_bits(a[n], b[n]) for n in names)


def gpu_case(c, dev="cuda:0"):
    """Everything test_gpu_tower_reference.py asserts of one case, as a dict."""
    inp = inputs(c)
    bufs, r = Buffers(c, inp), route(c)
    res = {"id": case_id(c), "path": r["path"], "want_launches": r["launches"], "short": None, "repeat_same": None, "pair_same": None,
           "single_launches": None}
    out = run_gpu(c, inp, bufs, dev)
    rep = check(c, inp, bufs, out["after"], out["flag"])
    res.update(rc=out["rc"], launches=out["launches"], ws_bytes=out["ws_bytes"], ws_want=r.get("ws", []), worst=rep.worst,
               band=rep.band, bad=rep.bad, nonfinite=rep.nonfinite, rows=rep.rows, clean=rep.clean, flag=rep.flag, ok=rep.ok, report=repr(rep), per=rep.per)
    results = [n for n in bufs.outputs() if not n.startswith("ws")]
    if c.entry == "wgrad":
        again = run_gpu(c, inp, bufs, dev)
        res["repeat_same"] = _same(again["after"], out["after"], results)
        short = run_gpu(c, inp, bufs, dev, ws_short=1)  # one byte less: refused, nothing launched, nothing written
        res["short"] = (short["rc"], sum(short["launches"].values()), _same(short["after"], bufs.buf, bufs.outputs()))
    if c.sides == 2:  # the pair is the two one-sided calls bit for bit
        res["pair_same"], res["single_launches"] = True, []
        for k in range(2):
            one = run_gpu(c, inp, bufs, dev, only=k)
            res["pair_same"] = res["pair_same"] and one["rc"] == 0 and _same(one["after"], out["after"], [n for n in results if n[-1] == str(k)])
            want = route(c._replace(sides=1, F=F_of(c, k) if c.entry != "bwd" else c.F))["launches"]
            res["single_launches"].append(one["launches"] == want)
    return res


def gpu_line(res):
    ran = {k: v for k, v in res["launches"].items() if v}
    per = " ".join(f"{k} {v:.3f}" for k, v in res["per"].items())
    return f"tower-ref {res['id']} err/E {res['worst']:.3f} ({per}) band {res['band']} path {res['path']} launches {ran}"


def assert_gpu_case(c, res):
    assert res["rc"] == 0, res
    assert res["launches"] == res["want_launches"], (res["launches"], res["want_launches"])
    assert res["ws_bytes"] == res["ws_want"], (res["ws_bytes"], res["ws_want"])
    assert res["short"] in (None, (E_WORKSPACE, 0, True)), res
    assert res["repeat_same"] in (None, True), res
    assert res["pair_same"] in (None, True) and res["single_launches"] in (None, [True, True]), res
    assert res["ok"], res
    if c.cls == "exact":
        assert res["worst"] == 0.0, res


# ------------------------------------------------------------------ the cases
DS = ((32, 4), (64, 8), (128, 16))
BS = ((1, 1), (31, 1), (32, 1), (33, 1), (64, 1), (65, 1), (4096, 1), (4097, 2), (4128, 2), (4160, 2))  # (B, row tiles)
FS = (1, 15, 16, 17, 63, 64)
CLS = ("flat", "exact", "range")
# n_blocks of the weight-gradient reduce: (most unrolled trips, most tail trips) of a sixteenth; at 129 and 130 a sixteenth
# runs the unrolled loop and then the tail
NBS = {1: (0, 1), 2: (0, 1), 16: (0, 1), 17: (0, 2), 112: (0, 7), 113: (1, 7), 128: (1, 0), 129: (1, 1), 130: (1, 1)}
LDS_MAX = 149504  # D = 128, F = 64, two row tiles: 64 260 4 + 64 260 4 + 64 64 4 bytes of dynamic LDS


def _one_side():
    cs, i = [], 0
    for D, e8 in DS:
        for E, x in ((0, "false"), (2 * D, "true")):
            for B, rt in BS:  # every B at some F, class and stride form
                F, cls, strided = FS[i % 6], CLS[(i + i // 6) % 3], (i + i // 10) % 2 == 0
                i += 1
                cs.append(_c("one", "fwd", 1, D, E, B, F, cls, strided, f"tower_fwd_kernel<{e8},{x},{rt}>", rt=rt))
                cs.append(_c("one", "bwd", 1, D, E, B, 0, cls, strided, f"tower_bwd_kernel<{e8},{x},{rt}>", rt=rt))
            for j, F in enumerate(FS):  # every F on both row-tile forms, ldf > F and a misaligned feats base on every other one
                for B, rt in ((65, 1), (4097, 2)):
                    cs.append(_c("feat", "fwd", 1, D, E, B, F, CLS[(j + rt) % 3], (j + rt) % 2, f"tower_fwd_kernel<{e8},{x},{rt}>", rt=rt))
            for B, rt in ((65, 1), (4097, 2)):  # out-of-range ids with a flag and with oob_flag = NULL
                cs.append(_c("oob", "fwd", 1, D, E, B, 17, "flat", rt == 1, f"tower_fwd_kernel<{e8},{x},{rt}>", ids="oob", rt=rt))
                cs.append(_c("oob", "fwd", 1, D, E, B, 8, "exact", rt == 2, f"tower_fwd_kernel<{e8},{x},{rt}>", ids="oobnull", rt=rt))
    for E, x in ((0, "false"), (256, "true")):  # the most LDS a forward asks for; its second 32-row tile lies past B
        cs.append(_c("lds", "fwd", 1, 128, E, 4097, 64, "flat", True, f"tower_fwd_kernel<16,{x},2>", rt=2, lds=LDS_MAX, last_rows=1))
        cs.append(_c("lds", "fwd", 1, 128, E, 4160, 64, "exact", False, f"tower_fwd_kernel<16,{x},2>", rt=2, lds=LDS_MAX, last_rows=64))
    return cs


def _two_sides():
    cs, i = [], 0
    for D, e8 in DS:
        for B, rt in ((1, 1), (33, 1), (65, 1), (4096, 1), (4097, 2), (4128, 2), (4160, 2)):
            F = ((3, 64), (17, 5), (64, 3))[i % 3]
            cls, strided = CLS[i % 3], i % 2
            i += 1
            cs.append(_c("pair", "fwd", 2, D, 0, B, F, cls, strided, f"tower_fwd_pair_kernel<{e8},{rt}>", rt=rt))
            cs.append(_c("pair", "bwd", 2, D, 0, B, (0, 0), cls, strided, f"tower_bwd_pair_kernel<{e8},{rt}>", rt=rt))
        cs.append(_c("pair", "fwd", 2, D, 0, 65, (3, 64), "flat", True, f"tower_fwd_pair_kernel<{e8},1>", ids="oob", rt=1))
        cs.append(_c("pair", "fwd", 2, D, 0, 4160, (3, 64), "exact", False, f"tower_fwd_pair_kernel<{e8},2>", rt=2))
    return cs


def _nb_rows(nb):
    """A batch size with nb 64-row blocks: B = 8257 for 130 (its last block holds one row), whole and ragged blocks else."""
    return 64 * (nb - 1) + (1 if nb in (130, 17) else 64 if nb in (16, 128, 2) else 37)


def _wgrad():
    cs, i = [], 0
    for D, e8 in DS:
        for E, x in ((0, "false"), (2 * D, "true")):
            nbs = tuple(NBS) if (D, E) in ((32, 0), (128, 256)) else (1, 2, 17, 113, 129, 130)
            for nb in nbs:
                F, cls, strided = FS[i % 6], CLS[(i + i // 6) % 3], i % 2
                if nb == 130 and cls == "range":  # (one row in the last block: under the row scales it can vanish in the bound)
                    cls = "flat"
                i += 1
                cs.append(_c("wgrad", "wgrad", 1, D, E, _nb_rows(nb), F, cls, strided, f"tower_wgrad_kernel<{e8},{x}>", nb=nb, trips=NBS[nb]))
        for nb in (1, 2, 17, 113, 129, 130):
            F = ((3, 64), (64, 3), (17, 15))[i % 3]
            cs.append(_c("wpair", "wgrad", 2, D, 0, _nb_rows(nb), F, "flat" if (nb == 130 and i % 3 == 2) else CLS[i % 3], i % 2, f"tower_wgrad_pair_kernel<{e8}>", nb=nb, trips=NBS[nb]))
            i += 1
    cs.append(_c("wgrad", "wgrad", 1, 128, 0, 1, 64, "flat", False, "tower_wgrad_kernel<16,false>", nb=1, trips=(0, 1)))
    return cs


CASES = _one_side() + _two_sides() + _wgrad()
_DUP = [k for k, v in collections.Counter(case_id(c) for c in CASES).items() if v > 1]
assert not _DUP, ("case ids must be distinct", _DUP)


def main():
    print("float32 index-order evaluation against float64: worst |s32 - s64| / (2^-24 Abs) per class and band")
    ok = True
    for cls in YARD:
        w = measure(cls)
        for band in BANDS:
            print(f"{cls:<6} {band:<4} {w[band][0]:8.3f} {YARD[cls][band]:6.2f}   {w[band][1]}")
            ok = ok and w[band][0] <= YARD[cls][band] <= 1.1 * w[band][0]
    worst_abs, worst_share = 0.0, 0.0
    for c in CASES:
        inp = inputs(c)
        if c.cls == "exact":
            worst_abs = max(worst_abs, exact_abs(c, inp))
        worst_share = max(worst_share, band_share(c, inp))
    print(f"\nexact class: largest sum of |terms| {worst_abs:.0f} = 2^{np.log2(worst_abs):.2f} (limit 2^22)")
    print(f"largest ReLU band share of a case {100 * worst_share:.4f} % (limit {100 * BAND_SHARE} %)")
    print(f"{len(CASES)} cases: " + ", ".join(f"{g} {n}" for g, n in collections.Counter(c.group for c in CASES).items()))
    assert ok and worst_abs < EXACT_LIMIT and worst_share <= BAND_SHARE


if __name__ == "__main__":
    main()
