"""The fused tower on MI355X (`pytest -m gpu`) against the float64 reference of tests/tower_ref.py: every template
instantiation behind tt_tower_fwd, tt_tower_bwd_data and tt_tower_bwd_weights -- D = 32 / 64 / 128, with and without the
third input block, on the 32-row and the 64-row form, one side and two; B = 1 .. 65 and the 4096 / 4097 / 4128 / 4160 boundary
of tower_row_tiles; F = 1, 15, 16, 17, 63, 64 around layer 1's register cache; the 149 504-byte LDS request; ids out of range
with a flag and with oob_flag = NULL; the weight-gradient reduce at 1 .. 130 blocks.

Every call goes through the C ABI with explicit pointers and leading dimensions; every operand and output is a view into a
NaN-filled buffer (y, d_emb, extra, d_extra as 16-byte aligned column slices, feats with ldf > F off a misaligned base).
Every case asserts rc == 0, exactly the launches its table entry names (through the library's launch counters), the
workspace size, every result finite and within E (the exact class: equal), no byte outside any output view changed; two
sides: each side against float64 on its own and the pair equal to the two one-sided calls bit for bit; wgrad: two calls
bit-identical and a workspace one byte short refused before anything is written.
profiles/tower_reference_tolerance.txt records what a run printed."""
import pytest
import torch

import tower_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def by_group(*groups):
    return [c for c in TR.CASES if c.group in groups]


def ids(cases):
    return [TR.case_id(c) for c in cases]


def run(case):
    res = TR.gpu_case(case, DEV)
    print(TR.gpu_line(res))
    TR.assert_gpu_case(case, res)


@pytest.mark.parametrize("case", by_group("one", "lds"), ids=ids(by_group("one", "lds")))
def test_forward_and_backward_one_side(case):
    """tower_fwd_kernel / tower_bwd_kernel <4 | 8 | 16, false | true, 1 | 2> at B = 1, 31, 32, 33, 64, 65, 4096, 4097 (one
    row in the last 64-row workgroup), 4128 (its second tile empty), 4160; packed and strided; h planted with -0.0, +0.0
    and +-2^-126; D = 128, F = 64 on the 64-row form: 149 504 bytes of dynamic LDS."""
    run(case)


@pytest.mark.parametrize("case", by_group("feat", "oob"), ids=ids(by_group("feat", "oob")))
def test_forward_features_and_out_of_range_ids(case):
    """F = 1, 15, 16, 17, 63, 64 on both row-tile forms of every instantiation, ldf > F with the feats base one float off a
    16-byte boundary; ids -1, n_rows, 2^40, -2^63 give zero rows, set the flag, and with oob_flag = NULL still zero rows."""
    run(case)


@pytest.mark.parametrize("case", by_group("pair"), ids=ids(by_group("pair")))
def test_forward_and_backward_two_sides(case):
    """tower_fwd_pair_kernel / tower_bwd_pair_kernel <4 | 8 | 16, 1 | 2>: the sides differ in F, n_rows and strides; each
    against float64 on its own, and the pair equal to the two one-sided calls bit for bit."""
    run(case)


@pytest.mark.parametrize("case", by_group("wgrad", "wpair"), ids=ids(by_group("wgrad", "wpair")))
def test_weight_gradients(case):
    """tower_wgrad_kernel <4 | 8 | 16, false | true>, tower_wgrad_pair_kernel <4 | 8 | 16> and both reduce kernels at
    n_blocks = 1, 2, 16, 17, 112, 113, 128, 129, 130 (B = 8257: one row in the last block): the six tensors against float64,
    two calls bit-identical, the floats past the reported workspace size untouched, one byte less refused."""
    run(case)


# ------------------------------------------------------------------ refusals
def _nan(*s):
    return torch.full(s, float("nan"), device=DEV)


class _Call:
    """A well-formed call of one entry (B = 5, D = 32, F = 3, generous leading dimensions) whose arguments a refusal case
    then spoils one at a time.  Outputs are NaN-prefilled."""

    def __init__(self, entry, E=0, n_sides=1):
        from two_tower_models_amd import _native as N
        self.N, self.entry, self.B, self.D, self.hidden, self.E, self.n_sides = N, entry, 5, 32, 256, E, n_sides
        self.keep, self.outs, sides = [], [], []
        B, D = self.B, self.D
        for _ in range(2):
            t = lambda *s: self._t(torch.zeros(*s, device=DEV))
            o = lambda *s: self._o(_nan(*s))
            if entry == "fwd":
                ids_ = self._t(torch.zeros(B, dtype=torch.int64, device=DEV))
                sides.append(N.TowerFwdSide(t(50, 128), 50, ids_, t(B, 80), 80, 3, t(256, 80), t(256), t(128, 256), t(128), t(128, 512),
                                            t(128), o(B, 256), 256, o(B, 256), o(B, 256), t(B, 256), 256))
            elif entry == "bwd":
                sides.append(N.TowerBwdSide(t(B, 256), 256, t(128, 256), t(128, 512), t(B, 256), o(B, 256), 256, o(B, 128), o(B, 256),
                                            o(B, 256), 256))
            else:
                ws = 1 << 20
                sides.append(N.TowerWgradSide(t(B, 256), 256, t(B, 256), t(B, 128), t(B, 256), t(B, 256), t(B, 80), 80, 3, o(256, 80),
                                              o(256), o(128, 256), o(128), o(128, 512), o(128), t(ws // 4), ws, t(B, 256), 256))
        self.sides = (type(sides[0]) * 2)(*sides)
        self.flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def _t(self, x):
        self.keep.append(x)
        return x.data_ptr()

    def _o(self, x):
        self.outs.append(x)
        return x.data_ptr()

    def call(self):
        lib, N = self.N.load(), self.N
        with TR.Launches(TR.KERNELS) as n:
            if self.entry == "fwd":
                rc = lib.tt_tower_fwd(self.sides, self.n_sides, self.B, self.D, self.hidden, self.E, self.flag.data_ptr(), N.stream())
            elif self.entry == "bwd":
                rc = lib.tt_tower_bwd_data(self.sides, self.n_sides, self.B, self.D, self.hidden, self.E, N.stream())
            else:
                rc = lib.tt_tower_bwd_weights(self.sides, self.n_sides, self.B, self.D, self.hidden, self.E, N.stream())
        torch.cuda.synchronize()
        untouched = all(bool(torch.isnan(o).all()) for o in self.outs) and int(self.flag.item()) == 0
        return rc, sum(n.values()), untouched


def _set(field, value=None, add=None):
    def f(call):
        s = call.sides[0]
        setattr(s, field, getattr(s, field) + add if add is not None else value)
    return f


def _arg(**kw):
    def f(call):
        for k, v in kw.items():
            setattr(call, k, v)
    return f


def _exact_ws(short):
    def f(call):
        need = call.N.load().tt_tower_bwd_weights_workspace_bytes(call.B, call.D, 3, 256, call.E)
        call.sides[0].ws_bytes = need - short
    return f


BAD, UNS, WSP = TR.E_BADARG, TR.E_UNSUPPORTED, TR.E_WORKSPACE
ALL3 = ("fwd", "bwd", "wgrad")
REFUSALS = [  # (what, entries, E of the call, how the call is spoiled, the documented code)
    ("ldy % 4", ALL3, 0, _set("ldy", 258), UNS),
    ("y misaligned", ("fwd",), 0, _set("y", add=4), UNS),
    ("extra misaligned", ("fwd", "wgrad"), 64, _set("extra", add=4), UNS),
    ("ldx % 4", ("fwd", "wgrad"), 64, _set("ldx", 258), UNS),
    ("d_emb misaligned", ("bwd",), 0, _set("d_emb", add=4), UNS),
    ("ld_demb % 4", ("bwd",), 0, _set("ld_demb", 258), UNS),
    ("d_extra misaligned", ("bwd",), 64, _set("d_extra", add=4), UNS),
    ("F = 0", ("fwd", "wgrad"), 0, _set("F", 0), UNS),
    ("F = 65", ("fwd", "wgrad"), 0, _set("F", 65), UNS),
    ("D = 96", ALL3, 0, _arg(D=96), UNS),
    ("hidden = 128", ALL3, 0, _arg(hidden=128), UNS),
    ("E = D", ALL3, 32, lambda call: None, UNS),
    ("two sides, E != 0", ALL3, 64, _arg(n_sides=2), UNS),
    ("n_sides = 0", ALL3, 0, _arg(n_sides=0), BAD),
    ("n_sides = 3", ALL3, 0, _arg(n_sides=3), BAD),
    ("B = 0", ALL3, 0, _arg(B=0), BAD),
    ("ldf < F", ("fwd", "wgrad"), 0, _set("ldf", 2), BAD),
    ("ldy < D", ALL3, 0, _set("ldy", 28), BAD),
    ("workspace one byte short", ("wgrad",), 0, _exact_ws(1), WSP),
]


@pytest.mark.parametrize("what,entry,E,spoil,code", [(w, e, E, s, c) for w, es, E, s, c in REFUSALS for e in es],
                         ids=[f"{e}-{w}".replace(" ", "_") for w, es, _, _, _ in REFUSALS for e in es])
def test_refusals_return_their_code_before_anything_is_launched_or_written(what, entry, E, spoil, code):
    """Each refusal of include/tt_hotpath.h: the documented code, zero launches, every output and the flag untouched.  The
    same call unspoiled is accepted (so it is the spoiled argument that is refused)."""
    call = _Call(entry, E)
    spoil(call)
    rc, launches, untouched = call.call()
    assert rc == code and launches == 0 and untouched, (what, entry, rc, launches, untouched)


@pytest.mark.parametrize("entry,E", [(e, E) for e in ALL3 for E in (0, 64)])
def test_the_refusal_base_call_is_accepted(entry, E):
    call = _Call(entry, E)
    if entry == "wgrad":
        _exact_ws(0)(call)
    rc, launches, _ = call.call()
    assert rc == 0 and launches == (2 if entry == "wgrad" else 1), (rc, launches)
