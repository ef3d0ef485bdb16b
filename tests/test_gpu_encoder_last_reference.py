"""The collapsed last encoder layer on MI355X (`pytest -m gpu`) against the float64 reference of tests/encoder_last_ref.py: the
uncollapsed layer with torch autograd, the saved tensors from the header's definitions.  Four input classes (flat, peaked,
scores near +-200, a K bias of 1e3); B = 1 .. 257 (32-sample groups with 1, 31, 32 samples in the last, the reduce over 1, 2, 3,
4, 5, 8, 9 partials); every tile edge of the MFMA loop (D = 4 .. 128, 1 .. 16 heads); H = 1 .. 64; per-sample lengths, the
out-of-contract ones included, with NaN in the forward's padded rows; operands one float off alignment and strided.

Every call goes through the C ABI; every operand and output is a view into a NaN-filled buffer, the workspace is NaN-filled
and exactly as long as reported.  Every case asserts rc == 0, exactly the launches of each entry (through the library's launch
counters), all eleven quantities finite and within their bound, db_in[D:2D] == 0.0, no byte outside an output view changed,
tt_enc_last_bwd == _data then _weights bit for bit, and a second backward call the same bits.
profiles/encoder_last_reference_tolerance.txt records what a run printed."""
import pytest
import torch

import encoder_last_ref as ER

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def by_group(*groups):
    return [c for c in ER.CASES if c.group in groups]


def ids(cases):
    return [ER.case_id(c) for c in cases]


def run(case):
    res = ER.gpu_case(case, DEV)
    print(ER.gpu_line(res))
    ER.assert_gpu_case(case, res)


@pytest.mark.parametrize("case", by_group("batch"), ids=ids(by_group("batch")))
def test_batch_sizes_and_the_partial_reduce(case):
    """H = 50, D = 128, 4 heads: nb = 1, 31, 32 samples in the last 32-sample group; enc_last_reduce_kernel over 1, 2, 3, 4, 5,
    8 and 9 partials (tail only, one unrolled trip, unrolled plus tail, two unrolled plus tail)."""
    run(case)


@pytest.mark.parametrize("case", by_group("width"), ids=ids(by_group("width")))
def test_tile_edges_of_every_width(case):
    """mma_tile / el_fetch at every edge: the smallest widths; dh = 12 (a tile of three heads, a last tile of 4 columns); dh = 4
    (a tile of eight heads); D around the lane + 64 column of the main kernels; a head boundary mid-tile; K % 8 == 4; a last
    tile of 28 columns; four trips of the k loop.  Flat and peaked."""
    run(case)


@pytest.mark.parametrize("case", by_group("history", "kbias"), ids=ids(by_group("history", "kbias")))
def test_history_lengths_of_the_shape_and_every_input_class(case):
    """H = 1, 2, 31, 32, 33, 50, 63, 64 at (128, 4) and (64, 16): flat, peaked, scores near +200 / -200 (the -3.0e38 sentinel,
    the max subtraction, __expf), and a K bias of 1e3 that the kernels' algebra drops."""
    run(case)


@pytest.mark.parametrize("case", by_group("lengths"), ids=ids(by_group("lengths")))
def test_per_sample_lengths(case):
    """tt_enc_last_fwd_len, then the unchanged backward: lengths 1 .. H; 0, -3, H + 1 and 2^31 - 1 clamped to [1, H]; the
    forward's x holds NaN in its padded rows, the backward's copy finite garbage of scale 50; padded probs and dx rows exactly
    zero; lengths = NULL the very bits (and the very kernels) of tt_enc_last_fwd."""
    run(case)


@pytest.mark.parametrize("case", by_group("placement"), ids=ids(by_group("placement")))
def test_operand_placement(case):
    """recent one float off a 16-byte boundary with ld = D + 3, or as out[:, 0, :] of [B, 2, D]; d_recent with ld = 2D; q0,
    ctx0, probs, b_in, b_out one float off alignment."""
    run(case)


# ------------------------------------------------------------------ refusals
ARGS = {
    "fwd": "x B H D heads w_in b_in w_out b_out recent ld_recent q0 t probs xbar ctx0",
    "fwd_len": "x B H D heads lengths w_in b_in w_out b_out recent ld_recent q0 t probs xbar ctx0",
    "data": "x B H D heads w_in w_out d_recent ld_dr t probs dx ws ws_bytes",
    "weights": "x B H D heads d_recent ld_dr q0 xbar ctx0 dW_in db_in dW_out db_out ws ws_bytes",
    "whole": "x B H D heads w_in w_out d_recent ld_dr q0 t probs xbar ctx0 dx dW_in db_in dW_out db_out ws ws_bytes",
}
OUTPUTS = {"fwd": "recent q0 t probs xbar ctx0", "fwd_len": "recent q0 t probs xbar ctx0", "data": "dx ws",
           "weights": "dW_in db_in dW_out db_out ws", "whole": "dx dW_in db_in dW_out db_out ws"}
LAUNCHES = {"fwd": 3, "fwd_len": 3, "data": 3, "weights": 2, "whole": 5}
SCALARS = ("B", "H", "D", "heads", "ld_recent", "ld_dr", "ws_bytes")


class _Call:
    """A well-formed call of one entry (B = 5, H = 6, D = 8, 2 heads, leading dimensions of 136; fwd_len with lengths of 3)
    whose arguments a refusal case then spoils one at a time.  Inputs are zeros, outputs and the workspace NaN-prefilled, all
    16-byte aligned."""

    def __init__(self, entry):
        from two_tower_models_amd import _native as N
        self.N, self.entry = N, entry
        lib = N.load()
        self.v = dict(B=5, H=6, D=8, heads=2, ld_recent=136, ld_dr=136)
        self.v["ws_bytes"] = lib.tt_enc_last_bwd_workspace_bytes(5, 6, 8, 2)
        self.bufs = {}
        for name in ARGS[entry].split():
            if name in SCALARS:
                continue
            out = name in OUTPUTS[entry].split()
            if name == "lengths":
                self.bufs[name] = torch.full((64,), 3, dtype=torch.int32, device=DEV)
            else:
                self.bufs[name] = torch.full((1 << 16,), float("nan") if out else 0.0, device=DEV)
            self.v[name] = self.bufs[name].data_ptr()

    def call(self):
        lib = self.N.load()
        f = {"fwd": lib.tt_enc_last_fwd, "fwd_len": lib.tt_enc_last_fwd_len, "data": lib.tt_enc_last_bwd_data,
             "weights": lib.tt_enc_last_bwd_weights, "whole": lib.tt_enc_last_bwd}[self.entry]
        with ER.Launches(ER.KERNELS) as n:
            rc = f(*[self.v[a] for a in ARGS[self.entry].split()], self.N.stream())
        torch.cuda.synchronize()
        untouched = all(bool(torch.isnan(self.bufs[o]).all()) for o in OUTPUTS[self.entry].split())
        return rc, sum(n.values()), untouched


def _set(**kw):
    return lambda call: call.v.update(kw)


def _off(name):
    return lambda call: call.v.update({name: call.v[name] + 4})


def _null(name):
    return lambda call: call.v.update({name: None})


def _short(call):
    call.v["ws_bytes"] -= 1


BAD, UNS, WSP = ER.E_BADARG, ER.E_UNSUPPORTED, ER.E_WORKSPACE
FWD, BWD = ("fwd", "fwd_len"), ("data", "weights", "whole")
ALL = FWD + BWD
REFUSALS = [  # (what, entries, how the call is spoiled, the documented code)
    ("H = 0", ALL, _set(H=0), UNS), ("H = 65", ALL, _set(H=65), UNS),
    ("D = 0", ALL, _set(D=0), UNS), ("D = 6", ALL, _set(D=6), UNS), ("D = 132", ALL, _set(D=132, heads=1), UNS),
    ("heads = 0", ALL, _set(heads=0), UNS), ("heads = 17", ALL, _set(D=68, heads=17), UNS),
    ("D % heads", ALL, _set(D=40, heads=3), UNS), ("head width % 4", ALL, _set(D=40, heads=4), UNS),
    ("ld_recent < D", FWD, _set(ld_recent=4), UNS), ("ld_dr < D", BWD, _set(ld_dr=4), UNS),
    ("ld_dr % 4", BWD, _set(ld_dr=138), BAD),
    ("x misaligned", ALL, _off("x"), BAD),
    ("w_in misaligned", FWD + ("data", "whole"), _off("w_in"), BAD),
    ("w_out misaligned", FWD + ("data", "whole"), _off("w_out"), BAD),
    ("t misaligned", FWD + ("data", "whole"), _off("t"), BAD),
    ("xbar misaligned", FWD + ("weights", "whole"), _off("xbar"), BAD),
    ("dx misaligned", ("data", "whole"), _off("dx"), BAD),
    ("d_recent misaligned", BWD, _off("d_recent"), BAD),
    ("ws misaligned", BWD, _off("ws"), BAD),
    ("B < 0", ALL, _set(B=-1), BAD),
    ("workspace one byte short", BWD, _short, WSP),
]
REFUSALS += [(f"{name} = NULL", (entry,), _null(name), BAD) for entry in ALL for name in ARGS[entry].split()
             if name not in SCALARS + ("lengths",)]
CASES = [(w, e, s, c) for w, es, s, c in REFUSALS for e in es]


@pytest.mark.parametrize("what,entry,spoil,code", CASES, ids=[f"{e}-{w}".replace(" ", "_") for w, e, _, _ in CASES])
def test_refusals_return_their_code_before_anything_is_launched_or_written(what, entry, spoil, code):
    """Each refusal of include/tt_hotpath.h: the documented code, zero launches, every NaN-prefilled output and the
    workspace untouched.  (The same call unspoiled is accepted: the test below.)"""
    call = _Call(entry)
    spoil(call)
    rc, launches, untouched = call.call()
    assert rc == code and launches == 0 and untouched, (what, entry, rc, launches, untouched)


@pytest.mark.parametrize("entry", ALL)
def test_the_refusal_base_call_is_accepted(entry):
    rc, launches, _ = _Call(entry).call()
    assert rc == 0 and launches == LAUNCHES[entry], (rc, launches)


@pytest.mark.parametrize("entry", ALL)
def test_an_empty_batch_is_accepted(entry):
    """B = 0: the forward and _data write nothing; _weights (and so the whole backward) writes zero gradients."""
    call = _Call(entry)
    call.v["B"] = 0
    rc, launches, untouched = call.call()
    assert rc == 0 and launches == 0, (rc, launches)
    if entry in FWD + ("data",):
        assert untouched
    else:
        D = call.v["D"]
        for name, n in (("dW_in", 3 * D * D), ("db_in", 3 * D), ("dW_out", D * D), ("db_out", D)):
            assert float(call.bufs[name][:n].abs().max()) == 0.0 and bool(torch.isnan(call.bufs[name][n:]).all()), name
        assert bool(torch.isnan(call.bufs["ws"]).all()) and (entry == "weights" or bool(torch.isnan(call.bufs["dx"]).all()))
