"""The row gathers and the history pool on MI355X (`pytest -m gpu`) against tests/gather_ref.py: tt_hist_embed_pool(_len) on
the float4 and the scalar path through one and two rounds of history positions and one and two trips of the column loop, in
the ids form and the embedded form, with and without pe, reached by every switch (dim % 4, ld_pooled % 4, pe / pooled / x one
float off); ids out of range in both rounds; per-sample lengths with out-of-range ids and NaN in the padded slots;
tt_gather_rows in all four instantiations around their rows-per-workgroup; tt_hist_pool_bwd(_len) through a second trip of
its grid-stride loop.

Every call goes through the C ABI; every operand and output is a view into a NaN-filled buffer.  Every case asserts rc == 0,
exactly the instantiation that ran (through the library's launch counters), x and the gathered rows bit-equal to the
reference, pooled and the pool backward within their derived bounds, the flag, and no byte outside an output view changed."""
import pytest
import torch

import gather_ref as GA

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a, b):
    return bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


@pytest.mark.parametrize("c", GA.POOL_CASES, ids=[GA.pool_id(c) for c in GA.POOL_CASES])
def test_hist_embed_pool(c):
    inp = GA.pool_inputs(c)
    ref = GA.pool_reference(c, inp)
    got = GA.gpu_pool(c, inp, DEV)
    with_len = c.lens in ("list", "bad_lo", "bad_hi")
    print(f"gather-ref pool {GA.pool_id(c)} pooled err/E {GA.pool_worst(ref, got['pooled']):.3f} {got['launches']}")
    assert got["rc"] == 0 and got["launches"] == {GA.POOL_KERNELS[(GA.pool_path(c), with_len)]: 1}, (got["rc"], got["launches"])
    assert bool(torch.isfinite(got["x"]).all()) and bool(torch.isfinite(got["pooled"]).all())
    assert not GA.pool_problems(ref, got["x"], got["pooled"], got["flag"])
    assert got["clean"], "a byte outside an output view changed"
    if c.how and c.dim % 4 == 0:  # the scalar path, reached by a switch: the float4 path's bits on x
        vec = GA.gpu_pool(c, inp, DEV, how=None)
        assert vec["launches"] == {GA.POOL_KERNELS[("v4", with_len)]: 1} and _bits(vec["x"], got["x"])
    if c.lens == "null":  # lengths = NULL: the call without `_len`, bit for bit
        plain = GA.gpu_pool(c, inp, DEV, lengths=False)
        assert plain["launches"] == got["launches"] and _bits(plain["x"], got["x"]) and _bits(plain["pooled"], got["pooled"])


@pytest.mark.parametrize("c", GA.GATHER_CASES, ids=[GA.gather_id(c) for c in GA.GATHER_CASES])
def test_gather_rows(c):
    """gather_rows_kernel<4, 8 | 16 | 32> and <1, 64> at n_ids = 1, rows per workgroup -+ 1 and 1000: ids repeat and go out of
    range (zero rows; the flag set, or oob_flag = NULL); out a strided view of a NaN buffer."""
    table, ids = GA.gather_inputs(c)
    want, flag = GA.gather_reference(c, table, ids)
    got = GA.gpu_gather(c, table, ids, DEV)
    assert got["rc"] == 0 and got["launches"] == {GA.GATHER_KERNELS[GA.gather_instantiation(c)]: 1}, (got["rc"], got["launches"])
    assert _bits(got["out"], want) and got["flag"] == flag and got["clean"]


@pytest.mark.parametrize("c", GA.BWD_CASES, ids=[GA.bwd_id(c) for c in GA.BWD_CASES])
def test_hist_pool_bwd(c):
    """dx += d_pooled / len on the valid rows, d_pooled strided; 100 x 128 x 128 elements take a second trip of the grid-stride
    loop; padded dx rows keep their bits; lengths = NULL is the plain kernel."""
    dx0, dp, lens = GA.bwd_inputs(c)
    got = GA.gpu_bwd(c, dx0, dp, lens, DEV, entry_len=c.lens is not None)
    print(f"gather-ref bwd {GA.bwd_id(c)} err/E {GA.bwd_worst(c, dx0, dp, lens, got['dx']):.3f} {got['launches']}")
    assert got["rc"] == 0 and got["launches"] == {GA.BWD_KERNELS[c.lens == "cycle"]: 1}, (got["rc"], got["launches"])
    assert bool(torch.isfinite(got["dx"]).all()) and not GA.bwd_problems(c, dx0, dp, lens, got["dx"]) and got["clean"]
    if c.lens == "null":
        plain = GA.gpu_bwd(c, dx0, dp, lens, DEV, entry_len=False)
        assert _bits(plain["dx"], got["dx"])


# ------------------------------------------------------------------ refusals
ARGS = {
    "gather": "table n_rows dim ids n_ids out ld_out flag",
    "pool": "table n_rows dim ids B H pe x pooled ld_pooled flag",
    "pool_len": "table n_rows dim ids B H lengths pe x pooled ld_pooled flag",
    "bwd": "dx B H dim d_pooled ld_pooled",
    "bwd_len": "dx B H dim lengths d_pooled ld_pooled",
}
OUTPUTS = {"gather": ("out",), "pool": ("x", "pooled"), "pool_len": ("x", "pooled"), "bwd": ("dx",), "bwd_len": ("dx",)}
LAUNCHES = {"gather": 1, "pool": 1, "pool_len": 1, "bwd": 1, "bwd_len": 1}
MAY_BE_NULL = {"gather": ("flag",), "pool": ("ids", "pe"), "pool_len": ("ids", "pe", "lengths"), "bwd": (), "bwd_len": ("lengths",)}
SCALARS = ("n_rows", "dim", "n_ids", "ld_out", "B", "H", "ld_pooled")


class _Call:
    """A well-formed call of one entry (dim = 8, B = 3, H = 5, 7 ids of 10 rows) whose arguments a refusal case then spoils
    one at a time.  Outputs are NaN-prefilled."""

    def __init__(self, entry):
        from two_tower_models_amd import _native as N
        self.N, self.entry = N, entry
        self.v = dict(n_rows=10, dim=8, n_ids=7, ld_out=8, B=3, H=5, ld_pooled=8)
        self.bufs = {}
        for name in ARGS[entry].split():
            if name in SCALARS:
                continue
            if name == "ids":
                t = torch.zeros(64, dtype=torch.int64, device=DEV)
            elif name in ("lengths", "flag"):
                t = (torch.ones if name == "lengths" else torch.zeros)(64, dtype=torch.int32, device=DEV)
            else:
                t = torch.full((4096,), float("nan") if name in OUTPUTS[entry] else 0.0, device=DEV)
            self.bufs[name] = t
            self.v[name] = t.data_ptr()

    def call(self):
        lib = self.N.load()
        f = {"gather": lib.tt_gather_rows, "pool": lib.tt_hist_embed_pool, "pool_len": lib.tt_hist_embed_pool_len,
             "bwd": lib.tt_hist_pool_bwd, "bwd_len": lib.tt_hist_pool_bwd_len}[self.entry]
        with GA.Launches(GA.KERNELS) as n:
            rc = f(*[self.v[a] for a in ARGS[self.entry].split()], self.N.stream())
        torch.cuda.synchronize()
        untouched = all(bool(torch.isnan(self.bufs[o]).all()) for o in OUTPUTS[self.entry])
        if "flag" in self.bufs:
            untouched = untouched and int(self.bufs["flag"].abs().sum()) == 0
        return rc, sum(n.values()), untouched


def _set(**kw):
    return lambda call: call.v.update(kw)


POOLS, BWDS = ("pool", "pool_len"), ("bwd", "bwd_len")
REFUSALS = [  # (what, entries, how the call is spoiled): every one is TT_E_BADARG
    ("dim = 0", ("gather",) + POOLS + BWDS, _set(dim=0)), ("dim = -4", ("gather",) + POOLS + BWDS, _set(dim=-4)),
    ("H = 0", POOLS + BWDS, _set(H=0)), ("H = -1", POOLS + BWDS, _set(H=-1)),
    ("ld_out < dim", ("gather",), _set(ld_out=7)), ("ld_pooled < dim", POOLS + BWDS, _set(ld_pooled=7)),
    ("n_rows = 0", ("gather",) + POOLS, _set(n_rows=0)), ("n_rows = -1", ("gather",) + POOLS, _set(n_rows=-1)),
    ("n_ids = -1", ("gather",), _set(n_ids=-1)), ("B = -1", POOLS + BWDS, _set(B=-1)),
]
REFUSALS += [(f"{name} = NULL", (entry,), _set(**{name: None})) for entry in ARGS for name in ARGS[entry].split()
             if name not in SCALARS and name not in MAY_BE_NULL[entry]]
CASES = [(w, e, s) for w, es, s in REFUSALS for e in es]


@pytest.mark.parametrize("what,entry,spoil", CASES, ids=[f"{e}-{w}".replace(" ", "_") for w, e, _ in CASES])
def test_refusals_return_their_code_before_anything_is_launched_or_written(what, entry, spoil):
    call = _Call(entry)
    spoil(call)
    rc, launches, untouched = call.call()
    assert rc == GA.E_BADARG and launches == 0 and untouched, (what, entry, rc, launches, untouched)


@pytest.mark.parametrize("entry", list(ARGS))
def test_the_refusal_base_call_and_an_empty_one_are_accepted(entry):
    """The unspoiled call runs its one kernel; B = 0 (n_ids = 0) returns 0 and writes nothing."""
    rc, launches, _ = _Call(entry).call()
    assert rc == 0 and launches == LAUNCHES[entry], (rc, launches)
    call = _Call(entry)
    call.v.update(n_ids=0, B=0)
    rc, launches, untouched = call.call()
    assert rc == 0 and launches == 0 and untouched, (rc, launches, untouched)
