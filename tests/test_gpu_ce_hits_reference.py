"""The in-batch softmax with accidental hits masked (tt_inbatch_ce_masked_fwd / _bwd: the MASK forms of csrc/inbatch_ce.hip,
the key argument of ce_wide.hip) against the float64 reference of tests/ce_hits_ref.py, on MI355X (`pytest -m gpu`):
every forward form and backward through the C ABI at every width class, staging form and key pattern of
ce_hits_ref.CASES, operands in ce_ref's strided and misaligned layouts inside NaN-filled buffers, outputs inside
sentinel-filled ones.  Every forward runs twice into NaN-filled outputs with the workspace overwritten in between and must
agree with itself bit for bit.  Bounds: ce_hits_ref.tol (ce_ref's flat figures; 4 x the float32 CPU yardstick for the twin
class); profiles/ce_hits_reference_tolerance.txt records what the GPU showed.  Then: distinct keys and no keys are the
same bits, no keys is the _bias_ call, and every refusal."""
import pytest
import torch

import ce_hits_ref as H
from test_gpu_logq import DEV, _ld, abi_bwd, abi_bwd_kept, abi_fwd

C = H.C
pytestmark = pytest.mark.gpu
NAN = float("nan")
TAIL = 64  # floats behind the padded logits buffer that no call may touch


@pytest.fixture(scope="module")
def T():
    from two_tower_models_amd import _native as N
    from two_tower_models_amd import ops
    N.load()
    return ops, N


def bits(t):
    return t.contiguous().view(torch.int32)


def output(shape, lay):
    buf, view = C.place(shape, lay, C.SENTINEL, DEV)
    view.fill_(NAN)
    return buf, view


def workspace(T, M, Nn, D):
    ops, N = T
    return ops._ws(torch.device(DEV), N.load().tt_inbatch_ce_masked_workspace_bytes(M, Nn, D), "hits_test")


def masked_fwd(T, U, I, off, bias, key, form="plain", labels=None, uvw=None, *, du_unit=None, logits=None, fill=NAN):
    """tt_inbatch_ce_masked_fwd in one of its four forms; bias / key None = NULL.  -> dict of its outputs."""
    ops, N = T
    lib = N.load()
    M, D = U.shape
    Nn = I.shape[0]
    e = lambda *shape: torch.empty(*shape, device=DEV).fill_(fill)
    out = dict(lse=e(M), ce=e(M))
    wsp, wsn = workspace(T, M, Nn, D)
    du, zn, tail = None, 0, (None, 1, None, None, None, None)
    if form != "plain":
        du = out["du_unit"] = e(M, D) if du_unit is None else du_unit
    if form == "keep":
        zn = lib.tt_inbatch_ce_logits_bytes(M, Nn)
        logits = out["logits"] = torch.empty(zn // 4, device=DEV).fill_(fill) if logits is None else logits
    else:
        logits = None
    if form == "loss":
        out.update(w=e(M), coef=e(M), loss=e(()))
        tail = (N.ptr(labels), labels.shape[1] if labels is not None else 1, uvw.data_ptr(), out["w"].data_ptr(),
                out["coef"].data_ptr(), out["loss"].data_ptr())
    N.check(lib.tt_inbatch_ce_masked_fwd(U.data_ptr(), _ld(U), I.data_ptr(), _ld(I), M, Nn, D, off, N.ptr(bias), N.ptr(key),
                                         out["lse"].data_ptr(), out["ce"].data_ptr(), N.ptr(du), _ld(du) if du is not None else D,
                                         N.ptr(logits), zn, *tail, wsp, wsn, N.stream()), "tt_inbatch_ce_masked_fwd")
    return out


def masked_bwd(T, U, I, off, bias, key, lse, coef, with_du=True, *, dU=None, dI=None):
    ops, N = T
    lib = N.load()
    M, D = U.shape
    Nn = I.shape[0]
    wsp, wsn = workspace(T, M, Nn, D)
    if with_du and dU is None:
        dU = torch.empty(M, D, device=DEV).fill_(NAN)
    dU = dU if with_du else None
    dI = torch.empty(Nn, D, device=DEV).fill_(NAN) if dI is None else dI
    N.check(lib.tt_inbatch_ce_masked_bwd(U.data_ptr(), _ld(U), I.data_ptr(), _ld(I), M, Nn, D, off, N.ptr(bias), N.ptr(key),
                                         lse.data_ptr(), coef.data_ptr(), N.ptr(dU), _ld(dU) if dU is not None else D, dI.data_ptr(),
                                         _ld(dI), wsp, wsn, N.stream()), "tt_inbatch_ce_masked_bwd")
    return dU, dI


def forward_twice(T, c, Uv, Iv, bd, kd, lab, uvw):
    """The forward of case c, twice; -> the outputs of the second run."""
    wsbuf = T[1].scratch.get(torch.device(DEV), T[1].load().tt_inbatch_ce_masked_workspace_bytes(c.M, c.N, c.D), "hits_test")
    Mp, Np = -(-c.M // 128) * 128, -(-c.N // 128) * 128
    runs = []
    for _ in range(2):
        dubuf, duv = output((c.M, c.D), c.ldun) if c.entry != "plain" else (None, None)
        zbuf = torch.full((Mp * Np + TAIL,), C.SENTINEL, device=DEV) if c.entry == "keep" else None
        out = masked_fwd(T, Uv, Iv, c.off, bd, kd, c.entry, labels=lab, uvw=uvw, du_unit=duv, logits=zbuf)
        torch.cuda.synchronize()
        if duv is not None:
            assert C.slack_intact(dubuf, duv), "du_unit: a write outside the view"
        if zbuf is not None:
            assert bool((zbuf[Mp * Np:] == C.SENTINEL).all()), "logits: a write behind the padded buffer"
            unwritten = zbuf[:Mp * Np].view(Mp, Np)[:, -(-c.N // 64) * 64:]
            assert bool((unwritten == C.SENTINEL).all()), "logits: a write into the unwritten columns of the padded buffer"
        runs.append(out)
        wsbuf.fill_(0xA5)
    for k in runs[0]:
        assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), f"{k}: the second run differs from the first"
    return runs[1]


def run_case(T, c):
    """A HIP error ends the session: after a fault nothing more is started on the device."""
    try:
        return _run_case(T, c)
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"device error at {H.case_id(c)}: {e}", returncode=3)
        raise


def _run_case(T, c):
    ref = H.case_reference(c)
    U, I, b, kv, coef, labels = H.inputs(H.math_key(c))
    _, Uv = C.place(U, c.lu, NAN, DEV)
    _, Iv = C.place(I, c.li, NAN, DEV)
    bd, kd, cd = (None if b is None else b.to(DEV)), kv.to(DEV), coef.to(DEV)
    out = forward_twice(T, c, Uv, Iv, bd, kd, labels.to(DEV), C.UVW.to(DEV))
    got = {"ce": out["ce"]}
    if c.D <= 128:
        got["lse"] = out["lse"].double() * C.LN2
    if "du_unit" in out:
        got["du_unit"] = out["du_unit"]
    if "logits" in out:
        Mp, Np = -(-c.M // 128) * 128, -(-c.N // 128) * 128
        got["logits"] = out["logits"][:Mp * Np].view(Mp, Np)[:c.M, :c.N]
    kind, with_du = H.ENTRIES[c.entry]
    dibuf, div = output((c.N, c.D), c.ldi)
    if kind == "kept":
        abi_bwd_kept(T, Uv, c.N, c.off, out["lse"], cd, out["logits"], dI=div)  # unchanged: the kept logits carry the mask
    else:
        dubuf, duv = output((c.M, c.D), c.ldu) if with_du else (None, None)
        masked_bwd(T, Uv, Iv, c.off, bd, kd, out["lse"], cd, with_du, dU=duv, dI=div)
        if with_du:
            assert C.slack_intact(dubuf, duv), "dU: a write outside the view"
            got["dU"] = duv
    torch.cuda.synchronize()
    assert C.slack_intact(dibuf, div), "dI: a write outside the view"
    got["dI"] = div
    assert set(got) == H.compared(c)  # (what the mutants of test_ce_hits_reference_cpu.py are counted against)
    r = H.ratios(got, ref, c.cls)
    if "loss" in out:
        lt = H.loss_tolerances(ref, c.cls)
        r["w"] = C.ratio(out["w"], ref["w"], lt["w"])
        r["coef_w"] = C.ratio(out["coef"], ref["coef_w"], lt["coef_w"])
        r["loss"] = C.ratio(out["loss"], ref["loss"], lt["loss"])
    if c.pattern == "all_same":  # every row keeps its positive only: exactly 0, from the kernels as in float64
        for q in ("ce", "du_unit", "dU", "dI"):
            if q in got:
                assert float(got[q].abs().max()) == 0.0, f"all_same: {q} is not exactly 0"
    return r


@pytest.mark.parametrize("c", H.CASES, ids=H.case_id)
def test_masked_ce_matches_float64(T, c):
    r = run_case(T, c)
    p = H.case_plan(c)
    print(f"CE_HITS {c.entry} dp8={p['dp8']} {H.staging_of(c)} di={p['stage_di']} {c.cls} {c.pattern} {H.case_id(c)} "
          + " ".join(f"{q}={v:.3g}" for q, v in r.items()))
    assert max(r.values()) <= 1.0, r


def test_unmasked_kernels_miss_every_twin_bound_by_orders_of_magnitude(T):
    """What the feature is for: the calls WITHOUT keys at twin inputs with hits are off by far more than the bound."""
    for c in [c for c in H.CASES if c.cls == "twin" and c.pattern in ("pairs", "mod61", "zipf") and c.entry == "du"][:4]:
        ref = H.case_reference(c)
        U, I, b, kv, coef, labels = H.inputs(H.math_key(c))
        out = abi_fwd(T, U.to(DEV), I.to(DEV), c.off, None if b is None else b.to(DEV), "du", fill=NAN)
        r = H.ratios({"ce": out["ce"]}, ref, "twin")
        assert r["ce"] > 1000.0, (H.case_id(c), r)


# ------------------------------------------------------------------ no hits / no keys: the same bits
SAME = [(77, 203, 126, 24, "odd_ld"), (130, 700, 200, 32, "dense"), (300, 300, 0, 50, "pad4"), (321, 577, 256, 64, "strided16"),
        (385, 449, 64, 100, "misaligned"), (129, 1000, 871, 128, "dense"), (130, 700, 200, 200, "dense"), (1, 1, 0, 64, "dense")]


def all_forms(T, fwd, bwd, Uv, Iv, off, bd, kd, cd, lab, uvw, keep_ok):
    """{name: tensor} of every output of the four forward forms and the backwards behind them."""
    res = {}
    for form in ("plain", "du", "loss") + (("keep",) if keep_ok else ()):
        out = fwd(form)
        res.update({f"{form}.{k}": v for k, v in out.items()})
        if form in ("plain", "du"):
            dU, dI = bwd(out["lse"], form == "plain")
            res[f"{form}.dI"] = dI
            if dU is not None:
                res[f"{form}.dU"] = dU
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("term", ["zipf", "none"])
@pytest.mark.parametrize("M,Nn,off,D,lay", SAME)
def test_distinct_keys_and_no_keys_give_the_same_bits(T, M, Nn, off, D, lay, term):
    """`none` keys against item_key = NULL, and NULL against the _bias_ call: bit-identical in every form, with a term
    (the same BIAS = true kernels, the mask never firing) and without one (the MASK forms carry a zero term, and
    fma(acc, log2 e, 0) rounds like the plain multiply; the wide path adds nothing to an unmasked logit)."""
    key = (M, Nn, D, off, "flat", "none", term)
    U, I, b, kv, coef, labels = H.inputs(key)
    _, Uv = C.place(U, lay, NAN, DEV)
    _, Iv = C.place(I, lay, NAN, DEV)
    bd, kd, cd, lab, uvw = (None if b is None else b.to(DEV)), kv.to(DEV), coef.to(DEV), labels.to(DEV), C.UVW.to(DEV)
    keep_ok = D in (32, 64, 128) and lay in ("dense", "strided16")
    runs = {}
    for name, k in (("keys", kd), ("null", None)):
        runs[name] = all_forms(T, lambda form: masked_fwd(T, Uv, Iv, off, bd, k, form, labels=lab, uvw=uvw),
                               lambda lse, with_du: masked_bwd(T, Uv, Iv, off, bd, k, lse, cd, with_du), Uv, Iv, off, bd, k, cd, lab,
                               uvw, keep_ok)
    runs["bias"] = all_forms(T, lambda form: abi_fwd(T, Uv, Iv, off, bd, form, labels=lab, uvw=uvw, fill=NAN),
                             lambda lse, with_du: abi_bwd(T, Uv, Iv, off, bd, lse, cd, with_du), Uv, Iv, off, bd, None, cd, lab, uvw,
                             keep_ok)
    for name in runs["null"]:
        a, n, bb = runs["keys"][name], runs["null"][name], runs["bias"][name]
        if name == "keep.logits":  # (the _bias_ helper allocates bytes, and columns past the last tile stay unwritten)
            Mp, Np = -(-M // 128) * 128, -(-Nn // 128) * 128
            cut = lambda z: z.view(torch.float32)[:Mp * Np].view(Mp, Np)[:, :-(-Nn // 64) * 64]
            a, n, bb = cut(a), cut(n), cut(bb)
        assert torch.equal(bits(n), bits(bb)), f"{name}: item_key = NULL differs from the _bias_ call"
        assert torch.equal(bits(a), bits(n)), f"{name}: distinct keys differ from item_key = NULL"


# ------------------------------------------------------------------ refusals
def test_refusals(T):
    ops, N = T
    lib = N.load()
    M, Nn, D = 130, 200, 64
    U, I = torch.zeros(M, D, device=DEV), torch.zeros(Nn, D, device=DEV)
    key = torch.arange(Nn, dtype=torch.int32, device=DEV)
    lse, ce = torch.zeros(M, device=DEV), torch.zeros(M, device=DEV)
    du, dI, coef = torch.zeros(M, D, device=DEV), torch.zeros(Nn, D, device=DEV), torch.zeros(M, device=DEV)
    w, cf, loss, uvw = torch.zeros(M, device=DEV), torch.zeros(M, device=DEV), torch.zeros((), device=DEV), torch.ones(1, device=DEV)
    zn = lib.tt_inbatch_ce_logits_bytes(M, Nn)
    z = torch.zeros(zn // 4, device=DEV)
    wsp, wsn = workspace(T, M, Nn, D)
    assert wsn >= lib.tt_inbatch_ce_masked_workspace_bytes(M, Nn, D) == lib.tt_inbatch_ce_bias_workspace_bytes(M, Nn, D)
    assert lib.tt_inbatch_ce_masked_workspace_bytes(0, Nn, D) == 0
    P = lambda t: None if t is None else t.data_ptr()

    def fwd(U=U, ldu=D, I=I, ldi=D, M=M, Nn=Nn, D=D, off=0, key=key, lse=lse, ce=ce, du=None, ld_du=D, z=None, zn=0, T_=1, uvw=None,
            w=None, cf=None, loss=None, ws=wsp, wsn=wsn):
        return lib.tt_inbatch_ce_masked_fwd(P(U), ldu, P(I), ldi, M, Nn, D, off, None, P(key), P(lse), P(ce), P(du), ld_du, P(z), zn,
                                            None, T_, P(uvw), P(w), P(cf), P(loss), ws, wsn, N.stream())

    def bwd(U=U, ldu=D, I=I, ldi=D, M=M, Nn=Nn, D=D, off=0, key=key, lse=lse, coef=coef, dU=du, lddu=D, dI=dI, lddi=D, ws=wsp, wsn=wsn):
        return lib.tt_inbatch_ce_masked_bwd(P(U), ldu, P(I), ldi, M, Nn, D, off, None, P(key), P(lse), P(coef), P(dU), lddu, P(dI), lddi,
                                            ws, wsn, N.stream())

    def refused(rc, code, text):
        assert rc == code, (rc, code, text)
        msg = lib.tt_last_error_string().decode()
        assert text in msg, (msg, text)

    BAD, UNS, WSE = N.TT_E_BADARG, N.TT_E_UNSUPPORTED, N.TT_E_WORKSPACE
    assert fwd() == 0 and fwd(du=du) == 0 and bwd() == 0 and fwd(key=None) == 0 and bwd(key=None) == 0
    for kw in (dict(U=None), dict(I=None), dict(lse=None), dict(ce=None), dict(ws=None)):
        refused(fwd(**kw), BAD, "tt_inbatch_ce_masked_fwd: null pointer")
    for kw in (dict(M=0), dict(Nn=0), dict(D=0), dict(ldu=D - 1), dict(ldi=D - 1), dict(du=du, ld_du=D - 1)):
        refused(fwd(**kw), BAD, "tt_inbatch_ce_masked_fwd: sizes")
    for kw in (dict(off=-1), dict(off=Nn - M + 1)):
        refused(fwd(**kw), BAD, "tt_inbatch_ce_masked_fwd: diagonal outside the item block")
        refused(bwd(**kw), BAD, "tt_inbatch_ce_masked_bwd: diagonal outside the item block")
    refused(fwd(z=z, zn=zn), BAD, "kept logits and the loss tail need du_unit")
    refused(fwd(uvw=uvw, w=w, cf=cf, loss=loss), BAD, "kept logits and the loss tail need du_unit")
    refused(fwd(du=du, uvw=uvw, w=w, cf=cf), BAD, "tt_inbatch_ce_masked_fwd: null pointer")
    refused(fwd(du=du, z=z, zn=zn, uvw=uvw, w=w, cf=cf, loss=loss), UNS, "kept logits and the fused loss tail together")
    refused(fwd(wsn=lib.tt_inbatch_ce_masked_workspace_bytes(M, Nn, D) - 1), WSE, "tt_inbatch_ce_masked_fwd: workspace")
    refused(fwd(du=du, z=z, zn=zn - 4), WSE, "logits buffer")
    for kw in (dict(U=None), dict(I=None), dict(lse=None), dict(coef=None), dict(dI=None), dict(ws=None)):
        refused(bwd(**kw), BAD, "tt_inbatch_ce_masked_bwd: null pointer")
    for kw in (dict(M=0), dict(ldu=D - 1), dict(ldi=D - 1), dict(lddu=D - 1), dict(lddi=D - 1)):
        refused(bwd(**kw), BAD, "tt_inbatch_ce_masked_bwd: sizes")
    refused(bwd(wsn=lib.tt_inbatch_ce_masked_workspace_bytes(M, Nn, D) - 1), WSE, "tt_inbatch_ce_masked_bwd: workspace")
    assert bwd(dU=None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the ops, with keys
@pytest.mark.parametrize("term", ["none", "zipf"])
@pytest.mark.parametrize("keep", [None, True, False])
@pytest.mark.parametrize("keys", ["mod61", "zipf", "sixth_argument_None"])
def test_op_with_keys_and_wide_negatives(T, keys, keep, term):
    """ops.InBatchSoftmaxCE.apply(U, I, off, keep_logits, item_bias, item_key) at N >= 4 M (130 x 700, D = 128: the kept-logits
    pair is the default there) through forward AND backward: ce, dU, dI against float64, and the kept pair running exactly
    when asked for.  `sixth_argument_None`: item_key = None passed explicitly -- the unmasked result, six inputs."""
    ops, N = T
    M, Nn, D, off = 130, 700, 128, 200
    explicit_none = keys == "sixth_argument_None"
    key = (M, Nn, D, off, "flat", "none", term) if explicit_none else (M, Nn, D, off, "twin", keys, term)
    U, I, b, kv, coef, _ = H.inputs(key)
    ref = H.key_reference(key)
    Ud, Id = U.to(DEV).requires_grad_(True), I.to(DEV).requires_grad_(True)
    N.trace = []
    try:
        ce = ops.InBatchSoftmaxCE.apply(Ud, Id, off, keep, None if b is None else b.to(DEV), None if explicit_none else kv.to(DEV))
        (ce * coef.to(DEV)).sum().backward()
        calls = list(N.trace)
    finally:
        N.trace = None
    assert ("tt_inbatch_ce_bwd_kept" in calls) == (keep is None or keep), calls
    assert ("tt_inbatch_ce_masked_fwd" in calls) == (not explicit_none), calls
    r = H.ratios({"ce": ce.detach(), "dU": Ud.grad, "dI": Id.grad}, ref, key[4])
    print(f"CE_HITS_OP keys={keys} keep={keep} term={term} " + " ".join(f"{q}={v:.3g}" for q, v in r.items()))
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("term", ["none", "zipf"])
@pytest.mark.parametrize("keys", ["pairs", "sixth_argument_None"])
def test_fused_loss_op_with_keys(T, keys, term):
    """ops.InBatchSoftmaxWeightedLoss.apply(U, I, labels, uvw, item_bias, item_key), forward and backward (300 x 300, D = 64)."""
    ops, N = T
    M, Nn, D, off = 300, 300, 64, 0
    explicit_none = keys == "sixth_argument_None"
    key = (M, Nn, D, off, "flat", "none", term) if explicit_none else (M, Nn, D, off, "twin", keys, term)
    U, I, b, kv, _, labels = H.inputs(key)
    ref = H.reference(key)  # (its dU / dI are those of sum(coef ce): redone below for the loss)
    Ud, Id = U.to(DEV).requires_grad_(True), I.to(DEV).requires_grad_(True)
    loss = ops.InBatchSoftmaxWeightedLoss.apply(Ud, Id, labels.to(DEV), C.UVW.to(DEV), None if b is None else b.to(DEV),
                                                None if explicit_none else kv.to(DEV))
    loss.backward()
    U64, I64 = U.double().requires_grad_(True), I.double().requires_grad_(True)
    S = U64 @ I64.t() + (0.0 if b is None else b.double()[None, :])
    rows = torch.arange(M)
    ce64 = torch.logsumexp(S.masked_fill(ref["hit"], float("-inf")), dim=1) - S[rows, rows + off]
    assert torch.equal(ce64.detach(), ref["ce"])
    dU, dI = torch.autograd.grad((ce64 * ref["coef_w"]).sum(), [U64, I64])
    want = dict(ref, dU=dU, dI=dI)
    want["scale"] = dict(ref["scale"], dU=float(ref["coef_w"].abs().max()) * float(I.abs().max()),
                         dI=float(ref["coef_w"].abs().max()) * float(U.abs().max()))
    r = H.ratios({"dU": Ud.grad, "dI": Id.grad}, want, key[4])
    r["loss"] = C.ratio(loss.detach(), ref["loss"], H.loss_tolerances(ref, key[4])["loss"])
    print(f"CE_HITS_OP loss keys={keys} term={term} " + " ".join(f"{q}={v:.3g}" for q, v in r.items()))
    assert max(r.values()) <= 1.0, r
