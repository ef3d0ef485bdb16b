"""The fp32 GEMM family on MI355X (`pytest -m gpu`) against the float64 reference of tests/gemm_ref.py: every dispatch path
behind tt_gemm_f32, tt_gemm_tn_colsum_f32, tt_colsum_f32 and tt_hist_dx_pool_bwd -- the generic kernel at both tile sizes,
FULL and ragged, in NT / NN / TN, with and without split-K and every epilogue branch of the reduce; gemm_ws in every launch
variant (dp8 4 .. 32, LDS-DMA and register staging, WS_PLAIN / WS_ACC / WS_GENERIC), with one to six tiles per workgroup and
both kinds of ragged last tile, and its two-pass form; gemm_ws16 in all five shapes with one stage per workgroup, three, and
a wrapped ring; the pool form; tn_stream at M = 384 and, in ONE child process under TT_GEMM_TN_STREAM_ALL=1 (the variable is
read once per process), at M = 256 and 128; the column sums; and every fall-through between them.

Every call goes through the C ABI with explicit pointers and leading dimensions; every operand is a view into a NaN-filled
buffer and C is NaN-prefilled unless it accumulates.  Every case asserts exactly the launches its table entry names, through
the library's launch counters (tt_profile_*), that every result is finite and within E (the exact class: equal), that no
byte outside the C view changed, that tt_gemm_workspace_bytes is the restated plan's, and -- split-K -- that one byte less
is refused with TT_E_WORKSPACE before anything is written.  profiles/gemm_reference_tolerance.txt records what a run printed."""
import json
import os
import subprocess
import sys

import pytest
import torch

import gemm_ref as GR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ids(cases):
    return [GR.case_id(c) for c in cases]


def by_group(*groups):
    return [c for c in GR.DEFAULT_CASES if c.group in groups]


def run(case):
    res = GR.gpu_case(case, DEV)
    print(GR.gpu_line(res))
    GR.assert_gpu_case(case, res)


@pytest.mark.parametrize("case", by_group("g64", "g128"), ids=ids(by_group("g64", "g128")))
def test_generic_kernel_both_tiles(case):
    """64^2: ragged with scalar loads (ld % 4 != 0; a base pointer one float off), FULL, K = 0 (bias only) / 1 / 31 / 32 / 33,
    M = 1, N = 1, M = 0, N = 0, every epilogue into a strided, misaligned C with a misaligned aux.  128^2 through >= 192
    tiles: 2048 x 1536 FULL and 2053 x 1539 ragged and misaligned, NT and NN."""
    run(case)


@pytest.mark.parametrize("case", by_group("sk64", "sk128"), ids=ids(by_group("sk64", "sk128")))
def test_split_k(case):
    """Both tile sizes, NT / NN / TN and tt_gemm_tn_colsum_f32: whole splits, a shorter last split, splits at both caps
    (ktiles / 4 and 256), and bias, ReLU, ReLU-mask and accumulate in the reduce kernel."""
    run(case)


@pytest.mark.parametrize("case", by_group("ws", "wsloop", "ws2", "wsfall"), ids=ids(by_group("ws", "wsloop", "ws2", "wsfall")))
def test_weights_stationary(case):
    """gemm_ws: every (dp8, staging, store mode); 1 - 2, 2 - 3, 3 - 4 and 5 - 6 tiles per workgroup with a last tile of 5 and
    of 37 rows; K in (256, 512] as two passes (K2 = 128, 44, 1); and the three ways back to the generic kernel."""
    run(case)


@pytest.mark.parametrize("case", by_group("ws16", "ws16fall", "pool"), ids=ids(by_group("ws16", "ws16fall", "pool")))
def test_ws16_and_pool(case):
    """gemm_ws16 <1,1> <2,1> <3,1> <1,2> <1,3>, NT and NN: M = 16384, exactly three stages per workgroup, a wrapped ring with
    a 5-row last stage; a misaligned bias, ld % 4 != 0 and accumulate send the call to gemm_ws.  tt_hist_dx_pool_bwd with
    H = 1, 29 (a group straddles a stage), 32, B H = 16384 exactly, a wrapped ring, a strided d_pooled."""
    run(case)


@pytest.mark.parametrize("case", by_group("tns", "tnsfall", "tnsall"), ids=ids(by_group("tns", "tnsfall", "tnsall")))
def test_tn_stream_default_process(case):
    """M = 384: K = 8192, 8193 and 24 605 (four to five stages per workgroup, a ragged tail), with and without accumulate
    and a_colsum, strided and contiguous, two calls bit-identical; a misaligned pointer and K = 8191 fall to the tiled
    kernel -- as do, in this process, the M = 256 / 128 shapes the child process streams."""
    run(case)


@pytest.mark.parametrize("case", by_group("colsum"), ids=ids(by_group("colsum")))
def test_colsum(case):
    """tt_colsum_f32: M = 1, 63, 64, 65, more than 512 parts of 64 rows (rows_per_part doubles), N = 1, 63, 65, a strided
    and misaligned X."""
    run(case)


CHILD = r'''
import json, os, sys
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests", "golden"))
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import gemm_ref as GR
out = []
for c in GR.CHILD_CASES:
    out.append(GR.gpu_case(c, "cuda:0"))
    print("RESULT " + json.dumps(out[-1]), flush=True)
print("DONE " + str(len(out)))
'''


@pytest.fixture(scope="module")
def child_results():
    """The M = 256 / 128 streaming cases, all in one fresh process with TT_GEMM_TN_STREAM_ALL=1 in its environment."""
    env = dict(os.environ, **{GR.STREAM_ALL: "1"})
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300,
                       stdin=subprocess.DEVNULL)
    assert r.returncode == 0 and f"DONE {len(GR.CHILD_CASES)}" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    res = [json.loads(l[7:]) for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    return {x["id"]: x for x in res}


@pytest.mark.parametrize("case", GR.CHILD_CASES, ids=ids(GR.CHILD_CASES))
def test_tn_stream_all_child_process(case, child_results):
    """tn_stream_kernel<2> (M = 256) and <1> (M = 128, 768 workgroups): K = 8192, 8193 and a K that gives a workgroup four
    to five stages with a ragged tail, with and without accumulate and a_colsum, strided and contiguous, two calls
    bit-identical; a misaligned pointer and K = 8191 fall to the tiled kernel there too."""
    res = child_results[GR.case_id(case)]
    print(GR.gpu_line(res))
    GR.assert_gpu_case(case, res)


def test_entry_points_refuse_what_they_do_not_take():
    """tt_gemm_tn_colsum_f32 refuses K = 0 (tt_gemm_f32 takes it: the K = 0 cases); tt_hist_dx_pool_bwd refuses B H < 16384;
    tt_colsum_f32 a workspace one byte short -- all before anything is written."""
    from two_tower_models_amd import _native as N
    lib = N.load()
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    A, B, Cm, db, ws = nan(4, 70), nan(4, 50), nan(70, 50), nan(70), torch.empty(256, dtype=torch.uint8, device=DEV)
    with GR.Launches() as n:
        rc = lib.tt_gemm_tn_colsum_f32(70, 50, 0, A.data_ptr(), 70, B.data_ptr(), 50, Cm.data_ptr(), 50, 0, db.data_ptr(), ws.data_ptr(), 256,
                                       N.stream())
    assert rc == GR.E_BADARG and bool(torch.isnan(Cm).all()) and bool(torch.isnan(db).all()) and not any(n.values())
    dq, w, pool, dx = nan(16383, 384), nan(384, 128), nan(16383, 128), nan(16383, 128)
    with GR.Launches() as n:
        rc = lib.tt_hist_dx_pool_bwd(dq.data_ptr(), w.data_ptr(), 16383, 1, 128, pool.data_ptr(), 128, dx.data_ptr(), N.stream())
    assert rc == GR.E_UNSUPPORTED and bool(torch.isnan(dx).all()) and not any(n.values())
    X, out = torch.ones(65, 65, device=DEV), nan(65)
    need = lib.tt_colsum_workspace_bytes(65, 65)
    wsc = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = lib.tt_colsum_f32(X.data_ptr(), 65, 65, 65, out.data_ptr(), wsc.data_ptr(), need - 1, N.stream())
    torch.cuda.synchronize()
    assert rc == GR.E_WORKSPACE and bool(torch.isnan(out).all())
