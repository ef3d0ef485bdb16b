"""What leaving each user's seen items out of the top-K costs (BASELINE config 5 shape on one GPU): BaselineMIPSModule.search
at C = 10 M, D = 128, B = 1024, K = 1000, E = 50 excluded keys per query, fp32 and bf16 storage.  Four numbers per dtype:
    search(K)            the search as it was (the figure to compare against)
    search(K + E)        the same search asked for E more candidates
    filter               tt_mips_exclude alone on the [B, K + E] list (kernel time from the library's profile scope, and the
                         host clock around back-to-back launches)
    search(K, exclude)   end to end: search at K + E, filter, and the 4-byte read of the short flag
The variants alternate inside each round, every round prints its own line: the spread is on the page.
    python tools/bench_mips_exclude.py [C] [B] [K] [E]"""
import ctypes as C
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import two_tower_models_amd as A
from two_tower_models_amd import _native as N
from two_tower_models_amd import ops

lib = N.load()
Cn = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
K = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
E = int(sys.argv[4]) if len(sys.argv) > 4 else 50
D, ROUNDS, REPS = 128, 3, 10
dev = "cuda:0"
g = torch.Generator(device=dev).manual_seed(0)
m = A.BaselineMIPSModule(corpus_size=8, embedding_dim=D)
m.corpus = torch.randn(Cn, D, device=dev, generator=g)
m.corpus_size = Cn
q = torch.randn(B, D, device=dev, generator=g)


def timed(fn, reps=REPS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


for name in ("fp32", "bf16"):
    if name == "bf16":
        m.use_bf16_storage()
    idx_e, sc_e = m.search(q, K + E)  # warm-up of both sizes (allocates the workspace)
    m.search(q, K)
    # half of each query's own top-E plus random rows: the exclusions bite, differently per query
    exclude = torch.cat([idx_e[:, 0:E:2], torch.randint(0, Cn, (B, E - idx_e[:, 0:E:2].shape[1]), device=dev, generator=g)], dim=1)
    got, _ = m.search(q, K, exclude)
    want, _ = ops.mips_exclude(idx_e, sc_e, K, exclude)
    gone = int((idx_e[:, :K].unsqueeze(2) == exclude[:, :E // 2].unsqueeze(1)).any(dim=2).sum()) / B
    assert torch.equal(got, want) and not (got.unsqueeze(2) == exclude.unsqueeze(1)).any()
    print(f"{name}: C={Cn} B={B} D={D} K={K} E={E}; {gone:.1f} of each query's unfiltered top-{K} are excluded on average", flush=True)
    for r in range(ROUNDS):
        t_k, _ = timed(lambda: m.search(q, K))
        t_ke, _ = timed(lambda: m.search(q, K + E))
        t_f, _ = timed(lambda: ops.mips_exclude(idx_e, sc_e, K, exclude), reps=10 * REPS)
        lib.tt_profile_filter(b"mips_exclude_kernel")
        lib.tt_profile_enable(1)  # (events around every launch: a pass of its own, after the host-clock one)
        timed(lambda: ops.mips_exclude(idx_e, sc_e, K, exclude), reps=2 * REPS)
        ms, cnt = C.c_double(0), C.c_int64(0)
        lib.tt_profile_read(b"mips_exclude_kernel", C.byref(ms), C.byref(cnt))
        lib.tt_profile_enable(0)
        lib.tt_profile_filter(None)
        t_x, _ = timed(lambda: m.search(q, K, exclude))
        k_ms = ms.value / max(cnt.value, 1)
        print(f"  round {r}: search(K) {t_k:.2f} ms | search(K+E) {t_ke:.2f} ms | filter kernel {k_ms * 1e3:.1f} us "
              f"(host clock, back to back: {t_f * 1e3:.1f} us per call) | search(K, exclude) {t_x:.2f} ms "
              f"= {100.0 * (t_x / t_k - 1.0):+.1f} % of search(K); filter kernel = {100.0 * k_ms / t_k:.2f} % of search(K)",
              flush=True)
