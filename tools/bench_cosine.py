"""Cosine logits against plain on one build: eager (dense-exact Adam, forward-announced sweep) and graphed (deferred Adam),
alternating blocks in one process; the two kernels' own times from tt_profile_read.
usage: python tools/bench_cosine.py WORKLOAD [steps per block] [blocks]      (profiles/cosine_logits_bench.txt: C2 and P, 100, 4)"""
import ctypes as C
import gc
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import two_tower_models_amd as A  # noqa: E402
from two_tower_models_amd import _native as N  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "C2"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
blocks = int(sys.argv[3]) if len(sys.argv) > 3 else 4
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
cfg = dict(bench.WORKLOADS[wl])
batches = bench.make_batches(cfg, 8, dev)
MODES = ("plain", "fixed", "learn")


def build(mode, lazy):
    model = bench.build_model(cfg, dev)
    if mode != "plain":
        model.use_cosine_logits(0.05, learnable=mode == "learn")
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep=False if lazy else "forward", lazy=lazy)
    return model, opt


def timed_block(step, first):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(steps):
        step(first + i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def report(tag, res):
    for mode in MODES:
        v = res[mode]
        print(f"{wl} {tag} {mode:5s}: ms/step per block " + " ".join(f"{x:.4f}" for x in v) + f"  | min {min(v):.4f} median {sorted(v)[len(v) // 2]:.4f}")


# ---- eager
runs = {}
for mode in MODES:
    model, opt = build(mode, lazy=False)

    def step(i, model=model, opt=opt):
        loss = model.train_forward(*batches[i % 8])
        opt.zero_grad()
        loss.backward()
        opt.step()
    for i in range(80):
        step(i)
    torch.cuda.synchronize()
    runs[mode] = (model, opt, step)
gc.collect()
gc.disable()
res = {m: [] for m in MODES}
for b in range(blocks):
    for mode in MODES:
        res[mode].append(timed_block(runs[mode][2], 80 + b * steps))
gc.enable()
report("eager", res)

# the kernels' own times (event pairs around these kernels only), learnable and fixed
lib = N.load()
for mode in ("fixed", "learn"):
    lib.tt_profile_filter(b"l2norm_fwd_kernel,l2norm_bwd_kernel,l2norm_finish_kernel")
    lib.tt_profile_enable(1)
    for i in range(50):
        runs[mode][2](i)
    torch.cuda.synchronize()
    for k in ("l2norm_fwd_kernel", "l2norm_bwd_kernel", "l2norm_finish_kernel"):
        ms, n = C.c_double(), C.c_int64()
        lib.tt_profile_read(k.encode(), C.byref(ms), C.byref(n))
        print(f"{wl} {mode} {k}: {n.value} launches, {ms.value / max(n.value, 1) * 1e3:.2f} us each")
    lib.tt_profile_enable(0)
    lib.tt_profile_filter(None)
for mode in MODES:
    runs[mode][1].flush()
del runs
gc.collect()
torch.cuda.empty_cache()

# ---- graphed (deferred Adam: the single-stream schedule a whole-step capture takes)
runs = {}
for mode in MODES:
    model, opt = build(mode, lazy=True)
    g = A.GraphedTrainStep(model, opt, batches[0], warmup=3)

    def step(i, g=g):
        g(*batches[i % 8])
    for i in range(40):
        step(i)
    torch.cuda.synchronize()
    runs[mode] = (model, opt, step, g)
gc.disable()
res = {m: [] for m in MODES}
for b in range(blocks):
    for mode in MODES:
        res[mode].append(timed_block(runs[mode][2], 40 + b * steps))
gc.enable()
report("graphed(deferred Adam)", res)
print(f"{wl} learned temperature after the run: {runs['learn'][0].logit_temperature:.5f}")
