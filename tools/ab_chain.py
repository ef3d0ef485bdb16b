"""A/B of the chained dense-exact step on ONE box, one process, ONE model and optimiser (one table arena: no placement
difference between the modes): alternating blocks of steps under
    old          TT_ADAM_CHAIN=0                        rows parked, sweep -> finish -> dense -> begin -> sweep in series
    chain        TT_ADAM_CHAIN=1 TT_SWEEP_ALONE_WGS=0   rows marked, the next sweep follows on the sweep's stream
    chain+thin   TT_ADAM_CHAIN=1                        ... and the sweep thins itself once the main stream has run dry
(events around every step, no host sync inside a block; any schedule may follow any other).  Prints every block's p50 and
mean, then per mode the p50s' median and spread, and the margin the issue of this tool asks a difference to beat: three
times the largest spread of block p50s within one mode.
usage: python tools/ab_chain.py [workload] [steps per block] [rounds] [alone workgroups for chain+thin]   e.g.  P 200 3"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import two_tower_models_amd as A  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "P"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
alone = sys.argv[4] if len(sys.argv) > 4 else None
MODES = {"old": {"TT_ADAM_CHAIN": "0"}, "chain": {"TT_ADAM_CHAIN": "1", "TT_SWEEP_ALONE_WGS": "0"},
         "chain+thin": {"TT_ADAM_CHAIN": "1", "TT_SWEEP_ALONE_WGS": alone}}
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
cfg = dict(bench.WORKLOADS[wl])
batches = bench.make_batches(cfg, 16, dev)
model = bench.build_model(cfg, dev)
opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep="forward")


def step(i):
    loss = model.train_forward(*batches[i % 16])
    opt.zero_grad()
    loss.backward()
    opt.step()


def block(mode):
    for k in ("TT_ADAM_CHAIN", "TT_SWEEP_ALONE_WGS"):
        os.environ.pop(k, None)
    os.environ.update({k: v for k, v in MODES[mode].items() if v is not None})
    for i in range(20):  # the first steps of a block overlap the previous mode's tail
        step(i)
    torch.cuda.synchronize()
    evs = []
    for i in range(steps):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        evs.append(e)
        step(i)
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    evs.append(e)
    torch.cuda.synchronize()
    ms = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(steps))
    return ms[steps // 2], sum(ms) / steps


# spin up until two consecutive blocks of steps agree to 0.3 % (at most 12): the first steps of a process on an idle box run at
# cold clocks, and a slow first block would set the margin below
prev = None
for _ in range(12):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if prev is not None and abs(dt - prev) <= 0.003 * prev:
        break
    prev = dt
p50s = {m: [] for m in MODES}
for r in range(rounds):
    for mode in MODES:
        p50, mean = block(mode)
        p50s[mode].append(p50)
        print(f"{wl} round {r} {mode:>10}: p50 {p50:.3f} ms, mean {mean:.3f} ms   [sweep: {opt.sweep_level_note()}]", flush=True)
spread = max(max(v) - min(v) for v in p50s.values())
med = {m: sorted(v)[len(v) // 2] for m, v in p50s.items()}
for m, v in p50s.items():
    print(f"{wl} {m:>10}: block p50s {[round(x, 3) for x in v]}  median {med[m]:.3f}  spread {max(v) - min(v):.3f}")
print(f"{wl} margin = 3 x largest spread = {3 * spread:.3f} ms;  old - chain = {med['old'] - med['chain']:.3f} ms;  "
      f"chain - chain+thin = {med['chain'] - med['chain+thin']:.3f} ms")
print(f"arena: {getattr(opt, 'arena_note', None)}")
