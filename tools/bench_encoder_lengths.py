"""Per-step GPU time of a history workload (default: the C3 shape) with and without per-sample history lengths, in ONE process
on one box: the step with lengths=None, with every length = H, and with lengths uniform in [1, H] -- alternating blocks, events
around every step, no host sync in the loop.  The run-to-run spread of the lengths=None step (its blocks' p50s) is the
yardstick for the other two.  `--out FILE` appends the summary as a markdown section (profiles/HISTORY.md).
usage: python tools/bench_encoder_lengths.py [--workload C3] [--steps 200] [--blocks 3] [--warmup 120] [--out FILE] [--kernels]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import two_tower_models_amd as A  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="C3")
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--blocks", type=int, default=3)
ap.add_argument("--warmup", type=int, default=120)
ap.add_argument("--out", default=None)
ap.add_argument("--kernels", action="store_true", help="time the attention kernels and the pool-backward tail alone instead")
args = ap.parse_args()

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
cfg = dict(bench.WORKLOADS[args.workload])
B, H = cfg["B"], cfg["H"]
batches = bench.make_batches(cfg, 16, dev)
gen = torch.Generator(device=dev).manual_seed(1234)
LENGTHS = {"none": [None] * 16,
           "full": [torch.full((B,), H, dtype=torch.int32, device=dev)] * 16,
           "uniform": [torch.randint(1, H + 1, (B,), device=dev, generator=gen, dtype=torch.int32) for _ in range(16)]}


def run(mode):
    model = bench.build_model(cfg, dev)
    opt = A.DenseExactAdam(model.parameters(), lr=1e-3, overlap_sweep="forward")
    lengths = LENGTHS[mode]

    def step(i):
        ln = lengths[i % 16]
        if ln is None:
            loss = model.train_forward(*batches[i % 16])
        else:
            loss = model.train_forward(*batches[i % 16], user_history_lengths=ln)
        opt.zero_grad()
        loss.backward()
        opt.step()

    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    evs = []
    for i in range(args.steps + 1):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        evs.append(e)
        if i < args.steps:
            step(i)
    torch.cuda.synchronize()
    ms = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps))
    del model, opt
    torch.cuda.empty_cache()
    return ms[args.steps // 2], sum(ms) / args.steps


def kernels_alone():
    """Where a difference between the three steps comes from: the attention kernels and the first layer's input-gradient +
    pool-backward tail alone at the workload's shape, 100 launches each, us per launch."""
    from two_tower_models_amd import _native as N
    from two_tower_models_amd import ops
    lib = N.load()
    D, heads = cfg["D"], 4
    qkv = torch.randn(B * H, 3 * D, device=dev) * 0.5
    ctx, lse = torch.empty(B * H, D, device=dev), torch.empty(B, heads, H, device=dev)
    d_ctx, d_qkv = torch.randn(B * H, D, device=dev), torch.empty(B * H, 3 * D, device=dev)
    w_in, dx, d_pooled = torch.randn(3 * D, D, device=dev) * 0.1, torch.empty(B * H, D, device=dev), torch.randn(B, 2 * D, device=dev)
    out = []

    def timed(name, fn):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(100):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(f"- {name}: {a.elapsed_time(b) * 10:.1f} us")
        print(out[-1], flush=True)

    timed("attention forward, no lengths", lambda: N.check(lib.tt_attn_fwd(
        qkv.data_ptr(), B, H, D, heads, ctx.data_ptr(), lse.data_ptr(), N.stream()), "tt_attn_fwd"))
    for mode in ("full", "uniform"):
        ln = LENGTHS[mode][0]
        timed(f"attention forward, lengths={mode}", lambda: N.check(lib.tt_attn_fwd_len(
            qkv.data_ptr(), B, H, D, heads, ln.data_ptr(), ctx.data_ptr(), lse.data_ptr(), N.stream()), "tt_attn_fwd_len"))
    timed("attention backward, no lengths (workgroup kernel at H <= 56, 4 heads x 32)", lambda: N.check(lib.tt_attn_bwd(
        qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), d_ctx.data_ptr(), B, H, D, heads, d_qkv.data_ptr(), N.stream()), "tt_attn_bwd"))
    for mode in ("full", "uniform"):
        ln = LENGTHS[mode][0]
        timed(f"attention backward, lengths={mode} (matrix-core kernel)", lambda: N.check(lib.tt_attn_bwd_len(
            qkv.data_ptr(), ctx.data_ptr(), lse.data_ptr(), d_ctx.data_ptr(), B, H, D, heads, ln.data_ptr(), d_qkv.data_ptr(),
            N.stream()), "tt_attn_bwd_len"))
    if lib.tt_hist_dx_pool_bwd(d_qkv.data_ptr(), w_in.data_ptr(), B, H, D, d_pooled.data_ptr(), 2 * D, dx.data_ptr(), N.stream()) == 0:
        timed("dx product with the pool backward in its epilogue, no lengths", lambda: N.check(lib.tt_hist_dx_pool_bwd(
            d_qkv.data_ptr(), w_in.data_ptr(), B, H, D, d_pooled.data_ptr(), 2 * D, dx.data_ptr(), N.stream()), "tt_hist_dx_pool_bwd"))
    ln = LENGTHS["uniform"][0]

    def pair():
        ops.gemm(N.TT_GEMM_NN, d_qkv, w_in, dx, B * H, D, 3 * D)
        N.check(lib.tt_hist_pool_bwd_len(dx.data_ptr(), B, H, D, ln.data_ptr(), d_pooled.data_ptr(), 2 * D, N.stream()),
                "tt_hist_pool_bwd_len")

    timed("dx product, then tt_hist_pool_bwd_len (with lengths)", pair)
    return out


if args.kernels:
    klines = kernels_alone()
    if args.out:
        with open(args.out, "a") as f:
            f.write(f"\nKernels alone at the {args.workload} shape (100 launches each):\n" + "\n".join(klines) + "\n")
    sys.exit(0)

p50 = {m: [] for m in LENGTHS}
for b in range(args.blocks):
    for mode in LENGTHS:
        med, mean = run(mode)
        p50[mode].append(med)
        print(f"{args.workload} block {b} lengths={mode}: p50 {med:.3f} ms, mean {mean:.3f} ms", flush=True)

best = {m: min(v) for m, v in p50.items()}
spread = max(p50["none"]) - min(p50["none"])
lines = [f"{args.workload} (B = {B}, H = {H}), {args.blocks} alternating blocks of {args.steps} steps, p50 per block in ms:"]
for m in LENGTHS:
    lines.append(f"- lengths={m}: " + " / ".join(f"{v:.3f}" for v in p50[m]) + f"  (best {best[m]:.3f})")
lines.append(f"- run-to-run spread of the lengths=None step: {spread:.3f} ms; all-H minus None (best blocks): "
             f"{best['full'] - best['none']:+.3f} ms; uniform [1, H] minus None: {best['uniform'] - best['none']:+.3f} ms")
print("\n".join(lines))
if args.out:
    with open(args.out, "a") as f:
        f.write("\n### Variable-length histories: the step with and without lengths (`tools/bench_encoder_lengths.py`)\n\n")
        f.write("\n".join(lines) + "\n")
