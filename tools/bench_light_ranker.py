"""TwoTowerPlusLightRanker measurements (bench.py is not involved):

  1. rerank at B = 1024, NI = 1000, num_items = 100, NU = 4, T = 4, DI = 128 over a 10 M-row corpus, fp32 and bf16:
     ops.light_ranker_rerank (rows read from the corpus by index) as gathered bytes / time (B * NI * DI * bytes per
     element), next to the torch composition of the same forward on the GPU (gather [B, NI, DI], bmm, softmax, bmm, cat,
     Linear, value weights, topk, gather) and next to the MIPS search it follows (ops.mips_topk, K = NI);
  2. the light-ranker train step (forward, backward, DenseExactAdam step) at the P shape (B = 8192, 10 M items, 1 M users,
     D = 128, H = 50) against TwoTowerWithDebiasing on the same batch.

    python tools/bench_light_ranker.py [--json OUT] [--skip-train]

Times are CUDA-event medians of 5 blocks of `reps` calls each, after warm-up calls."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import two_tower_models_amd as A  # noqa: E402
from two_tower_models_amd import ops  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps, warmup=3, blocks=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) / reps)
    return sorted(per)[len(per) // 2]


def torch_composition(R, corpus, idx, scores, W, b, uvw, k):
    rows = corpus[idx].float()  # [B, NI, DI]
    s = torch.bmm(R, rows.transpose(1, 2)).transpose(1, 2)
    t = torch.bmm(torch.softmax(s, dim=2), R)
    z = torch.cat([rows, t, s, scores.unsqueeze(2)], dim=2)
    val = torch.sum(torch.nn.functional.linear(z, W, b) * uvw, dim=2)
    return torch.gather(idx, 1, torch.topk(val, k, dim=1).indices)


def bench_rerank(out):
    B, NI, K, NU, T, DI, C = 1024, 1000, 100, 4, 4, 128, 10_000_000
    g = torch.Generator(device=DEV).manual_seed(0)
    corpus32 = torch.randn(C, DI, device=DEV, generator=g)
    q = torch.randn(B, DI, device=DEV, generator=g)
    R = torch.randn(B, NU, DI, device=DEV, generator=g) * 0.1
    W = torch.randn(T, 2 * DI + NU + 1, device=DEV, generator=g) * 0.05
    b = torch.randn(T, device=DEV, generator=g)
    uvw = torch.rand(T, device=DEV, generator=g)
    for name in ("fp32", "bf16"):
        corpus = corpus32 if name == "fp32" else corpus32.to(torch.bfloat16)
        if name == "bf16":
            del corpus32
        idx, scores = ops.mips_topk(q, corpus, NI)
        t_mips = timed(lambda: ops.mips_topk(q, corpus, NI), reps=3)
        t_rr = timed(lambda: ops.light_ranker_rerank(R, W, b, uvw, idx, scores, K, corpus=corpus), reps=50)
        t_torch = timed(lambda: torch_composition(R, corpus, idx, scores, W, b, uvw, K), reps=10)
        nbytes = B * NI * DI * corpus.element_size()
        rec = dict(rerank_ms=t_rr, rerank_gathered_GBps=nbytes / t_rr / 1e6, gathered_GB=nbytes / 1e9,
                   torch_composition_ms=t_torch, mips_search_ms=t_mips)
        out[f"rerank_{name}"] = rec
        print(f"rerank {name}: {t_rr:.4f} ms ({rec['rerank_gathered_GBps']:.0f} GB/s of {nbytes / 1e9:.2f} GB rows) | "
              f"torch composition {t_torch:.3f} ms | MIPS search (K={NI}) {t_mips:.3f} ms", flush=True)
        del idx, scores
    del corpus


def bench_train(out):
    B, n_users, n_items, D, F, H, T, NU = 8192, 1_000_000, 10_000_000, 128, 8, 50, 4, 4
    g = torch.Generator().manual_seed(1)
    batch = [torch.randint(0, n_users, (B,), generator=g), torch.randn(B, F, generator=g),
             torch.randint(0, n_items, (B, H), generator=g), torch.randint(0, n_items, (B,), generator=g),
             torch.randn(B, F, generator=g), torch.randint(0, 10, (B,), generator=g),
             (torch.rand(B, T, generator=g) > 0.5).float()]
    batch = [x.to(DEV) for x in batch]
    uvw = [0.4, 0.3, 0.2, 0.1]
    common = dict(num_items=100, user_id_hash_size=n_users, user_id_embedding_dim=D, user_features_size=F,
                  user_history_seqlen=H, item_id_hash_size=n_items, item_id_embedding_dim=D, item_features_size=F,
                  user_value_weights=uvw)
    for name in ("TwoTowerWithDebiasing", "TwoTowerPlusLightRanker"):
        torch.manual_seed(0)
        with torch.device(DEV):
            mips = A.BaselineMIPSModule(corpus_size=1024, embedding_dim=D)
            if name == "TwoTowerWithDebiasing":
                model = A.TwoTowerWithDebiasing(mips_module=mips, **common)
            else:
                model = A.TwoTowerPlusLightRanker(num_mips_items=1000, num_ranker_user_embeddings=NU, mips_module=mips,
                                                  **common)
        model = model.to(DEV)
        opt = A.DenseExactAdam(model.parameters(), lr=1e-3)

        def step():
            loss = model.train_forward(*batch)
            opt.zero_grad()
            loss.backward()
            opt.step()

        out[f"train_P_{name}_ms"] = t = timed(step, reps=5, warmup=3)
        print(f"train step P (B={B}, N_i={n_items}, H={H}): {name} {t:.3f} ms", flush=True)
        del model, opt, mips
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--skip-train", action="store_true")
    a = ap.parse_args()
    out = {}
    bench_rerank(out)
    torch.cuda.empty_cache()
    if not a.skip_train:
        bench_train(out)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
