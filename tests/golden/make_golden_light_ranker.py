#!/usr/bin/env python
"""Golden vectors of TwoTowerPlusLightRanker (tests/golden/g9_light_ranker_*.npz), produced by the REFERENCE class
(ref:src/two_tower_plus_light_ranker.py) with its three upstream bugs fixed by shims, not copies:

  * a subclass overrides only ``compute_user_embedding``: it passes ``user_history`` to ``process_user_features`` and
    views the ranker embeddings as ``[B, NU, -1]`` (upstream reads ``self.item_id_embedding_dim``, which no class sets);
  * ``torch.cat`` is patched around ``train_forward`` so that ``dim=2`` over 2-D tensors means the last axis.

Run in the build container only, next to make_golden.py (same reference checkout, same helpers):

    python tests/golden/make_golden_light_ranker.py

No committed file may exceed 1 MiB: a case whose arrays do not fit one file continues in ``<name>.p1.npz``,
``<name>.p2.npz``, ... (tests/test_gpu_light_ranker.py reads them back together).  The d128 case does not store its
initial parameters: they are the seeded default init (``torch.manual_seed(0)``, the MIPS module's random corpus drawn
first, as here), which the test rebuilds and checks against the per-parameter sums recorded below.
"""
from __future__ import annotations

import os
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the reference on sys.path)
import fixture_gen as fg  # noqa: E402
from src.baseline_mips_module import BaselineMIPSModule  # noqa: E402
from src.two_tower_plus_light_ranker import TwoTowerPlusLightRanker  # noqa: E402

PART_BYTES = 900_000  # raw bytes per file: random fp32 compresses by a few percent only


class FixedLightRanker(TwoTowerPlusLightRanker):
    def compute_user_embedding(self, user_id, user_features, user_history):
        x = self.process_user_features(user_id=user_id, user_features=user_features, user_history=user_history)
        r = self.ranker_user_tower(x)
        return self.user_tower_arch(x), r.view(r.size(0), self.num_ranker_user_embeddings, -1)


_cat = torch.cat


def _cat_last_axis(tensors, dim=0, **kw):
    if dim == 2 and all(x.dim() == 2 for x in tensors):
        dim = 1
    return _cat(tensors, dim=dim, **kw)


def train_forward(model, batch):
    with mock.patch.object(torch, "cat", _cat_last_axis):
        return model.train_forward(*batch)


def save_parts(name, arrays):
    parts, cur, size = [], {}, 0
    for k, v in arrays.items():
        if cur and size + v.nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    parts.append(cur)
    for i, p in enumerate(parts):
        mg.save(name if i == 0 else f"{name}.p{i}", **p)


def light_ranker_case(name, *, n_users, du, iu, n_items, di, ii, T, uvw, B, H, NU, NI, K, C, store_init):
    torch.manual_seed(0)
    mips = BaselineMIPSModule(corpus_size=C, embedding_dim=di)
    mips.corpus = mg.t(fg.bf16_round(fg.gaussianish((C, di), 903)))
    model = FixedLightRanker(num_items=K, num_mips_items=NI, num_ranker_user_embeddings=NU, user_id_hash_size=n_users,
                             user_id_embedding_dim=du, user_features_size=iu, user_history_seqlen=H,
                             item_id_hash_size=n_items, item_id_embedding_dim=di, item_features_size=ii,
                             user_value_weights=uvw, mips_module=mips)
    head = {"cfg": np.array([n_users, du, iu, n_items, di, ii, T, B, H, NU, NI, K, C], dtype=np.int64),
            "uvw": np.array(uvw, dtype=np.float32)}
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}  # the init (Adam moves the live tensors)
    head["state_keys"] = np.array(list(sd), dtype="U")
    head["state_shapes"] = np.array([",".join(str(n) for n in v.shape) for v in sd.values()], dtype="U")
    head["init_sum"] = np.array([v.double().sum().item() for v in sd.values()], dtype=np.float64)
    head["init_abs"] = np.array([v.double().abs().sum().item() for v in sd.values()], dtype=np.float64)
    b = mg.make_batch(B, n_users, n_items, iu, ii, H, T, seed=9100)
    head.update({"in." + k: v for k, v in b.items()})
    bt = mg.batch_tensors(b)
    nuv = bt[6] @ model.user_value_weights
    assert float(nuv.max()) != 1.0  # a head that divides by the batch maximum must not pass
    with torch.no_grad():
        top = model(bt[0], bt[1], bt[2])
        u, R = model.compute_user_embedding(bt[0], bt[1], bt[2])
    head["top_items"] = top.numpy()
    loss = train_forward(model, bt)
    model.zero_grad()
    loss.backward()
    head["loss"] = np.array(loss.item(), dtype=np.float64)
    # two steps of the reference train loop body (ref:train/train.py:112-132) with torch.optim.Adam(lr=1e-3)
    grads = mg.grads_np(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    traj = []
    for s in range(2):
        bs = mg.make_batch(B, n_users, n_items, iu, ii, H, T, seed=9200 + 100 * s)
        head.update({f"step{s}.in." + k: v for k, v in bs.items()})
        ls = train_forward(model, mg.batch_tensors(bs))
        opt.zero_grad()
        ls.backward()
        opt.step()
        traj.append(ls.item())
    head["adam_losses"] = np.array(traj, dtype=np.float64)
    arrays = dict(head)
    if store_init:
        arrays.update({"p." + k: v.numpy() for k, v in sd.items()})
    arrays["user_emb"] = u.numpy()
    arrays["ranker_emb"] = R.numpy()
    arrays.update(grads)
    arrays.update(mg.sd_np(model, prefix="after."))
    save_parts(name, arrays)


if __name__ == "__main__":
    light_ranker_case("g9_light_ranker_tiny", n_users=30, du=6, iu=5, n_items=50, di=8, ii=4, T=2, uvw=[0.6, 0.9], B=13,
                      H=5, NU=3, NI=10, K=4, C=64, store_init=True)
    light_ranker_case("g9_light_ranker_d128", n_users=64, du=32, iu=8, n_items=256, di=128, ii=8, T=3,
                      uvw=[0.7, 0.5, 0.3], B=256, H=8, NU=4, NI=200, K=20, C=4096, store_init=False)
