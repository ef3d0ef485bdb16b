"""Sampling probabilities for the log-Q correction of the in-batch softmax
(``TwoTowerBaseRetrieval.train_forward(item_log_q=..., negative_log_q=...)``): plain torch on
device tensors, natural-log units.

In-batch negatives are drawn with probability proportional to item popularity (the unigram
distribution of the training stream); uniform extra negatives mix a flat term in (Yang et al.
2020, "Mixed negative sampling").  ``log q_j`` of a candidate is what the logit of its column is
corrected by (Yi et al. 2019, "Sampling-bias-corrected neural modeling", eq. 3).
"""
from __future__ import annotations

import torch


def log_q_from_counts(counts: torch.Tensor) -> torch.Tensor:
    """[N_items] occurrence counts -> float32 [N_items] table ``log(max(counts, 1) / counts.sum())``.
    An item that never occurred counts as one occurrence (a finite correction for a uniform negative)."""
    c = counts.to(torch.float32)
    return torch.log(torch.clamp(c, min=1.0) / c.sum())


def mixture_log_q(log_p_table: torch.Tensor, ids: torch.Tensor, n_inbatch: int, n_uniform: int, num_items: int) -> torch.Tensor:
    """log q of the items ``ids`` under the proposal of a candidate set that mixes ``n_inbatch`` unigram draws
    (``log_p_table``: their log probabilities per item id) with ``n_uniform`` uniform draws over ``num_items`` items:

        log((n_inbatch * p_j + n_uniform / num_items) / (n_inbatch + n_uniform))

    ``n_uniform = 0`` gives back ``log_p_table[ids]``."""
    log_p = log_p_table[ids].to(torch.float32)
    if n_uniform == 0:
        return log_p
    total = float(n_inbatch + n_uniform)
    return torch.log(torch.exp(log_p) * (n_inbatch / total) + n_uniform / (total * num_items))
