"""TwoTowerPlusLightRanker on MI355X (mirror of ref:src/two_tower_plus_light_ranker.py:13-340).

Retrieval by MIPS, then a small pointwise ranker: target-aware attention of each candidate over ``NU`` extra user
embeddings, ``T`` task logits combined with ``user_value_weights``, the best ``num_items`` of the ``num_mips_items``
candidates returned.  Training adds the ranker's BCE on the impressed item to the in-batch softmax loss.

Hot paths: the ranker's training head (``ops.LightRankerHead``: two launches per direction) and the rerank that follows
the search (``ops.light_ranker_rerank``: one launch from the candidate ids to the item ids, candidate rows read from the
corpus by index -- the [B, NI, DI] gather and the [B, NI, 2 DI + NU + 1] concat of upstream are never formed).  Sizes
outside the kernels' range (NU > 32, T > 16, DI % 4 != 0, DI > 256) take the reference's own tensor expressions on the
GPU.  There is no CPU path.

Differences, all deliberate:
  * upstream's ``compute_user_embedding`` calls ``process_user_features`` without ``user_history`` (a TypeError in both
    ``forward`` and ``train_forward``): the history is passed;
  * upstream views the ranker embeddings with ``self.item_id_embedding_dim``, which no class sets (an AttributeError):
    the view is [B, NU, DI] from the known sizes;
  * upstream's ``train_forward`` concatenates 2-D tensors with ``torch.cat(..., dim=2)`` (an IndexError): the last
    axis, as in ``forward``;
  * the MIPS term is ``mean(row_ce * clamp(net_user_value, 1e-6)) + aux`` exactly as upstream's ``train_forward`` writes
    it -- WITHOUT the division by the batch maximum that the base ``compute_training_loss`` applies;
  * ``forward`` orders ties by the lower candidate position (the MIPS rank) -- ``torch.topk`` leaves them arbitrary --
    and raises ``RuntimeError("selected index k out of range")`` when ``num_items > num_mips_items``, as ``torch.topk``;
  * row-sharded models (``parallel``) are not supported: ``train_forward`` and ``forward`` raise NotImplementedError.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as N
from . import ops
from .baseline_mips_module import BaselineMIPSModule
from .two_tower_base_retrieval import takes_history_lengths
from .two_tower_with_debiasing import TwoTowerWithDebiasing

_WEIGHT_MIN = 1.0e-6  # ref :282-284
_RERANK_MAX_CANDIDATES = 4096  # tt_light_ranker_rerank's NI limit


class TwoTowerPlusLightRanker(TwoTowerWithDebiasing):
    # constructor keywords = ref :24-38, in the reference's order
    def __init__(self, num_items: int, num_mips_items: int, num_ranker_user_embeddings: int, user_id_hash_size: int,
                 user_id_embedding_dim: int, user_features_size: int, user_history_seqlen: int, item_id_hash_size: int,
                 item_id_embedding_dim: int, item_features_size: int, user_value_weights: List[float],
                 mips_module: nn.Module) -> None:
        super().__init__(num_items=num_items, user_id_hash_size=user_id_hash_size,
                         user_id_embedding_dim=user_id_embedding_dim, user_features_size=user_features_size,
                         user_history_seqlen=user_history_seqlen, item_id_hash_size=item_id_hash_size,
                         item_id_embedding_dim=item_id_embedding_dim, item_features_size=item_features_size,
                         user_value_weights=user_value_weights, mips_module=mips_module)
        self.num_mips_items: int = num_mips_items
        self.num_ranker_user_embeddings: int = num_ranker_user_embeddings
        DU, DI, NU = user_id_embedding_dim, item_id_embedding_dim, num_ranker_user_embeddings
        # creation order == reference order (:79-88) so a seeded init is bit-identical
        self.ranker_user_tower = nn.Linear(2 * DU + 2 * DI, NU * DI)  # user tower input -> [B, NU, DI]
        self.light_ranker = nn.Linear(2 * DI + NU + 1, len(user_value_weights))  # [v | t | s | m] -> T logits

    def _check_unsharded(self, what: str) -> None:
        if self._sharded():
            raise NotImplementedError(f"TwoTowerPlusLightRanker.{what}: row-sharded models are not supported")

    def _check_cosine_supported(self) -> None:
        # the ranker's feature m = <u, v> and the MIPS scores it reranks would each need a decision of their own
        raise NotImplementedError("TwoTowerPlusLightRanker: cosine logits (use_cosine_logits) are not supported")

    def _fused_sizes(self) -> bool:
        return ops.light_ranker_supported(self.num_ranker_user_embeddings, self.item_tower_arch.out_features,
                                          self.light_ranker.out_features)

    def compute_user_embedding(self, user_id: torch.Tensor, user_features: torch.Tensor,
                               user_history: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(MIPS query [B, DI], light ranker user embeddings [B, NU, DI]) from ONE user tower input
        [B, 2 DU + 2 DI] (ref :90-129, with the history passed and the view's width known)."""
        if user_id.is_cuda:
            N.oob.poll(user_id.device)  # surfaces an out-of-range id seen by an earlier launch
        x = self.process_user_features(user_id=user_id, user_features=user_features, user_history=user_history)
        u = ops.Linear.apply(x, self.user_tower_arch.weight, self.user_tower_arch.bias)  # [B, DI]
        r = ops.Linear.apply(x, self.ranker_user_tower.weight, self.ranker_user_tower.bias)  # [B, NU * DI]
        return u, r.view(r.shape[0], self.num_ranker_user_embeddings, u.shape[1])

    # ------------------------------------------------------------------ inference
    def _history_lengths(self, user_history_lengths):
        """The keyword ``user_history_lengths`` of forward / train_forward is refused: this model's two user-side outputs have
        no masked reference to be checked against.  (Refused before anything of the model is used.)"""
        raise NotImplementedError("TwoTowerPlusLightRanker: user_history_lengths is not implemented for the light-ranker model")

    @takes_history_lengths
    def forward(self, user_id: torch.Tensor, user_features: torch.Tensor, user_history: torch.Tensor, *,
                exclude_history: bool = False, exclude_item_id: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Top ``num_items`` of the ``num_mips_items`` MIPS candidates by the light ranker's net value, [B, num_items]
        int64 item ids (ref :131-209).  ``exclude_history`` / ``exclude_item_id``: as TwoTowerBaseRetrieval.forward -- the
        ``num_mips_items`` candidates handed to the rerank already leave those items out; the rerank itself is unchanged."""
        self._check_unsharded("forward")
        if self.num_items > self.num_mips_items:
            raise RuntimeError("selected index k out of range")  # torch.topk's message (ref :202-204)
        exclude = self._exclusion_list(user_history, exclude_history, exclude_item_id)
        with torch.no_grad():
            u, R = self.compute_user_embedding(user_id, user_features, user_history)
            mips = self.mips_module
            corpus = rows = None
            if type(mips).forward is BaselineMIPSModule.forward and not mips.is_sharded():
                # this package's module: ids and scores only, the rerank reads the rows from the corpus itself
                if exclude is None:
                    idx, scores = mips.search(u, self.num_mips_items)
                else:
                    idx, scores = mips.search(u, self.num_mips_items, exclude)
                corpus = mips.corpus
            elif exclude is not None:  # (this package's module with a row-sharded corpus: it filters before it fetches)
                idx, scores, rows = mips(query_embedding=u, num_items=self.num_mips_items, exclude=exclude)
            else:  # any other mips_module: the reference's call, keyword for keyword (ref :153-155)
                idx, scores, rows = mips(query_embedding=u, num_items=self.num_mips_items)
            lin = self.light_ranker
            if u.is_cuda and self._fused_sizes() and self.num_mips_items <= _RERANK_MAX_CANDIDATES:
                top = ops.light_ranker_rerank(R, lin.weight, lin.bias, self.user_value_weights, idx, scores,
                                              self.num_items, corpus=corpus, rows=rows)
            else:
                if rows is None:
                    rows = ops.gather_corpus_rows(corpus, idx)
                top = self._rerank_reference(R, rows.to(torch.float32), scores, idx)
        N.oob.poll(u.device, blocking=True)
        return top

    def _rerank_reference(self, R, rows, scores, idx) -> torch.Tensor:
        """ref :165-207 as written (sizes the kernel does not take); ties by the lower candidate position."""
        s = torch.bmm(R, rows.permute(0, 2, 1)).permute(0, 2, 1)  # [B, NI, NU]
        p = F.softmax(s, dim=2)
        t = torch.bmm(p, R)  # [B, NI, DI]
        z = torch.cat([rows, t, s, scores.unsqueeze(2)], dim=2)
        value = torch.sum(self.light_ranker(z) * self.user_value_weights, dim=2)  # [B, NI]
        order = torch.sort(value, dim=1, descending=True, stable=True).indices[:, :self.num_items]
        return torch.gather(idx, dim=1, index=order)

    # ------------------------------------------------------------------ training
    @takes_history_lengths
    def train_forward(self, user_id: torch.Tensor, user_features: torch.Tensor, user_history: torch.Tensor,
                      item_id: torch.Tensor, item_features: torch.Tensor, position: torch.Tensor,
                      labels: torch.Tensor, item_log_q=None, negative_item_id=None, negative_item_features=None,
                      negative_log_q=None, *, remove_accidental_hits: bool = False) -> torch.Tensor:
        """MIPS term + light ranker term (ref :211-340).  No host synchronisation: GraphedTrainStep captures it.
        The log-Q / extra-negative keywords of TwoTowerBaseRetrieval.train_forward are refused: the ranker term scores
        the impressed item only and has no corrected form here.  ``user_history_lengths`` is refused as well
        (`_history_lengths`).  ``remove_accidental_hits``: as in TwoTowerBaseRetrieval.train_forward, on the MIPS term."""
        if any(t is not None for t in (item_log_q, negative_item_id, negative_item_features, negative_log_q)):
            raise NotImplementedError("TwoTowerPlusLightRanker.train_forward: item_log_q / negative_* are not implemented "
                                      "for the light-ranker model")
        self._check_unsharded("train_forward")
        if remove_accidental_hits and self.item_id_embedding_arch.num_embeddings > 2 ** 31:
            raise ValueError("train_forward: remove_accidental_hits compares item ids as 32-bit values; "
                             f"item_id_hash_size = {self.item_id_embedding_arch.num_embeddings} > 2 ** 31")
        self._announce_lookups(user_id, user_history, item_id)
        u, R = self.compute_user_embedding(user_id, user_features, user_history)  # [B, DI], [B, NU, DI]
        v = self.compute_item_embeddings(item_id, item_features)  # [B, DI]
        return self._mips_loss(u, v, position, labels, item_id if remove_accidental_hits else None) + self._ranker_loss(u, R, v, labels)

    def _mips_loss(self, u, v, position, labels, item_key=None) -> torch.Tensor:
        """ref :256-296: in-batch softmax CE per row, weighted by the (debiased) net user value clamped at 1e-6 -- no
        division by the batch maximum here (module docstring)."""
        # [B], the [B, B] logits never written; item_key: accidental hits masked
        row_ce = ops.InBatchSoftmaxCE.apply(u, v, 0, None, None, item_key)
        net_user_value = torch.matmul(labels, self.user_value_weights)  # [B]
        net_user_value, additional_loss = self.debias_net_user_value(net_user_value, position, u)
        net_user_value = torch.clamp(net_user_value, min=_WEIGHT_MIN)
        return torch.mean(row_ce * net_user_value) + additional_loss

    def _ranker_loss(self, u, R, v, labels) -> torch.Tensor:
        """ref :298-339: BCE of the light ranker's task logits on the impressed item."""
        lin = self.light_ranker
        if (u.is_cuda and labels.dtype == torch.float32 and labels.dim() == 2 and labels.shape == (u.shape[0], lin.out_features)
                and self._fused_sizes()):
            return ops.LightRankerHead.apply(R, u, v, labels, lin.weight, lin.bias)
        s = torch.bmm(R, v.unsqueeze(2)).squeeze(2)  # [B, NU]
        p = F.softmax(s, dim=1)
        t = torch.bmm(p.unsqueeze(1), R).squeeze(1)  # [B, DI]
        m = torch.sum(u * v, dim=1)  # diag(u v^T)
        z = torch.cat([v, t, s, m.unsqueeze(1)], dim=-1)  # [B, 2 DI + NU + 1]
        return F.binary_cross_entropy_with_logits(lin(z), labels)
