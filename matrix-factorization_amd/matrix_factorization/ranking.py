"""Batched top-k and exact ranking shared by the factor models (KernelMF and
its subclasses: mf_topk / mf_rank) and the neighbourhood models (ItemItemCF /
UserUserCF: mf_cf_topk / mf_cf_rank).

The estimator supplies ``_ranking_backend()``: an object with

    topk(uid, amount, ex_ptr, ex_items) -> (item ids [n, amount], scores)
    rank(uid, tgt_ptr, tgt_items, ex_ptr, ex_items) -> (ranks, n_candidates)

over internal ids (-1 = unknown user), exclusions and targets as CSR lists per
position of ``uid``; everything else here is id mapping and frame assembly.
"""

from __future__ import annotations

from typing import Union

import numpy as np
import pandas as pd

from .utils import ranking_metrics_from_ranks


class RankingMixin:
    """``recommend_batch``, ``rank_items`` and ``evaluate_topk`` for a
    RecommenderBase with ``_ranking_backend()``."""

    def _ranking_backend(self):
        raise NotImplementedError

    def _exclusion_csr(self, users: list, exclude_known):
        """``exclude_known`` (DataFrame[user_id, item_id], or None) as a CSR
        list of internal item ids per position of ``users``: (ptr, items), or
        (None, None) without exclusions.  Pairs with an unknown item or a user
        outside ``users`` are dropped."""
        ex_ptr = ex_items = None
        if exclude_known is not None and len(exclude_known):
            pos = pd.Series(np.arange(len(users)), index=pd.Index(users, dtype=object))
            pos = pos[~pos.index.duplicated(keep="first")]
            q = exclude_known["user_id"].map(pos)
            it = self._remap(exclude_known["item_id"], self.item_id_map)
            ok = q.notna().to_numpy() & (it >= 0)
            qv = q[ok].to_numpy().astype(np.int64)
            iv = it[ok].astype(np.int32)
            # duplicate users in `users` share the first position's list
            first = pos.reindex(pd.Index(users, dtype=object)).to_numpy().astype(np.int64)
            order = np.argsort(qv, kind="stable")
            qv, iv = qv[order], iv[order]
            cnt = np.bincount(qv, minlength=len(users)).astype(np.int64)
            start = np.concatenate([[0], np.cumsum(cnt)])
            per = [iv[start[f]:start[f + 1]] for f in first]
            ex_ptr = np.concatenate([[0], np.cumsum([len(x) for x in per])]).astype(np.int64)
            ex_items = (np.concatenate(per) if len(per) else np.zeros(0)).astype(np.int32)
        return ex_ptr, ex_items

    def recommend_batch(self, users, amount: int = 10, exclude_known=None,
                        bound_ratings: bool = True) -> pd.DataFrame:
        """Top ``amount`` items for many users on the GPU (mf_topk; mf_cf_topk
        for the neighbourhood models) -- the batched form of ``recommend``
        (recommender_base.py:214-271).

        ``exclude_known``: optional DataFrame[user_id, item_id] of pairs to
        skip (recommend's ``items_known`` per user), passed to the device as
        a CSR list.  Scores are recommend()'s (the unbounded prediction);
        equal scores rank the lower internal item id first -- the order a
        stable sort gives; the reference's ``sort_values`` default quicksort
        leaves tie order unspecified.  Users go in chunks (engine
        ``topk_ws_budget``).  Returns DataFrame[user_id, item_id,
        rating_pred] ordered by user then rank."""
        users = list(users)
        uid = self._remap(pd.Series(users, dtype=object), self.user_id_map)
        ex_ptr, ex_items = self._exclusion_csr(users, exclude_known)
        amount = min(amount, self.n_items)
        items, scores = self._ranking_backend().topk(uid, amount, ex_ptr, ex_items)
        inv = np.asarray(list(self.item_id_map.keys()), dtype=object)
        valid = items >= 0
        out = pd.DataFrame({
            "user_id": np.repeat(np.asarray(users, dtype=object), valid.sum(axis=1)),
            "item_id": inv[items[valid]],
            "rating_pred": scores[valid],
        })
        if bound_ratings:
            out["rating_pred"] = out["rating_pred"].clip(lower=self.min_rating,
                                                         upper=self.max_rating)
        return out

    def _rank_pairs(self, X: pd.DataFrame, exclude_known=None):
        """Ranks of X's (user_id, item_id) rows on the GPU (mf_rank /
        mf_cf_rank): per row the code of its user among X's distinct users and
        its rank (-1: unknown user or item, or an excluded pair), per distinct
        user the label and the candidate count."""
        ucode, ulabel = pd.factorize(X["user_id"].astype(object))
        users = list(ulabel)
        uid = self._remap(pd.Series(users, dtype=object), self.user_id_map)
        iid = self._remap(X["item_id"], self.item_id_map)
        ex_ptr, ex_items = self._exclusion_csr(users, exclude_known)
        # targets: the rows of known users, grouped by user (unknown items stay -1)
        rows = np.flatnonzero(uid[ucode] >= 0) if len(ucode) else np.zeros(0, np.int64)
        rows = rows[np.argsort(ucode[rows], kind="stable")]
        ptr = np.zeros(len(users) + 1, np.int64)
        np.cumsum(np.bincount(ucode[rows], minlength=len(users)), out=ptr[1:])
        r, cand = self._ranking_backend().rank(uid, ptr, iid[rows], ex_ptr, ex_items)
        rank = np.full(len(ucode), -1, np.int32)
        rank[rows] = r
        return ucode, rank, ulabel, cand

    def rank_items(self, X: pd.DataFrame, exclude_known=None) -> pd.DataFrame:
        """Exact rank of each (user_id, item_id) row of X among the user's
        candidate items: the number of candidates ``recommend`` would list
        before it (0 = first), without building any list and with no cap.

        Candidates are all known items minus the user's ``exclude_known``
        pairs (as in ``recommend_batch``); scores and tie order are
        ``recommend_batch``'s.  Pairs with an unknown user or item, and pairs
        that are themselves excluded, get rank -1.  Returns
        DataFrame[user_id, item_id, rank, n_candidates] in X's row order."""
        ucode, rank, _, cand = self._rank_pairs(X, exclude_known)
        return pd.DataFrame({
            "user_id": X["user_id"].to_numpy(),
            "item_id": X["item_id"].to_numpy(),
            "rank": rank,
            "n_candidates": cand[ucode] if len(ucode) else np.zeros(0, np.int32),
        })

    def evaluate_topk(self, X: pd.DataFrame, k: Union[int, list] = 10, exclude_known=None,
                      ndcg_ideal: str = "hits"):
        """Ranking quality on held-out pairs X (DataFrame[user_id, item_id]):
        ``rank_items`` followed by ``utils.ranking_metrics_from_ranks`` --
        precision, recall, NDCG, MAP and MRR at ``k``, and AUC, averaged over
        the users with at least one rankable held-out item.  Pass the training
        pairs as ``exclude_known`` (evaluate.py's ``items_known``).  ``k`` may
        be a list: one GPU pass, a dict of results keyed by k."""
        X = X[["user_id", "item_id"]].drop_duplicates()
        ucode, rank, ulabel, cand = self._rank_pairs(X, exclude_known)
        order = np.argsort(ucode, kind="stable")
        ptr = np.zeros(len(ulabel) + 1, np.int64)
        np.cumsum(np.bincount(ucode, minlength=len(ulabel)), out=ptr[1:])
        one = lambda kk: ranking_metrics_from_ranks(  # noqa: E731
            rank[order], ptr, cand, np.diff(ptr), kk, ndcg_ideal=ndcg_ideal)
        if isinstance(k, (int, np.integer)):
            return one(int(k))
        return {int(kk): one(int(kk)) for kk in k}
