"""train_update_test_split (utils.py:8-72 of the reference) and the host side
of ranking evaluation (ranking_metrics_from_ranks).

Host-side data preparation for update_users experiments; exported because
examples/example.py imports it.  Draws from NumPy's global RandomState in the
reference's order (choice -> sample -> sklearn's train_test_split), so a seeded
run splits identically.
"""

from __future__ import annotations

from typing import Tuple

import numpy as np
import pandas as pd
from sklearn.model_selection import train_test_split


def train_update_test_split(
    X: pd.DataFrame, frac_new_users: float
) -> Tuple[pd.DataFrame, pd.Series, pd.DataFrame, pd.Series, pd.DataFrame, pd.Series]:
    """Split ratings into (initial training, update training, update test).

    A fraction ``frac_new_users`` of the users is held out of the initial
    training set; each held-out user's ratings are split 50/50 (stratified by
    user) into an update set and a test set.  Returns
    X_train_initial, y_train_initial, X_train_update, y_train_update,
    X_test_update, y_test_update.
    """
    users = X["user_id"].unique()
    held_out = np.random.choice(users, size=round(frac_new_users * len(users)),
                                replace=False)
    is_new = X["user_id"].isin(held_out)
    initial = X[~is_new].sample(frac=1, replace=False)
    data_update = X[is_new]
    upd, test = train_test_split(data_update, stratify=data_update["user_id"],
                                 test_size=0.5)
    cols = ["user_id", "item_id"]
    return (initial[cols], initial["rating"], upd[cols], upd["rating"],
            test[cols], test["rating"])


def ranking_metrics_from_ranks(ranks, target_ptr, n_candidates, n_relevant, k: int,
                               ndcg_ideal: str = "hits") -> dict:
    """Top-k metrics and AUC from exact ranks (host side, float64).

    ``ranks[target_ptr[u]:target_ptr[u + 1]]`` are the 0-based ranks of user
    u's held-out items among the user's ``n_candidates[u]`` candidate items
    (``rank_items`` / ``SGDEngine.rank``; -1 = not rankable: unknown or
    excluded item).  ``n_relevant[u]`` counts all of the user's held-out items,
    rankable or not (the reference's ``relevant = set(test_items)``,
    project_template/pipeline/evaluate.py:93).

    Per user, with R the ranks >= 0, m = |R|, L = min(k, n_candidates) and
    h = #{r in R : r < k}:

    * ``precision`` = h / L (0 if L = 0): evaluate.py's ``hit.mean()`` over
      the returned list;
    * ``recall`` = h / max(1, n_relevant);
    * ``ndcg`` = sum_{r < k} 1 / log2(r + 2) over the ideal's
      sum_{p < n} 1 / log2(p + 2): n = h with ``ndcg_ideal="hits"`` (the
      reference's, evaluate.py:21-30: the ideal is the sorted hit vector),
      n = min(n_relevant, L) with ``"relevant"`` (the textbook form);
    * ``map`` = sum_{r < k} (hits at ranks <= r) / (r + 1) over
      max(1, min(n_relevant, L));
    * ``mrr`` = 1 / (min R + 1) if min R < k, else 0;
    * ``auc`` = 1 - (sum R - m (m - 1) / 2) / (m (n_candidates - m)), not cut
      at k; users with n_candidates = m are left out of its mean.

    Means run over the users with m >= 1 (``n_users_evaluated``); with none,
    every metric is 0.0.
    """
    if ndcg_ideal not in ("hits", "relevant"):
        raise ValueError("ndcg_ideal must be 'hits' or 'relevant'")
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    ptr = np.asarray(target_ptr, np.int64)
    nu = len(ptr) - 1
    ncand = np.asarray(n_candidates, np.int64)
    mrel = np.asarray(n_relevant, np.int64)
    if nu < 0 or len(ncand) != nu or len(mrel) != nu:
        raise ValueError("target_ptr needs one more entry than n_candidates / n_relevant")
    names = ("precision", "recall", "ndcg", "map", "mrr", "auc")
    out = {name: 0.0 for name in names}
    out["n_users_evaluated"] = 0
    if nu == 0:
        return out
    r = np.asarray(ranks, np.int64)[ptr[0]:ptr[-1]]
    seg = np.repeat(np.arange(nu, dtype=np.int64), np.diff(ptr))
    ok = r >= 0
    seg, r = seg[ok], r[ok]
    m = np.bincount(seg, minlength=nu).astype(np.int64)
    ev = m >= 1
    if not ev.any():
        return out
    L = np.minimum(k, ncand)
    hit = r < k
    hseg, hr = seg[hit], r[hit]
    h = np.bincount(hseg, minlength=nu).astype(np.int64)
    precision = np.where(L > 0, h / np.maximum(L, 1), 0.0)
    recall = h / np.maximum(1, mrel)
    dcg = np.bincount(hseg, weights=1.0 / np.log2(hr + 2.0), minlength=nu)
    ideal = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(k) + 2.0))])
    n_ideal = h if ndcg_ideal == "hits" else np.clip(np.minimum(mrel, L), 0, k)
    idcg = ideal[n_ideal]
    ndcg = np.where(idcg > 0, dcg / np.where(idcg > 0, idcg, 1.0), 0.0)
    # hits at ranks <= r: position of r's last equal among the user's sorted ranks
    key = (seg << 32) + r
    skey = np.sort(key, kind="stable")
    le = np.searchsorted(skey, key, side="right") - np.searchsorted(skey, seg << 32, side="left")
    ap = (np.bincount(hseg, weights=(le / (r + 1.0))[hit], minlength=nu)
          / np.maximum(1, np.minimum(mrel, L)))
    minr = np.full(nu, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(minr, seg, r)
    mrr = np.where(minr < k, 1.0 / (np.minimum(minr, k) + 1.0), 0.0)
    den = m * (ncand - m)
    has_auc = ev & (den > 0)
    sum_r = np.bincount(seg, weights=r.astype(np.float64), minlength=nu)
    auc = 1.0 - (sum_r - m * (m - 1) / 2.0) / np.where(den > 0, den, 1)
    for name, v in (("precision", precision), ("recall", recall), ("ndcg", ndcg),
                    ("map", ap), ("mrr", mrr)):
        out[name] = float(np.mean(v[ev].astype(np.float64)))
    out["auc"] = float(np.mean(auc[has_auc])) if has_auc.any() else 0.0
    out["n_users_evaluated"] = int(ev.sum())
    return out
