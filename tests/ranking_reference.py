"""NumPy restatement of exact ranking (mf_rank's contract, include/mf_hip.h).

Candidates of a query are the items not in its exclusion list; they are
ordered by ``order_key(score)`` descending, then item id ascending (NaN below
every number, all NaNs tie); a target's rank is the number of candidates in
front of it, -1 when it is out of range or excluded.  Pinned against the
reference's evaluate_topk in test_ranking_cpu.py, reused by test_gpu_rank.py.
"""

import numpy as np


def order_key(scores) -> np.ndarray:
    """float64 scores -> uint64 keys whose unsigned order is the score order;
    NaN -> 1, below every number (-0.0 sorts below +0.0, as the bits do)."""
    s = np.ascontiguousarray(scores, np.float64)
    b = s.view(np.uint64)
    top = np.uint64(1) << np.uint64(63)
    key = np.where(b & top != 0, ~b, b | top)
    key[np.isnan(s)] = np.uint64(1)
    return key


def ranks_from_scores(scores, tgt_ptr, tgt_items, ex_ptr=None, ex_items=None):
    """(ranks int32[n_targets], n_candidates int32[n_query]) from a score
    matrix [n_query, n_items] by a stable sort per query."""
    scores = np.asarray(scores, np.float64)
    nq, n_items = scores.shape
    tgt_ptr = np.asarray(tgt_ptr, np.int64)
    tgt_items = np.asarray(tgt_items, np.int64)
    ranks = np.full(int(tgt_ptr[-1]) if nq else 0, -1, np.int32)
    ncand = np.zeros(nq, np.int32)
    for q in range(nq):
        gone = np.zeros(n_items, bool)
        if ex_ptr is not None:
            ex = np.asarray(ex_items[ex_ptr[q]:ex_ptr[q + 1]], np.int64)
            gone[ex[(ex >= 0) & (ex < n_items)]] = True
        cand = np.flatnonzero(~gone)                     # ascending ids
        # stable ascending sort of ~key = key descending, equal keys by id ascending
        order = np.argsort(~order_key(scores[q, cand]), kind="stable")
        pos = np.full(n_items, -1, np.int64)
        pos[cand[order]] = np.arange(len(cand))
        ncand[q] = len(cand)
        for t in range(tgt_ptr[q], tgt_ptr[q + 1]):
            it = tgt_items[t]
            if 0 <= it < n_items:
                ranks[t] = pos[it]
    return ranks, ncand
