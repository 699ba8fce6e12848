"""CPU tests of ranking evaluation: utils.ranking_metrics_from_ranks against
the reference's evaluate_topk (tests/golden/ranking_eval.json, written by
tools/make_ranking_fixture.py from project_template/pipeline/evaluate.py) and
against hand-computed values; tests/ranking_reference.py (the NumPy ranks the
GPU tests compare with) is pinned on the same fixture; mf_rank validates its
arguments before any device work.  No GPU."""

import json
import os
from math import log2

import numpy as np
import pytest

import ranking_reference as rr
from conftest import GOLDEN
from matrix_factorization import ranking_metrics_from_ranks

MF_OK, MF_ERR_INVALID = 0, 1


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "ranking_eval.json")) as f:
        d = json.load(f)
    d["scores"] = np.asarray(d["scores"], np.float64)
    return d


def case_csr(case):
    users = np.asarray([x["user"] for x in case["users"]], np.int64)
    tgt = [x["test"] for x in case["users"]]
    ex = [x["known"] for x in case["users"]]

    def ptr(ls):
        return np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int64)

    def cat(ls):
        return np.asarray([i for x in ls for i in x], np.int32)

    return users, ptr(tgt), cat(tgt), ptr(ex), cat(ex)


# ------------------------------------------------------------ reference's numbers
@pytest.mark.parametrize("ci", range(6))
def test_metrics_reproduce_the_reference(fixture, ci):
    """Ranks from the fixture's score table (NumPy) -> ranking_metrics_from_ranks
    = the reference's precision / recall / NDCG.  Both sides are float64 means
    of at most 40 values in [0, 1]: |diff| <= 1e-12 is n * eps with two orders
    of margin."""
    case = fixture["cases"][ci]
    users, tp, ti, ep, ei = case_csr(case)
    assert {(case["k"], case["n_test"]) for case in fixture["cases"]} == {
        (k, n) for k in (1, 5, 10) for n in (1, 3)}
    assert len(case["skipped_users"]) >= 1              # the reference skipped them
    ranks, ncand = rr.ranks_from_scores(fixture["scores"][users], tp, ti, ep, ei)
    assert np.all(ranks >= 0)
    got = ranking_metrics_from_ranks(ranks, tp, ncand, np.diff(tp), case["k"])
    for name in ("precision", "recall", "ndcg"):
        print(f"k={case['k']} n_test={case['n_test']} {name}: {got[name]!r} vs {case[name]!r}")
        assert abs(got[name] - case[name]) <= 1e-12
    assert got["n_users_evaluated"] == len(users)
    assert 0.0 < got["auc"] < 1.0


def test_reference_ranks_are_counts_of_items_in_front(fixture):
    """ranking_reference (stable sort) = the definition (count the candidates
    with a higher score, or an equal score and a lower id), on the fixture's
    table with its many equal scores."""
    case = fixture["cases"][-1]
    users, tp, ti, ep, ei = case_csr(case)
    S = fixture["scores"][users]
    ranks, ncand = rr.ranks_from_scores(S, tp, ti, ep, ei)
    for q in range(len(users)):
        known = set(ei[ep[q]:ep[q + 1]].tolist())
        cand = [j for j in range(S.shape[1]) if j not in known]
        assert ncand[q] == len(cand)
        for t in range(tp[q], tp[q + 1]):
            it = ti[t]
            front = sum(1 for j in cand if S[q, j] > S[q, it] or (S[q, j] == S[q, it] and j < it))
            assert ranks[t] == front


def test_reference_edges():
    S = np.array([[1.0, np.nan, 1.0, 3.0, -0.0, 0.0]])
    tp = np.array([0, 8])
    ti = np.array([0, 1, 2, 3, 4, 5, 6, -1])
    ranks, ncand = rr.ranks_from_scores(S, tp, ti)
    # 3.0 | 1.0 (id 0) | 1.0 (id 2) | +0.0 | -0.0 | NaN; out of range: -1
    assert ranks.tolist() == [1, 5, 2, 0, 4, 3, -1, -1] and ncand.tolist() == [6]
    ranks, ncand = rr.ranks_from_scores(S, tp, ti, np.array([0, 4]), np.array([3, 3, 0, 77]))
    assert ranks.tolist() == [-1, 3, 0, -1, 2, 1, -1, -1] and ncand.tolist() == [4]


# ------------------------------------------------------------ hand-computed
# user A: 10 candidates, held-out ranks 0, 3, 7 and one unknown item (-1), k = 5
A = dict(ranks=[0, 3, 7, -1], ncand=10, mrel=4)
A_WANT = dict(
    precision=2 / 5,                                     # hits at 0 and 3, L = 5
    recall=2 / 4,
    ndcg=(1 / log2(2) + 1 / log2(5)) / (1 / log2(2) + 1 / log2(3)),
    map=(1 / 1 + 2 / 4) / 4,                             # min(m_rel, L) = 4
    mrr=1.0,
    auc=1 - (10 - 3) / (3 * 7),                          # sum R = 10, m(m-1)/2 = 3
)
A_NDCG_RELEVANT = (1 + 1 / log2(5)) / (1 + 1 / log2(3) + 1 / log2(4) + 1 / log2(5))
# user B: 3 candidates (L = 3 < k), one held-out item at rank 1
B = dict(ranks=[1], ncand=3, mrel=1)
B_WANT = dict(precision=1 / 3, recall=1.0, ndcg=1 / log2(3), map=1 / 2, mrr=1 / 2,
              auc=1 - 1 / (1 * 2))
# user C: nothing rankable
C = dict(ranks=[-1, -1], ncand=10, mrel=2)
# user D: the only held-out item beyond k
D = dict(ranks=[7], ncand=10, mrel=1)
D_WANT = dict(precision=0.0, recall=0.0, ndcg=0.0, map=0.0, mrr=0.0, auc=1 - 7 / 9)
# user E: every candidate is a held-out item (no AUC)
E = dict(ranks=[1, 0], ncand=2, mrel=2)
E_WANT = dict(precision=1.0, recall=1.0, ndcg=1.0, map=1.0, mrr=1.0)
NAMES = ("precision", "recall", "ndcg", "map", "mrr", "auc")


def run(users, k=5, **kw):
    ptr = np.concatenate([[0], np.cumsum([len(u["ranks"]) for u in users])])
    ranks = [r for u in users for r in u["ranks"]]
    return ranking_metrics_from_ranks(np.asarray(ranks, np.int32), ptr,
                                      [u["ncand"] for u in users],
                                      [u["mrel"] for u in users], k, **kw)


def close(got, want, names=NAMES):
    for n in names:
        assert abs(got[n] - want[n]) <= 1e-15 * 4, (n, got[n], want[n])


def test_hand_single_users():
    got = run([A])
    close(got, A_WANT)
    assert got["n_users_evaluated"] == 1
    close(run([B]), B_WANT)                              # L < k
    close(run([D]), D_WANT)                              # mrr / map cut at k, auc is not
    got = run([E])
    close(got, E_WANT, NAMES[:5])
    assert got["auc"] == 0.0                             # left out of the AUC mean: none left


def test_hand_ndcg_relevant():
    got = run([A], ndcg_ideal="relevant")
    assert abs(got["ndcg"] - A_NDCG_RELEVANT) <= 4e-15
    close(got, A_WANT, ("precision", "recall", "map", "mrr", "auc"))
    # L caps the ideal: B has min(m_rel, L) = 1 ideal position
    assert abs(run([B], ndcg_ideal="relevant")["ndcg"] - 1 / log2(3)) <= 4e-15
    with pytest.raises(ValueError):
        run([A], ndcg_ideal="other")


def test_hand_means_skip_users_without_ranks():
    got = run([A, C, B, E])
    assert got["n_users_evaluated"] == 3
    for n in NAMES[:5]:
        assert abs(got[n] - (A_WANT[n] + B_WANT[n] + E_WANT[n]) / 3) <= 4e-15
    assert abs(got["auc"] - (A_WANT["auc"] + B_WANT["auc"]) / 2) <= 4e-15    # E has none


def test_hand_other_k():
    got = run([A], k=8)                                  # all three within k
    assert abs(got["precision"] - 3 / 8) <= 4e-15 and abs(got["recall"] - 3 / 4) <= 4e-15
    assert abs(got["map"] - (1 + 2 / 4 + 3 / 8) / 4) <= 4e-15
    want = (1 + 1 / log2(5) + 1 / log2(9)) / (1 + 1 / log2(3) + 1 / log2(4))
    assert abs(got["ndcg"] - want) <= 4e-15
    assert abs(got["auc"] - A_WANT["auc"]) <= 4e-15      # not cut at k


def test_empty():
    zero = {n: 0.0 for n in NAMES}
    zero["n_users_evaluated"] = 0
    assert run([C]) == zero
    assert ranking_metrics_from_ranks(np.zeros(0, np.int32), [0], [], [], 10) == zero
    assert run([dict(ranks=[], ncand=5, mrel=0)]) == zero


# ------------------------------------------------------------ C ABI validation
def test_mf_rank_validates_before_device_work():
    """Bad dtype / kernel / n_factors: MF_ERR_INVALID with the argument named,
    from NULL pointers (nothing is touched); empty input is MF_OK."""
    from matrix_factorization import _lib
    lib = _lib.load()

    def call(nq=4, n_items=10, k=8, kernel=0, dtype=0):
        return lib.mf_rank(None, nq, 0.0, None, None, None, None, n_items, k, kernel, dtype,
                           1.0, 1.0, 5.0, None, None, None, None, None, None, None, None)

    for kw, word in ((dict(dtype=2), "dtype=2"), (dict(dtype=-1), "dtype=-1"),
                     (dict(kernel=3), "kernel=3"), (dict(k=-1), "n_factors=-1"),
                     (dict(k=lib.mf_max_factors() + 1), "n_factors="),
                     (dict(nq=-1), "n_query=-1"), (dict(n_items=-2), "n_items=-2"),
                     (dict(), "query_users")):
        assert call(**kw) == MF_ERR_INVALID
        assert word in _lib.last_error() and "mf_rank" in _lib.last_error()
    assert call(nq=0) == MF_OK
    assert lib.mf_rank_workspace_bytes(0, 5, 10) == 0
    assert lib.mf_rank_workspace_bytes(3, 0, 10) == 0
    assert lib.mf_rank_workspace_bytes(3, 5, 10) >= 5 * 12
