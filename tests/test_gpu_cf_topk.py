"""GPU tests of the neighbourhood models' all-targets pass: mf_cf_scores /
mf_cf_topk / mf_cf_rank through NeighbourEngine.scores / topk / rank, and
recommend_batch / rank_items / evaluate_topk of ItemItemCF / UserUserCF.

Oracles.  Scores: the engine's own ``predict`` (mf_cf_predict, pinned against
tests/cf_reference.py in test_gpu_cf.py) on the explicit (entity, other) pairs.
Order: tests/ranking_reference.py (order keys, a stable NumPy sort) on those
scores.  Every comparison is exact: array_equal on ids, ranks, candidate
counts and on the float64 bits of the scores.
"""

import os
import pickle

import numpy as np
import pandas as pd
import pytest

from cf_reference import CASES, load_case
from ranking_reference import order_key, ranks_from_scores
from matrix_factorization import ItemItemCF, UserUserCF
from matrix_factorization.utils import ranking_metrics_from_ranks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OTHER, ENTITY = 0, 1
GM = 3.25
NNS = (1, 5, 62, 1000)


def half_integers(rs, size):
    return rs.randint(1, 11, size=size) / 2.0            # 0.5 .. 5.0


def engine(stored, R):
    from matrix_factorization.neighbours import NeighbourEngine

    ent, oth = np.nonzero(stored)
    r = R[ent, oth]
    p = np.random.RandomState(len(ent)).permutation(len(ent))
    return NeighbourEngine(ent[p], oth[p], r[p], R.shape[0], R.shape[1], DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def oracle_scores(eng, queries, side, nn):
    """predict(bound=False) on the explicit pairs: [n_query, n_targets]."""
    nt = eng.n_entities if side == OTHER else eng.n_others
    q = np.repeat(np.asarray(queries), nt)
    t = np.tile(np.arange(nt), len(queries))
    ent, oth = (t, q) if side == OTHER else (q, t)
    # a query of -1 makes the pair unknown whatever the target is
    return eng.predict(ent, oth, nn, GM, 0.0, 5.0, False).reshape(len(queries), nt)


def oracle_topk(scores, amount, ex_ptr=None, ex_items=None):
    """(ids, scores) by (order key descending, id ascending) among the targets
    not excluded; -1 / NaN padding."""
    nq, nt = scores.shape
    ids = np.full((nq, amount), -1, np.int32)
    out = np.full((nq, amount), np.nan)
    for q in range(nq):
        gone = np.zeros(nt, bool)
        if ex_ptr is not None:
            ex = np.asarray(ex_items[ex_ptr[q]:ex_ptr[q + 1]], np.int64)
            gone[ex[(ex >= 0) & (ex < nt)]] = True
        cand = np.flatnonzero(~gone)
        best = cand[np.argsort(~order_key(scores[q, cand]), kind="stable")][:amount]
        ids[q, :len(best)] = best
        out[q, :len(best)] = scores[q, best]
    return ids, out


def check_topk(got, want):
    assert np.array_equal(got[0], want[0])
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64
    pad = want[0] < 0
    assert np.isnan(got[1][pad]).all()
    assert np.array_equal(bits(got[1])[~pad], bits(want[1])[~pad])


def tie_group_straddles(scores, amount):
    """Is there a query whose amount-th and (amount+1)-th best scores are equal,
    in a group of more than ``amount`` equal scores?"""
    for row in scores:
        s = np.sort(row)[::-1]
        if amount < len(s) and s[amount - 1] == s[amount] and (row == s[amount]).sum() > amount:
            return True
    return False


# ------------------------------------------------------------------ case 1
LENS = [1, 63, 65, 257, 296, 5, 0] + [40] * 9
TIE_LO, TIE_HI, TIE_TARGET, EMPTY = 10, 11, 12, 13
O_TIE, O_SWAP, O_ZERO = 8, 9, 16
CLONES = np.arange(20, 32)                   # 12 identical entities: equal means, equal S rows
Q_OTHER = np.concatenate([np.arange(17), [-1]])
Q_ENTITY = np.concatenate([np.arange(300), [-1]])
QUERIES = {OTHER: Q_OTHER, ENTITY: Q_ENTITY}


@pytest.fixture(scope="module")
def edges():
    """300 entities x 17 others.  Others 0..15 have lists of LENS[o] entries;
    every stored entry of other 16 has rating 0 (no candidate: each score is
    m_e).  Entity 13 has no ratings.  Entities 10 and 11 are identical except
    that their ratings by others 8 and 9 are swapped and entity 12 is entity 10
    without those two (test_gpu_cf.py's tie across an n_neighbors = 1 cut).
    Entities 20..31 are identical (5.0 from other 4 and others 7..15): the
    twelve highest means, all equal -- a tie group across an amount = 10 cut
    for query other 16 -- and twelve equal similarities in every row."""
    rs = np.random.RandomState(7)
    ne, no = 300, 17
    special = [TIE_LO, TIE_HI, TIE_TARGET, EMPTY]
    pool = np.setdiff1d(np.arange(ne), special)                  # 296
    plain = np.setdiff1d(pool, CLONES)                           # 284
    stored = np.zeros((ne, no), bool)
    for o, n in enumerate(LENS[:7]):
        stored[rs.choice(pool if n == len(pool) else plain, n, replace=False), o] = True
    R = half_integers(rs, stored.shape)
    stored[TIE_LO, 7:16] = True
    R[TIE_LO, O_TIE], R[TIE_LO, O_SWAP] = 4.5, 1.0
    stored[TIE_HI], R[TIE_HI] = stored[TIE_LO], R[TIE_LO]
    R[TIE_HI, O_TIE], R[TIE_HI, O_SWAP] = 1.0, 4.5
    stored[TIE_TARGET], R[TIE_TARGET] = stored[TIE_LO], R[TIE_LO]
    stored[TIE_TARGET, [O_TIE, O_SWAP]] = False
    stored[CLONES, 7:16] = True
    R[CLONES] = 5.0
    for o in range(7, 16):                                       # filled up to 40 entries
        n = LENS[o] - int(stored[:, o].sum())
        stored[rs.choice(plain, n, replace=False), o] = True
    stored[rs.choice(plain, 30, replace=False), O_ZERO] = True
    R[:, O_ZERO] = 0.0
    R = np.where(stored, R, 0.0)
    assert [int(stored[:, o].sum()) for o in range(16)] == LENS
    assert not stored[EMPTY].any() and stored[:, O_ZERO].sum() == 30 and not R[:, O_ZERO].any()
    eng = engine(stored, R)
    want = {(side, nn): oracle_scores(eng, QUERIES[side], side, nn)
            for side in (OTHER, ENTITY) for nn in NNS}
    return dict(eng=eng, stored=stored, R=R, want=want, mean=eng.mean.cpu().numpy())


@pytest.mark.parametrize("side", [OTHER, ENTITY])
@pytest.mark.parametrize("nn", NNS)
def test_scores_equal_predict_bit_for_bit(edges, nn, side):
    eng, want = edges["eng"], edges["want"][side, nn]
    got = eng.scores(QUERIES[side], side, nn, GM)
    assert got.dtype == np.float64 and same_bits(got, want)
    assert (got[-1] == GM).all()                                 # the unknown query
    m = edges["mean"]
    if side == OTHER:
        assert same_bits(got[O_ZERO], m)                         # no candidate: m_e
        assert same_bits(got[6], m)                              # an empty list
    else:
        assert (got[EMPTY] == 0.0).all() and m[EMPTY] == 0.0     # every similarity 0
    # the blocking of the targets changes nothing
    try:
        for tpb in (1, 7):
            eng.targets_per_block = tpb
            assert same_bits(eng.scores(QUERIES[side], side, nn, GM), want)
    finally:
        eng.targets_per_block = 0


@pytest.mark.parametrize("nn", [5, 1000])
def test_entity_row_staged_in_lds_gives_the_same_bits(edges, nn):
    old = os.environ.get("MF_CF_ROW_LDS")
    try:
        for v in ("0", "1"):
            os.environ["MF_CF_ROW_LDS"] = v
            got = edges["eng"].scores(Q_ENTITY, ENTITY, nn, GM)
            assert same_bits(got, edges["want"][ENTITY, nn])
    finally:
        if old is None:
            os.environ.pop("MF_CF_ROW_LDS", None)
        else:
            os.environ["MF_CF_ROW_LDS"] = old


def test_the_data_hold_tie_groups_across_the_cut(edges):
    """Groups of equal scores larger than ``amount`` that straddle the cut, in
    the oracle scores: other 16 (scores m_e; the twelve clones share the
    highest mean) and the empty entity (all targets tie and come back in id
    order)."""
    eng = edges["eng"]
    w = edges["want"][OTHER, 5]
    top = np.sort(w[O_ZERO])[::-1]
    assert top[0] == top[11] > top[12] and set(np.flatnonzero(w[O_ZERO] == top[0])) == set(CLONES)
    assert tie_group_straddles(w[[O_ZERO]], 10) and tie_group_straddles(w[[O_ZERO]], 1)
    ids, sc = eng.topk(np.asarray([O_ZERO]), OTHER, 5, GM, 10)
    assert ids[0].tolist() == CLONES[:10].tolist() and (sc[0] == top[0]).all()
    w = edges["want"][ENTITY, 5]
    assert (w[EMPTY] == w[EMPTY, 0]).all() and tie_group_straddles(w[[EMPTY]], 10)
    ids, _ = eng.topk(np.asarray([EMPTY]), ENTITY, 5, GM, 10)
    assert ids[0].tolist() == list(range(10))


# ------------------------------------------------------------------ case 3
def exclusion_lists(nq, nt, seed):
    """Per query a shuffled list with duplicates and ids out of range; query 0
    loses every target, query 1 keeps three."""
    rs = np.random.RandomState(seed)
    per = []
    for q in range(nq):
        if q == 0:
            ex = np.arange(nt)
        elif q == 1:
            ex = np.setdiff1d(np.arange(nt), rs.choice(nt, 3, replace=False))
        else:
            ex = rs.choice(nt, rs.randint(0, nt // 2 + 1), replace=False)
        ex = np.concatenate([ex, ex[:len(ex) // 3], [-5, nt, nt + 100, -1]])
        per.append(rs.permutation(ex))
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in per])]).astype(np.int64)
    return ptr, np.concatenate(per).astype(np.int32)


@pytest.mark.parametrize("side", [OTHER, ENTITY])
@pytest.mark.parametrize("amount", [1, 10, 299, 300])
def test_topk_equals_the_sorted_oracle(edges, amount, side):
    eng, nn = edges["eng"], 5
    q, w = QUERIES[side], edges["want"][side, nn]
    check_topk(eng.topk(q, side, nn, GM, amount), oracle_topk(w, amount))
    ptr, ex = exclusion_lists(len(q), w.shape[1], 100 + side)
    ids, sc = eng.topk(q, side, nn, GM, amount, ptr, ex)
    check_topk((ids, sc), oracle_topk(w, amount, ptr, ex))
    assert (ids[0] == -1).all()                                  # every target excluded
    assert (ids[1] >= 0).sum() == min(amount, 3)                 # three candidates left
    if amount > 3:
        assert (ids[1, 3:] == -1).all()


@pytest.mark.parametrize("side", [OTHER, ENTITY])
def test_ranks_equal_the_counting_oracle(edges, side):
    eng, nn = edges["eng"], 5
    q, w = QUERIES[side], edges["want"][side, nn]
    nq, nt = w.shape
    ptr, ex = exclusion_lists(nq, nt, 100 + side)
    rs = np.random.RandomState(5 + side)
    per = []
    for i in range(nq):
        if i == 2:
            per.append(np.zeros(0, np.int64))                    # a query with no targets
            continue
        t = rs.choice(nt, min(nt, 9), replace=False)
        mine = ex[ptr[i]:ptr[i + 1]]
        gone = mine[(mine >= 0) & (mine < nt)][:1]               # an excluded target
        per.append(np.concatenate([t, t[:2], gone, [nt, -1]]))   # repeats, out of range
    tp = np.concatenate([[0], np.cumsum([len(x) for x in per])]).astype(np.int64)
    ti = np.concatenate(per).astype(np.int32)
    for e_ptr, e_items in ((None, None), (ptr, ex)):
        want_r, want_c = ranks_from_scores(w, tp, ti, e_ptr, e_items)
        got_r, got_c = eng.rank(q, side, nn, GM, tp, ti, e_ptr, e_items)
        assert got_r.dtype == np.int32 and got_c.dtype == np.int32
        assert np.array_equal(got_r, want_r) and np.array_equal(got_c, want_c)
    assert got_c[0] == 0 and got_c[1] == 3 and (got_r[tp[0]:tp[1]] == -1).all()
    assert (got_r >= 0).any() and (got_r == -1).any()


# ------------------------------------------------------------------ case 4
@pytest.mark.parametrize("side,chunk", [(OTHER, 7), (ENTITY, 128)])
def test_query_chunks_give_the_single_launch_results(edges, side, chunk):
    eng, nn, amount = edges["eng"], 62, 10
    q = QUERIES[side]
    nq, nt = len(q), eng.n_targets(side)
    assert nq > 2 * chunk and nq % chunk                         # >= 3 chunks, the last partial
    ptr, ex = exclusion_lists(nq, nt, 7)
    tp = np.arange(nq + 1, dtype=np.int64) * 3
    ti = np.random.RandomState(3).randint(0, nt, 3 * nq).astype(np.int32)
    run = lambda: (eng.scores(q, side, nn, GM),) + eng.topk(q, side, nn, GM, amount, ptr, ex) \
        + eng.rank(q, side, nn, GM, tp, ti, ptr, ex)             # noqa: E731
    whole = run()
    assert eng._query_chunk(side) >= nq
    try:
        eng.topk_ws_budget = 8 * nt * chunk
        assert eng._query_chunk(side) == chunk
        parts = run()
    finally:
        del eng.topk_ws_budget
    assert same_bits(parts[0], edges["want"][side, nn])
    for a, b in zip(whole, parts):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------ case 2
def test_long_lists_beyond_the_staged_bound():
    """A 3000-entry list (beyond the 1024 entries staged in LDS) and 300-entry
    ones: scores, and the top 2048 of 3100 targets."""
    rs = np.random.RandomState(9)
    ne, no = 3100, 40
    stored = np.zeros((ne, no), bool)
    stored[rs.choice(ne, 3000, replace=False), 0] = True
    for o in range(1, no):
        stored[rs.choice(ne, 300, replace=False), o] = True
    R = np.where(stored, half_integers(rs, stored.shape), 0.0)
    eng = engine(stored, R)
    assert stored[:, 0].sum() == 3000
    q_o = np.asarray([0, 1])
    q_e = rs.choice(ne, 12, replace=False)
    for nn in (1, 5, 2900, 5000):
        want = oracle_scores(eng, q_o, OTHER, nn)
        assert same_bits(eng.scores(q_o, OTHER, nn, GM), want)
        assert same_bits(eng.scores(q_e, ENTITY, nn, GM), oracle_scores(eng, q_e, ENTITY, nn))
        if nn == 5:
            check_topk(eng.topk(q_o, OTHER, nn, GM, 2048), oracle_topk(want, 2048))


# ------------------------------------------------------------------ case 5
def fit_case(case, cls):
    Model = ItemItemCF if cls == "itemitemcf" else UserUserCF
    X = pd.DataFrame({"user_id": case["train_user"], "item_id": case["train_item"]})
    np.random.seed(3)
    model = Model(min_rating=float(case["min_rating"]), max_rating=float(case["max_rating"]),
                  n_neighbors=int(case["n_neighbors"]), device=DEV)
    return model.fit(X, pd.Series(case["train_rating"]))


@pytest.mark.parametrize("data,cls", CASES)
def test_estimators_rank_like_predict(data, cls):
    case = load_case(data, cls)
    model = fit_case(case, cls)
    train = pd.DataFrame({"user_id": case["train_user"], "item_id": case["train_item"]})
    items = list(model.item_id_map.keys())                       # internal id order
    unknown = max(case["user_ids"].tolist()) + 1000
    users = case["user_ids"].tolist() + [unknown]
    ni, lo, hi = len(items), model.min_rating, model.max_rating
    frame = pd.DataFrame({"user_id": np.repeat(users, ni), "item_id": np.tile(items, len(users))})
    P = np.asarray(model.predict(frame, bound_ratings=False)).reshape(len(users), ni)
    assert (P[-1] == model.global_mean).all()
    upos = {u: p for p, u in enumerate(users)}
    known = np.zeros(P.shape, bool)
    known[[upos[u] for u in case["train_user"].tolist()],
          [model.item_id_map[i] for i in case["train_item"].tolist()]] = True

    # recommend_batch: per user the candidates by (score descending, internal id ascending)
    got = model.recommend_batch(users, amount=7, exclude_known=train, bound_ratings=False)
    clipped = model.recommend_batch(users, amount=7, exclude_known=train)
    assert list(got.columns) == ["user_id", "item_id", "rating_pred"]
    assert got["user_id"].tolist() == clipped["user_id"].tolist()
    assert got["item_id"].tolist() == clipped["item_id"].tolist()
    at = 0
    for p, u in enumerate(users):
        cand = np.flatnonzero(~known[p])
        best = cand[np.argsort(~order_key(P[p, cand]), kind="stable")][:7]
        rows = got.iloc[at:at + len(best)]
        assert rows["user_id"].tolist() == [u] * len(best)
        assert rows["item_id"].tolist() == [items[i] for i in best]
        assert np.array_equal(bits(rows["rating_pred"].to_numpy()), bits(P[p, best]))
        assert np.array_equal(bits(clipped["rating_pred"].to_numpy()[at:at + len(best)]),
                              bits(np.clip(P[p, best], lo, hi)))
        at += len(best)
    assert at == len(got) == len(clipped)
    # the one-user recommend() lists the same scores
    for u in users[:3]:
        mine = train["item_id"][train["user_id"] == u].tolist()
        rec = model.recommend(u, 7, items_known=mine, bound_ratings=False)
        assert rec["rating_pred"].tolist() == got["rating_pred"][got["user_id"] == u].tolist()

    # rank_items: the test pairs, an unknown user, an unknown item, a training pair
    X = pd.DataFrame({"user_id": case["test_user"], "item_id": case["test_item"]})
    n_test = len(X)
    extra = pd.DataFrame({"user_id": [unknown, users[0], train["user_id"].iloc[0]],
                          "item_id": [items[0], max(items) + 1000, train["item_id"].iloc[0]]})
    Xr = pd.concat([X, extra], ignore_index=True)

    def oracle_rank(u, i):
        if u not in upos or u == unknown or i not in model.item_id_map:
            return -1
        p, t = upos[u], model.item_id_map[i]
        if known[p, t]:
            return -1
        key = order_key(P[p])
        cand = ~known[p]
        before = (key > key[t]) | ((key == key[t]) & (np.arange(ni) < t))
        return int((before & cand).sum())

    want = np.asarray([oracle_rank(u, i) for u, i in zip(Xr["user_id"], Xr["item_id"])], np.int32)
    ranked = model.rank_items(Xr, exclude_known=train)
    assert list(ranked.columns) == ["user_id", "item_id", "rank", "n_candidates"]
    assert np.array_equal(ranked["rank"].to_numpy(), want)
    assert (want[:n_test] >= 0).all() and (want[n_test:] == -1).all()
    ncand = np.asarray([ni - known[upos[u]].sum() if u in upos else -1 for u in Xr["user_id"]])
    assert np.array_equal(ranked["n_candidates"].to_numpy()[:n_test], ncand[:n_test])

    # evaluate_topk: ranking_metrics_from_ranks on the oracle ranks
    Xd = X.drop_duplicates()
    ucode, ulabel = pd.factorize(Xd["user_id"].astype(object))
    r = np.asarray([oracle_rank(u, i) for u, i in zip(Xd["user_id"], Xd["item_id"])], np.int32)
    order = np.argsort(ucode, kind="stable")
    ptr = np.zeros(len(ulabel) + 1, np.int64)
    np.cumsum(np.bincount(ucode, minlength=len(ulabel)), out=ptr[1:])
    cand = np.asarray([ni - known[upos[u]].sum() for u in ulabel], np.int32)
    res = model.evaluate_topk(X, k=[5, 10], exclude_known=train)
    assert sorted(res) == [5, 10]
    for k in (5, 10):
        assert res[k] == ranking_metrics_from_ranks(r[order], ptr, cand, np.diff(ptr), k,
                                                    ndcg_ideal="hits")
    assert model.evaluate_topk(X, k=5, exclude_known=train) == res[5]

    loaded = pickle.loads(pickle.dumps(model))
    assert loaded.__dict__.get("_engine") is None
    again = loaded.recommend_batch(users, amount=7, exclude_known=train, bound_ratings=False)
    pd.testing.assert_frame_equal(again, got, check_exact=True)
