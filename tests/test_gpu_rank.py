"""GPU tests of exact ranking (mf_rank, SGDEngine.rank, KernelMF.rank_items /
evaluate_topk).  Ranks are integers and compared for equality with
tests/ranking_reference.py fed with mf_predict's unbounded scores of every
(user, item) pair -- which also pins the score bits to predict's: a score that
differed in its last bit would reorder near-ties somewhere in these cases."""

import pickle

import numpy as np
import pandas as pd
import pytest

import ranking_reference as rr

pytestmark = pytest.mark.gpu

MF_ERR_INVALID = 1


def make_engine(k, nu, ni, seed, kernel="linear", dtype="float32"):
    from matrix_factorization.device_model import DeviceModel

    rs = np.random.RandomState(seed)
    P = rs.normal(0, 0.3, (nu, k))
    Q = rs.normal(0, 0.3, (ni, k))
    bu = rs.normal(0, 0.1, nu)
    bi = rs.normal(0, 0.1, ni)
    eng = DeviceModel(nu, ni, k, kernel, dtype, "cuda:0", gamma=0.7, min_rating=1.0,
                      max_rating=5.0, global_mean=3.5)
    eng.load_params(P, Q, bu, bi)
    return eng, (P, Q, bu, bi)


def scores_of(eng, users):
    """mf_predict (bound_ratings = 0) of every item for each query user."""
    ni = eng.n_items
    u = np.repeat(np.asarray(users, np.int32), ni)
    i = np.tile(np.arange(ni, dtype=np.int32), len(users))
    return eng.predict(u, i, False).reshape(len(users), ni)


def csr(lists, dtype=np.int32):
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    flat = np.asarray([v for x in lists for v in x], dtype)
    return ptr, flat


def check(eng, users, tgt, ex=None):
    tp, ti = csr(tgt)
    ep, ei = csr(ex) if ex is not None else (None, None)
    ranks, ncand = eng.rank(np.asarray(users, np.int32), tp, ti, ep, ei)
    want_r, want_c = rr.ranks_from_scores(scores_of(eng, users), tp, ti, ep, ei)
    assert ranks.dtype == np.int32 and ncand.dtype == np.int32
    assert np.array_equal(ncand, want_c)
    assert np.array_equal(ranks, want_r)
    return ranks, ncand


def random_case(rs, nu, ni, nq, max_t=5, max_ex=40):
    users = rs.randint(0, nu, nq)
    tgt = [rs.randint(0, ni, rs.randint(0, max_t + 1)).tolist() for _ in range(nq)]
    # exclusions with repeats and ids out of range on both sides
    ex = [rs.randint(-3, ni + 3, rs.randint(0, max_ex + 1)).tolist() for _ in range(nq)]
    return users, tgt, ex


CASES = ([("linear", k) for k in (1, 3, 16, 33, 64, 100, 128)] +
         [("sigmoid", k) for k in (3, 64)] + [("rbf", k) for k in (3, 64)])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("kernel,k", CASES)
def test_ranks_match_numpy(kernel, k, dtype):
    """70 users x 300 items (no multiple of a wave's item step, a ragged last
    user block), random exclusions, 0-5 targets per user, some of them
    excluded themselves."""
    nu, ni, nq = 90, 300, 70
    eng, _ = make_engine(k, nu, ni, 100 + k, kernel, dtype)
    rs = np.random.RandomState(k)
    users, tgt, ex = random_case(rs, nu, ni, nq)
    for q in range(0, nq, 9):                            # targets that are excluded
        if tgt[q]:
            ex[q].append(tgt[q][0])
    ranks, ncand = check(eng, users, tgt, ex)
    assert (ranks >= 0).sum() > nq and (ranks == -1).sum() >= 1
    assert ncand.min() >= ni - 40 - 1


def test_ties_rank_by_item_id():
    """A zero user row with zero item biases scores every item alike: the rank
    is the position by id among the candidates.  Pairs of identical item rows
    tie for every user: the lower id comes first."""
    nu, ni, k = 6, 200, 16
    eng, (P, Q, bu, bi) = make_engine(k, nu, ni, 7)
    P[0] = 0.0
    for j in range(0, 60, 2):
        Q[j + 1] = Q[j]
        bi[j + 1] = bi[j]
    eng.load_params(P, Q, bu, bi)
    users = [1, 2, 3]
    tgt = [list(range(0, 60)), [1, 0, 59, 58], [11, 10]]
    ranks, _ = check(eng, users, tgt, [[], [5], [10]])
    r0 = ranks[:60]
    assert np.all(r0[1::2] == r0[0::2] + 1)              # the twin follows directly
    eng.load_params(P, Q, bu, np.zeros(ni))
    ex = [3, 50, 50, 120]
    tgt = [0, 2, 3, 4, 51, 121, 199]
    ranks, ncand = check(eng, [0, -1], [tgt, tgt], [ex, []])
    assert ranks.tolist() == [0, 2, -1, 3, 49, 118, 196] + tgt
    assert ncand.tolist() == [197, 200]


def test_nan_ranks_last():
    nu, ni, k = 4, 150, 8
    eng, (P, Q, bu, bi) = make_engine(k, nu, ni, 3)
    Q[17] = np.nan
    eng.load_params(P, Q, bu, bi)
    ranks, ncand = check(eng, [0, 1], [[17, 3], [140, 17, 0]], [[], [1, 2]])
    assert ranks[0] == ncand[0] - 1 == 149 and ranks[3] == ncand[1] - 1 == 147
    Q[90] = np.nan                                       # two NaNs tie: by id
    eng.load_params(P, Q, bu, bi)
    ranks, ncand = check(eng, [2], [[90, 17]])
    assert ranks.tolist() == [149, 148]


def test_edge_cases():
    nu, ni, k = 5, 130, 12
    eng, _ = make_engine(k, nu, ni, 11)
    everything = list(range(ni))
    users = [0, 1, 2, 3, -1, 4]
    tgt = [[5, 5, 9, 5],                                 # duplicates: equal ranks
           [7, ni, -1, 2 ** 31 - 1, 8],                  # out of range: -1
           [4, 6],                                       # 4 is excluded: -1
           [],                                           # no targets
           [0, 129],                                     # query user -1: the zero row
           [3, 100]]                                     # every item excluded
    ex = [[], [], [4, 4, 4, 60, 60, -5, ni + 7], [1], [2], everything + everything]
    ranks, ncand = check(eng, users, tgt, ex)
    assert ranks[0] == ranks[1] == ranks[3] >= 0
    assert ranks[[5, 6, 7]].tolist() == [-1, -1, -1] and ranks[4] >= 0 and ranks[8] >= 0
    assert ranks[9] == -1 and ranks[10] >= 0
    assert ncand.tolist() == [ni, ni, ni - 2, ni - 1, ni - 1, 0]   # duplicates count once
    assert ranks[-2:].tolist() == [-1, -1]
    # no exclusion lists at all, and nothing to do
    check(eng, users, tgt)
    r, c = eng.rank(np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32))
    assert len(r) == 0 and len(c) == 0
    r, c = eng.rank(np.array([1, 2], np.int32), np.zeros(3, np.int64), np.zeros(0, np.int32))
    assert len(r) == 0 and c.tolist() == [ni, ni]


def test_many_targets_take_segments():
    """All 5000 items of one user as targets (far more than the lanes of a
    group hold at once): a permutation of 0..4999 that agrees with NumPy."""
    ni = 5000
    eng, _ = make_engine(8, 3, ni, 21)
    order = np.random.RandomState(0).permutation(ni)
    ranks, ncand = check(eng, [1, 2], [order.tolist(), [4999]])
    assert np.array_equal(np.sort(ranks[:ni]), np.arange(ni)) and ncand[0] == ni
    ranks, ncand = check(eng, [1], [order.tolist()], [[10, 20, 30]])
    assert np.array_equal(np.sort(ranks), np.concatenate([[-1] * 3, np.arange(ni - 3)]))


def test_item_splits_and_user_chunks():
    """8 users x 20,000 items: the item range is split over workgroups whose
    partial counts are added; forcing a small rank_ws_budget runs the users in
    several launches.  Both equal NumPy, so they equal each other."""
    nu, ni, k = 8, 20000, 16
    eng, _ = make_engine(k, nu, ni, 5)
    rs = np.random.RandomState(1)
    users, tgt, ex = random_case(rs, nu, ni, 8, max_t=6, max_ex=200)
    tgt[3] = rs.randint(0, ni, 40).tolist()              # more than one chunk's budget alone
    one, c1 = check(eng, users, tgt, ex)
    eng.rank_ws_budget = 16 * 7
    try:
        many, c2 = check(eng, users, tgt, ex)
    finally:
        del eng.rank_ws_budget
    assert np.array_equal(one, many) and np.array_equal(c1, c2)


@pytest.mark.parametrize("mfma", ["1", "0"])
def test_rank_agrees_with_topk(mfma, monkeypatch):
    """The item eng.topk returns at position p has rank p: through the MFMA
    candidate filter and through the exact kernels."""
    monkeypatch.setenv("MF_TOPK_MFMA", mfma)
    nu, ni, k, amount = 80, 3000, 32, 64
    eng, _ = make_engine(k, nu, ni, 13)
    rs = np.random.RandomState(2)
    users = rs.choice(nu, 64, replace=False).astype(np.int32)
    ex = [rs.randint(0, ni, rs.randint(0, 60)).tolist() for _ in users]
    ep, ei = csr(ex)
    items, _ = eng.topk(users, amount, ep, ei)
    assert items.shape == (64, amount) and items.min() >= 0
    tp = np.arange(65, dtype=np.int64) * amount
    ranks, ncand = eng.rank(users, tp, items.reshape(-1), ep, ei)
    assert np.array_equal(ranks.reshape(64, amount), np.tile(np.arange(amount), (64, 1)))
    assert np.array_equal(ncand, [ni - len(set(x)) for x in ex])


def test_validation_before_device_work():
    from matrix_factorization import _lib

    lib = _lib.load()

    def call(k=8, kernel=0, dtype=0):
        return lib.mf_rank(None, 4, 0.0, None, None, None, None, 10, k, kernel, dtype,
                           1.0, 1.0, 5.0, None, None, None, None, None, None, None, None)

    for kw, word in ((dict(dtype=7), "dtype=7"), (dict(kernel=-1), "kernel=-1"),
                     (dict(k=lib.mf_max_factors() + 1), "n_factors=")):
        assert call(**kw) == MF_ERR_INVALID
        assert word in _lib.last_error()


def test_bias_only_engine_refuses():
    from matrix_factorization.engine import SGDEngine

    eng = SGDEngine(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), 3, 4, 0,
                    "bias", "float64", "cuda:0")
    assert eng.bias_only
    with pytest.raises(NotImplementedError):
        eng.rank(np.zeros(1, np.int32), np.array([0, 1]), np.zeros(1, np.int32))


# ------------------------------------------------------------ estimator level
def tiny_data(seed, nu=60, ni=80, n=1500):
    rs = np.random.RandomState(seed)
    pairs = np.unique(np.stack([rs.randint(0, nu, n), rs.randint(0, ni, n)], 1), axis=0)
    df = pd.DataFrame({"user_id": pairs[:, 0] + 1000, "item_id": pairs[:, 1] + 500})
    df["rating"] = rs.randint(1, 6, len(df)).astype(np.float64)
    held = df.groupby("user_id").cumcount() < 2          # two held-out items per user
    return df[~held].reset_index(drop=True), df[held].reset_index(drop=True)


def fit_model(which):
    from matrix_factorization import ImplicitALSMF, KernelMF

    train, test = tiny_data(4)
    np.random.seed(3)
    if which == "ials":
        m = ImplicitALSMF(n_factors=8, n_epochs=2, alpha=10, reg=0.1, verbose=0)
    else:
        m = KernelMF(n_factors=8, n_epochs=2, verbose=0)
    m.fit(train[["user_id", "item_id"]], train["rating"])
    return m, train, test


def ndcg_reference(hit):
    """The reference's _ndcg_at_k (evaluate.py:21-30) on a 0/1 hit vector."""
    if hit.size == 0:
        return 0.0
    disc = np.log2(np.arange(2, hit.size + 2))
    idcg = float(np.sum(np.sort(hit)[::-1] / disc))
    return float(np.sum(hit / disc)) / idcg if idcg > 0 else 0.0


@pytest.mark.parametrize("which", ["ials", "kernelmf"])
def test_estimator_rank_items_and_evaluate_topk(which):
    from matrix_factorization import ranking_metrics_from_ranks

    m, train, test = fit_model(which)
    # one unknown user and one unknown item (for a known user with a known held-out item)
    u_known = test["user_id"].iloc[0]
    X = pd.concat([test[["user_id", "item_id"]],
                   pd.DataFrame({"user_id": [77, u_known], "item_id": [500, 99999]})],
                  ignore_index=True).sample(frac=1.0, random_state=0).reset_index(drop=True)
    got = m.rank_items(X, exclude_known=train)
    assert got[["user_id", "item_id"]].equals(X[["user_id", "item_id"]])
    # ranks recomputed from predict(bound_ratings=False) over all items
    inv = list(m.item_id_map)
    want = np.full(len(X), -1)
    want_c = np.zeros(len(X), np.int64)
    for user, rows in X.groupby("user_id").groups.items():
        known = set(train.loc[train.user_id == user, "item_id"])
        cand = [i for i in inv if i not in known]
        want_c[rows] = len(cand)
        if user not in m.user_id_map:
            continue
        s = np.asarray(m.predict(pd.DataFrame({"user_id": user, "item_id": cand}),
                                 bound_ratings=False))
        ids = np.asarray([m.item_id_map[i] for i in cand])
        order = ids[np.argsort(~rr.order_key(s), kind="stable")]     # cand ids ascend
        pos = {int(j): p for p, j in enumerate(order)}
        for r in rows:
            it = X.at[r, "item_id"]
            if it in m.item_id_map and it not in known:
                want[r] = pos[m.item_id_map[it]]
    assert np.array_equal(got["rank"].to_numpy(), want)
    assert np.array_equal(got["n_candidates"].to_numpy(), want_c)
    assert got.loc[X.user_id == 77, "rank"].tolist() == [-1]
    assert got.loc[X.item_id == 99999, "rank"].tolist() == [-1]
    # held-out items the training set never saw are unknown to the model: -1 too
    rankable = X.item_id.isin(list(m.item_id_map)) & X.user_id.isin(list(m.user_id_map))
    assert np.array_equal(got["rank"].to_numpy() >= 0, rankable.to_numpy())
    assert 60 < rankable.sum() < len(test)
    evaluated = sorted(got.loc[got["rank"] >= 0, "user_id"].unique())

    # evaluate_topk = ranking_metrics_from_ranks on those ranks
    ks = [1, 5, 10]
    res = m.evaluate_topk(X, k=ks, exclude_known=train)
    assert sorted(res) == ks
    g = got.sort_values("user_id", kind="stable")
    ptr = np.concatenate([[0], np.cumsum(g.groupby("user_id", sort=True).size())])
    per_user = g.groupby("user_id", sort=True)
    for k in ks:
        ref = ranking_metrics_from_ranks(g["rank"].to_numpy(), ptr,
                                         per_user["n_candidates"].first().to_numpy(),
                                         per_user.size().to_numpy(), k)
        assert res[k]["n_users_evaluated"] == ref["n_users_evaluated"] == len(evaluated)
        for name in ("precision", "recall", "ndcg", "map", "mrr", "auc"):
            assert abs(res[k][name] - ref[name]) <= 1e-12
    assert m.evaluate_topk(X, k=5, exclude_known=train) == res[5]
    assert m.evaluate_topk(X, k=5, exclude_known=train, ndcg_ideal="relevant")["ndcg"] <= \
        res[5]["ndcg"] + 1e-15

    # ... = the reference's loop, with recommend_batch answering for recommend
    for k in ks:
        rec = m.recommend_batch(evaluated, amount=k, exclude_known=train)
        prec, rec_, nd = [], [], []
        for user in evaluated:
            relevant = set(X.loc[X.user_id == user, "item_id"])
            items = rec.loc[rec.user_id == user, "item_id"].tolist()
            hit = np.array([1 if i in relevant else 0 for i in items], np.int32)
            prec.append(float(hit.mean()) if hit.size else 0.0)
            rec_.append(float(hit.sum() / max(1, len(relevant))))
            nd.append(ndcg_reference(hit))
        assert abs(res[k]["precision"] - np.mean(prec)) <= 1e-12
        assert abs(res[k]["recall"] - np.mean(rec_)) <= 1e-12
        assert abs(res[k]["ndcg"] - np.mean(nd)) <= 1e-12

    # after a pickle round trip
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.evaluate_topk(X, k=ks, exclude_known=train) == res
    assert m2.rank_items(X, exclude_known=train).equals(got)
