"""GPU tests of ContentBasedRecommender: mf_content_profiles /
mf_content_normalize / mf_content_similarity (through
matrix_factorization.content_based.ContentEngine) against the NumPy FP64
restatement tests/content_reference.py (pinned against the reference's class in
tests/test_content_cpu.py), and the estimator end to end on the reference's
fixtures (tools/make_content_fixture.py) in its three scorings.

Bars:
  profiles     1e-12: FP64 sums in the restatement's order.
  similarity   per entry (d + 4) 2^-24 A[a,b] with A = |F^| |F^|^T in FP64: two
               input roundings, a d-term f32 chain, margin for a split k;
               entries with A = 0 exactly 0; S equal to its transpose bit for bit.
  cosine       (d + 4) 2^-24 sum |p^ f^| per pair, the same terms.
  neighbors    tests/test_gpu_cf.py's: 4 n_neighbors max_rating 2^-24 / den + 1e-9,
               leaving out pairs whose cut margin is below 1e-5 or whose denominator
               is below 0.05 -- at most 2 % of the pairs.
Every test prints its measured maximum.
"""

import pickle

import numpy as np
import pandas as pd
import pytest

import cf_reference as cfref
import content_reference as cref
import ranking_reference as rref
from matrix_factorization import ContentBasedRecommender

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 2.0 ** -24


def content_engine(F, has=None):
    from matrix_factorization.content_based import ContentEngine

    return ContentEngine(F, np.ones(len(F), bool) if has is None else has, DEV)


# ---------------------------------------------------------------- profiles
NO_PAIR, ONE_PAIR, LONG, NO_FEATURES, ZERO_SUM, NEGATIVE_SUM = range(6)


def profile_data(d):
    """50 items (7 without features) and 26 users: the six special ones and
    twenty with 1..40 pairs; weights are multiples of 1/2 in [-1, 4.5]."""
    rs = np.random.RandomState(100 + d)
    n_items, n_users = 50, 26
    F = rs.normal(0, 1, (n_items, d))
    has = np.ones(n_items, bool)
    bare = rs.choice(n_items, 7, replace=False)
    has[bare], F[bare] = False, 0.0
    good = np.flatnonzero(has)
    lists = {ONE_PAIR: ([good[3]], [2.0]),
             LONG: (rs.randint(0, n_items, 3000), rs.randint(1, 10, 3000) / 2.0),
             NO_FEATURES: (bare[:4], [1.0, 2.0, 3.0, 4.0]),
             ZERO_SUM: (good[[1, 2, 5]], [2.0, -0.5, -1.5]),
             NEGATIVE_SUM: (good[[4, 6]], [0.5, -1.0])}
    for u in range(6, n_users):
        n = rs.randint(1, 41)
        lists[u] = (rs.choice(n_items, n, replace=False), rs.randint(-2, 10, n) / 2.0)
    u = np.concatenate([np.full(len(v[0]), k) for k, v in lists.items()])
    i = np.concatenate([np.asarray(v[0]) for v in lists.values()])
    w = np.concatenate([np.asarray(v[1], np.float64) for v in lists.values()])
    # the pairs come interleaved; a user's own pairs keep their order
    p = np.argsort(rs.rand(len(u)), kind="stable")
    return F, has, u[p], i[p], w[p], n_users


@pytest.mark.parametrize("d", [1, 19, 130, 1024])
def test_profiles_match_the_restatement(d):
    F, has, u, i, w, n_users = profile_data(d)
    want = cref.profiles(u, i, w, F, has, n_users, 0.0)
    eng = content_engine(F, has)
    got = eng.profiles(u, i, w, n_users).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (n_users, d)
    err = float(np.max(np.abs(got - want)))
    print(f"d={d}: {len(u)} pairs, max |dP| {err:.3e}")
    assert err <= 1e-12
    assert not got[NO_PAIR].any() and not got[NO_FEATURES].any()
    assert np.array_equal(got[ONE_PAIR], F[i[u == ONE_PAIR][0]])       # w F / w
    ws = lambda k: w[(u == k) & has[i]].sum()  # noqa: E731
    assert (u == LONG).sum() == 3000 and ws(ZERO_SUM) == 0 and ws(NEGATIVE_SUM) < 0
    again = eng.profiles(u, i, w, n_users).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))  # two runs, equal bits


# -------------------------------------------------------------- similarity
SIM_SHAPES = [(n, d) for n in (1, 33, 257) for d in (1, 19, 130)] + [(1000, 1024), (3000, 384)]


def check_similarity(S, F, what):
    """S (float32, from the GPU) against the FP64 cosine of F's rows."""
    ref, bar = cref.similarity(F), cref.similarity_bar(F)
    assert S.dtype == np.float32 and S.shape == ref.shape
    err = np.abs(S.astype(np.float64) - ref)
    zero = bar == 0
    worst = float(np.max(np.where(zero, 0.0, err / np.where(zero, 1.0, bar)), initial=0.0))
    print(f"{what}: max |dS| {err.max():.3e}, worst fraction of its bar {worst:.3f}")
    assert not S[zero].any()                                       # exact zeros
    assert worst <= 1.0
    assert np.array_equal(S.view(np.uint32), S.T.view(np.uint32))  # bit for bit


@pytest.mark.parametrize("n,d", SIM_SHAPES)
def test_similarity_matches_the_restatement(n, d):
    rs = np.random.RandomState(7 * n + d)
    F = rs.normal(0, 1, (n, d))
    F[rs.choice(n, 1 + n // 50, replace=False)] = 0.0               # zero rows
    eng = content_engine(F)
    X = eng.normalize(eng.F)
    S = eng.similarity(X).cpu().numpy()
    check_similarity(S, F, f"n={n} d={d}")
    Xh = X.cpu().numpy()
    assert Xh.dtype == np.float32 and Xh.shape == (n, d)
    assert np.max(np.abs(Xh.astype(np.float64) - cref.unit_rows(F))) <= EPS
    zero = ~F.any(axis=1)
    assert zero.any() and not Xh[zero].any() and not S[zero].any() and not S[:, zero].any()
    # a padded stride: the same bits, zeros behind them
    Xp = eng.normalize(eng.F, min(d + 3, 1024)).cpu().numpy()      # (a stride is at most 1024)
    assert np.array_equal(Xp[:, :d].view(np.uint32), Xh.view(np.uint32)) and not Xp[:, d:].any()


# --------------------------------------------------------------- estimator
def fit_case(case, scoring="reference", features=True, **kw):
    X = pd.DataFrame({"user_id": case["train_user"], "item_id": case["train_item"]})
    frame = None
    if features:
        frame = pd.DataFrame(case["feat_values"], columns=case["feat_cols"].tolist())
        frame.insert(0, "item_id", case["feat_item"])
    np.random.seed(3)
    model = ContentBasedRecommender(min_rating=float(case["min_rating"]),
                                    max_rating=float(case["max_rating"]), scoring=scoring,
                                    device=DEV, **kw)
    return model.fit(X, pd.Series(case["train_rating"]), item_features=frame)


def restated(case, model):
    """The restatement in the MODEL's internal ids: F, has, P, R (items x users)."""
    u = np.asarray([model.user_id_map[x] for x in case["train_user"].tolist()])
    i = np.asarray([model.item_id_map[x] for x in case["train_item"].tolist()])
    fi = np.asarray([model.item_id_map.get(x, -1) for x in case["feat_item"].tolist()])
    F, has = cref.feature_matrix(fi, case["feat_values"], model.n_items)
    P = cref.profiles(u, i, case["train_rating"], F, has, model.n_users, float(case["min_rating"]))
    R = cfref.dense(i, u, case["train_rating"], model.n_items, model.n_users)
    return F, has, P, R


def held_pairs(case, model):
    X = pd.DataFrame({"user_id": case["test_user"], "item_id": case["test_item"]})
    tu = np.asarray([model.user_id_map.get(x, -1) for x in case["test_user"].tolist()])
    ti = np.asarray([model.item_id_map.get(x, -1) for x in case["test_item"].tolist()])
    return X, tu, ti


@pytest.mark.parametrize("name", cref.CASES)
def test_default_scoring_matches_the_reference(name):
    case = cref.load_case(name)
    model = fit_case(case)
    assert model.scoring == "reference"
    X, tu, ti = held_pairs(case, model)
    assert ((tu < 0) | (ti < 0)).sum() >= 12
    for bound, ref in ((False, case["pred"]), (True, case["pred_bounded"])):
        got = np.asarray(model.predict(X, bound_ratings=bound))
        err = float(np.max(np.abs(got - ref)))
        print(f"{name} bound={bound}: predict {err:.3e}")
        assert err <= 1e-12
    assert abs(model.global_mean - float(case["global_mean"])) <= 1e-12
    ua = np.asarray([model.user_id_map[x] for x in case["user_ids"].tolist()])
    P = model.user_profile_matrix
    assert P.dtype == np.float64 and P.shape == case["profiles"].shape
    dP = float(np.max(np.abs(P[ua] - case["profiles"])))
    prof = model.user_profiles
    assert sorted(prof) == list(range(model.n_users)) and np.array_equal(prof[5], P[5])
    # the reference's similarity through its row -> item map (first rows: a
    # duplicate's row has no counterpart)
    rows = cref.first_rows(case["sim_item"])
    ia = np.asarray([model.item_id_map[x] for x in case["item_ids"].tolist()])
    at = ia[case["sim_item"][rows]]
    S = model.item_similarity_matrix
    assert S.dtype == np.float32 and S.shape == (model.n_items, model.n_items)
    F, has, _, _ = restated(case, model)
    bar = cref.similarity_bar(F)[np.ix_(at, at)]
    dS = np.abs(S[np.ix_(at, at)].astype(np.float64) - case["similarity"][np.ix_(rows, rows)])
    worst = float(np.max(np.where(bar > 0, dS / np.where(bar > 0, bar, 1.0), 0.0)))
    print(f"{name}: profiles {dP:.3e}, similarity {dS.max():.3e}, worst fraction of its bar "
          f"{worst:.3f}")
    assert dP <= 1e-12 and worst <= 1.0 and not dS[bar == 0].any()
    assert np.array_equal(model.has_features, has) and (~has).any()
    assert not S[~has].any() and not S[:, ~has].any()
    feats = model.item_features
    assert list(feats.columns) == ["item_id"] + case["feat_cols"].tolist()
    assert len(feats) == (np.isin(case["feat_item"], case["item_ids"])).sum()

    # the notebook's sequence; recommend = sorting predict
    user = case["user_ids"][0]
    known = case["train_item"][case["train_user"] == user].tolist()
    rec = model.recommend(user, items_known=known, amount=10)
    cand = [i for i in model.item_id_map if i not in set(known)]
    frame = pd.DataFrame({"user_id": user, "item_id": cand})
    frame["rating_pred"] = model.predict(frame, bound_ratings=False)
    want = frame.sort_values(by="rating_pred", ascending=False).head(10)
    assert rec["item_id"].tolist() == want["item_id"].tolist() and len(rec) == 10
    assert rec["rating_pred"].tolist() == want["rating_pred"].clip(
        lower=model.min_rating, upper=model.max_rating).tolist()
    with pytest.raises(ValueError, match=r'scoring="cosine" or scoring="neighbors"'):
        model.recommend_batch([user])


def test_without_item_features_the_profile_is_the_users_mean():
    case = cref.load_case("genres")
    model = fit_case(case, features=False)
    X, tu, ti = held_pairs(case, model)
    got = np.asarray(model.predict(X, bound_ratings=False))
    means = pd.Series(case["train_rating"]).groupby(case["train_user"]).mean()
    known = (tu >= 0) & (ti >= 0)
    want = np.where(known, means.reindex(case["test_user"]).to_numpy(), model.global_mean)
    assert np.max(np.abs(got - want)) <= 1e-12
    assert model.item_features is None and model.item_similarity_matrix is None
    assert model.user_profile_matrix.shape == (model.n_users, 1)
    assert isinstance(model.user_profiles[0], float)


def wide_case():
    """The embed fixture's triples with d = 130 Gaussian features."""
    case = dict(cref.load_case("embed"))
    rs = np.random.RandomState(130)
    items = case["item_ids"][:-2]                        # two items without features
    case["feat_item"] = items
    case["feat_values"] = rs.normal(0, 1, (len(items), 130))
    case["feat_cols"] = np.asarray([f"w{c:03d}" for c in range(130)])
    return case


def all_scores(model, users):
    """predict(bound_ratings=False) of every internal item for the users."""
    items = list(model.item_id_map)
    frame = pd.DataFrame({"user_id": np.repeat(np.asarray(users, dtype=object), len(items)),
                          "item_id": items * len(users)})
    return np.asarray(model.predict(frame, bound_ratings=False)).reshape(len(users), len(items))


def check_ranking(case, model):
    """recommend_batch = a stable sort of predict's scores; rank_items =
    ranking_reference on them; exclusions are the users' training pairs."""
    users = case["user_ids"][[0, 3, 17, 31, 44]].tolist()
    scores = all_scores(model, users)
    known = pd.DataFrame({"user_id": case["train_user"], "item_id": case["train_item"]})
    items = np.asarray(list(model.item_id_map), dtype=object)
    rec = model.recommend_batch(users, amount=10, exclude_known=known, bound_ratings=False)
    ex = [np.asarray([model.item_id_map[i] for i in known["item_id"][known["user_id"] == u]])
          for u in users]
    for q, u in enumerate(users):
        cand = np.setdiff1d(np.arange(model.n_items), ex[q])
        top = cand[np.argsort(-scores[q, cand], kind="stable")][:10]
        got = rec[rec["user_id"] == u]
        assert got["item_id"].tolist() == items[top].tolist()
        assert got["rating_pred"].tolist() == scores[q, top].tolist()        # the same bits
    held = pd.DataFrame({"user_id": np.repeat(np.asarray(users, dtype=object), 6),
                         "item_id": np.concatenate([items[np.setdiff1d(
                             np.arange(model.n_items), e)[[0, 5, 9, 20, 33, 40]]] for e in ex])})
    got = model.rank_items(held, exclude_known=known)
    ex_ptr = np.concatenate([[0], np.cumsum([len(e) for e in ex])])
    tgt = np.asarray([model.item_id_map[i] for i in held["item_id"]])
    ranks, ncand = rref.ranks_from_scores(scores, np.arange(0, 6 * len(users) + 1, 6), tgt,
                                          ex_ptr, np.concatenate(ex))
    assert got["rank"].tolist() == ranks.tolist() and (ranks >= 0).all()
    assert got["n_candidates"].tolist() == np.repeat(ncand, 6).tolist()
    res = model.evaluate_topk(held, k=10, exclude_known=known)
    assert res["n_users_evaluated"] == len(users) and 0.0 <= res["auc"] <= 1.0


@pytest.mark.parametrize("name", ["genres", "wide"])
def test_cosine_scoring(name):
    case = cref.load_case("genres") if name == "genres" else wide_case()
    model = fit_case(case, "cosine")
    F, has, P, _ = restated(case, model)
    d = F.shape[1]
    assert d == (19 if name == "genres" else 130)
    eng = model._ranking_backend()
    assert eng.k == (d + 3) // 4 * 4 and eng.dtype == "float32"
    X, tu, ti = held_pairs(case, model)
    got = np.asarray(model.predict(X, bound_ratings=False))
    want, mag = cref.score_cosine(P, F, tu, ti)
    bar = (d + 4) * EPS * mag
    err = np.abs(got - want)
    worst = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), 0.0)))
    print(f"{name} d={d}: max |dcos| {err.max():.3e}, worst fraction of its bar {worst:.3f}")
    assert worst <= 1.0 and not got[bar == 0].any()
    assert ((tu < 0) | (ti < 0)).sum() >= 12 and (np.abs(got) <= 1 + 1e-6).all()
    check_ranking(case, model)


def test_neighbors_scoring():
    case = cref.load_case("embed")
    nn = 10
    model = fit_case(case, "neighbors", n_neighbors=nn)
    F, has, _, R = restated(case, model)
    S = cref.similarity(F)
    m, _ = cfref.stats(R)
    X, tu, ti = held_pairs(case, model)
    gm, lo, hi = float(model.global_mean), float(case["min_rating"]), float(case["max_rating"])
    known = (tu >= 0) & (ti >= 0)
    margin = np.full(len(tu), np.inf)
    den = np.full(len(tu), np.inf)
    for p in np.flatnonzero(known):
        margin[p] = cfref.cut_margin(S[ti[p]], R[:, tu[p]], ti[p], nn)
        keep = cfref.select(S[ti[p]], R[:, tu[p]], ti[p], nn)
        den[p] = np.abs(S[ti[p], keep]).sum()
    use = (margin >= 1e-5) & (den >= 0.05)
    print(f"{int((~use).sum())} of {len(use)} pairs left out")
    assert (~use).sum() <= 0.02 * len(use)
    with np.errstate(divide="ignore"):                 # den = 0: left out above
        tol = 4 * nn * hi * EPS / den + 1e-9
    for bound in (False, True):
        got = np.asarray(model.predict(X, bound_ratings=bound))
        want = cfref.predict(R, S, m, ti, tu, nn, gm, (lo, hi) if bound else None)
        worst = float(np.max((np.abs(got - want) / tol)[use]))
        print(f"bound={bound}: {int(use.sum())} pairs, max |dp| "
              f"{np.max(np.abs(got - want)[use]):.3e}, worst fraction of its bar {worst:.3f}")
        assert worst <= 1.0
        assert (got[~known] == gm).all()
    dS = np.abs(model.item_similarity_matrix.astype(np.float64) - S)
    assert (dS <= cref.similarity_bar(F)).all()
    check_ranking(case, model)


def test_pickle_predicts_the_same_bits():
    case = cref.load_case("embed")
    X, _, _ = held_pairs(case, fit_case(case))
    for scoring in ("reference", "cosine", "neighbors"):
        model = fit_case(case, scoring, n_neighbors=10)
        before = model.predict(X, bound_ratings=False)
        loaded = pickle.loads(pickle.dumps(model))
        assert not set(ContentBasedRecommender._DEVICE_STATE) & set(loaded.__dict__)
        assert loaded.predict(X, bound_ratings=False) == before
        assert np.array_equal(loaded.item_similarity_matrix, model.item_similarity_matrix)
    with pytest.raises(ValueError, match="max_similarity_bytes=1"):
        fit_case(case, "neighbors", max_similarity_bytes=1)
    model = fit_case(case, max_similarity_bytes=1)
    with pytest.raises(ValueError, match="max_similarity_bytes=1"):
        model.item_similarity_matrix
