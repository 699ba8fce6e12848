"""CPU tests of ContentBasedRecommender: the NumPy restatement of its
arithmetic (tests/content_reference.py) is pinned against the reference's own
class (tests/golden/content_*.npz, written by tools/make_content_fixture.py),
the three mf_content_* entry points validate their arguments before any device
work, ``fit`` refuses what it must before touching a device, and a pickle
carries NumPy and builtins only.  No GPU."""

import ctypes
import pickle
import warnings

import numpy as np
import pandas as pd
import pytest

import content_reference as cref
from matrix_factorization import ContentBasedRecommender

MF_OK, MF_ERR_INVALID, MF_F32, MF_F64 = 0, 1, 0, 1


# ------------------------------------------------------------ reference pin
@pytest.mark.parametrize("name", cref.CASES)
def test_restatement_reproduces_the_reference(name):
    case = cref.load_case(name)
    u, i, r, fi, tu, ti = cref.internal(case)
    n_users, n_items = len(case["user_ids"]), len(case["item_ids"])
    lo, hi, gm = float(case["min_rating"]), float(case["max_rating"]), float(case["global_mean"])
    F, has = cref.feature_matrix(fi, case["feat_values"], n_items)
    assert (~has).sum() >= 1 and (fi < 0).sum() == (2 if name == "genres" else 0)
    P = cref.profiles(u, i, r, F, has, n_users, lo)
    dP = float(np.max(np.abs(P - case["profiles"])))
    rows = cref.first_rows(case["sim_item"])
    it = case["sim_item"][rows]
    S = cref.similarity(F)
    dS = float(np.max(np.abs(S[np.ix_(it, it)] - case["similarity"][np.ix_(rows, rows)])))
    pred = cref.score_reference(P, tu, ti, gm)
    pred_b = cref.score_reference(P, tu, ti, gm, (lo, hi))
    dp = float(np.max(np.abs(pred - case["pred"])))
    db = float(np.max(np.abs(pred_b - case["pred_bounded"])))
    print(f"{name}: profiles {dP:.3e}, similarity {dS:.3e}, predict {dp:.3e}, bounded {db:.3e}")
    assert dP <= 1e-12 and dS <= 1e-12 and dp <= 1e-12 and db <= 1e-12
    assert ((tu < 0) | (ti < 0)).sum() >= 12
    # items without features: zero rows and columns, the diagonal included
    assert not S[~has].any() and not S[:, ~has].any()


def test_restatement_edge_cases():
    F = np.array([[1.0, 0, 1], [0, 0, 0], [2, 2, 0], [9, 9, 9]])
    has = np.array([True, True, True, False])
    # user 0: items 0 and 2; user 1: only the item without features; user 2: nothing;
    # user 3: weights sum to 0 (undivided); user 4: a negative sum (undivided)
    u = np.array([0, 0, 1, 3, 3, 4])
    i = np.array([0, 2, 3, 0, 2, 2])
    r = np.array([3.0, 2.0, 5.0, 2.0, 0.0, 0.5])
    P = cref.profiles(u, i, r, F, has, 5, 1.0)
    assert P[0].tolist() == [(2 * 1 + 1 * 2) / 3, 2 / 3, 2 / 3]
    assert not P[1].any() and not P[2].any()
    assert P[3].tolist() == [1 * 1 - 1 * 2, -2, 1]
    assert P[4].tolist() == [-1, -1, 0]
    S = cref.similarity(F[:3])
    assert S[1].tolist() == [0, 0, 0] and S[1, 1] == 0 and abs(S[0, 2] - 0.5) < 1e-15
    assert cref.score_reference(P, [0, -1, 2], [1, 0, -1], 9.0).tolist() == [
        np.mean(P[0]), 9.0, 9.0]
    assert cref.score_reference(P[:, :0], [0], [1], 9.0).tolist() == [9.0]
    assert cref.score_cosine(P, F, [1, -1], [0, 0])[0].tolist() == [0.0, 0.0]


# ---------------------------------------------------------------- estimator
def test_constructor_defaults_params_and_clone():
    from sklearn.base import clone

    from matrix_factorization import RecommenderBase

    m = ContentBasedRecommender()
    assert isinstance(m, RecommenderBase)
    assert m.get_params() == dict(min_rating=0, max_rating=5, verbose=0, scoring="reference",
                                  n_neighbors=50, device=None, max_similarity_bytes=16 << 30)
    q = ContentBasedRecommender(1, 4, 1)                   # the reference's positional order
    assert (q.min_rating, q.max_rating, q.verbose) == (1, 4, 1)
    c = clone(ContentBasedRecommender(scoring="cosine", n_neighbors=7))
    assert c.scoring == "cosine" and c.n_neighbors == 7
    assert m.item_features is None and m.user_profiles == {} and m.user_profile_matrix is None
    assert m.item_similarity_matrix is None


X4 = pd.DataFrame({"user_id": [1, 1, 2, 3], "item_id": [5, 6, 5, 7]})
Y4 = pd.Series([1.0, 2.0, 0.5, 3.0])
F4 = pd.DataFrame({"item_id": [5, 6, 7], "a": [1.0, 0.0, 1.0], "b": [0.0, 1.0, 1.0]})


def test_fit_refusals_come_before_any_device_work():
    with pytest.raises(ValueError, match="Unknown scoring: 'tfidf'"):
        ContentBasedRecommender(scoring="tfidf").fit(X4, Y4, item_features=F4)
    with pytest.raises(ValueError, match="n_neighbors"):
        ContentBasedRecommender(scoring="neighbors", n_neighbors=0).fit(X4, Y4, item_features=F4)
    with pytest.raises(ValueError, match="item_features must contain 'item_id' column"):
        ContentBasedRecommender().fit(X4, Y4, item_features=F4.drop(columns="item_id"))
    bad = F4.copy()
    bad.loc[1, "b"] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        ContentBasedRecommender().fit(X4, Y4, item_features=bad)
    bad.loc[1, "b"] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        ContentBasedRecommender().fit(X4, Y4, item_features=bad)
    text = F4.assign(title=["x", "y", "z"])
    with pytest.raises(ValueError, match="numeric"):
        ContentBasedRecommender().fit(X4, Y4, item_features=text)
    from matrix_factorization import _lib

    kmax = _lib.load().mf_max_factors()
    wide = pd.DataFrame(np.ones((3, kmax + 1)), columns=[f"c{c}" for c in range(kmax + 1)])
    wide.insert(0, "item_id", [5, 6, 7])
    with pytest.raises(ValueError, match=rf"d = {kmax + 1}.*mf_max_factors\(\) = {kmax}"):
        ContentBasedRecommender(scoring="cosine").fit(X4, Y4, item_features=wide)
    for scoring in ("cosine", "neighbors"):
        with pytest.raises(ValueError, match="needs item_features"):
            ContentBasedRecommender(scoring=scoring).fit(X4, Y4)
    with pytest.raises(ValueError, match=r"36 bytes.*max_similarity_bytes=35\b"):
        ContentBasedRecommender(scoring="neighbors", max_similarity_bytes=35).fit(
            X4, Y4, item_features=F4)                      # 3 items: 3 * 3 * 4
    with pytest.raises(ValueError, match="Duplicate"):
        ContentBasedRecommender().fit(pd.concat([X4, X4]), pd.concat([Y4, Y4]), item_features=F4)


def fitted_state(scoring="reference", **kw):
    """A fitted model's state, put together without a device."""
    m = ContentBasedRecommender(min_rating=1, scoring=scoring, **kw)
    m.user_id_map = {np.int64(10): 0, np.int64(11): 1}
    m.item_id_map = {"a": 0, "b": 1, "c": 2}
    m.n_users, m.n_items = 2, 3
    m.global_mean = np.float64(2.5)
    m._train_users = np.array([0, 0, 1], np.int32)
    m._train_items = np.array([0, 1, 2], np.int32)
    m._train_ratings = np.array([1.0, 4.0, 2.5])
    m._feature_cols = ["g0", "g1"]
    m._feat_ids = np.array([0, 2, 0], np.int64)
    m._feat_values = np.array([[1.0, 0.0], [1.0, 1.0], [5.0, 5.0]])
    m._F = np.array([[1.0, 0.0], [0.0, 0.0], [1.0, 1.0]])
    m._has = np.array([True, False, True])
    m._profiles = np.array([[0.0, 0.0], [1.0, 1.0]])
    m._profile_means = np.array([0.0, 1.0])
    return m


def test_pickle_state_is_numpy_and_builtins():
    m = fitted_state()
    for key in ContentBasedRecommender._DEVICE_STATE:
        setattr(m, key, object())                          # device state never travels
    state = m.__getstate__()
    assert not set(ContentBasedRecommender._DEVICE_STATE) & set(state)
    ok = (np.ndarray, np.generic, dict, list, tuple, str, int, float, bool, type(None))

    def walk(v):
        assert isinstance(v, ok), type(v)
        if isinstance(v, dict):
            for k, x in v.items():
                walk(k), walk(x)
        elif isinstance(v, (list, tuple)):
            for x in v:
                walk(x)
        elif isinstance(v, np.ndarray):
            assert v.dtype != object

    walk(state)
    for key in ContentBasedRecommender._DEVICE_STATE:
        delattr(m, key)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)    # no HIP device on this host
        c = pickle.loads(pickle.dumps(m))
    assert c.get_params() == m.get_params() and c.item_id_map == m.item_id_map
    assert np.array_equal(c.user_profile_matrix, m._profiles)
    assert c.user_profile_matrix.dtype == np.float64
    assert sorted(c.user_profiles) == [0, 1] and c.user_profiles[1].tolist() == [1.0, 1.0]
    frame = c.item_features
    assert list(frame.columns) == ["item_id", "g0", "g1"]
    assert frame["item_id"].tolist() == [0, 2, 0] and frame["g1"].tolist() == [0.0, 1.0, 5.0]
    assert c.has_features.tolist() == [True, False, True]
    # the reference scoring needs no device: mean(P_u), the global mean for unknown ids
    X = pd.DataFrame({"user_id": [10, 11, 11, 12], "item_id": ["a", "c", "zz", "a"]})
    assert c.predict(X, bound_ratings=False) == [0.0, 1.0, 2.5, 2.5]
    assert c.predict(X) == [1.0, 1.0, 2.5, 2.5]
    with pytest.raises(ValueError, match=r'scoring="cosine" or scoring="neighbors"'):
        c.recommend_batch([10])
    with pytest.raises(ValueError, match="cosine"):
        c.rank_items(X)
    with pytest.raises(ValueError, match="neighbors"):
        c.evaluate_topk(X)
    # the similarity is refused beyond the budget on the first read, before any device work
    c.max_similarity_bytes = 35
    with pytest.raises(ValueError, match=r"36 bytes.*max_similarity_bytes=35\b"):
        c.item_similarity_matrix
    old = dict(state)
    for key in ("device", "scoring", "n_neighbors", "max_similarity_bytes"):
        del old[key]
    d = ContentBasedRecommender.__new__(ContentBasedRecommender)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        d.__setstate__(old)
    assert (d.device, d.scoring, d.n_neighbors, d.max_similarity_bytes) == \
        (None, "reference", 50, 16 << 30)


# ---------------------------------------------------------------------- ABI
_PTR = ctypes.c_void_p(4096)         # non-NULL, never dereferenced: validation comes first


def _profiles(lib, **kw):
    a = dict(user_ptr=_PTR, item_ids=_PTR, weights=_PTR, features=_PTR, has_features=_PTR,
             n_users=3, n_items=4, d=5, dtype=MF_F64, profiles=_PTR)
    a.update(kw)
    return lib.mf_content_profiles(a["user_ptr"], a["item_ids"], a["weights"], a["features"],
                                   a["has_features"], a["n_users"], a["n_items"], a["d"],
                                   a["dtype"], a["profiles"], None)


def _normalize(lib, **kw):
    a = dict(rows=_PTR, n=3, d=5, out_stride=0, dtype=MF_F64, out=_PTR)
    a.update(kw)
    return lib.mf_content_normalize(a["rows"], a["n"], a["d"], a["out_stride"], a["dtype"],
                                    a["out"], None)


def _similarity(lib, **kw):
    a = dict(rows=_PTR, n=3, d=5, dtype=MF_F32, similarity=_PTR)
    a.update(kw)
    return lib.mf_content_similarity(a["rows"], a["n"], a["d"], a["dtype"], a["similarity"], None)


@pytest.mark.parametrize("fn,call,bad,name", [
    ("mf_content_profiles", _profiles, dict(dtype=MF_F32), "dtype"),
    ("mf_content_profiles", _profiles, dict(n_users=-1), "n_users"),
    ("mf_content_profiles", _profiles, dict(n_items=-1), "n_items"),
    ("mf_content_profiles", _profiles, dict(d=-1), "d="),
    ("mf_content_profiles", _profiles, dict(d=1025), "d="),
    ("mf_content_profiles", _profiles, dict(user_ptr=None), "user_ptr"),
    ("mf_content_profiles", _profiles, dict(profiles=None), "profiles"),
    ("mf_content_profiles", _profiles, dict(features=None), "features"),
    ("mf_content_profiles", _profiles, dict(has_features=None), "has_features"),
    ("mf_content_normalize", _normalize, dict(dtype=MF_F32), "dtype"),
    ("mf_content_normalize", _normalize, dict(n=-1), "n="),
    ("mf_content_normalize", _normalize, dict(n=1 << 31), "n="),
    ("mf_content_normalize", _normalize, dict(d=-2), "d="),
    ("mf_content_normalize", _normalize, dict(d=1025), "d="),
    ("mf_content_normalize", _normalize, dict(out_stride=4), "out_stride"),
    ("mf_content_normalize", _normalize, dict(out_stride=1028), "out_stride"),
    ("mf_content_normalize", _normalize, dict(rows=None), "rows"),
    ("mf_content_normalize", _normalize, dict(out=None), "out"),
    ("mf_content_similarity", _similarity, dict(dtype=MF_F64), "dtype"),
    ("mf_content_similarity", _similarity, dict(n=-1), "n="),
    ("mf_content_similarity", _similarity, dict(d=-1), "d="),
    ("mf_content_similarity", _similarity, dict(d=1025), "d="),
    ("mf_content_similarity", _similarity, dict(rows=None), "rows"),
    ("mf_content_similarity", _similarity, dict(similarity=None), "similarity")])
def test_entry_points_reject_invalid_arguments(fn, call, bad, name):
    from matrix_factorization import _lib

    assert call(_lib.load(), **bad) == MF_ERR_INVALID
    err = _lib.last_error()
    assert fn in err and name in err


def test_zero_sizes_are_ok_without_a_device():
    from matrix_factorization import _lib

    lib = _lib.load()
    assert _profiles(lib, n_users=0) == MF_OK
    assert _profiles(lib, n_users=0, user_ptr=None, profiles=None, features=None) == MF_OK
    assert _profiles(lib, d=0, profiles=None) == MF_OK
    assert _profiles(lib, n_users=0, dtype=MF_F32) == MF_ERR_INVALID     # checked all the same
    assert _normalize(lib, n=0, rows=None, out=None) == MF_OK
    assert _normalize(lib, n=0, d=1025) == MF_ERR_INVALID
    assert _similarity(lib, n=0, rows=None, similarity=None) == MF_OK
    assert _similarity(lib, n=0, dtype=MF_F64) == MF_ERR_INVALID
    assert lib.mf_abi_version() == 1
