"""CPU tests of the neighbourhood models (ItemItemCF / UserUserCF): the NumPy
restatement of their arithmetic (tests/cf_reference.py) is pinned against the
reference's own classes (tests/golden/cf_*.npz, written by
tools/make_cf_fixture.py), the estimators keep the reference's constructor,
the three mf_cf_* entry points validate their arguments before any device
work, and a pickle carries NumPy and builtins only.  No GPU."""

import ctypes
import pickle
import warnings

import numpy as np
import pandas as pd
import pytest

import cf_reference as cfref
from cf_reference import CASES, load_case
from matrix_factorization import ItemItemCF, UserUserCF

MF_OK, MF_ERR_INVALID, MF_F32, MF_F64 = 0, 1, 0, 1


def internal(case, cls):
    """The fixture's triples and test pairs in the reference's internal ids,
    as (entity, other) for the model's orientation, and the dense matrix."""
    upos = {u: n for n, u in enumerate(case["user_ids"].tolist())}
    ipos = {i: n for n, i in enumerate(case["item_ids"].tolist())}
    u = np.asarray([upos[x] for x in case["train_user"].tolist()])
    i = np.asarray([ipos[x] for x in case["train_item"].tolist()])
    tu = np.asarray([upos[x] for x in case["test_user"].tolist()])
    ti = np.asarray([ipos[x] for x in case["test_item"].tolist()])
    if cls == "itemitemcf":
        R = cfref.dense(i, u, case["train_rating"], len(ipos), len(upos))
        return R, ti, tu
    R = cfref.dense(u, i, case["train_rating"], len(upos), len(ipos))
    return R, tu, ti


# ------------------------------------------------------------ reference pin
@pytest.mark.parametrize("data,cls", CASES)
def test_restatement_reproduces_the_reference(data, cls):
    case = load_case(data, cls)
    R, te, to = internal(case, cls)
    m, w = cfref.stats(R)
    S = cfref.similarity(R, m, w)
    ds = float(np.max(np.abs(S - case["similarity"])))
    dm = float(np.max(np.abs(m - case["means"])))
    print(f"{data}/{cls}: similarity {ds:.3e}, means {dm:.3e}")
    assert ds <= 1e-12 and dm <= 1e-12
    assert np.array_equal(S, S.T)
    nn = int(case["n_neighbors"])
    gm = float(case["global_mean"])
    pred = cfref.predict(R, S, m, te, to, nn, gm)
    pred_b = cfref.predict(R, S, m, te, to, nn, gm,
                           (float(case["min_rating"]), float(case["max_rating"])))
    sure = case["margin"] > 1e-9
    assert sure.sum() >= 0.98 * len(sure)
    dp = float(np.max(np.abs(pred - case["pred"])[sure]))
    db = float(np.max(np.abs(pred_b - case["pred_bounded"])[sure]))
    print(f"{data}/{cls}: predictions {dp:.3e}, bounded {db:.3e} on {int(sure.sum())} pairs")
    assert dp <= 1e-10 and db <= 1e-10
    # the stored margins and denominators are the restatement's too
    mg = np.asarray([cfref.cut_margin(S[e], R[:, o], e, nn) for e, o in zip(te, to)])
    fin = np.isfinite(case["margin"])
    assert np.array_equal(fin, np.isfinite(mg))
    assert np.max(np.abs(mg[fin] - case["margin"][fin]), initial=0.0) <= 1e-12


def test_restatement_edge_cases():
    """Self-exclusion, rating 0 is no neighbour, the lower id wins a tie at the
    cut, negative similarities are taken when the cut needs them, all-zero
    similarities give the mean."""
    # entities 0 and 1 identical, 2 anti-correlated, 3 constant (norm 0)
    R = np.array([[5, 1, 4, 2, 0, 3.0],
                  [5, 1, 4, 2, 0, 3.0],
                  [1, 5, 2, 4, 0, 3.0],
                  [2, 2, 2, 2, 2, 2.0],
                  [4, 2, 5, 1, 3, 0.0]])
    m, w = cfref.stats(R)
    S = cfref.similarity(R, m, w)
    assert w[3] == 0 and not S[3].any() and not S[:, 3].any() and S[3, 3] == 0
    assert S[0, 1] == S[0, 0] and abs(S[0, 1] - 1) < 1e-15 and S[0, 2] < 0
    # target 4, other 0: candidates 0, 1, 2, 3 (4 itself is excluded)
    assert cfref.select(S[4], R[:, 0], 4, 10).tolist() == [0, 1, 2, 3]
    assert cfref.select(S[4], R[:, 0], 4, 1).tolist() == [0]          # tie 0 ~ 1: lower id
    # other 4: entities 0, 1, 2 rated it 0 -> only 3 is a candidate (S = 0) -> the mean
    assert cfref.select(S[4], R[:, 4], 4, 10).tolist() == [3]
    assert cfref.predict(R, S, m, [4], [4], 10, 9.0)[0] == m[4]
    assert cfref.predict(R, S, m, [-1, 2], [0, -1], 10, 9.0).tolist() == [9.0, 9.0]
    # target 2, other 0: similarities 0 (entity 3) > S[2,0] = S[2,1] > S[2,4], all the
    # others negative (2 is 0 reversed, and 4 is closer still to the reverse of 2)
    assert 0 > S[2, 0] == S[2, 1] > S[2, 4]
    assert sorted(cfref.select(S[2], R[:, 0], 2, 3).tolist()) == [0, 1, 3]   # two negative ones
    assert sorted(cfref.select(S[2], R[:, 0], 2, 2).tolist()) == [0, 3]      # tie: the lower id
    assert np.isinf(cfref.cut_margin(S[2], R[:, 0], 2, 4))
    assert cfref.cut_margin(S[4], R[:, 0], 4, 1) == 0.0
    assert cfref.cut_margin(S[2], R[:, 0], 2, 2) == 0.0


# ---------------------------------------------------------------- estimator
def test_constructor_defaults_params_and_clone():
    from sklearn.base import clone

    from matrix_factorization import RecommenderBase

    for cls in (ItemItemCF, UserUserCF):
        m = cls()
        assert isinstance(m, RecommenderBase)
        p = m.get_params()
        assert list(p)[:0] == [] and p == dict(
            min_rating=0, max_rating=5, n_neighbors=50, similarity_metric="cosine", verbose=0,
            device=None, max_similarity_bytes=16 << 30)
        # the reference's positional order comes first
        q = cls(1, 4, 7, "pearson", 1)
        assert (q.min_rating, q.max_rating, q.n_neighbors, q.similarity_metric, q.verbose) == \
            (1, 4, 7, "pearson", 1)
        c = clone(q)
        assert type(c) is cls and c.get_params() == q.get_params()
        assert m.user_item_matrix is None
    assert ItemItemCF().item_similarity_matrix is None and ItemItemCF().item_mean_ratings is None
    assert UserUserCF().user_similarity_matrix is None and UserUserCF().user_mean_ratings is None


def test_unknown_metric_raises_from_fit():
    X = pd.DataFrame({"user_id": [1, 1, 2, 3], "item_id": [5, 6, 5, 7]})
    y = pd.Series([1.0, 2.0, 0.5, 3.0])
    for cls in (ItemItemCF, UserUserCF):
        m = cls(similarity_metric="jaccard")            # accepted by the constructor
        with pytest.raises(ValueError, match="Unknown similarity metric: jaccard"):
            m.fit(X, y)
        with pytest.raises(ValueError, match="n_neighbors"):
            cls(n_neighbors=0).fit(X, y)
        with pytest.raises(ValueError, match="Duplicate"):
            cls().fit(pd.concat([X, X]), pd.concat([y, y]))


def test_similarity_budget_refusal_names_the_size():
    X = pd.DataFrame({"user_id": [1, 1, 2, 3], "item_id": [5, 6, 5, 7]})
    y = pd.Series([1.0, 2.0, 0.5, 3.0])
    with pytest.raises(ValueError, match=r"36 bytes.*max_similarity_bytes=1\b"):
        ItemItemCF(max_similarity_bytes=1).fit(X, y)       # 3 items: 3 * 3 * 4
    with pytest.raises(ValueError, match=r"36 bytes.*max_similarity_bytes=35\b"):
        UserUserCF(max_similarity_bytes=35).fit(X, y)      # 3 users


def test_pickle_state_is_numpy_and_builtins():
    m = ItemItemCF(n_neighbors=3)
    # a fitted model's state, put together without a device
    m.user_id_map = {np.int64(10): 0, np.int64(11): 1}
    m.item_id_map = {"a": 0, "b": 1, "c": 2}
    m.n_users, m.n_items = 2, 3
    m.global_mean = np.float64(2.5)
    m._train_users = np.array([0, 0, 1], np.int32)
    m._train_items = np.array([0, 1, 2], np.int32)
    m._train_ratings = np.array([1.0, 4.0, 2.5])
    m._means = np.array([0.5, 2.0, 1.25])
    m._engine = object()                                  # device state never travels
    state = m.__getstate__()
    assert "_engine" not in state
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
    assert {"user_id_map", "item_id_map", "global_mean", "_train_users", "_train_items",
            "_train_ratings", "_means"} <= set(state)
    m._engine = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)    # no HIP device on this host
        c = pickle.loads(pickle.dumps(m))
    assert c.get_params() == m.get_params() and c.item_id_map == m.item_id_map
    assert c.item_mean_ratings.tolist() == [0.5, 2.0, 1.25]
    assert c.item_mean_ratings.dtype == np.float64
    assert c.user_item_matrix.to_numpy().tolist() == [[1.0, 4.0, 0.0], [0.0, 0.0, 2.5]]
    old = dict(state)
    del old["device"], old["max_similarity_bytes"]
    d = ItemItemCF.__new__(ItemItemCF)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        d.__setstate__(old)
    assert d.device is None and d.max_similarity_bytes == 16 << 30


# ---------------------------------------------------------------------- ABI
_PTR = ctypes.c_void_p(4096)         # non-NULL, never dereferenced: validation comes first


def _stats(lib, **kw):
    a = dict(entity_ptr=_PTR, ratings=_PTR, n_entities=3, n_others=4, dtype=MF_F32, mean=_PTR,
             norm=_PTR)
    a.update(kw)
    return lib.mf_cf_stats(a["entity_ptr"], a["ratings"], a["n_entities"], a["n_others"],
                           a["dtype"], a["mean"], a["norm"], None)


def _similarity(lib, **kw):
    a = dict(entity_ptr=_PTR, other_ids=_PTR, ratings=_PTR, other_ptr=_PTR, entity_ids=_PTR,
             other_ratings=_PTR, n_entities=3, n_others=4, dtype=MF_F32, mean=_PTR, norm=_PTR,
             pass_cols=0, similarity=_PTR)
    a.update(kw)
    return lib.mf_cf_similarity(a["entity_ptr"], a["other_ids"], a["ratings"], a["other_ptr"],
                                a["entity_ids"], a["other_ratings"], a["n_entities"],
                                a["n_others"], a["dtype"], a["mean"], a["norm"], a["pass_cols"],
                                a["similarity"], None)


def _predict(lib, **kw):
    a = dict(entity_ids=_PTR, other_ids=_PTR, n_pairs=5, other_ptr=_PTR, list_entity_ids=_PTR,
             list_ratings=_PTR, similarity=_PTR, mean=_PTR, n_entities=3, n_others=4,
             dtype=MF_F32, n_neighbors=5, out=_PTR)
    a.update(kw)
    return lib.mf_cf_predict(a["entity_ids"], a["other_ids"], a["n_pairs"], a["other_ptr"],
                             a["list_entity_ids"], a["list_ratings"], a["similarity"], a["mean"],
                             a["n_entities"], a["n_others"], a["dtype"], a["n_neighbors"], 2.5,
                             0.0, 5.0, 1, a["out"], None)


@pytest.mark.parametrize("fn,call,bad,name", [
    ("mf_cf_stats", _stats, dict(dtype=MF_F64), "dtype"),
    ("mf_cf_stats", _stats, dict(n_entities=-1), "n_entities"),
    ("mf_cf_stats", _stats, dict(n_others=-1), "n_others"),
    ("mf_cf_stats", _stats, dict(entity_ptr=None), "entity_ptr"),
    ("mf_cf_stats", _stats, dict(mean=None), "mean"),
    ("mf_cf_stats", _stats, dict(norm=None), "norm"),
    ("mf_cf_similarity", _similarity, dict(dtype=MF_F64), "dtype"),
    ("mf_cf_similarity", _similarity, dict(n_entities=-1), "n_entities"),
    ("mf_cf_similarity", _similarity, dict(n_others=-2), "n_others"),
    ("mf_cf_similarity", _similarity, dict(pass_cols=-1), "pass_cols"),
    ("mf_cf_similarity", _similarity, dict(pass_cols=4097), "pass_cols"),
    ("mf_cf_similarity", _similarity, dict(entity_ptr=None), "entity_ptr"),
    ("mf_cf_similarity", _similarity, dict(other_ptr=None), "other_ptr"),
    ("mf_cf_similarity", _similarity, dict(mean=None), "mean"),
    ("mf_cf_similarity", _similarity, dict(norm=None), "norm"),
    ("mf_cf_similarity", _similarity, dict(similarity=None), "similarity"),
    ("mf_cf_predict", _predict, dict(dtype=MF_F64), "dtype"),
    ("mf_cf_predict", _predict, dict(n_neighbors=0), "n_neighbors"),
    ("mf_cf_predict", _predict, dict(n_neighbors=-3), "n_neighbors"),
    ("mf_cf_predict", _predict, dict(n_pairs=-1), "n_pairs"),
    ("mf_cf_predict", _predict, dict(n_pairs=(1 << 25) + 1), "n_pairs"),
    ("mf_cf_predict", _predict, dict(n_entities=-1), "n_entities"),
    ("mf_cf_predict", _predict, dict(n_others=-1), "n_others"),
    ("mf_cf_predict", _predict, dict(entity_ids=None), "entity_ids"),
    ("mf_cf_predict", _predict, dict(other_ids=None), "other_ids"),
    ("mf_cf_predict", _predict, dict(out=None), "out"),
    ("mf_cf_predict", _predict, dict(other_ptr=None), "other_ptr"),
    ("mf_cf_predict", _predict, dict(similarity=None), "similarity"),
    ("mf_cf_predict", _predict, dict(mean=None), "mean")])
def test_entry_points_reject_invalid_arguments(fn, call, bad, name):
    from matrix_factorization import _lib

    assert call(_lib.load(), **bad) == MF_ERR_INVALID
    err = _lib.last_error()
    assert fn in err and name in err


def test_zero_sizes_are_ok_without_a_device():
    from matrix_factorization import _lib

    lib = _lib.load()
    assert _stats(lib, n_entities=0) == MF_OK
    assert _stats(lib, n_entities=0, entity_ptr=None, mean=None, norm=None) == MF_OK
    assert _stats(lib, n_entities=0, dtype=MF_F64) == MF_ERR_INVALID     # checked all the same
    assert _similarity(lib, n_entities=0, similarity=None) == MF_OK
    assert _similarity(lib, n_entities=0, pass_cols=-1) == MF_ERR_INVALID
    assert _predict(lib, n_pairs=0, out=None) == MF_OK
    assert _predict(lib, n_pairs=0, n_neighbors=0) == MF_ERR_INVALID
    assert lib.mf_cf_pass_cols(77, 0) == 77 and lib.mf_cf_pass_cols(77, 32) == 32
    assert lib.mf_cf_pass_cols(5000, 0) == 2048 and lib.mf_cf_pass_cols(5000, 9000) == 0
    assert lib.mf_abi_version() == 1
