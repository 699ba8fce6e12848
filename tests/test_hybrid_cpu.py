"""CPU tests of HybridRecommender: the NumPy restatement of its arithmetic
(tests/hybrid_reference.py) is pinned against the reference's own
``evaluate_hybrid`` (tests/golden/hybrid_small.npz, written by
tools/make_hybrid_fixture.py), mf_hybrid_rerank validates its arguments before
any device work, the constructor and ``fit`` refuse what they must, and a
pickle carries NumPy and builtins only.  No GPU."""

import ctypes
import pickle
import warnings

import numpy as np
import pandas as pd
import pytest

import hybrid_reference as href
from matrix_factorization import HybridRecommender, KernelMF, _lib

MF_OK, MF_ERR_INVALID, MF_F32, MF_F64 = 0, 1, 0, 1


@pytest.fixture(scope="module")
def fx():
    return href.load_fixture()


# ------------------------------------------------------------ reference pin
def test_restatement_reproduces_the_reference(fx):
    k, ck, mp = int(fx["k"]), int(fx["candidate_k"]), int(fx["min_profile_items"])
    assert (len(fx["users"]), len(fx["items"]), fx["embeddings"].shape) == (60, 150, (147, 24))
    assert fx["embeddings"].dtype == np.float32 and (ck, k, mp) == (40, 10, 2)
    for alpha, want in zip(fx["alphas"], fx["metrics"]):
        detail = {}
        got = href.evaluate(fx, float(alpha), True, k, ck, mp, detail)
        print(f"alpha {alpha}: restatement {got}, reference {want.tolist()}")
        assert max(abs(a - b) for a, b in zip(got, want)) <= 1e-12
        assert sorted(detail) == fx["cand_user"].tolist()
        for j, u in enumerate(fx["cand_user"]):
            rec = fx["cand_rows"][fx["cand_ptr"][j]:fx["cand_ptr"][j + 1]]
            assert np.array_equal(detail[int(u)]["kept"], rec)
    got = href.evaluate(fx, 0.7, False, k, ck, mp)
    assert max(abs(a - b) for a, b in zip(got, fx["metrics_no_model"])) <= 1e-12
    # the drop after the retrieval shortens lists: the fixture exercises it
    assert (np.diff(fx["cand_ptr"]) < ck).any() and (np.diff(fx["cand_ptr"]) > 0).all()


def test_restatement_edge_cases():
    f = lambda *v: np.asarray(v, np.float32)  # noqa: E731
    assert href.minmax(f(2, 2, 2)).tolist() == [0, 0, 0]
    assert href.minmax(f(5)).tolist() == [0]
    assert href.minmax(f(1, 3, 2)).tolist() == [0, 1, 0.5]
    assert np.isnan(href.minmax(f(1, np.nan, 2))).all()
    # stable ties, NaN last, the drop, -1 padding inside the candidates
    rows, sc, mo, si = href.rerank_one([4, -1, 2, 9, 7, 3], f(.9, .8, .7, .6, .5, .4),
                                       lambda r: np.zeros(len(r)), 9, {7}, 1.0)
    assert rows.tolist() == [4, 2, 3] and sc.tolist() == [0, 0, 0]
    assert si.tolist() == f(.9, .7, .4).tolist()
    rows, sc, _, _ = href.rerank_one([0, 1, 2], f(.1, .2, .3), lambda r: f(1, np.nan, 2), 3,
                                     set(), 0.5)
    assert rows.tolist() == [0, 1, 2] and np.isnan(sc).all()
    out = href.rerank([[0, 1, 2]], [f(.1, .3, .2)], lambda q, r: np.zeros(len(r)), 3, [{0}], 0.0, 3)
    assert out[0].tolist() == [[1, 2, -1]] and out[4].tolist() == [2]
    assert out[1][0, :2].tolist() == [1, 0] and np.isnan(out[1][0, 2])
    assert href.same_bits(f(1, np.nan), f(1, np.nan)) and not href.same_bits(f(0.0), f(-0.0))


# ---------------------------------------------------------------------- ABI
_PTR = ctypes.c_void_p(4096)         # non-NULL, never dereferenced: validation comes first


def _rerank(lib, **kw):
    a = dict(n_query=3, n_cand=40, n_rows=100, n_items=90, n_factors=16, kernel=0, dtype=MF_F32,
             alpha=0.7, amount=10)
    a.update(kw)
    return lib.mf_hybrid_rerank(
        _PTR, a["n_query"], _PTR, _PTR, a["n_cand"], _PTR, a["n_rows"], 3.0, _PTR, _PTR, _PTR,
        _PTR, a["n_items"], a["n_factors"], a["kernel"], a["dtype"], 0.0, 0.0, 5.0, _PTR, _PTR,
        a["alpha"], a["amount"], None, _PTR, _PTR, _PTR, _PTR, _PTR, None)


def test_entry_points_are_exported():
    lib = _lib.load()
    assert lib.mf_abi_version() == 1
    assert "mf_hybrid_rerank" in _lib.SIGNATURES
    assert lib.mf_hybrid_rerank_workspace_bytes(1024, 2048) >= 0
    assert len(_lib.SIGNATURES["mf_hybrid_rerank"][1]) == 30


@pytest.mark.parametrize("kw,name", [
    (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"),
    (dict(kernel=3), "kernel"), (dict(kernel=-1), "kernel"),
    (dict(n_factors=-1), "n_factors"), (dict(n_factors=1025), "n_factors"),
    (dict(n_cand=0), "n_cand"), (dict(n_cand=2049), "n_cand"), (dict(n_cand=-3), "n_cand"),
    (dict(amount=-1), "amount"), (dict(amount=41), "amount"),
    (dict(alpha=float("nan")), "alpha"), (dict(alpha=float("inf")), "alpha"),
    (dict(n_query=-1), "n_query"), (dict(n_rows=-1), "n_rows"), (dict(n_items=-1), "n_items"),
])
def test_invalid_arguments_are_refused_without_a_device(kw, name):
    lib = _lib.load()
    assert _rerank(lib, **kw) == MF_ERR_INVALID
    msg = _lib.last_error()
    assert msg.startswith("mf_hybrid_rerank: " + name + "="), msg


def test_zero_queries_return_ok_without_a_device():
    assert _rerank(_lib.load(), n_query=0) == MF_OK
    # ... but only after the other arguments were checked
    assert _rerank(_lib.load(), n_query=0, n_cand=0) == MF_ERR_INVALID


# ---------------------------------------------------------------- estimator
X3 = pd.DataFrame({"user_id": [1, 1, 2], "item_id": [5, 6, 5]})
E3 = pd.DataFrame({"item_id": [5, 6, 7], "a": [1.0, 0.0, 1.0], "b": [0.0, 1.0, 1.0]})


def test_constructor_refusals():
    m = HybridRecommender()
    assert (m.model, m.alpha, m.candidate_k, m.min_profile_items, m.normalize_items, m.device) \
        == (None, 0.7, 200, 1, True, None)
    assert m.user_profiles is None and m.index_item_ids is None
    for bad in (0, 2049, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="candidate_k"):
            HybridRecommender(candidate_k=bad)
    for bad in (-0.01, 1.01, float("nan"), "x", None):
        with pytest.raises(ValueError, match="alpha"):
            HybridRecommender(alpha=bad)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="min_profile_items"):
            HybridRecommender(min_profile_items=bad)
    with pytest.raises(ValueError, match="model must be a KernelMF-family"):
        HybridRecommender(model=object())
    assert HybridRecommender(alpha=0, candidate_k=2048).alpha == 0
    assert HybridRecommender(alpha=1, candidate_k=1).candidate_k == 1


def test_fit_refusals_come_before_any_device_work():
    with pytest.raises(ValueError, match="model is not fitted"):
        HybridRecommender(model=KernelMF(n_factors=4)).fit(X3, E3)
    m = HybridRecommender()
    m.candidate_k = 0                                      # set after construction
    with pytest.raises(ValueError, match="candidate_k"):
        m.fit(X3, E3)
    with pytest.raises(ValueError, match="X must contain 'item_id' column"):
        HybridRecommender().fit(X3.drop(columns="item_id"), E3)
    with pytest.raises(ValueError, match="must contain 'item_id' column"):
        HybridRecommender().fit(X3, E3.drop(columns="item_id"))
    bad = E3.copy()
    bad.loc[1, "b"] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        HybridRecommender().fit(X3, bad)
    with pytest.raises(ValueError, match="numeric"):
        HybridRecommender().fit(X3, E3.assign(title=["x", "y", "z"]))
    with pytest.raises(ValueError, match="d = 0 numeric columns"):
        HybridRecommender().fit(X3, E3[["item_id"]])
    kmax = _lib.load().mf_max_factors()
    wide = pd.DataFrame(np.ones((3, kmax + 1)), columns=[f"c{c}" for c in range(kmax + 1)])
    wide.insert(0, "item_id", [5, 6, 7])
    with pytest.raises(ValueError, match=rf"d = {kmax + 1}.*mf_max_factors\(\) = {kmax}"):
        HybridRecommender().fit(X3, wide)
    with pytest.raises(AttributeError, match="not fitted"):
        HybridRecommender().recommend_batch([1])


def fitted_state(model=None):
    """A fitted recommender's state, put together without a device."""
    m = HybridRecommender(model=model, alpha=0.25, candidate_k=2, min_profile_items=1)
    m._index_ids = np.asarray(["a", "b", "c"])
    m._E = np.eye(3, 2, dtype=np.float32)
    m._user_ids = np.asarray([10, 11], np.int64)
    m._hist_ptr = np.asarray([0, 2, 2], np.int64)
    m._hist_rows = np.asarray([0, 1], np.int32)
    m._has_profile = np.asarray([True, False])
    m._profiles = np.asarray([[0.6, 0.8], [0.0, 0.0]], np.float32)
    return m


def test_pickle_state_is_numpy_and_builtins():
    m = fitted_state()
    assert m._user_codes([11, 12, 10]).tolist() == [1, -1, 0]      # builds the lookups
    assert m._index_rows(["c", "zz"]).tolist() == [2, -1]
    m._engine = m._row_item = object()                             # device state never travels
    state = m.__getstate__()
    assert not set(HybridRecommender._DEVICE_STATE) & set(state)
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
    del m._engine, m._row_item
    with pytest.warns(RuntimeWarning, match="HybridRecommender loaded, but no HIP device"):
        c = pickle.loads(pickle.dumps(m))
    assert (c.alpha, c.candidate_k, c.model) == (0.25, 2, None)
    assert c.index_item_ids.tolist() == ["a", "b", "c"] and c.user_ids.tolist() == [10, 11]
    assert np.array_equal(c.user_profiles, m._profiles) and c.user_profiles.dtype == np.float32
    assert np.array_equal(c.item_embeddings, m._E) and c.has_profile.tolist() == [True, False]
    pos, codes = c._queries([11, 10, 99, 10])
    assert pos.tolist() == [1, 3] and codes.tolist() == [0, 0]
    # the model travels by its own NumPy-only state
    km = KernelMF(n_factors=2)
    km.user_features = np.zeros((2, 2))
    km.item_id_map = {"a": 0}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        c2 = pickle.loads(pickle.dumps(fitted_state(km)))
    assert isinstance(c2.model, KernelMF) and c2.model.item_id_map == {"a": 0}
