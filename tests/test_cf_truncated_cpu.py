"""CPU tests of the stored-neighbours (top-M) neighbourhood model: the NumPy
restatement (tests/cf_truncated_reference.py) against the dense one, the new
entry points' argument validation before any device work (mf_cf_neighbours,
mf_cf_predict_nbr, mf_cf_scores_nbr, mf_cf_topk_nbr, mf_cf_rank_nbr), and the
estimators' ``stored_neighbors`` parameter.  No GPU."""

import ctypes
import pickle
import warnings

import numpy as np
import pandas as pd
import pytest

import cf_reference as cfref
import cf_truncated_reference as tref
from cf_reference import load_case
from matrix_factorization import ItemItemCF, UserUserCF
from test_cf_cpu import internal

MF_OK, MF_ERR_INVALID, MF_F32, MF_F64 = 0, 1, 0, 1
OTHER, ENTITY = 0, 1
_PTR = ctypes.c_void_p(4096)         # non-NULL, never dereferenced: validation comes first


# ------------------------------------------------------------- restatement
@pytest.mark.parametrize("cls", ["itemitemcf", "userusercf"])
def test_every_neighbour_stored_is_the_dense_restatement(cls):
    case = load_case("small", cls)
    R, te, to = internal(case, cls)
    n = R.shape[0]
    m, w = cfref.stats(R)
    S = cfref.similarity(R, m, w)
    nn, gm = int(case["n_neighbors"]), float(case["global_mean"])
    te, to = np.concatenate([te, [-1, 0]]), np.concatenate([to, [0, -1]])
    want = cfref.predict(R, S, m, te, to, nn, gm)
    for M in (n - 1, n + 10):
        ids = tref.neighbour_sets(S, M)
        assert ids.shape == (n, M) and (ids[:, n - 1:] == -1).all()
        assert all(ids[a, :n - 1].tolist() == [b for b in range(n) if b != a] for a in range(n))
        assert np.array_equal(tref.predict_truncated(R, S, m, ids, te, to, nn, gm), want)
    lo, hi = float(case["min_rating"]), float(case["max_rating"])
    assert np.array_equal(tref.predict_truncated(R, S, m, ids, te, to, nn, gm, (lo, hi)),
                          cfref.predict(R, S, m, te, to, nn, gm, (lo, hi)))
    # a short row does change predictions on this fixture
    few = tref.neighbour_sets(S, 3)
    assert not np.array_equal(tref.predict_truncated(R, S, m, few, te, to, nn, gm), want)


def test_neighbour_sets_on_a_hand_made_matrix():
    """A tie at the cut (the lower id wins), a +-0 pair (they tie, the id
    decides) and a zero row (the lowest ids)."""
    S = np.array([[1.0, 0.5, 0.5, 0.5, 0.2, -0.1],
                  [0.5, 1.0, -0.0, 0.0, -0.3, -0.2],
                  [0.5, -0.0, 1.0, 0.9, 0.8, 0.7],
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                  [0.2, -0.3, 0.8, 0.0, 1.0, -0.0],
                  [-0.1, -0.2, 0.7, 0.0, -0.0, 1.0]])
    two = tref.neighbour_sets(S, 2)
    assert two[0].tolist() == [1, 2]             # 0.5 three times: ids 1 and 2, not 3
    assert two[1].tolist() == [0, 2]             # -0 (id 2) ties with +0 (id 3): the lower id
    assert two[3].tolist() == [0, 1]             # a zero row: the lowest ids, never itself
    assert two[2].tolist() == [3, 4]
    assert two[4].tolist() == [0, 2]
    assert two[5].tolist() == [2, 3]             # 0.7, then +0 (id 3) before -0 (id 4)
    assert tref.neighbour_sets(S, 1)[:, 0].tolist() == [1, 0, 3, 0, 2, 2]
    three = tref.neighbour_sets(S, 3)
    assert three[0].tolist() == [1, 2, 3] and three[3].tolist() == [0, 1, 2]
    assert three[1].tolist() == [0, 2, 3]
    seven = tref.neighbour_sets(S, 7)
    assert seven[3].tolist() == [0, 1, 2, 4, 5, -1, -1]
    # a candidate outside N_M(e) is no candidate: target 0 with M = 2 ignores entity 3
    R = np.array([[0.0], [0.0], [0.0], [4.0], [2.0], [0.0]])
    m = np.zeros(6)
    assert tref.n_candidates(R, two, 0, 0) == (0, 2)
    assert tref.predict_truncated(R, S, m, two, [0], [0], 5, 9.0)[0] == m[0]
    assert cfref.predict(R, S, m, [0], [0], 5, 9.0)[0] != m[0]


# --------------------------------------------------------------------- ABI
_LISTS = dict(other_ptr=_PTR, list_entity_ids=_PTR, list_ratings=_PTR, nbr_ids=_PTR,
              nbr_sims=_PTR, n_stored=8, mean=_PTR, n_entities=3, n_others=4, dtype=MF_F32,
              n_neighbors=5)
_QUERY = dict(_LISTS, query_ids=_PTR, n_query=5, query_side=OTHER, targets_per_block=0)


def _neighbours(lib, **kw):
    a = dict(entity_ptr=_PTR, other_ids=_PTR, ratings=_PTR, other_ptr=_PTR, entity_ids=_PTR,
             other_ratings=_PTR, n_entities=3, n_others=4, dtype=MF_F32, mean=_PTR, norm=_PTR,
             pass_cols=0, n_stored=8, workspace=_PTR, nbr_ids=_PTR, nbr_sims=_PTR)
    a.update(kw)
    return lib.mf_cf_neighbours(a["entity_ptr"], a["other_ids"], a["ratings"], a["other_ptr"],
                                a["entity_ids"], a["other_ratings"], a["n_entities"],
                                a["n_others"], a["dtype"], a["mean"], a["norm"], a["pass_cols"],
                                a["n_stored"], a["workspace"], a["nbr_ids"], a["nbr_sims"], None)


def _predict(lib, **kw):
    a = dict(_LISTS, entity_ids=_PTR, other_ids=_PTR, n_pairs=5, out=_PTR)
    a.update(kw)
    return lib.mf_cf_predict_nbr(a["entity_ids"], a["other_ids"], a["n_pairs"], a["other_ptr"],
                                 a["list_entity_ids"], a["list_ratings"], a["nbr_ids"],
                                 a["nbr_sims"], a["n_stored"], a["mean"], a["n_entities"],
                                 a["n_others"], a["dtype"], a["n_neighbors"], 2.5, 0.0, 5.0, 1,
                                 a["out"], None)


def _model_args(a):
    return (a["query_ids"], a["n_query"], a["query_side"], a["other_ptr"], a["list_entity_ids"],
            a["list_ratings"], a["nbr_ids"], a["nbr_sims"], a["n_stored"], a["mean"],
            a["n_entities"], a["n_others"], a["dtype"], a["n_neighbors"], 2.5,
            a["targets_per_block"])


def _scores(lib, **kw):
    a = dict(_QUERY, out=_PTR)
    a.update(kw)
    return lib.mf_cf_scores_nbr(*_model_args(a), a["out"], None)


def _topk(lib, **kw):
    a = dict(_QUERY, exclude_ptr=None, exclude_items=None, amount=10, workspace=_PTR,
             out_items=_PTR, out_scores=_PTR)
    a.update(kw)
    return lib.mf_cf_topk_nbr(*_model_args(a), a["exclude_ptr"], a["exclude_items"], a["amount"],
                              a["workspace"], a["out_items"], a["out_scores"], None)


def _rank(lib, **kw):
    a = dict(_QUERY, exclude_ptr=None, exclude_items=None, target_ptr=_PTR, target_items=_PTR,
             workspace=_PTR, out_rank=_PTR, out_candidates=_PTR)
    a.update(kw)
    return lib.mf_cf_rank_nbr(*_model_args(a), a["exclude_ptr"], a["exclude_items"],
                              a["target_ptr"], a["target_items"], a["workspace"], a["out_rank"],
                              a["out_candidates"], None)


QUERY_CALLS = {"mf_cf_scores_nbr": _scores, "mf_cf_topk_nbr": _topk, "mf_cf_rank_nbr": _rank}
STORED = [(dict(n_stored=0), "n_stored"), (dict(n_stored=-1), "n_stored"),
          (dict(n_stored=4097), "n_stored"), (dict(nbr_ids=None), "nbr_ids"),
          (dict(nbr_sims=None), "nbr_sims"), (dict(dtype=MF_F64), "dtype"),
          (dict(n_entities=-1), "n_entities"), (dict(n_others=-2), "n_others")]
QUERY_BAD = STORED + [(dict(query_side=2), "query_side"), (dict(n_neighbors=0), "n_neighbors"),
                      (dict(targets_per_block=-1), "targets_per_block"),
                      (dict(n_query=-1), "n_query"), (dict(query_ids=None), "query_ids"),
                      (dict(other_ptr=None), "other_ptr"), (dict(mean=None), "mean")]
BAD = ([("mf_cf_neighbours", _neighbours, b, n) for b, n in STORED + [
            (dict(pass_cols=-1), "pass_cols"), (dict(pass_cols=4097), "pass_cols"),
            (dict(workspace=None), "workspace"), (dict(entity_ptr=None), "entity_ptr"),
            (dict(other_ptr=None), "other_ptr"), (dict(mean=None), "mean"),
            (dict(norm=None), "norm")]]
       + [("mf_cf_predict_nbr", _predict, b, n) for b, n in STORED + [
            (dict(n_neighbors=0), "n_neighbors"), (dict(n_pairs=-1), "n_pairs"),
            (dict(n_pairs=(1 << 25) + 1), "n_pairs"), (dict(entity_ids=None), "entity_ids"),
            (dict(other_ids=None), "other_ids"), (dict(out=None), "out"),
            (dict(other_ptr=None), "other_ptr"), (dict(mean=None), "mean")]]
       + [(fn, call, b, n) for fn, call in QUERY_CALLS.items() for b, n in QUERY_BAD]
       + [("mf_cf_scores_nbr", _scores, dict(out=None), "out"),
          ("mf_cf_topk_nbr", _topk, dict(amount=0), "amount"),
          ("mf_cf_topk_nbr", _topk, dict(amount=2049), "amount"),
          ("mf_cf_topk_nbr", _topk, dict(workspace=None), "workspace"),
          ("mf_cf_topk_nbr", _topk, dict(out_items=None), "out_items"),
          ("mf_cf_topk_nbr", _topk, dict(out_scores=None), "out_scores"),
          ("mf_cf_rank_nbr", _rank, dict(target_ptr=None), "target_ptr"),
          ("mf_cf_rank_nbr", _rank, dict(workspace=None), "workspace"),
          ("mf_cf_rank_nbr", _rank, dict(out_rank=None), "out_rank"),
          ("mf_cf_rank_nbr", _rank, dict(out_candidates=None), "out_candidates")])


@pytest.mark.parametrize("fn,call,bad,name", BAD)
def test_entry_points_reject_invalid_arguments(fn, call, bad, name):
    from matrix_factorization import _lib

    assert call(_lib.load(), **bad) == MF_ERR_INVALID
    err = _lib.last_error()
    assert fn in err and name in err


def test_zero_sizes_are_ok_without_a_device():
    from matrix_factorization import _lib

    lib = _lib.load()
    assert _neighbours(lib, n_entities=0) == MF_OK
    assert _neighbours(lib, n_entities=0, workspace=None, nbr_ids=None, nbr_sims=None) == MF_OK
    assert _neighbours(lib, n_entities=0, n_stored=0) == MF_ERR_INVALID   # checked all the same
    assert _neighbours(lib, n_entities=0, dtype=MF_F64) == MF_ERR_INVALID
    assert _predict(lib, n_pairs=0, out=None, nbr_ids=None) == MF_OK
    assert _predict(lib, n_pairs=0, n_stored=4097) == MF_ERR_INVALID
    for call in QUERY_CALLS.values():
        for side in (OTHER, ENTITY):
            assert call(lib, n_query=0, query_side=side) == MF_OK
        assert call(lib, n_query=0, query_ids=None, nbr_ids=None, nbr_sims=None) == MF_OK
        assert call(lib, n_query=0, n_stored=0) == MF_ERR_INVALID
    assert _scores(lib, query_side=OTHER, n_entities=0, out=None) == MF_OK
    assert _scores(lib, query_side=ENTITY, n_others=0, out=None) == MF_OK
    assert lib.mf_abi_version() == 1


def test_the_workspace_scales_with_the_rows_in_flight():
    from matrix_factorization import _lib

    fn = _lib.load().mf_cf_neighbours_workspace_bytes
    # one float32 scratch row per workgroup, 2048 workgroups at the most
    assert fn(77, 5) == 4 * 77 * 77 and fn(1, 1) == 4
    assert fn(2048, 64) == 4 * 2048 * 2048 and fn(100000, 256) == 4 * 2048 * 100000
    assert fn(100000, 1) == fn(100000, 4096)
    assert fn(0, 8) == 0 and fn(-1, 8) == 0 and fn(10, 0) == 0 and fn(10, 4097) == 0
    assert fn(1000000, 256) < 4 * 1000000 * 1000000 // 100


# -------------------------------------------------------------- estimators
X = pd.DataFrame({"user_id": [1, 1, 2, 3], "item_id": [5, 6, 5, 7]})
Y = pd.Series([1.0, 2.0, 0.5, 3.0])


@pytest.mark.parametrize("cls", [ItemItemCF, UserUserCF])
def test_stored_neighbors_is_validated_in_fit(cls):
    for bad in (0, 4097, 2.5, True, -1, "8"):
        m = cls(stored_neighbors=bad)                    # accepted by the constructor
        with pytest.raises(ValueError, match="stored_neighbors"):
            m.fit(X, Y)


@pytest.mark.parametrize("cls", [ItemItemCF, UserUserCF])
def test_params_and_pickle_carry_stored_neighbors(cls):
    from sklearn.base import clone

    m = cls(n_neighbors=3, stored_neighbors=16)
    assert m.get_params()["stored_neighbors"] == 16
    c = clone(m)
    assert c.stored_neighbors == 16 and c.get_params() == m.get_params()
    assert cls().stored_neighbors is None
    assert cls().set_params(stored_neighbors=8).get_params()["stored_neighbors"] == 8
    assert m.set_params(stored_neighbors=None).stored_neighbors is None
    m.set_params(stored_neighbors=16, n_neighbors=4)
    assert (m.stored_neighbors, m.n_neighbors) == (16, 4)
    assert m.similarity_neighbors is None                # before fit
    with pytest.raises(AttributeError, match="similarity_matrix"):
        cls().similarity_neighbors                       # a dense model has none
    # a fitted model's state, put together without a device
    m.user_id_map, m.item_id_map = {10: 0, 11: 1}, {"a": 0, "b": 1, "c": 2}
    m.n_users, m.n_items = 2, 3
    m.global_mean = np.float64(2.5)
    m._train_users = np.array([0, 0, 1], np.int32)
    m._train_items = np.array([0, 1, 2], np.int32)
    m._train_ratings = np.array([1.0, 4.0, 2.5])
    m._engine = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)    # no HIP device on this host
        c = pickle.loads(pickle.dumps(m))
        assert c.stored_neighbors == 16 and c.get_params() == m.get_params()
        old = m.__getstate__()
        del old["stored_neighbors"]                      # a pickle from before the parameter
        d = cls.__new__(cls)
        d.__setstate__(old)
    assert d.stored_neighbors is None
    name = "item_similarity_matrix" if cls is ItemItemCF else "user_similarity_matrix"
    with pytest.raises(AttributeError, match="similarity_neighbors"):
        getattr(c, name)                                 # no silent densifying


def test_the_byte_check_raises_before_touching_the_device():
    # 3 items, M = 8: 8 * 3 * 8 = 192 bytes of lists + 3 * 3 * 4 = 36 of workspace
    with pytest.raises(ValueError, match=r"192 bytes.*36 bytes.*228 bytes.*max_similarity_bytes=227\b"):
        ItemItemCF(stored_neighbors=8, max_similarity_bytes=227).fit(X, Y)
    with pytest.raises(ValueError, match=r"max_similarity_bytes=1\b"):
        UserUserCF(stored_neighbors=1, max_similarity_bytes=1).fit(X, Y)
    from matrix_factorization.neighbours import NeighbourEngine, check_neighbour_bytes

    check_neighbour_bytes(3, 8, 228)
    with pytest.raises(ValueError, match="max_similarity_bytes=227"):
        NeighbourEngine(np.zeros(1), np.zeros(1), np.ones(1), 3, 4, "cuda:0", 227,
                        stored_neighbors=8)
    # C2 user-user (100 K users), which the dense model refuses at the default budget
    from matrix_factorization.neighbours import DEFAULT_MAX_SIMILARITY_BYTES, check_similarity_bytes

    with pytest.raises(ValueError):
        check_similarity_bytes(100000, DEFAULT_MAX_SIMILARITY_BYTES)
    check_neighbour_bytes(100000, 256, DEFAULT_MAX_SIMILARITY_BYTES)
