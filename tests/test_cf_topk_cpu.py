"""Host-side checks of the neighbourhood models' all-targets entry points
(mf_cf_scores / mf_cf_topk / mf_cf_rank, include/mf_hip.h) and of the three
estimator methods built on them: argument validation before any device work,
zero sizes, the workspace formula, the estimator interface and the pickled
state.  No device is touched.
"""

import ctypes
import inspect
import pickle
import warnings

import numpy as np
import pytest

from matrix_factorization import ItemItemCF, KernelMF, UserUserCF

MF_OK, MF_ERR_INVALID = 0, 1
MF_F32, MF_F64 = 0, 1
OTHER, ENTITY = 0, 1
_PTR = ctypes.c_void_p(4096)         # non-NULL, never dereferenced: validation comes first

_MODEL = dict(query_ids=_PTR, n_query=5, query_side=OTHER, other_ptr=_PTR, list_entity_ids=_PTR,
              list_ratings=_PTR, similarity=_PTR, mean=_PTR, n_entities=3, n_others=4,
              dtype=MF_F32, n_neighbors=5, targets_per_block=0)


def _model_args(a):
    return (a["query_ids"], a["n_query"], a["query_side"], a["other_ptr"], a["list_entity_ids"],
            a["list_ratings"], a["similarity"], a["mean"], a["n_entities"], a["n_others"],
            a["dtype"], a["n_neighbors"], 2.5, a["targets_per_block"])


def _scores(lib, **kw):
    a = dict(_MODEL, out=_PTR)
    a.update(kw)
    return lib.mf_cf_scores(*_model_args(a), a["out"], None)


def _topk(lib, **kw):
    a = dict(_MODEL, exclude_ptr=None, exclude_items=None, amount=10, workspace=_PTR,
             out_items=_PTR, out_scores=_PTR)
    a.update(kw)
    return lib.mf_cf_topk(*_model_args(a), a["exclude_ptr"], a["exclude_items"], a["amount"],
                          a["workspace"], a["out_items"], a["out_scores"], None)


def _rank(lib, **kw):
    a = dict(_MODEL, exclude_ptr=None, exclude_items=None, target_ptr=_PTR, target_items=_PTR,
             workspace=_PTR, out_rank=_PTR, out_candidates=_PTR)
    a.update(kw)
    return lib.mf_cf_rank(*_model_args(a), a["exclude_ptr"], a["exclude_items"],
                          a["target_ptr"], a["target_items"], a["workspace"], a["out_rank"],
                          a["out_candidates"], None)


CALLS = {"mf_cf_scores": _scores, "mf_cf_topk": _topk, "mf_cf_rank": _rank}
COMMON = [(dict(dtype=MF_F64), "dtype"),
          (dict(query_side=2), "query_side"),
          (dict(query_side=-1), "query_side"),
          (dict(n_neighbors=0), "n_neighbors"),
          (dict(n_neighbors=-3), "n_neighbors"),
          (dict(targets_per_block=-1), "targets_per_block"),
          (dict(n_query=-1), "n_query"),
          (dict(n_entities=-1), "n_entities"),
          (dict(n_others=-2), "n_others"),
          (dict(query_ids=None), "query_ids"),
          (dict(other_ptr=None), "other_ptr"),
          (dict(similarity=None), "similarity"),
          (dict(mean=None), "mean")]
OWN = [("mf_cf_scores", dict(out=None), "out"),
       ("mf_cf_topk", dict(amount=0), "amount"),
       ("mf_cf_topk", dict(amount=-1), "amount"),
       ("mf_cf_topk", dict(amount=2049), "amount"),
       ("mf_cf_topk", dict(workspace=None), "workspace"),
       ("mf_cf_topk", dict(out_items=None), "out_items"),
       ("mf_cf_topk", dict(out_scores=None), "out_scores"),
       ("mf_cf_rank", dict(target_ptr=None), "target_ptr"),
       ("mf_cf_rank", dict(target_items=None), "target_items"),
       ("mf_cf_rank", dict(workspace=None), "workspace"),
       ("mf_cf_rank", dict(out_rank=None), "out_rank"),
       ("mf_cf_rank", dict(out_candidates=None), "out_candidates")]


@pytest.mark.parametrize("fn,bad,name",
                         [(fn, bad, name) for fn in CALLS for bad, name in COMMON] + OWN)
def test_entry_points_reject_invalid_arguments(fn, bad, name):
    from matrix_factorization import _lib

    assert CALLS[fn](_lib.load(), **bad) == MF_ERR_INVALID
    err = _lib.last_error()
    assert fn in err and name in err


def test_a_grid_beyond_the_launch_limit_is_refused():
    from matrix_factorization import _lib

    lib = _lib.load()
    # 2^30 queries x ceil(300 / 64) = 5 blocks of targets
    assert _scores(lib, n_query=1 << 30, n_entities=300) == MF_ERR_INVALID
    assert "n_query" in _lib.last_error() and "workgroups" in _lib.last_error()


def test_zero_sizes_are_ok_without_a_device():
    from matrix_factorization import _lib

    lib = _lib.load()
    for call in CALLS.values():
        for side in (OTHER, ENTITY):
            assert call(lib, n_query=0, query_side=side) == MF_OK
        assert call(lib, n_query=0, query_ids=None, other_ptr=None, similarity=None,
                    mean=None) == MF_OK
        assert call(lib, n_query=0, dtype=MF_F64) == MF_ERR_INVALID     # checked all the same
        assert call(lib, n_query=0, n_neighbors=0) == MF_ERR_INVALID
    assert _scores(lib, n_query=0, out=None) == MF_OK
    assert _topk(lib, n_query=0, workspace=None, out_items=None, out_scores=None) == MF_OK
    assert _topk(lib, n_query=0, amount=0) == MF_ERR_INVALID
    assert _rank(lib, n_query=0, target_ptr=None, out_rank=None) == MF_OK
    # no target on the queried side: nothing to score, nothing to write
    assert _scores(lib, query_side=OTHER, n_entities=0, out=None) == MF_OK
    assert _scores(lib, query_side=ENTITY, n_others=0, out=None) == MF_OK


def test_workspace_and_blocking_functions():
    from matrix_factorization import _lib

    lib = _lib.load()
    for fn in (lib.mf_cf_topk_workspace_bytes, lib.mf_cf_rank_workspace_bytes):
        # one uint64 order key per query and target
        for nq, nt in ((1, 1), (7, 300), (1024, 10000), (65536, 100000)):
            assert fn(nq, nt) == 8 * nq * nt
        assert fn(0, 10) == 0 and fn(10, 0) == 0 and fn(-1, 10) == 0 and fn(10, -1) == 0
        sizes = [fn(nq, 977) for nq in range(0, 40)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
        sizes = [fn(13, nt) for nt in range(0, 40)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert lib.mf_cf_targets_per_block(300, 0) == 64 and lib.mf_cf_targets_per_block(17, 0) == 17
    assert lib.mf_cf_targets_per_block(300, 7) == 7 and lib.mf_cf_targets_per_block(300, 999) == 300
    assert lib.mf_cf_targets_per_block(0, 0) == 0 and lib.mf_cf_targets_per_block(300, -1) == 0


@pytest.mark.parametrize("cls", [ItemItemCF, UserUserCF])
def test_estimators_expose_the_factor_models_ranking_interface(cls):
    for name in ("recommend_batch", "rank_items", "evaluate_topk"):
        assert inspect.signature(getattr(cls, name)) == inspect.signature(getattr(KernelMF, name))
        # one implementation for both families
        assert getattr(cls, name) is getattr(KernelMF, name)
    assert "recommend" in dir(cls)                       # the reference's one-user form stays


def test_query_chunks_follow_the_budget_and_the_grid():
    from matrix_factorization.neighbours import NeighbourEngine

    eng = NeighbourEngine.__new__(NeighbourEngine)       # no device: only the arithmetic
    eng.n_entities, eng.n_others = 300, 17
    assert NeighbourEngine.topk_ws_budget == 1 << 30
    assert eng.n_targets(OTHER) == 300 and eng.n_targets(ENTITY) == 17
    assert eng._query_chunk(OTHER) == (1 << 30) // (8 * 300)
    eng.topk_ws_budget = 8 * 300 * 5 + 7
    assert eng._query_chunk(OTHER) == 5
    eng.topk_ws_budget = 1
    assert eng._query_chunk(ENTITY) == 1                 # never below one query
    eng.topk_ws_budget = 1 << 62
    eng.targets_per_block = 1
    assert eng._query_chunk(OTHER) == (2**31 - 1) // 300  # one workgroup per query and target


def test_pickled_state_is_still_numpy_and_builtins():
    m = UserUserCF(n_neighbors=3)
    m.user_id_map = {np.int64(10): 0, np.int64(11): 1}
    m.item_id_map = {"a": 0, "b": 1, "c": 2}
    m.n_users, m.n_items = 2, 3
    m.global_mean = np.float64(2.5)
    m._train_users = np.array([0, 0, 1], np.int32)
    m._train_items = np.array([0, 1, 2], np.int32)
    m._train_ratings = np.array([1.0, 4.0, 2.5])
    m._means = np.array([2.5, 2.5])
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
    m._engine = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)    # no HIP device on this host
        c = pickle.loads(pickle.dumps(m))
    assert c.get_params() == m.get_params()
    assert callable(c.recommend_batch) and callable(c.rank_items) and callable(c.evaluate_topk)
    assert c.__dict__.get("_engine") is None               # rebuilt on first use
