"""GPU tests of the stored-neighbours (top-M) neighbourhood model:
mf_cf_neighbours and the list variants of predict / scores / topk / rank
through NeighbourEngine(stored_neighbors=M), and ItemItemCF / UserUserCF with
``stored_neighbors``.

Oracles.  Neighbour lists: tests/cf_truncated_reference.neighbour_sets of the
GPU's own dense S (a dense engine on the same triples), exactly -- ids by
array_equal, similarities by their bits.  Predictions: predict_truncated fed
the GPU's similarities, within test_gpu_cf.py's prediction bar (1e-12 relative
to max(1, |value|): FP64 sums of at most 3000 terms in another order than
NumPy's).  With every neighbour stored (M >= n - 1) and for the all-targets
pass every comparison is exact.  Every test prints its measured maximum.
"""

import pickle

import numpy as np
import pandas as pd
import pytest

import cf_reference as cfref
import cf_truncated_reference as tref
from cf_reference import load_case
from ranking_reference import ranks_from_scores
from matrix_factorization import ItemItemCF, UserUserCF
from test_gpu_cf import (DEV, LENS, O_TIE, P_TOL, TIE_HI, TIE_LO, TIE_TARGET, engine, fetch,
                         half_integers, pred_model, sim_data, triples)  # noqa: F401 (fixture)
from test_gpu_cf_topk import (check_topk, exclusion_lists, oracle_scores, oracle_topk, same_bits)

pytestmark = pytest.mark.gpu

OTHER, ENTITY = 0, 1
GM = 3.25


def engine_nbr(stored, R, M, pass_cols=0):
    from matrix_factorization.neighbours import NeighbourEngine

    ent, oth, r = triples(stored, R)
    p = np.random.RandomState(len(ent)).permutation(len(ent))
    return NeighbourEngine(ent[p], oth[p], r[p], R.shape[0], R.shape[1], DEV,
                           pass_cols=pass_cols, stored_neighbors=M)


def lists(eng):
    assert eng.S is None
    ids, sims = eng.nbr_ids.cpu().numpy(), eng.nbr_sims.cpu().numpy()
    assert ids.dtype == np.int32 and sims.dtype == np.float32
    assert ids.shape == sims.shape == (eng.n_entities, eng.stored)
    return ids, sims


def id_decided_ties(S, ids, lo=1, hi=2):
    """Rows in which ``lo`` is stored and ``hi``, of the same similarity, is not."""
    return [a for a in range(S.shape[0]) if a not in (lo, hi) and S[a, lo] == S[a, hi]
            and lo in ids[a] and hi not in ids[a]]


# --------------------------------------------------------- neighbour lists
NBR_SHAPES = {
    "1-M4": (dict(n_entities=1), 4, 0),
    "77-M1": (dict(n_entities=77), 1, 0),
    "77-M2": (dict(n_entities=77), 2, 0),             # a zero row cut between entities 1 and 2
    "77-M5": (dict(n_entities=77), 5, 0),
    "77-M76": (dict(n_entities=77), 76, 0),
    "77-M100": (dict(n_entities=77), 100, 0),
    "130-M7-cols32": (dict(n_entities=130), 7, 32),
    "130-M40-cols32": (dict(n_entities=130), 40, 32),  # M beyond a column range
    "300x6-M16-cols64": (dict(n_entities=300, n_others=6, seed=3, full_other=True), 16, 64),
}
TIES = {}


@pytest.mark.parametrize("shape", list(NBR_SHAPES))
def test_neighbour_lists_are_the_dense_rows_best(shape):
    data, M, cols = NBR_SHAPES[shape]
    stored, R = sim_data(**data)
    n = R.shape[0]
    S, _, w = fetch(engine(stored, R))
    ids, sims = lists(engine_nbr(stored, R, M, cols))
    want = tref.neighbour_sets(S, M)
    assert np.array_equal(ids, want)
    pad = ids < 0
    assert (pad == (np.arange(M)[None, :] >= n - 1)).all()
    dense = np.where(pad, np.float32(0), S[np.arange(n)[:, None], np.where(pad, 0, ids)])
    assert np.array_equal(sims.view(np.uint32), dense.view(np.uint32))    # bit for bit
    assert (np.diff(np.where(pad, 2**31 - 1, ids.astype(np.int64)), axis=1) >= 0).all()
    for run_cols in (cols, 32, 0):                   # two runs; 32-column passes; one pass
        again = lists(engine_nbr(stored, R, M, run_cols))
        assert np.array_equal(again[0], ids)
        assert np.array_equal(again[1].view(np.uint32), sims.view(np.uint32))
    zero = np.flatnonzero(w == 0)
    for z in zero:                                   # an all-zero row keeps the lowest ids
        assert ids[z, :min(M, n - 1)].tolist() == [b for b in range(n) if b != z][:M]
    if n > 5:
        assert 5 in zero and (data.get("full_other") or 3 in zero)
        assert np.array_equal(S[1], S[2])
        TIES[shape] = id_decided_ties(S, ids)
    print(f"{shape}: {n} x {M}, {int((~pad).sum())} stored, zero rows {zero.tolist()}, "
          f"rows where the id decides 1 | 2: {TIES.get(shape)}")
    if shape == "77-M2":
        assert 3 in TIES[shape]                      # S[3,1] == S[3,2] == 0: 1 kept, 2 not
    if shape in ("77-M2", "77-M5", "130-M7-cols32", "130-M40-cols32"):
        # the fixture has the tie in a row of non-zero similarities too
        assert [a for a in TIES[shape] if S[a, 1] != 0]


# -------------------------------------------------------------- prediction
@pytest.fixture(scope="module")
def pred_lists(pred_model):
    d = pred_model
    out = {}
    for M in (8, 64):
        eng = engine_nbr(d["stored"], d["R"], M)
        ids, sims = lists(eng)
        assert np.array_equal(ids, tref.neighbour_sets(d["S"], M))
        out[M] = dict(eng=eng, ids=ids)
    return out


def check_truncated(d, t, nn, bound, what):
    lo, hi = 1.5, 4.0                                 # a range that does clip
    got = t["eng"].predict(d["ent"], d["oth"], nn, GM, lo, hi, bound)
    want = tref.predict_truncated(d["R"], d["S"], d["m"], t["ids"], d["ent"], d["oth"], nn, GM,
                                  (lo, hi) if bound else None)
    err = np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))
    print(f"{what} n_neighbors={nn} bound={bound}: {len(got)} pairs, max rel diff {err:.3e}")
    assert got.dtype == np.float64 and np.all(np.isfinite(got))
    assert err <= P_TOL
    return got


@pytest.mark.parametrize("bound", [False, True])
@pytest.mark.parametrize("nn", [1, 5, 62])
@pytest.mark.parametrize("M", [8, 64])
def test_predict_matches_the_truncated_restatement(pred_model, pred_lists, M, nn, bound):
    d, t = pred_model, pred_lists[M]
    got = check_truncated(d, t, nn, bound, f"300 x 16, M={M}")
    if not bound:
        assert got[-3:].tolist() == [GM] * 3           # -1 for either id, or both
    if M == 8:                                         # the truncation bites
        fewer = [tref.n_candidates(d["R"], t["ids"], e, o)
                 for e, o in zip(d["ent"], d["oth"]) if e >= 0 and o >= 0]
        n_less = sum(a < b for a, b in fewer)
        print(f"M=8: {n_less} of {len(fewer)} pairs have fewer candidates than the dense model")
        assert n_less >= 1
        if not bound:
            dense = d["eng"].predict(d["ent"], d["oth"], nn, GM, 1.5, 4.0, False)
            assert not np.array_equal(dense, got)


def test_predict_list_lengths_and_the_tie_pair(pred_model, pred_lists):
    d = pred_model
    assert LENS[:7] == [1, 63, 65, 257, 296, 5, 0]
    assert d["stored"][d["zeros"], 7].all() and not d["R"][d["zeros"], 7].any()   # ratings of 0
    # the tie pair: S[12,10] == S[12,11] top 12's row, so both are stored at M = 8 and the
    # n_neighbors = 1 cut between them goes to the lower id, as in the dense model
    S, m, ids = d["S"], d["m"], pred_lists[8]["ids"]
    assert S[TIE_TARGET, TIE_LO] == S[TIE_TARGET, TIE_HI]
    assert TIE_LO in ids[TIE_TARGET] and TIE_HI in ids[TIE_TARGET]
    one = pred_lists[8]["eng"].predict(np.asarray([TIE_TARGET]), np.asarray([O_TIE]), 1, GM, 0, 5,
                                       False)[0]
    assert abs(one - (m[TIE_TARGET] + 4.5 - m[TIE_LO])) <= 1e-12


def test_predict_with_a_3000_entry_list():
    """A list beyond the 1024 keys that stay in LDS: every pass of the select
    searches the stored row again."""
    rs = np.random.RandomState(9)
    ne, no, M = 3100, 40, 64
    stored = np.zeros((ne, no), bool)
    stored[rs.choice(ne, 3000, replace=False), 0] = True
    for o in range(1, no):
        stored[rs.choice(ne, 300, replace=False), o] = True
    R = np.where(stored, half_integers(rs, stored.shape), 0.0)
    S = fetch(engine(stored, R))[0]
    eng = engine_nbr(stored, R, M)
    ids, sims = lists(eng)
    ents = rs.choice(ne, 12, replace=False)
    full = np.full((ne, M), -1, np.int32)
    for a in ents:                                     # the reference rows of the entities used
        b = np.delete(np.arange(ne), a)
        s = S[a, b].astype(np.float64) + 0.0
        full[a] = np.sort(b[np.lexsort((b, -s))][:M])
    assert np.array_equal(ids[ents], full[ents])
    assert np.array_equal(sims[ents].view(np.uint32),
                          S[ents[:, None], ids[ents]].view(np.uint32))
    d = dict(R=R, S=S, m=cfref.stats(R)[0], ent=np.repeat(ents, 2),
             oth=np.tile([0, 1], len(ents)))
    assert stored[:, 0].sum() == 3000
    for nn in (1, 5, 62):
        check_truncated(d, dict(eng=eng, ids=full), nn, nn == 5, "3100 x 40, M=64")


# ------------------------------------------------- every neighbour stored
def rank_targets(nq, nt, seed):
    rs = np.random.RandomState(seed)
    tp = np.arange(nq + 1, dtype=np.int64) * 4
    return tp, rs.randint(-1, nt + 1, 4 * nq).astype(np.int32)


Q = {OTHER: np.concatenate([np.arange(16), [-1]]),
     ENTITY: np.asarray([0, 1, 5, TIE_LO, TIE_HI, TIE_TARGET, 13, 50, 100, 299, -1])}


def all_targets(eng, side, nn, amount=10):
    q = Q[side]
    nt = eng.n_targets(side)
    ptr, ex = exclusion_lists(len(q), nt, 100 + side)
    tp, ti = rank_targets(len(q), nt, 5 + side)
    return ((eng.scores(q, side, nn, GM),) + eng.topk(q, side, nn, GM, amount, ptr, ex)
            + eng.topk(q, side, nn, GM, amount) + eng.rank(q, side, nn, GM, tp, ti, ptr, ex))


@pytest.mark.parametrize("M", [299, 310])
def test_every_neighbour_stored_is_the_dense_model_bit_for_bit(pred_model, M):
    d = pred_model
    dense = d["eng"]
    eng = engine_nbr(d["stored"], d["R"], M)
    assert dense.n_entities == 300
    for nn in (1, 5, 62):
        for bound in (False, True):
            a = dense.predict(d["ent"], d["oth"], nn, GM, 1.5, 4.0, bound)
            b = eng.predict(d["ent"], d["oth"], nn, GM, 1.5, 4.0, bound)
            assert same_bits(a, b)
        for side in (OTHER, ENTITY):
            for x, y in zip(all_targets(dense, side, nn), all_targets(eng, side, nn)):
                assert x.dtype == y.dtype and x.shape == y.shape
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    print(f"M={M}: predict, scores, topk (with and without exclusions) and rank equal the "
          "dense engine's bits on both query sides")


# ------------------------------------------------------ all-targets, M = 8
@pytest.mark.parametrize("side", [OTHER, ENTITY])
@pytest.mark.parametrize("nn", [1, 5, 62])
def test_all_targets_pass_on_short_rows(pred_lists, nn, side):
    eng = pred_lists[8]["eng"]
    q, nt = Q[side], eng.n_targets(side)
    want = oracle_scores(eng, q, side, nn)             # predict(bound=False) of the pairs
    ptr, ex = exclusion_lists(len(q), nt, 100 + side)
    tp, ti = rank_targets(len(q), nt, 5 + side)
    try:
        for tpb in (0, 5):
            eng.targets_per_block = tpb
            got = eng.scores(q, side, nn, GM)
            assert got.dtype == np.float64 and same_bits(got, want)
            assert (got[-1] == GM).all()               # the unknown query
            for amount in (1, 10, nt):
                check_topk(eng.topk(q, side, nn, GM, amount), oracle_topk(want, amount))
                check_topk(eng.topk(q, side, nn, GM, amount, ptr, ex),
                           oracle_topk(want, amount, ptr, ex))
            for e_ptr, e_items in ((None, None), (ptr, ex)):
                want_r, want_c = ranks_from_scores(want, tp, ti, e_ptr, e_items)
                got_r, got_c = eng.rank(q, side, nn, GM, tp, ti, e_ptr, e_items)
                assert np.array_equal(got_r, want_r) and np.array_equal(got_c, want_c)
    finally:
        eng.targets_per_block = 0


def test_the_longest_stored_row_is_staged_whole():
    """n_stored = 4096 with more entities than that: the 32 KiB row of a
    MF_CF_QUERY_ENTITY query in LDS beside the keys and bins."""
    rs = np.random.RandomState(11)
    ne, no, M = 4200, 12, 4096
    stored = rs.rand(ne, no) < 0.4
    R = np.where(stored, half_integers(rs, stored.shape), 0.0)
    eng = engine_nbr(stored, R, M)
    ids, _ = lists(eng)
    assert (ids >= 0).all()
    q = np.asarray([0, 7, 4199, -1])
    for nn in (5, 5000):
        assert same_bits(eng.scores(q, ENTITY, nn, GM), oracle_scores(eng, q, ENTITY, nn))


# --------------------------------------------------------------- estimators
def fit(case, cls, **kw):
    Model = ItemItemCF if cls == "itemitemcf" else UserUserCF
    X = pd.DataFrame({"user_id": case["train_user"], "item_id": case["train_item"]})
    np.random.seed(3)
    model = Model(min_rating=float(case["min_rating"]), max_rating=float(case["max_rating"]),
                  n_neighbors=int(case["n_neighbors"]), device=DEV, **kw)
    return model.fit(X, pd.Series(case["train_rating"]))


@pytest.mark.parametrize("cls", ["itemitemcf", "userusercf"])
def test_estimators_with_stored_neighbors(cls):
    case = load_case("medium", cls)
    n_ent = len(case["item_ids"] if cls == "itemitemcf" else case["user_ids"])
    X = pd.DataFrame({"user_id": case["test_user"], "item_id": case["test_item"]})
    train = pd.DataFrame({"user_id": case["train_user"], "item_id": case["train_item"]})
    dense = fit(case, cls)
    full = fit(case, cls, stored_neighbors=n_ent)
    for bound in (False, True):
        assert full.predict(X, bound_ratings=bound) == dense.predict(X, bound_ratings=bound)
    ids, sims = full.similarity_neighbors
    assert ids.shape == sims.shape == (n_ent, n_ent) and (ids[:, -1] == -1).all()
    S = dense.item_similarity_matrix if cls == "itemitemcf" else dense.user_similarity_matrix
    assert np.array_equal(sims[:, :-1].view(np.uint32),
                          S[np.arange(n_ent)[:, None], ids[:, :-1]].view(np.uint32))
    with pytest.raises(AttributeError, match="similarity_neighbors"):
        full.item_similarity_matrix if cls == "itemitemcf" else full.user_similarity_matrix
    with pytest.raises(AttributeError, match="similarity_matrix"):
        dense.similarity_neighbors

    model = fit(case, cls, stored_neighbors=16)
    assert model.get_params()["stored_neighbors"] == 16
    assert model.similarity_neighbors[0].shape == (n_ent, 16)
    assert np.array_equal(model.similarity_neighbors[0], tref.neighbour_sets(S, 16))
    users = case["user_ids"].tolist()[:20]
    items = list(model.item_id_map.keys())
    frame = pd.DataFrame({"user_id": np.repeat(users, len(items)),
                          "item_id": np.tile(items, len(users))})
    frame["rating_pred"] = model.predict(frame, bound_ratings=False)
    known = set(zip(train["user_id"].tolist(), train["item_id"].tolist()))
    frame = frame[[(u, i) not in known for u, i in zip(frame["user_id"], frame["item_id"])]]
    got = model.recommend_batch(users, amount=7, exclude_known=train, bound_ratings=False)
    for u in users:
        mine = got[got["user_id"] == u]
        best = frame[frame["user_id"] == u].sort_values("rating_pred", ascending=False,
                                                        kind="stable").head(7)
        assert mine["rating_pred"].tolist() == best["rating_pred"].tolist()
        assert len(mine) == 7
    u = users[0]
    rec = model.recommend(u, 7, items_known=train["item_id"][train["user_id"] == u].tolist(),
                          bound_ratings=False)
    assert rec["rating_pred"].tolist() == got["rating_pred"][got["user_id"] == u].tolist()
    res = model.evaluate_topk(X, k=[5, 10], exclude_known=train)
    assert sorted(res) == [5, 10]
    # the metrics are those of the ranks of the same predictions: the full-row model's
    # evaluate_topk equals the dense model's
    assert full.evaluate_topk(X, k=5, exclude_known=train) == \
        dense.evaluate_topk(X, k=5, exclude_known=train)
    ranked = model.rank_items(X, exclude_known=train)
    P = frame.set_index(["user_id", "item_id"])["rating_pred"]
    for (uu, ii, r) in zip(ranked["user_id"], ranked["item_id"], ranked["rank"]):
        if uu in users and (uu, ii) in P.index:
            assert r >= 0 and r >= int((P[uu] > P[(uu, ii)]).sum())

    before = model.predict(X)
    loaded = pickle.loads(pickle.dumps(model))
    assert loaded.__dict__.get("_engine") is None and loaded.stored_neighbors == 16
    assert loaded.predict(X) == before                 # the same bits
    assert not np.array_equal(np.asarray(before), np.asarray(dense.predict(X)))
    print(f"medium/{cls}: stored_neighbors={n_ent} equals the dense estimator; 16 ranks as it predicts")


def test_a_fit_the_dense_budget_refuses_succeeds_with_stored_neighbors():
    """3000 users: 36 MB dense, against 192 KB of lists and 24.6 MB of workspace."""
    rs = np.random.RandomState(21)
    nu, ni = 3000, 40
    stored = rs.rand(nu, ni) < 0.3
    u, i = np.nonzero(stored)
    X = pd.DataFrame({"user_id": u, "item_id": i})
    y = pd.Series(half_integers(rs, len(u)))
    budget = 30 << 20
    assert 4 * nu * nu > budget > 8 * nu * 8 + 4 * 2048 * nu
    with pytest.raises(ValueError, match=f"max_similarity_bytes={budget}"):
        UserUserCF(device=DEV, max_similarity_bytes=budget).fit(X, y)
    model = UserUserCF(device=DEV, max_similarity_bytes=budget, stored_neighbors=8).fit(X, y)
    pred = np.asarray(model.predict(X.head(200)))
    assert np.all(np.isfinite(pred)) and model.similarity_neighbors[0].shape == (nu, 8)
