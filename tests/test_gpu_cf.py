"""GPU tests of the neighbourhood models: mf_cf_stats / mf_cf_similarity /
mf_cf_predict (through matrix_factorization.neighbours.NeighbourEngine) against
the NumPy FP64 restatement tests/cf_reference.py (pinned against the
reference's classes in tests/test_cf_cpu.py), and ItemItemCF / UserUserCF end
to end on the reference's golden fixtures (tools/make_cf_fixture.py).

Bars:
  similarity   |dS| <= 1e-7.  Ratings are half-integers, exact in float32; the
               kernel accumulates and finishes in FP64 and rounds once to
               float32: within 2^-25 = 3e-8 for |S| <= 1.
  prediction   fed the GPU's own S, 1e-12 relative to max(1, |value|): FP64
               sums of at most 3000 terms in another order than NumPy's.
  estimators   similarity 1e-7 and means 1e-12 against the reference's;
               prediction within 4 n_neighbors max_rating 2^-24 / den_ref + 1e-9
               (the float32 rounding of S propagated, factor 2), leaving out
               pairs whose reference cut margin is below 1e-5 or whose
               denominator is below 0.05 -- at most 2 % of a fixture's pairs.
Every test prints its measured maximum.
"""

import pickle

import numpy as np
import pandas as pd
import pytest

import cf_reference as cfref
from cf_reference import CASES, load_case
from matrix_factorization import ItemItemCF, UserUserCF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S_TOL = 1e-7
P_TOL = 1e-12


def half_integers(rs, size):
    return rs.randint(1, 11, size=size) / 2.0            # 0.5 .. 5.0


def triples(stored, R):
    ent, oth = np.nonzero(stored)
    return ent, oth, R[ent, oth]


def engine(stored, R, pass_cols=0):
    from matrix_factorization.neighbours import NeighbourEngine

    ent, oth, r = triples(stored, R)
    # the engine must not depend on the order the triples come in
    p = np.random.RandomState(len(ent)).permutation(len(ent))
    return NeighbourEngine(ent[p], oth[p], r[p], R.shape[0], R.shape[1], DEV,
                           pass_cols=pass_cols)


def fetch(eng):
    return eng.S.cpu().numpy(), eng.mean.cpu().numpy(), eng.norm.cpu().numpy()


# ------------------------------------------------------------- similarity
def sim_data(n_entities, n_others=50, seed=0, full_other=False, long_entity=0):
    """Random half-integer ratings at ~30 % density with, where the shape has
    room: entity 3 empty, entity 5 rated 2.5 by every other (a constant column:
    norm 0), entities 1 and 2 identical.  ``full_other``: other 0 rates every
    entity (no empty entity then).  ``long_entity``: entity 0 is rated by that
    many others."""
    rs = np.random.RandomState(1000 + seed)
    stored = rs.rand(n_entities, n_others) < 0.3
    R = half_integers(rs, stored.shape)
    if n_entities > 5:
        stored[3] = False
        stored[5], R[5] = True, 2.5
        stored[2], R[2] = stored[1], R[1]
    if full_other:
        stored[:, 0] = True
    if long_entity:
        stored[0] = False
        stored[0, rs.choice(n_others, long_entity, replace=False)] = True
    return stored, np.where(stored, R, 0.0)


SIM_SHAPES = {
    "1": dict(n_entities=1),
    "77": dict(n_entities=77),
    "130": dict(n_entities=130),
    "full_other": dict(n_entities=77, full_other=True, seed=1),
    "600_others": dict(n_entities=40, n_others=700, long_entity=600, seed=2),
}


@pytest.mark.parametrize("shape", list(SIM_SHAPES))
def test_similarity_matches_the_restatement(shape):
    stored, R = sim_data(**SIM_SHAPES[shape])
    m_ref, w_ref = cfref.stats(R)
    S_ref = cfref.similarity(R, m_ref, w_ref)
    eng = engine(stored, R)
    S, m, w = fetch(eng)
    assert S.dtype == np.float32 and S.shape == (R.shape[0],) * 2
    dm = np.max(np.abs(m - m_ref))
    dw = np.max(np.abs(w - w_ref) / np.maximum(1.0, w_ref))
    ds = np.max(np.abs(S.astype(np.float64) - S_ref))
    print(f"{shape}: |dS| {ds:.3e}, means {dm:.3e}, norms {dw:.3e}")
    assert dm <= 1e-12 and dw <= 1e-12
    assert ds <= S_TOL
    assert np.array_equal(S, S.T)                                  # bit for bit
    S2 = fetch(engine(stored, R))[0]
    assert np.array_equal(S.view(np.uint32), S2.view(np.uint32))   # two runs, equal bits
    for z in np.flatnonzero(w_ref == 0):                           # a zero row and column
        assert w[z] == 0 and not S[z].any() and not S[:, z].any()
    if R.shape[0] > 5:
        assert w_ref[5] == 0                                       # the constant column
        assert shape == "full_other" or (w_ref[3] == 0 and not stored[3].any())
        assert np.array_equal(S[1], S[2]) and S[1, 2] == S[1, 1]   # identical columns
    if shape == "full_other":
        assert stored[:, 0].all()
    if shape == "600_others":
        assert stored[0].sum() == 600


def test_similarity_in_column_passes_gives_the_same_bits():
    stored, R = sim_data(77)
    whole = fetch(engine(stored, R))[0]
    passes = fetch(engine(stored, R, pass_cols=32))[0]             # 3 passes: 32 + 32 + 13
    assert np.array_equal(whole.view(np.uint32), passes.view(np.uint32))
    # lists longer than the range-search threshold (128), several passes
    stored, R = sim_data(300, n_others=6, seed=3, full_other=True)
    whole = fetch(engine(stored, R))[0]
    passes = fetch(engine(stored, R, pass_cols=64))[0]
    assert np.array_equal(whole.view(np.uint32), passes.view(np.uint32))
    assert np.max(np.abs(whole.astype(np.float64) - cfref.similarity(R))) <= S_TOL


# -------------------------------------------------------------- prediction
LENS = [1, 63, 65, 257, 296, 5, 0] + [40] * 9
TIE_LO, TIE_HI, TIE_TARGET, EMPTY = 10, 11, 12, 13
O_ZERO, O_TIE, O_SWAP = 7, 8, 9


@pytest.fixture(scope="module")
def pred_model():
    """300 entities x 16 others.  Others 0..6 have lists of LENS[o] entries.
    Other 7 holds five entries of rating exactly 0.  Entities 10 and 11 are
    identical except that their ratings by others 8 and 9 are swapped; entity
    12 is entity 10 without those two ratings -- so S[12,10] == S[12,11] bit
    for bit (every sum involved is exact), and they top 12's candidates in
    other 8's list: a tie across an n_neighbors = 1 cut, with different
    ratings behind its two sides.  Entity 13 has no ratings."""
    rs = np.random.RandomState(7)
    ne, no = 300, len(LENS)
    special = [TIE_LO, TIE_HI, TIE_TARGET, EMPTY]
    pool = np.setdiff1d(np.arange(ne), special)
    stored = np.zeros((ne, no), bool)
    for o, n in enumerate(LENS):
        stored[rs.choice(pool, n, replace=False), o] = True
    R = half_integers(rs, stored.shape)
    zeros = np.flatnonzero(stored[:, O_ZERO])[:5]
    R[zeros, O_ZERO] = 0.0
    stored[TIE_LO, 7:] = True
    R[TIE_LO, O_TIE], R[TIE_LO, O_SWAP] = 4.5, 1.0
    stored[TIE_HI], R[TIE_HI] = stored[TIE_LO], R[TIE_LO]
    R[TIE_HI, O_TIE], R[TIE_HI, O_SWAP] = 1.0, 4.5
    stored[TIE_TARGET], R[TIE_TARGET] = stored[TIE_LO], R[TIE_LO]
    stored[TIE_TARGET, [O_TIE, O_SWAP]] = False
    R = np.where(stored, R, 0.0)
    assert [int(stored[:, o].sum()) for o in range(7)] == LENS[:7]
    eng = engine(stored, R)
    S, m, _ = fetch(eng)
    m_ref, _ = cfref.stats(R)
    assert np.array_equal(m, m_ref)                    # sums of half-integers are exact
    ents = np.asarray([0, 1, 5, TIE_LO, TIE_HI, TIE_TARGET, EMPTY, 50, 100, 299])
    ent = np.concatenate([np.repeat(ents, no), [-1, 4, -1]])
    oth = np.concatenate([np.tile(np.arange(no), len(ents)), [2, -1, -1]])
    return dict(stored=stored, R=R, eng=eng, S=S, m=m_ref, ent=ent, oth=oth, zeros=zeros)


def check_predict(d, nn, bound, what):
    lo, hi, gm = 1.5, 4.0, 3.25                        # a range that does clip
    got = d["eng"].predict(d["ent"], d["oth"], nn, gm, lo, hi, bound)
    want = cfref.predict(d["R"], d["S"], d["m"], d["ent"], d["oth"], nn, gm,
                         (lo, hi) if bound else None)
    err = np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))
    print(f"{what} n_neighbors={nn} bound={bound}: {len(got)} pairs, max rel diff {err:.3e}")
    assert got.dtype == np.float64 and np.all(np.isfinite(got))
    assert err <= P_TOL
    return got


@pytest.mark.parametrize("bound", [False, True])
@pytest.mark.parametrize("nn", [1, 5, 62, 1000])
def test_predict_matches_the_restatement(pred_model, nn, bound):
    d = pred_model
    got = check_predict(d, nn, bound, "300 x 16")
    if not bound:
        assert got[-3:].tolist() == [3.25] * 3         # -1 for either id, or both
    else:
        assert got.min() >= 1.5 and got.max() <= 4.0


def test_predict_edge_cases(pred_model):
    d = pred_model
    R, S, m, stored, eng = d["R"], d["S"], d["m"], d["stored"], d["eng"]

    def one(e, o, nn):
        return float(eng.predict(np.asarray([e]), np.asarray([o]), nn, 3.25, 0, 5, False)[0])

    # a tie across the cut: the lower id's rating (4.5) is used, not the higher's (1.0)
    e, o = TIE_TARGET, O_TIE
    assert S[e, TIE_LO] == S[e, TIE_HI] > 0 and not stored[e, o]
    cand = np.flatnonzero(stored[:, o])
    assert S[e, TIE_LO] == S[e, cand].max()
    assert abs(one(e, o, 1) - (m[e] + 4.5 - m[TIE_LO])) <= 1e-12
    assert abs((m[e] + 1.0 - m[TIE_HI]) - one(e, o, 1)) > 1.0
    # a cut that has to take negative similarities
    e, o = 50, 1
    keep = cfref.select(S[e].astype(np.float64), R[:, o], e, 62)
    assert len(keep) == 62 and (S[e, keep] < 0).sum() >= 2 and (S[e, keep] > 0).sum() >= 2
    # every kept similarity is 0 (the target has no ratings): the mean
    assert one(EMPTY, 3, 5) == m[EMPTY] == 0.0
    # no candidate (an empty list): the mean
    assert LENS[6] == 0 and one(5, 6, 5) == m[5]
    # the target is in the other's own list and is left out
    o = 3
    e = int(np.flatnonzero(stored[:, o])[0])
    full = cfref.predict(R, S, m, [e], [o], 1000, 3.25)[0]
    Rx = R.copy()
    Rx[e, o] = 0.0                                     # the same list without the target
    assert abs(one(e, o, 1000) - full) <= 1e-12
    assert abs(cfref.predict(Rx, S, m, [e], [o], 1000, 3.25)[0] - full) <= 1e-12
    # an entry of rating 0 is no neighbour: other 7's list with and without them
    z = d["zeros"]
    assert stored[z, O_ZERO].all() and not R[z, O_ZERO].any()
    only = np.flatnonzero(stored[:, O_ZERO] & (R[:, O_ZERO] > 0))
    only = only[only != 100]
    s = S[100, only].astype(np.float64)
    want = m[100] + (s * (R[only, O_ZERO] - m[only])).sum() / np.abs(s).sum()
    assert abs(one(100, O_ZERO, 1000) - want) <= 1e-12


def test_predict_with_a_3000_entry_list():
    """Lists beyond the 1024 keys that stay in LDS: the select re-reads S."""
    rs = np.random.RandomState(9)
    ne, no = 3100, 40
    stored = np.zeros((ne, no), bool)
    stored[rs.choice(ne, 3000, replace=False), 0] = True
    for o in range(1, no):
        stored[rs.choice(ne, 300, replace=False), o] = True
    R = np.where(stored, half_integers(rs, stored.shape), 0.0)
    eng = engine(stored, R)
    S, m, _ = fetch(eng)
    ents = rs.choice(ne, 12, replace=False)
    d = dict(eng=eng, R=R, S=S, m=cfref.stats(R)[0], ent=np.repeat(ents, 2),
             oth=np.tile([0, 1], len(ents)))
    assert stored[:, 0].sum() == 3000
    for nn in (1, 5, 2900, 5000):
        check_predict(d, nn, nn == 5, "3100 x 40")
    rows = S[ents].astype(np.float64)
    assert np.max(np.abs(rows - cfref.similarity(R)[ents])) <= S_TOL


# --------------------------------------------------------------- estimators
def fit_case(case, cls):
    Model = ItemItemCF if cls == "itemitemcf" else UserUserCF
    X = pd.DataFrame({"user_id": case["train_user"], "item_id": case["train_item"]})
    np.random.seed(3)
    model = Model(min_rating=float(case["min_rating"]), max_rating=float(case["max_rating"]),
                  n_neighbors=int(case["n_neighbors"]), device=DEV)
    return model.fit(X, pd.Series(case["train_rating"]))


@pytest.mark.parametrize("data,cls", CASES)
def test_estimators_match_the_reference(data, cls):
    case = load_case(data, cls)
    model = fit_case(case, cls)
    item_side = cls == "itemitemcf"
    ids = case["item_ids"] if item_side else case["user_ids"]
    id_map = model.item_id_map if item_side else model.user_id_map
    at = np.asarray([id_map[x] for x in ids.tolist()])       # the reference's order -> ours
    S = model.item_similarity_matrix if item_side else model.user_similarity_matrix
    means = model.item_mean_ratings if item_side else model.user_mean_ratings
    assert isinstance(S, np.ndarray) and S.dtype == np.float32
    assert isinstance(means, pd.Series) and means.dtype == np.float64
    ds = np.max(np.abs(S[np.ix_(at, at)].astype(np.float64) - case["similarity"]))
    dm = np.max(np.abs(means.to_numpy()[at] - case["means"]))
    print(f"{data}/{cls}: similarity {ds:.3e}, means {dm:.3e}")
    assert ds <= S_TOL and dm <= 1e-12
    assert abs(model.global_mean - float(case["global_mean"])) <= 1e-12
    M = model.user_item_matrix
    assert M.shape == (len(case["user_ids"]), len(case["item_ids"]))
    assert M.to_numpy().sum() == case["train_rating"].sum()

    X = pd.DataFrame({"user_id": case["test_user"], "item_id": case["test_item"]})
    nn, hi = int(case["n_neighbors"]), float(case["max_rating"])
    use = (case["margin"] >= 1e-5) & (case["den"] >= 0.05)
    assert (~use).sum() <= 0.02 * len(use)
    tol = 4 * nn * hi * 2.0 ** -24 / case["den"] + 1e-9
    for bound, ref in ((False, case["pred"]), (True, case["pred_bounded"])):
        got = np.asarray(model.predict(X, bound_ratings=bound))
        worst = np.max((np.abs(got - ref) / tol)[use])
        print(f"{data}/{cls} bound={bound}: {int(use.sum())} pairs, max |dp| "
              f"{np.max(np.abs(got - ref)[use]):.3e}, worst fraction of its bar {worst:.3f}")
        assert worst <= 1.0


def test_recommend_pickle_and_budget():
    import torch

    case = load_case("small", "itemitemcf")
    model = fit_case(case, "itemitemcf")
    user = case["user_ids"][0]
    known = case["train_item"][case["train_user"] == user].tolist()
    rec = model.recommend(user, amount=7, items_known=known, bound_ratings=False)
    cand = [i for i in model.item_id_map if i not in set(known)]
    frame = pd.DataFrame({"user_id": user, "item_id": cand})
    frame["rating_pred"] = model.predict(frame, bound_ratings=False)
    want = frame.sort_values(by="rating_pred", ascending=False).head(7)
    assert rec["item_id"].tolist() == want["item_id"].tolist()
    assert rec["rating_pred"].tolist() == want["rating_pred"].tolist()
    assert len(rec) == 7 and not set(rec["item_id"]) & set(known)

    X = pd.DataFrame({"user_id": case["test_user"], "item_id": case["test_item"]})
    before = model.predict(X)
    loaded = pickle.loads(pickle.dumps(model))
    assert "_engine" not in loaded.__dict__ or loaded.__dict__["_engine"] is None
    assert loaded.predict(X) == before                              # the same bits
    assert np.array_equal(loaded.item_similarity_matrix, model.item_similarity_matrix)

    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    Xt = pd.DataFrame({"user_id": case["train_user"], "item_id": case["train_item"]})
    for Model in (ItemItemCF, UserUserCF):
        with pytest.raises(ValueError, match="max_similarity_bytes=1"):
            Model(max_similarity_bytes=1, device=DEV).fit(Xt, pd.Series(case["train_rating"]))
    assert torch.cuda.memory_allocated() == held
