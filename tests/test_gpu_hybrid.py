"""GPU tests of HybridRecommender: mf_hybrid_rerank against the NumPy
restatement tests/hybrid_reference.py (pinned against the reference's
``evaluate_hybrid`` in tests/test_hybrid_cpu.py) -- rows, counts and the two raw
terms equal, the blended scores bit for bit, the model scores being the
engine's own mf_predict values for the same pairs -- and the estimator end to
end on the reference's fixture (tools/make_hybrid_fixture.py).

Bars: the kernel tests are exact.  The estimator reproduces the reference's
precision, recall and NDCG to 1e-12: the fixture's inputs keep every decision
(the retrieval cut, the order of the best k + 1) at least 1e-4 apart, about
100 x the float32 rounding of a d = 24 dot product, so the FP64 profile mean
and mf_topk's summation order cannot change an id.
"""

import numpy as np
import pandas as pd
import pytest
import torch

import hybrid_reference as href
from matrix_factorization import HybridRecommender, ImplicitALSMF, KernelMF, _lib
from matrix_factorization.engine import SGDEngine, _VOID, _tp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32
NQ = 12
UNKNOWN_USER = 3                                  # query position whose model user id is -1


# ----------------------------------------------------------------- the kernel
def make_engine(k, dtype, kernel, n_items, nan_item=None):
    rs = np.random.RandomState(7 * k + len(dtype) + len(kernel))
    n_users = 9
    eng = SGDEngine(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), n_users, n_items,
                    k, kernel, dtype, DEV, gamma=0.37, min_rating=1.0, max_rating=5.0,
                    global_mean=3.2)
    Q = rs.normal(0, 0.5, (n_items, k))
    if nan_item is not None:
        Q[nan_item, k // 2] = np.nan
    eng.load_params(rs.normal(0, 0.5, (n_users, k)), Q, rs.normal(0, 0.3, n_users),
                    rs.normal(0, 0.3, n_items))
    return eng


_TABLES = {}


def score_table(key, eng, users, row_item, n_rows):
    """float32 mf_predict scores [n_query, n_rows] of every (query, index row)
    pair, computed once per configuration and shared."""
    if key not in _TABLES:
        items = np.arange(n_rows, dtype=np.int32) if row_item is None else row_item
        items = np.where((items >= 0) & (items < eng.n_items), items, -1).astype(np.int32)
        u = np.repeat(np.asarray(users, np.int32), n_rows)
        _TABLES[key] = eng.predict(u, np.tile(items, len(users)), False).astype(F32).reshape(
            len(users), n_rows)
    return _TABLES[key]


def candidates(n_cand, n_rows, seed):
    """[NQ, n_cand] candidate rows (distinct per query, some -1 and one out of
    range), float32 similarities in descending order, and per query the
    sorted exclusion list: none for query 0, every candidate for query 1."""
    rs = np.random.RandomState(seed)
    rows = np.full((NQ, n_cand), -1, np.int32)           # more candidates than rows: -1 padding
    for q in range(NQ):
        at = np.sort(rs.choice(n_cand, min(n_cand, n_rows), replace=False))
        rows[q, at] = rs.permutation(n_rows)[:len(at)]
    if n_cand >= 8:
        rows[rs.randint(0, NQ, 6), rs.randint(0, n_cand, 6)] = -1
        rows[5, n_cand // 2] = n_rows + 5
    sims = -np.sort(-rs.uniform(-0.2, 0.9, (NQ, n_cand)).astype(F32), axis=1)
    ex = [set(rs.choice(n_rows, rs.randint(1, max(2, n_rows // 3)), replace=False).tolist())
          for _ in range(NQ)]
    ex[0] = set()
    ex[1] = set(int(r) for r in rows[1] if r >= 0) | {0}
    return rows, sims, ex


def launch(eng, users, rows, sims, row_item, n_rows, ex, alpha, amount, chunk=None, terms=True):
    """mf_hybrid_rerank on device copies of the arguments; host outputs."""
    dev = torch.device(DEV)
    nq, n_cand = rows.shape
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
    d_rows, d_sims = to(rows, np.int32), to(sims, F32)
    d_users = to(users, np.int32)
    d_ri = None if row_item is None else to(row_item, np.int32)
    ptr = np.concatenate([[0], np.cumsum([len(e) for e in ex])]).astype(np.int64)
    flat = np.concatenate([np.sort(np.fromiter(e, np.int64, len(e))) for e in ex] + [[0]])
    d_ptr, d_ex = to(ptr, np.int64), to(flat, np.int32)
    new = lambda dt: torch.full((nq, amount), -7, dtype=dt, device=dev)  # noqa: E731
    o_rows, o_sc, o_mo, o_si = new(torch.int32), new(torch.float32), new(torch.float32), \
        new(torch.float32)
    o_m = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    off = lambda t, n: _VOID(t.data_ptr() + t.element_size() * n)  # noqa: E731
    model = ((0.0, None, None, None, None, 0, 16, _lib.MF_LINEAR, _lib.MF_F32, 0.0, 0.0, 0.0)
             if eng is None else
             (eng.global_mean, _tp(eng.bu), _tp(eng.bi), _tp(eng.P), _tp(eng.Q), eng.n_items, eng.k,
              eng.kcode, eng.dcode, eng.gamma, eng.min_rating, eng.max_rating))
    chunk = chunk or nq
    with torch.cuda.device(dev):
        for q0 in range(0, nq, chunk):
            q1 = min(nq, q0 + chunk)
            _lib.call("mf_hybrid_rerank", off(d_users, q0), q1 - q0, off(d_rows, n_cand * q0),
                      off(d_sims, n_cand * q0), n_cand, None if d_ri is None else _tp(d_ri),
                      n_rows, *model, off(d_ptr, q0), _tp(d_ex), float(alpha), amount, None,
                      off(o_rows, amount * q0), off(o_sc, amount * q0),
                      off(o_mo, amount * q0) if terms else None,
                      off(o_si, amount * q0) if terms else None, off(o_m, q0),
                      _VOID(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize(dev)
    return tuple(t.cpu().numpy() for t in (o_rows, o_sc, o_mo, o_si, o_m))


def check(got, want, what):
    for name, g, w in zip(("rows", "scores", "model", "sims", "n_cand"), got, want):
        if name in ("rows", "n_cand"):
            assert np.array_equal(g, w), (what, name)
        else:
            assert href.same_bits(g, w), (what, name)


def users_of():
    u = (np.arange(NQ) * 5 % 9).astype(np.int32)
    u[UNKNOWN_USER] = -1
    return u


def run_config(k, dtype, kernel, n_cand, n_rows, mapped, amounts, alpha=0.7, model=True):
    """One configuration against the restatement at each amount."""
    rs = np.random.RandomState(n_rows + k)       # one row_item per (k, n_rows): shared tables
    n_items = n_rows - 10 if mapped else n_rows
    row_item = None
    if mapped:
        row_item = rs.randint(0, n_items, n_rows).astype(np.int32)
        row_item[rs.choice(n_rows, max(1, n_rows // 12), replace=False)] = -1
    users = users_of()
    rows, sims, ex = candidates(n_cand, n_rows, 1000 + n_cand)
    eng = make_engine(k, dtype, kernel, n_items) if model else None
    if model:
        table = score_table((k, dtype, kernel, n_rows, mapped), eng, users, row_item, n_rows)
        scores_of = lambda q, r: table[q, r]  # noqa: E731
    else:
        scores_of = lambda q, r: np.zeros(len(r), F32)  # noqa: E731
    for amount in amounts:
        want = href.rerank(rows, sims, scores_of, n_rows, ex, alpha, amount)
        got = launch(eng, users, rows, sims, row_item, n_rows, ex, alpha, amount)
        check(got, want, (k, dtype, kernel, n_cand, amount))
    assert want[4][0] > 0 or n_cand < 8
    assert want[4][1] == 0                               # every candidate excluded
    return want


@pytest.mark.parametrize("n_cand", [1, 37, 64, 65, 200, 2048])
def test_kernel_matches_the_restatement_at_every_list_length(n_cand):
    n_rows = 2100 if n_cand == 2048 else 150
    amounts = sorted({0, 1, min(10, n_cand), n_cand})
    want = run_config(32, "float32", "linear", n_cand, n_rows, n_cand != 64, amounts)
    if n_cand >= 37:
        assert (want[4] < n_cand).any() and (want[4][2:] > 1).all()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("k", [5, 32, 64, 100, 200, 300, 520])
def test_kernel_matches_the_restatement_in_every_row_layout(k, dtype):
    run_config(k, dtype, "linear", 200, 150, k != 100, [10, 200])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("kernel", ["sigmoid", "rbf"])
def test_kernel_matches_the_restatement_for_the_other_kernels(kernel, dtype):
    for k in (32, 100):                                  # V = 1 and V = 2
        run_config(k, dtype, kernel, 65, 150, True, [10, 65])


def test_without_a_model_the_order_is_the_similarities():
    want = run_config(0, "float32", "linear", 200, 150, False, [0, 10, 200], model=False)
    rows, sc, mo, si, m = want
    assert not mo[rows >= 0].any() and (np.diff(si[0, :m[0]]) <= 0).all()


def test_outputs_without_the_raw_terms_and_alpha_extremes():
    users, n_rows = users_of(), 150
    rows, sims, ex = candidates(65, n_rows, 5)
    eng = make_engine(32, "float32", "linear", n_rows)
    table = score_table((32, "float32", "linear", n_rows, False), eng, users, None, n_rows)
    for alpha in (0.0, 1.0, 0.3):
        want = href.rerank(rows, sims, lambda q, r: table[q, r], n_rows, ex, alpha, 65)
        got = launch(eng, users, rows, sims, None, n_rows, ex, alpha, 65, terms=False)
        check(got[:2] + want[2:4] + got[4:], want, alpha)
        assert (got[2] == -7).all() and (got[3] == -7).all()       # untouched
        m = want[4][0]
        if alpha == 0.0:                                 # the similarities' order: retrieval order
            kept = [r for r in rows[0] if 0 <= r < n_rows and r not in ex[0]]
            assert got[0][0, :m].tolist() == kept
        if alpha == 1.0:                                 # the model's order
            assert (np.diff(table[0, got[0][0, :m]]) <= 0).all()


def test_degenerate_candidate_sets():
    n_rows = 40
    users = np.zeros(4, np.int32)
    eng = make_engine(32, "float32", "linear", n_rows)
    table = score_table((32, "float32", "linear", n_rows, False), eng, users, None, n_rows)
    rows = np.tile(np.arange(8, dtype=np.int32), (4, 1))
    sims = np.tile(np.linspace(0.9, 0.2, 8).astype(F32), (4, 1))
    sims[3] = 0.5                                        # constant similarities
    ex = [set(range(8)), set(range(1, 8)), set(), set()]
    want = href.rerank(rows, sims, lambda q, r: table[q, r], n_rows, ex, 0.7, 8)
    got = launch(eng, users, rows, sims, None, n_rows, ex, 0.7, 8)
    check(got, want, "degenerate")
    o_rows, o_sc, o_mo, o_si, m = got
    assert m.tolist() == [0, 1, 8, 8]
    assert (o_rows[0] == -1).all() and np.isnan(o_sc[0]).all() and np.isnan(o_mo[0]).all()
    assert o_rows[1].tolist() == [0] + [-1] * 7 and o_sc[1, 0] == 0.0      # m = 1: both terms 0
    assert o_mo[1, 0] == table[1, 0] and o_si[1, 0] == sims[1, 0]
    # constant similarities: the model's order
    assert (np.diff(table[3, o_rows[3]]) <= 0).all()
    # constant model scores (every row is the same item): the similarities' order
    same_item = np.full(n_rows, 6, np.int32)
    got = launch(eng, users, rows, sims, same_item, n_rows, ex, 0.7, 8)
    want = href.rerank(rows, sims, lambda q, r: np.full(len(r), table[q, 6]), n_rows, ex, 0.7, 8)
    check(got, want, "constant model")
    assert got[0][2].tolist() == list(range(8)) and (got[2][2] == table[2, 6]).all()
    assert (got[1][3] == 0).all() and got[0][3].tolist() == list(range(8))  # both constant: ties


def test_ties_come_out_in_retrieval_order():
    """Duplicate index rows sharing a model item: 35 equal blended scores
    between 3 better and 7 worse candidates, cut by amount = 20."""
    n_rows, n_cand = 60, 45
    users = np.asarray([2, 4], np.int32)
    eng = make_engine(32, "float64", "linear", 30)
    base = score_table(("ties",), eng, users, None, 30)            # [2, 30] per item
    order = np.argsort(-base, axis=1, kind="stable")
    rs = np.random.RandomState(3)
    rows = np.stack([rs.permutation(n_rows)[:n_cand] for _ in range(2)]).astype(np.int32)
    sims = np.empty((2, n_cand), F32)
    sims[:, :3], sims[:, 3:38], sims[:, 38:] = [0.9, 0.8, 0.7], 0.5, np.linspace(0.4, 0.1, 7)
    # the tied rows are spread over the retrieval order
    spread = np.stack([rs.permutation(n_cand) for _ in range(2)])
    for q in range(2):
        rows[q], sims[q] = rows[q][spread[q]], sims[q][spread[q]]
    # one row_item per query: the query's 3 best items, its median item for the 35, 7 worst
    for q in range(2):
        items = np.concatenate([order[q, :3], np.full(35, order[q, 15]), order[q, -7:]])
        ri = np.full(n_rows, -1, np.int32)
        ri[rows[q]] = items[spread[q]]
        want = href.rerank(rows[q:q + 1], sims[q:q + 1], lambda _, r: base[q, ri[r]].astype(F32),
                           n_rows, [set()], 0.7, 20)
        got = launch(eng, users[q:q + 1], rows[q:q + 1], sims[q:q + 1], ri, n_rows, [set()], 0.7,
                     20)
        check(got, want, "ties")
        tied = [int(r) for r, s in zip(rows[q], sims[q]) if s == F32(0.5)]
        assert len(tied) == 35 and got[0][0, 3:20].tolist() == tied[:17]
        assert len(set(got[1][0, 3:20].tolist())) == 1 and got[1][0, 2] > got[1][0, 3]


def test_one_nan_model_score_makes_every_score_nan():
    n_rows = 150
    users = users_of()
    rows, sims, ex = candidates(65, n_rows, 11)
    bad = int(next(r for r in rows[0] if 0 <= r < n_rows and r not in ex[0]))
    eng = make_engine(32, "float32", "linear", n_rows, nan_item=bad)
    table = score_table(("nan", bad), eng, users, None, n_rows)
    assert np.isnan(table[:, bad]).all()
    want = href.rerank(rows, sims, lambda q, r: table[q, r], n_rows, ex, 0.7, 65)
    got = launch(eng, users, rows, sims, None, n_rows, ex, 0.7, 65)
    check(got, want, "nan")
    m = got[4][0]
    kept = [int(r) for r in rows[0] if 0 <= r < n_rows and r not in ex[0]]
    assert np.isnan(got[1][0, :m]).all() and got[0][0, :m].tolist() == kept
    # alpha = 0 keeps the term out of the order but not out of the score: NaN * 0 is NaN
    got0 = launch(eng, users, rows, sims, None, n_rows, ex, 0.0, 65)
    assert np.isnan(got0[1][0, :m]).all() and got0[0][0, :m].tolist() == kept


def test_output_does_not_depend_on_the_launch_geometry():
    n_rows = 2100
    users = users_of()
    rows, sims, ex = candidates(2048, n_rows, 21)
    eng = make_engine(100, "float64", "sigmoid", n_rows)
    one = launch(eng, users, rows, sims, None, n_rows, ex, 0.6, 2048)
    for chunk in (5, 1):
        parts = launch(eng, users, rows, sims, None, n_rows, ex, 0.6, 2048, chunk=chunk)
        for a, b in zip(one, parts):
            assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------- the estimator
@pytest.fixture(scope="module")
def fx():
    return href.load_fixture()


def frames(fx):
    users, items = fx["users"], fx["items"]
    seg = lambda ptr: np.repeat(np.arange(len(users)), np.diff(ptr))  # noqa: E731
    train = pd.DataFrame({"user_id": users[seg(fx["train_ptr"])],
                          "item_id": items[fx["train_codes"]]})
    test = pd.DataFrame({"user_id": users[seg(fx["test_ptr"])],
                         "item_id": items[fx["test_codes"]]})
    emb = pd.DataFrame(fx["embeddings"], columns=[f"e{c:02d}" for c in range(24)])
    emb.insert(0, "item_id", items[fx["index_codes"]])
    return train, test, emb


def stub_model(fx):
    """The fixture's stub as a KernelMF: FP64 linear, its internal ids permuted
    against the fixture's codes."""
    rs = np.random.RandomState(1)
    pu, pi = rs.permutation(len(fx["users"])), rs.permutation(len(fx["items"]))
    m = KernelMF(n_factors=fx["user_factors"].shape[1], kernel="linear", dtype="float64",
                 min_rating=0, max_rating=5, verbose=0, device=DEV)
    m.user_id_map = {str(fx["users"][c]): j for j, c in enumerate(pu)}
    m.item_id_map = {str(fx["items"][c]): j for j, c in enumerate(pi)}
    m.n_users, m.n_items = len(pu), len(pi)
    m.global_mean = float(fx["global_mean"])
    m.user_features = np.ascontiguousarray(fx["user_factors"][pu])
    m.item_features = np.ascontiguousarray(fx["item_factors"][pi])
    m.user_biases = np.ascontiguousarray(fx["user_biases"][pu])
    m.item_biases = np.ascontiguousarray(fx["item_biases"][pi])
    return m


@pytest.fixture(scope="module")
def fitted(fx):
    train, test, emb = frames(fx)
    h = HybridRecommender(model=stub_model(fx), alpha=0.7, candidate_k=int(fx["candidate_k"]),
                          min_profile_items=int(fx["min_profile_items"]), normalize_items=False,
                          device=DEV).fit(train, emb)
    return h, train, test


def test_estimator_reproduces_the_reference_metrics(fx, fitted):
    h, _, test = fitted
    k = int(fx["k"])
    model = h.model
    try:
        for alpha, want in list(zip(fx["alphas"], fx["metrics"])) + [(0.7, fx["metrics_no_model"])]:
            h.alpha = float(alpha)
            h.model = None if want is fx["metrics_no_model"] else model
            got = h.evaluate_topk(test, k=k)
            print(f"alpha {alpha} model {h.model is not None}: {got}, reference {want.tolist()}")
            assert set(got) == {"precision", "recall", "ndcg", "map", "mrr", "n_users_evaluated"}
            assert got["n_users_evaluated"] == len(fx["cand_user"])
            for name, w in zip(("precision", "recall", "ndcg"), want):
                assert abs(got[name] - w) <= 1e-12, (alpha, name)
            both = h.evaluate_topk(test, k=[3, k])
            assert both[k] == got and both[3]["n_users_evaluated"] == got["n_users_evaluated"]
    finally:
        h.alpha, h.model = 0.7, model


def test_estimator_candidates_and_ids_are_the_references(fx, fitted):
    h, _, test = fitted
    ck, k, mp = int(fx["candidate_k"]), int(fx["k"]), int(fx["min_profile_items"])
    users = fx["users"][fx["cand_user"]]
    items_of = lambda rows: fx["items"][fx["index_codes"][rows]].tolist()  # noqa: E731
    try:
        # alpha = 0: the similarities' order is the retrieval order, so the whole
        # list is the recorded candidate list after the drop
        h.alpha = 0.0
        rec = h.recommend_batch(users, amount=ck)
        for j, u in enumerate(users):
            want = fx["cand_rows"][fx["cand_ptr"][j]:fx["cand_ptr"][j + 1]]
            assert rec.loc[rec["user_id"] == u, "item_id"].tolist() == items_of(want), u
        for alpha in fx["alphas"]:
            h.alpha = float(alpha)
            detail = {}
            href.evaluate(fx, float(alpha), True, k, ck, mp, detail)
            rec = h.recommend_batch(users, amount=k)
            assert list(rec.columns) == ["user_id", "item_id", "score", "model_score", "similarity"]
            for u, pos in zip(users, fx["cand_user"]):
                d = detail[int(pos)]
                mine = rec[rec["user_id"] == u]
                assert mine["item_id"].tolist() == items_of(d["rows"][:k]), (alpha, u)
                # 2^-24 per float32 operation, a handful of them on values <= 1
                assert np.abs(mine["score"].to_numpy() - d["score"][:k]).max() < 1e-5
        # rank_items is the position in the whole list
        h.alpha = 0.7
        full = h.recommend_batch(users, amount=ck)
        where = {(u, i): p for u, g in full.groupby("user_id", sort=False)
                 for p, i in enumerate(g["item_id"])}
        ranks = h.rank_items(test)
        assert list(ranks.columns) == ["user_id", "item_id", "rank", "n_candidates"]
        want = [where.get((u, i), -1) for u, i in zip(test["user_id"], test["item_id"])]
        assert ranks["rank"].tolist() == want and (np.asarray(want) >= 0).sum() >= 10
        sizes = full.groupby("user_id", sort=False).size()
        assert (ranks["n_candidates"].to_numpy() == sizes.reindex(test["user_id"]).to_numpy()).all()
        one = h.recommend(users[0], amount=5)
        mine = full.loc[full["user_id"] == users[0], "item_id"].tolist()
        assert one["item_id"].tolist() == mine[:5]
        # unknown users and users without a profile get nothing
        assert len(h.recommend_batch(["nobody"], amount=5)) == 0
        r = h.rank_items(pd.DataFrame({"user_id": ["nobody"], "item_id": [fx["items"][0]]}))
        assert r["rank"].tolist() == [-1] and r["n_candidates"].tolist() == [0]
    finally:
        h.alpha = 0.7


def ratings_frame(fx):
    X = pd.DataFrame({"user_id": fx["users"][fx["rating_user"]],
                      "item_id": fx["items"][fx["rating_item"]]})
    return X, pd.Series(fx["rating"])


@pytest.mark.parametrize("which", ["kernelmf", "implicit_als"])
def test_model_score_is_the_models_own_prediction(fx, which):
    X, y = ratings_frame(fx)
    _, _, emb = frames(fx)
    np.random.seed(5)
    if which == "kernelmf":
        model = KernelMF(n_factors=12, n_epochs=3, lr=0.02, reg=0.05, verbose=0, dtype="float32",
                         device=DEV).fit(X, y)
    else:
        model = ImplicitALSMF(n_factors=12, n_epochs=2, verbose=0, device=DEV).fit(X, y)
    h = HybridRecommender(model=model, alpha=0.5, candidate_k=30, device=DEV).fit(X, emb)
    users = fx["users"][:20].tolist() + ["nobody"]
    rec = h.recommend_batch(users, amount=30)
    assert len(rec) > 200 and rec["user_id"].nunique() == 20
    pred = np.asarray(model.predict(rec[["user_id", "item_id"]], bound_ratings=False))
    assert href.same_bits(rec["model_score"].to_numpy(), pred.astype(F32))
    # normalize_items=True: unit rows, so the similarities are cosines
    assert np.abs(np.linalg.norm(h.item_embeddings, axis=1) - 1).max() < 1e-6
    assert rec["similarity"].abs().max() <= 1 + 1e-5
    # an item the model does not know is scored as predict scores it
    extra = emb.iloc[:1].copy()
    extra["item_id"] = "new-item"
    extra.iloc[0, 1:] = h.user_profiles[0]
    h2 = HybridRecommender(model=model, alpha=0.5, candidate_k=30, device=DEV).fit(
        X, pd.concat([emb, extra]))
    rec2 = h2.recommend_batch([fx["users"][0]], amount=30)
    new = rec2[rec2["item_id"] == "new-item"]
    assert len(new) == 1
    p = model.predict(new[["user_id", "item_id"]], bound_ratings=False)
    assert href.same_bits(new["model_score"].to_numpy(), np.asarray(p).astype(F32))
