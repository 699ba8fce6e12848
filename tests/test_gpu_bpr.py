"""GPU tests of BPR (mf_bpr_sample, mf_bpr_epoch, engine.BPR, BPRMF) against
the NumPy restatement tests/bpr_reference.py (pinned in tests/test_bpr_cpu.py)
on the planted 300 x 200 set.

Bars:
  sampler      integer for integer
  FP64 epoch   parameters and z: |diff| <= 1e-11 max(1, |v|) against the
               sequential sweep over serial_triples (the project's bar for FP64
               epochs against the oracle in serial order; the only rounding
               difference is the order of the k-long dot product and exp's last
               bit); loss and accuracy <= 1e-12
  chunks       n_chunks 1 and 4: the same bits
  FP32 epoch   see test_one_epoch_fp32
  estimator    parameters <= 1e-9, train_loss <= 1e-10 after 3 epochs
"""

import ctypes
import pickle

import numpy as np
import pandas as pd
import pytest

import bpr_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RANKS = [1, 3, 16, 17, 64, 100, 128, 300, 1024]      # no cap below mf_max_factors()


def _engine(case, k, dtype, bias=True):
    from matrix_factorization.engine import BPR, SGDEngine

    eng = SGDEngine(case["u"], case["i"], case["r"], ref.N_USERS, ref.N_ITEMS, k, "linear",
                    dtype, DEV, global_mean=0.0)
    eng.load_params(case["P"], case["Q"], np.zeros(ref.N_USERS),
                    case["b"] if bias else np.zeros(ref.N_ITEMS))
    return eng, BPR(eng)


def _one_epoch(case, k, dtype, update_item=True, n_chunks=1, seed=ref.SEEDS[0]):
    """The fixed case's epoch through engine.BPR's steps with the visit order
    and the seed given (no RNG draw).  Returns (P, Q, b, z by visit position,
    neg, loss, accuracy, n_levels)."""
    eng, bpr = _engine(case, k, dtype)
    assert np.array_equal(bpr.pu, case["pu"]) and np.array_equal(bpr.pi, case["pi"])
    bpr.order[:] = case["order"]
    bpr.sample(seed)
    triples = bpr.readback()
    assert np.array_equal(triples[0], case["triples"][0])
    assert np.array_equal(triples[1], case["triples"][1])
    neg = triples[2]
    sched, offs = bpr.levels(triples, True, update_item, n_chunks)
    kept = bpr.launch(sched, offs, ref.LR, ref.REG, True, update_item)
    loss, acc = bpr.stats_async(kept)
    z = np.full(bpr.n, np.nan)
    z[sched] = bpr.z[:kept].cpu().numpy().astype(np.float64)
    P, Q, _, b = eng.params_numpy()
    return P, Q, b, z, neg, float(loss.item()), float(acc.item()), len(offs) - 1


_CASES, _REFS = {}, {}


def case_of(k):
    if k not in _CASES:
        _CASES[k] = ref.epoch_case(k)
    return _CASES[k]


def ref_of(k, dtype=np.float64, update_item=True):
    """The reference sweep of the fixed case, computed once per (k, dtype)."""
    key = (k, np.dtype(dtype).name, update_item)
    if key not in _REFS:
        c = case_of(k)
        _REFS[key] = ref.sweep(c["P"], c["Q"], c["b"], ref.kept(c["triples"]), ref.LR, ref.REG,
                               dtype, True, update_item)
    return _REFS[key]


def _close(got, want, tol, what):
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"{what}: max scaled |diff| {err.max() if err.size else 0.0:.3e} (bar {tol:.1e})")
    assert err.size == 0 or err.max() <= tol, what


# ------------------------------------------------------------------ sampler
def test_reference_skips_only_the_saturated_users():
    """The condition the other tests rest on, on the reference alone."""
    c = case_of(16)
    for seed in ref.SEEDS:
        tu, _, tj = ref.epoch_triples(c["order"], c["pu"], c["pi"], c["ptr"], c["ids"],
                                      ref.N_ITEMS, seed)
        assert set(tu[tj < 0].tolist()) <= {ref.U_ALL, ref.U_ALMOST}
        assert np.all(tj[tu == ref.U_ALL] == -1) and np.any(tj[tu == ref.U_ALMOST] == -1)


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_sampler_equals_reference(seed):
    c = case_of(16)
    _, bpr = _engine(c, 16, "float32")
    bpr.order[:] = c["order"]
    bpr.sample(seed)
    got = bpr.neg_d[: bpr.n].cpu().numpy()
    want = ref.sample_negatives(c["order"], c["pu"], c["pi"], c["ptr"], c["ids"], ref.N_ITEMS,
                                seed)
    assert np.any(want < 0) and np.any(want >= 0)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- one epoch
@pytest.mark.parametrize("k", RANKS)
def test_one_epoch_fp64(k):
    c = case_of(k)
    P, Q, b, z, neg, loss, acc, nl = _one_epoch(c, k, "float64")
    tu, ti, tj = c["triples"]
    assert np.array_equal(neg, tj)
    rP, rQ, rb, rz = ref_of(k)
    _close(P, rP, 1e-11, f"k={k} P")
    _close(Q, rQ, 1e-11, f"k={k} Q")
    _close(b, rb, 1e-11, f"k={k} b_i")
    keep = tj >= 0
    assert np.all(np.isnan(z[~keep]))
    _close(z[keep], rz, 1e-11, f"k={k} z")
    rl, ra = ref.loss_auc(rz)
    print(f"k={k}: {nl} levels, loss {loss:.12f} (ref {rl:.12f}), accuracy {acc:.6f}")
    assert abs(loss - rl) <= 1e-12 and abs(acc - ra) <= 1e-12
    # users without a kept triple keep their bits: empty, r = 0 only, all skipped
    for u in (ref.U_EMPTY, ref.U_ZERO, ref.U_ALL):
        assert np.array_equal(P[u], c["P"][u])


def test_chunked_levels_give_the_same_bits():
    k = 17
    c = case_of(k)
    a = _one_epoch(c, k, "float64", n_chunks=1)
    b = _one_epoch(c, k, "float64", n_chunks=4)
    assert b[7] > a[7]                                   # more levels, the same sweep
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert np.array_equal(a[3], b[3], equal_nan=True)


# distance of the f32 NumPy run of the recurrence from the FP64 reference on
# the fixed case (max |diff| over P, Q, b_i), measured on the CPU
F32_NUMPY_DISTANCE = {16: 5.22e-7, 17: 2.01e-7, 100: 2.87e-7}


@pytest.mark.parametrize("k", sorted(F32_NUMPY_DISTANCE))
def test_one_epoch_fp32(k):
    """FP32 parameters after one epoch against the FP64 reference.

    An f32 NumPy run of the same recurrence (bpr_reference.sweep with
    dtype=float32, same f32-rounded start) sits at max |diff| = 5.22e-7
    (k = 16), 2.01e-7 (k = 17), 2.87e-7 (k = 100) from the FP64 reference;
    the GPU's fused multiply-adds and hardware exp / rcp differ from NumPy's
    f32 by a few ulp per update, so the bar is 10 x that figure: 5.22e-6,
    2.01e-6, 2.87e-6.  Measured on the MI355X: 4.03e-7, 2.02e-7, 2.87e-7.  The
    NumPy figure is re-measured and printed (it depends on the host's f32 dot
    product order in the last bits) and must itself meet the bar."""
    c = case_of(k)
    rP, rQ, rb, rz = ref_of(k)
    fP, fQ, fb, _ = ref_of(k, np.float32)
    fig = max(np.max(np.abs(x.astype(np.float64) - y)) for x, y in ((fP, rP), (fQ, rQ), (fb, rb)))
    want = F32_NUMPY_DISTANCE[k]
    print(f"k={k}: f32 NumPy distance {fig:.3e} (recorded {want:.3e})")
    bar = 10.0 * want
    assert fig <= bar
    P, Q, b, z, neg, loss, acc, _ = _one_epoch(c, k, "float32")
    assert np.array_equal(neg, c["triples"][2])
    gpu = max(np.max(np.abs(x - y)) for x, y in ((P, rP), (Q, rQ), (b, rb)))
    print(f"k={k}: GPU f32 max |diff| {gpu:.3e} (bar {bar:.3e})")
    assert gpu <= bar
    keep = c["triples"][2] >= 0
    print(f"k={k}: GPU f32 z max |diff| {np.max(np.abs(z[keep] - rz)):.3e}")


def test_frozen_items():
    k = 16
    c = case_of(k)
    P, Q, b, z, neg, _, _, nl = _one_epoch(c, k, "float64", update_item=False)
    assert np.array_equal(Q, c["Q"]) and np.array_equal(b, c["b"])
    tu, _, tj = c["triples"]
    present = np.zeros(ref.N_USERS, bool)
    present[tu[tj >= 0]] = True
    moved = np.any(P != c["P"], axis=1)
    assert np.array_equal(moved, present)
    assert nl == np.bincount(tu[tj >= 0]).max()          # levels by user only
    rP, _, _, rz = ref_of(k, update_item=False)
    _close(P, rP, 1e-11, "frozen items P")
    _close(z[tj >= 0], rz, 1e-11, "frozen items z")


def test_engine_requirements():
    from matrix_factorization.engine import BPR, SGDEngine

    c = case_of(16)
    eng = SGDEngine(c["u"], c["i"], c["r"], ref.N_USERS, ref.N_ITEMS, 16, "linear", "float64",
                    DEV, global_mean=0.5)
    eng.load_params(c["P"], c["Q"], np.zeros(ref.N_USERS), c["b"])
    with pytest.raises(ValueError, match="global mean"):
        BPR(eng)
    eng = SGDEngine(c["u"], c["i"], c["r"], ref.N_USERS, ref.N_ITEMS, 16, "linear", "float64",
                    DEV, global_mean=0.0)
    eng.load_params(c["P"], c["Q"], np.full(ref.N_USERS, 0.1), c["b"])
    with pytest.raises(ValueError, match="user biases"):
        BPR(eng)
    eng = SGDEngine(c["u"], c["i"], c["r"], ref.N_USERS, ref.N_ITEMS, 16, "sigmoid", "float64",
                    DEV, global_mean=0.0)
    eng.load_params(c["P"], c["Q"], np.zeros(ref.N_USERS), c["b"])
    with pytest.raises(ValueError, match="linear"):
        BPR(eng)


def test_epoch_draws_and_serial_triples():
    """BPR.epoch: shuffle then seed from the global RandomState; the recorded
    triples are the reference's kept triples of the same draws."""
    k = 3
    c = case_of(k)
    eng, bpr = _engine(c, k, "float64")
    bpr.record = True
    np.random.seed(12)
    stats = [bpr.epoch(ref.LR, ref.REG) for _ in range(2)]
    after = np.random.get_state()[1].copy()
    np.random.seed(12)
    order = np.arange(len(c["pu"]), dtype=np.int32)
    P, Q, b = c["P"], c["Q"], c["b"]
    for ep in range(2):
        np.random.shuffle(order)
        seed = int(np.random.randint(0, 2 ** 64, dtype=np.uint64))
        tr = ref.kept(ref.epoch_triples(order, c["pu"], c["pi"], c["ptr"], c["ids"],
                                        ref.N_ITEMS, seed))
        got = bpr.serial_triples(ep)
        assert all(np.array_equal(a, b_) for a, b_ in zip(got, tr))
        P, Q, b, z = ref.sweep(P, Q, b, tr, ref.LR, ref.REG)
        assert abs(float(stats[ep][0].item()) - ref.loss_auc(z)[0]) <= 1e-12
    assert np.array_equal(np.random.get_state()[1], after)
    gP, gQ, _, gb = eng.params_numpy()
    _close(gP, P, 1e-11, "two epochs P")
    _close(gQ, Q, 1e-11, "two epochs Q")
    _close(gb, b, 1e-11, "two epochs b_i")


# ---------------------------------------------------------------- estimator
HP = dict(n_factors=8, n_epochs=3, lr=0.05, reg=0.01)


def _frame():
    u, i, r = ref.make_dataset()
    X = pd.DataFrame({"user_id": u.astype(np.int64) + 1000, "item_id": i.astype(np.int64) + 50})
    return X, pd.Series(r)


@pytest.fixture(scope="module")
def fitted():
    from matrix_factorization import BPRMF

    X, y = _frame()
    np.random.seed(9)
    m = BPRMF(dtype="float64", verbose=0, device=DEV, **HP).fit(X, y)
    return m, X, y


def test_fit_matches_reference(fitted):
    import oracle

    m, X, y = fitted
    np.random.seed(9)
    Xp, uids, iids = oracle.preprocess_fit(X, y)
    k = HP["n_factors"]
    P = np.random.normal(0, 0.1, (len(uids), k))
    Q = np.random.normal(0, 0.1, (len(iids), k))
    arr = Xp.to_numpy(np.float64)
    uu, ii, rr = arr[:, 0].astype(np.int32), arr[:, 1].astype(np.int32), arr[:, 2]
    assert list(m.user_id_map) == list(uids) and list(m.item_id_map) == list(iids)
    pu, pi = ref.positives(uu, ii, rr)
    P, Q, b, loss, acc = ref.run_epochs(pu, pi, len(uids), len(iids), P, Q, np.zeros(len(iids)),
                                        HP["n_epochs"], HP["lr"], HP["reg"])
    assert np.max(np.abs(m.user_features - P)) <= 1e-9
    assert np.max(np.abs(m.item_features - Q)) <= 1e-9
    assert np.max(np.abs(m.item_biases - b)) <= 1e-9
    print("train_loss", m.train_loss, "reference", loss)
    assert len(m.train_loss) == 3 and np.max(np.abs(np.array(m.train_loss) - loss)) <= 1e-10
    assert len(m.train_auc) == 3 and np.max(np.abs(np.array(m.train_auc) - acc)) <= 1e-12
    assert m.global_mean == 0.0 and np.all(m.user_biases == 0)
    assert not hasattr(m, "train_rmse")
    # predict is the plain score, unclipped by default
    pairs = X.iloc[:200]
    ui = np.array([m.user_id_map[x] for x in pairs["user_id"]])
    ij = np.array([m.item_id_map[x] for x in pairs["item_id"]])
    want = np.einsum("nk,nk->n", P[ui], Q[ij]) + b[ij]
    pred = np.asarray(m.predict(pairs))
    assert np.max(np.abs(pred - want)) <= 1e-9
    assert pred.min() < 0 or pred.max() > 1                 # not clipped to [0, 1]


def test_serving(fitted):
    m, X, y = fitted
    user = int(X["user_id"].iloc[0])
    known = X.loc[X["user_id"] == user, "item_id"].tolist()
    rec = m.recommend(user, amount=10, items_known=known, bound_ratings=False)
    assert len(rec) == 10 and not set(rec["item_id"]) & set(known)
    assert np.all(np.diff(rec["rating_pred"].to_numpy()) <= 0)
    users = X["user_id"].unique()[:30].tolist()
    batch = m.recommend_batch(users, amount=5, exclude_known=X, bound_ratings=False)
    train = set(zip(X.user_id, X.item_id))
    assert len(batch) and not any((a, b) in train for a, b in zip(batch.user_id, batch.item_id))
    # held-out pairs: evaluate_topk runs and a trained model beats chance
    rs = np.random.RandomState(0)
    held = pd.DataFrame({"user_id": rs.choice(users, 200), "item_id": rs.randint(50, 250, 200)})
    held = held[~held.apply(tuple, axis=1).isin(train)]
    res = m.evaluate_topk(held, k=10, exclude_known=X)
    assert 0.0 <= res["auc"] <= 1.0 and np.isfinite(res["ndcg"])
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.train_loss == m.train_loss and m2.train_auc == m.train_auc
    assert all(isinstance(v, (np.ndarray, dict, list, int, float, str, bool, type(None)))
               for v in m.__getstate__().values())
    assert np.array_equal(np.asarray(m2.predict(X.iloc[:300])), np.asarray(m.predict(X.iloc[:300])))


def test_update_users_matches_reference():
    from matrix_factorization import BPRMF

    X, y = _frame()
    k = HP["n_factors"]
    np.random.seed(9)
    m = BPRMF(dtype="float64", verbose=0, device=DEV, **HP).fit(X, y)
    P0, Q0, b0 = m.user_features.copy(), m.item_features.copy(), m.item_biases.copy()
    sel = X["user_id"].isin([1003, 1004, 1010])
    Xn = X[sel].copy()
    Xn.loc[Xn["user_id"] == 1004, "user_id"] = 99_999        # a new user
    yn = y[sel]
    np.random.seed(21)
    m.update_users(Xn, yn, n_epochs=2)
    assert np.array_equal(m.item_features, Q0) and np.array_equal(m.item_biases, b0)
    assert m.user_features.shape[0] == P0.shape[0] + 1 and m.user_id_map[99_999] == P0.shape[0]
    others = [m.user_id_map[x] for x in m.user_id_map if x not in (1003, 1010, 99_999)]
    assert np.array_equal(m.user_features[others], P0[others])
    # the reference on the same draws: sample, one normal per known user in
    # first-appearance order, the new users' block, then the epochs' draws
    np.random.seed(21)
    Xs = Xn.assign(rating=yn).sample(frac=1, replace=False)
    P = np.vstack([P0, np.zeros((1, k))])
    for user in Xs["user_id"].unique():
        if user != 99_999:
            P[m.user_id_map[user]] = np.random.normal(0, 0.1, (1, k))
    P[-1:] = np.random.normal(0, 0.1, (1, k))
    uu = np.array([m.user_id_map[x] for x in Xs["user_id"]], np.int32)
    ii = np.array([m.item_id_map[x] for x in Xs["item_id"]], np.int32)
    pu, pi = ref.positives(uu, ii, Xs["rating"].to_numpy())
    P, _, _, loss, _ = ref.run_epochs(pu, pi, len(P), len(Q0), P, Q0, b0, 2, HP["lr"],
                                      HP["reg"], update_item=False)
    assert np.max(np.abs(m.user_features - P)) <= 1e-9
    assert len(m.train_loss) == 2 and np.max(np.abs(np.array(m.train_loss) - loss)) <= 1e-10


def test_validation_draws_nothing():
    from matrix_factorization import BPRMF

    X, y = _frame()
    for kw in (dict(lr=0.0), dict(lr=float("nan")), dict(reg=-0.1), dict(reg=float("inf"))):
        with pytest.raises(ValueError, match=next(iter(kw))):
            BPRMF(**kw)
    np.random.seed(3)
    before = np.random.get_state()
    for attr, val in (("lr", -1.0), ("reg", float("nan"))):
        m = BPRMF(verbose=0, device=DEV, **HP)
        setattr(m, attr, val)
        with pytest.raises(ValueError, match=attr):
            m.fit(X, y)
    for bad in (-1.0, float("nan"), float("inf")):
        yb = y.copy()
        yb.iloc[5] = bad
        with pytest.raises(ValueError, match="strengths"):
            BPRMF(verbose=0, device=DEV, **HP).fit(X, yb)
    after = np.random.get_state()
    assert before[2] == after[2] and np.array_equal(before[1], after[1])


# -------------------------------------------------------------------- C ABI
def test_c_abi_validation():
    import torch

    from matrix_factorization import _lib

    lib = _lib.load()
    assert lib.mf_bpr_max_factors() == lib.mf_max_factors()
    kmax = lib.mf_bpr_max_factors()
    d = torch.zeros(64, dtype=torch.float64, device=DEV)
    ids = torch.zeros(8, dtype=torch.int32, device=DEV)
    ptr64 = torch.zeros(8, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    offs = np.array([0, 1], np.int64)
    ho = offs.ctypes.data_as(ctypes.c_void_p)

    def epoch(**kw):
        a = dict(u=p(ids), i=p(ids), j=p(ids), n=1, order=None, offs=ho, nb=1, seq=None, nseq=0,
                 bi=p(d), P=p(d), Q=p(d), nu=1, ni=2, k=4, dtype=1, z=p(d))
        a.update(kw)
        return lib.mf_bpr_epoch(a["u"], a["i"], a["j"], a["n"], a["order"], a["offs"], a["nb"],
                                a["seq"], a["nseq"], a["bi"], a["P"], a["Q"], a["nu"], a["ni"],
                                a["k"], a["dtype"], 0.05, 0.01, 1, 1, a["z"], None)

    for kw, name in ((dict(dtype=7), "dtype"), (dict(k=kmax + 1), "n_factors"),
                     (dict(k=-1), "n_factors"), (dict(n=-1), "n_triples"),
                     (dict(nb=-1), "n_batches"), (dict(nu=-1), "n_users"),
                     (dict(ni=-1), "n_items"), (dict(u=None), "user_ids"),
                     (dict(i=None), "item_ids"), (dict(j=None), "neg_items"),
                     (dict(bi=None), "item_biases"), (dict(P=None), "user_features"),
                     (dict(Q=None), "item_features"), (dict(z=None), "z_out"),
                     (dict(offs=None), "batch_offsets"),
                     (dict(n=0, offs=np.array([0, 5], np.int64).ctypes.data_as(ctypes.c_void_p)),
                      None)):
        rc = epoch(**kw)
        if name is None:
            assert rc == 0                                   # no triples: MF_OK
        else:
            assert rc == 1 and name in _lib.last_error(), (kw, _lib.last_error())
    bad = np.array([0, 3], np.int64)                         # a batch past n_triples
    assert epoch(offs=bad.ctypes.data_as(ctypes.c_void_p)) == 1
    assert "batch_offsets" in _lib.last_error()
    assert epoch(nb=0) == 0                                  # no batch: MF_OK

    def sample(**kw):
        a = dict(order=None, pu=p(ids), pi=p(ids), n=1, ptr=p(ptr64), lst=p(ids), nu=1, ni=2,
                 neg=p(ids))
        a.update(kw)
        return lib.mf_bpr_sample(a["order"], a["pu"], a["pi"], a["n"], a["ptr"], a["lst"],
                                 a["nu"], a["ni"], 1, a["neg"], None)

    for kw, name in ((dict(n=-1), "n_pos"), (dict(nu=-1), "n_users"), (dict(ni=-1), "n_items"),
                     (dict(ni=0), "n_items"), (dict(pu=None), "pos_users"),
                     (dict(pi=None), "pos_items"), (dict(ptr=None), "user_ptr"),
                     (dict(lst=None), "user_items"), (dict(neg=None), "neg_items")):
        assert sample(**kw) == 1 and name in _lib.last_error(), (kw, _lib.last_error())
    assert sample(n=0, pu=None, pi=None, neg=None) == 0      # no positives: MF_OK
    torch.cuda.synchronize()
