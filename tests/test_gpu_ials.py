"""GPU tests of implicit-feedback ALS (mf_gramian, mf_ials_sweep, ImplicitALS,
ImplicitALSMF) against the NumPy FP64 restatement tests/ials_reference.py
(pinned in tests/test_ials_cpu.py).

The GPU forms the Gramians in f32 on MFMA and eliminates in f32; the reference
solves in f64 from the same f32-rounded inputs.  Bars (stated per test):
  Gramian      exact on small-integer data; on real data the worst case of an
               f32 summation, (n + 2) 2^-24 (|F|^T |F|)_ij
  parameters   max |diff| <= 2e-4 * max(1, |value|)   (test_gpu_als.py's bar for
               the f32 solve at these shapes; an f32 LAPACK solve of the same
               systems sits at 1.8e-5)
  train loss   relative diff <= 1e-5                  (the project's parity bar)
"""

import pickle

import numpy as np
import pandas as pd
import pytest

import ials_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _gramian(F, calls=1):
    """mf_gramian of a host f32 matrix: the (k, k) results of ``calls`` calls."""
    import ctypes

    import torch

    from matrix_factorization import _lib

    lib = _lib.load()
    n, k = F.shape
    Fd = torch.from_numpy(np.ascontiguousarray(F, np.float32)).to(DEV)
    ws = torch.empty(max(lib.mf_gramian_workspace_bytes(n, k), 4) // 4, dtype=torch.float32,
                     device=DEV)
    out = []
    for _ in range(calls):
        G = torch.full((k, k), float("nan"), dtype=torch.float32, device=DEV)
        stream = ctypes.c_void_p(torch.cuda.current_stream(Fd.device).cuda_stream)
        _lib.call("mf_gramian", ctypes.c_void_p(Fd.data_ptr()) if n else None, n, k, 0,
                  ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(G.data_ptr()), stream)
        out.append(G.cpu().numpy())
    return out


@pytest.mark.parametrize("k", [1, 20, 33, 64, 128])
@pytest.mark.parametrize("n", [1, 63, 65, 4097, 70001])
def test_gramian_is_exact_on_integer_data(n, k):
    """F integer-valued in [-3, 3]: every product and partial sum is an
    integer below 9 * 70001 < 2^24, exact in f32 in any order -- a dropped or
    duplicated row at a chunk, slab or tile tail changes the result."""
    rs = np.random.RandomState(1000 * k + n % 997)
    F = rs.randint(-3, 4, (n, k)).astype(np.float32)
    g1, g2 = _gramian(F, calls=2)
    want = F.astype(np.float64).T @ F.astype(np.float64)
    assert np.array_equal(g1.astype(np.float64), want)
    assert np.array_equal(g1, g1.T)
    assert np.array_equal(g1, g2)                      # same input, same bits


def test_gramian_of_no_rows_is_zero():
    (g,) = _gramian(np.zeros((0, 20), np.float32))
    assert g.shape == (20, 20) and np.all(g == 0)


def test_gramian_real_data_within_f32_summation_bound():
    n, k = 70001, 128
    F = np.random.RandomState(3).normal(0, 0.3, (n, k)).astype(np.float32)
    g1, g2 = _gramian(F, calls=2)
    F64 = F.astype(np.float64)
    want = F64.T @ F64
    bound = (n + 2) * 2.0 ** -24 * (np.abs(F64).T @ np.abs(F64))
    ratio = np.max(np.abs(g1 - want) / bound)
    print(f"gramian real data: max |G - G64| / bound = {ratio:.3e}")
    assert ratio <= 1.0
    assert np.array_equal(g1, g1.T) and np.array_equal(g1, g2)


# ------------------------------------------------------------ half-sweeps
NU, NI = 400, 260
EXACT = {390: 1, 391: 63, 392: 64, 393: 65, 394: 128, 395: 129, 396: 250}
ZERO_USER, EMPTY_USER = 397, 399


def _sweep_data():
    """14000 random pairs over users 0..398, then users 390..396 with lists of
    exactly 1, 63, 64, 65, 128, 129 and 250 items (chunk boundaries of the
    kernel), user 397 with all-zero strengths, user 399 without any pair."""
    rs = np.random.RandomState(42)
    keys = rs.choice((NU - 1) * NI, 14000, replace=False)
    u, i = keys // NI, keys % NI
    keep = ~np.isin(u, list(EXACT) + [ZERO_USER])
    u, i = u[keep], i[keep]
    r = rs.randint(0, 6, len(u)).astype(np.float64)
    us, its, rr = [u], [i], [r]
    for user, deg in EXACT.items():
        us.append(np.full(deg, user))
        its.append(rs.choice(NI, deg, replace=False))
        rr.append(rs.randint(0, 6, deg).astype(np.float64))
    us.append(np.full(17, ZERO_USER))
    its.append(rs.choice(NI, 17, replace=False))
    rr.append(np.zeros(17))
    u, i, r = np.concatenate(us), np.concatenate(its), np.concatenate(rr)
    p = rs.permutation(len(u))
    return u[p].astype(np.int32), i[p].astype(np.int32), r[p]


@pytest.fixture(scope="module")
def sweep_data():
    u, i, r = _sweep_data()
    deg = np.bincount(u, minlength=NU)
    assert all(deg[user] == d for user, d in EXACT.items()) and deg[EMPTY_USER] == 0
    assert 0.10 < np.mean(r == 0) < 0.22 and deg[:390].min() > 0
    return u, i, r


def _close(a, b, tol, what):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    err = np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))
    print(f"{what}: max rel diff {err:.3e}")
    assert err <= tol, f"{what}: max rel diff {err:.3e} > {tol:.0e}"


@pytest.mark.parametrize("alpha", [0.0, 40.0])
@pytest.mark.parametrize("k", [1, 8, 20, 33, 64, 100, 128])
def test_half_sweeps_match_reference(sweep_data, k, alpha):
    from matrix_factorization.engine import ImplicitALS, SGDEngine

    u, i, r = sweep_data
    rs = np.random.RandomState(100 + k)
    P = rs.normal(0, 0.3, (NU, k)).astype(np.float32)
    Q = rs.normal(0, 0.3, (NI, k)).astype(np.float32)
    reg = 0.1
    eng = SGDEngine(u, i, r, NU, NI, k, "linear", "float32", DEV, global_mean=0.0,
                    min_rating=0, max_rating=1)
    eng.load_params(P, Q, np.zeros(NU), np.zeros(NI))
    als = ImplicitALS(eng)
    als.sweep_users(alpha, reg)
    Pg, Qg, bug, big = eng.params_numpy()
    P_ref = ref.half_sweep(u, i, r, Q, NU, alpha, reg, X=P)
    assert np.array_equal(Pg[EMPTY_USER], P[EMPTY_USER].astype(np.float64))   # row kept
    assert np.all(Pg[ZERO_USER] == 0) and np.all(P_ref[ZERO_USER] == 0)
    assert np.array_equal(Qg, Q.astype(np.float64))          # the fixed side untouched
    assert np.all(bug == 0) and np.all(big == 0)
    _close(Pg, P_ref, 2e-4, f"user half-sweep k={k} alpha={alpha}")
    # item half-sweep from the GPU's user side
    als.sweep_items(alpha, reg)
    Pg2, Qg2, _, _ = eng.params_numpy()
    assert np.array_equal(Pg2, Pg)
    Q_ref = ref.half_sweep(i, u, r, Pg, NI, alpha, reg, X=Q)
    _close(Qg2, Q_ref, 2e-4, f"item half-sweep k={k} alpha={alpha}")
    # the device loss against the identity and the definition
    got = als.loss(alpha, reg)
    want = ref.loss_dense(u, i, r, Pg2, Qg2, alpha, reg)
    print(f"loss k={k} alpha={alpha}: rel diff {abs(got - want) / want:.3e}")
    assert abs(got - want) <= 1e-5 * want


def test_engine_requirements():
    from matrix_factorization.engine import ImplicitALS, SGDEngine

    u, i, r = np.array([0, 1], np.int32), np.array([1, 0], np.int32), np.array([1.0, 2.0])
    z2 = np.zeros(2)
    f = np.ones((2, 4), np.float32)
    eng = SGDEngine(u, i, r, 2, 2, 4, "linear", "float32", DEV, global_mean=0.5)
    eng.load_params(f, f, z2, z2)
    with pytest.raises(ValueError, match="global mean"):
        ImplicitALS(eng)
    eng = SGDEngine(u, i, r, 2, 2, 4, "linear", "float32", DEV, global_mean=0.0)
    eng.load_params(f, f, z2, np.array([0.0, 0.1]))
    with pytest.raises(ValueError, match="biases"):
        ImplicitALS(eng)
    eng = SGDEngine(u, i, r, 2, 2, 4, "linear", "float64", DEV, global_mean=0.0)
    eng.load_params(f, f, z2, z2)
    with pytest.raises(ValueError, match="float32"):
        ImplicitALS(eng)


# -------------------------------------------------------------- estimator
def _pairs(seed, nu, ni, nnz):
    rs = np.random.RandomState(seed)
    keys = rs.choice(nu * ni, nnz, replace=False)
    return (keys // ni).astype(np.int64), (keys % ni).astype(np.int64), \
        rs.randint(0, 6, nnz).astype(np.float64)


@pytest.fixture(scope="module")
def fitted():
    from matrix_factorization import ImplicitALSMF

    u, i, r = _pairs(5, 500, 300, 20000)
    X = pd.DataFrame({"user_id": u, "item_id": i})
    np.random.seed(9)
    m = ImplicitALSMF(n_factors=48, n_epochs=4, alpha=40, reg=0.05, verbose=0).fit(X, pd.Series(r))
    return m, X, r


def test_fit_matches_reference(fitted):
    import oracle

    m, X, r = fitted
    # reference: same preprocessing / RNG order as the estimator
    np.random.seed(9)
    Xp, uids, iids = oracle.preprocess_fit(X, pd.Series(r))
    P = np.random.normal(0, 0.1, (len(uids), 48)).astype(np.float32).astype(np.float64)
    Q = np.random.normal(0, 0.1, (len(iids), 48)).astype(np.float32).astype(np.float64)
    arr = Xp.to_numpy(np.float64)
    uu, ii, rr = arr[:, 0].astype(np.int64), arr[:, 1].astype(np.int64), arr[:, 2]
    assert list(m.user_id_map) == list(uids) and list(m.item_id_map) == list(iids)
    losses = []
    for _ in range(4):
        P = ref.half_sweep(uu, ii, rr, Q, len(uids), 40.0, 0.05, X=P)
        Q = ref.half_sweep(ii, uu, rr, P, len(iids), 40.0, 0.05, X=Q)
        losses.append(ref.loss(uu, ii, rr, P, Q, 40.0, 0.05))
    got, want = np.array(m.train_loss), np.array(losses)
    print("train_loss", got.tolist(), "reference", want.tolist(),
          "rel diff", (np.abs(got - want) / want).tolist())
    assert len(got) == 4 and np.max(np.abs(got - want) / want) <= 1e-5
    assert all(b < a for a, b in zip(got, got[1:]))
    assert not hasattr(m, "train_rmse")
    assert m.global_mean == 0.0 and np.all(m.user_biases == 0) and np.all(m.item_biases == 0)
    pred = np.asarray(m.predict(X.iloc[:200], bound_ratings=False))
    ui = np.array([m.user_id_map[x] for x in X["user_id"].iloc[:200]])
    ij = np.array([m.item_id_map[x] for x in X["item_id"].iloc[:200]])
    po = np.einsum("nk,nk->n", P[ui], Q[ij])
    print("predict: max |diff|", np.max(np.abs(pred - po)))
    assert np.max(np.abs(pred - po)) < 1e-3


def test_serving(fitted):
    m, X, r = fitted
    users = X["user_id"].unique()[:40].tolist()
    known = X[X["user_id"].isin(users)]
    rec = m.recommend_batch(users, amount=10, exclude_known=known, bound_ratings=False)
    assert len(rec) == 10 * len(users)
    train = set(zip(known.user_id, known.item_id))
    assert not any((a, b) in train for a, b in zip(rec.user_id, rec.item_id))
    pairs = pd.DataFrame({"user_id": rec["user_id"].astype(np.int64),
                          "item_id": rec["item_id"].astype(np.int64)})
    pred = np.asarray(m.predict(pairs, bound_ratings=False))
    assert np.array_equal(rec["rating_pred"].to_numpy(), pred)
    # scores are plain dot products of the synchronised parameters
    ui = np.array([m.user_id_map[x] for x in pairs["user_id"]])
    ij = np.array([m.item_id_map[x] for x in pairs["item_id"]])
    # (an f32 sum of k products: within k 2^-24 sum |x_j y_j| of the exact one)
    xy = m.user_features[ui] * m.item_features[ij]
    assert np.all(np.abs(pred - xy.sum(axis=1)) <= 48 * 2.0 ** -24 * np.abs(xy).sum(axis=1))
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.alpha == 40 and m2.train_loss == m.train_loss
    assert np.array_equal(np.asarray(m2.predict(X.iloc[:300], bound_ratings=False)),
                          np.asarray(m.predict(X.iloc[:300], bound_ratings=False)))


def test_update_users_folds_in_with_items_frozen():
    from matrix_factorization import ImplicitALSMF

    u, i, r = _pairs(6, 300, 200, 9000)
    X = pd.DataFrame({"user_id": u, "item_id": i})
    np.random.seed(1)
    m = ImplicitALSMF(n_factors=16, n_epochs=2, alpha=40, reg=0.1, verbose=0).fit(X, pd.Series(r))
    Q, P = m.item_features.copy(), m.user_features.copy()
    sel = X["user_id"].isin([3, 4])
    Xn = X[sel].copy()
    Xn.loc[Xn["user_id"] == 4, "user_id"] = 10_000          # a new user
    rn = r[sel.to_numpy()]
    m.update_users(Xn, pd.Series(rn, index=Xn.index), n_epochs=1)
    assert np.array_equal(m.item_features, Q) and np.all(m.item_biases == 0)
    others = [m.user_id_map[x] for x in m.user_id_map if x not in (3, 10_000)]
    assert np.array_equal(m.user_features[others], P[others])
    assert m.user_features.shape[0] == P.shape[0] + 1 and m.user_id_map[10_000] == P.shape[0]
    assert len(m.train_loss) == 1 and np.isfinite(m.train_loss[0])
    # the re-solved users against the reference half-sweep on the update data
    uu = np.array([m.user_id_map[x] for x in Xn["user_id"]])
    ii = np.array([m.item_id_map[x] for x in Xn["item_id"]])
    want = ref.half_sweep(uu, ii, rn, Q, P.shape[0] + 1, 40.0, 0.1)
    for user in (3, 10_000):
        x = m.user_id_map[user]
        _close(m.user_features[x], want[x], 2e-4, f"fold-in user {user}")
