"""GPU tests of the conjugate-gradient solver of implicit-feedback ALS
(mf_ials_sweep_cg, ImplicitALS(..., cg_steps), ImplicitALSMF(solver="cg"))
against the NumPy FP64 restatement of the recurrence, tests/ials_cg_reference.py
(pinned against the dense solve in tests/test_ials_cg_cpu.py).

The GPU assembles each system in f32 on MFMA and runs the recurrence in f32;
the reference does both in f64 from the same f32-rounded inputs.  Bars -- the
project's own (tests/test_gpu_ials.py):
  parameters   max |diff| <= 2e-4 * max(1, |value|)
  train loss   relative diff <= 1e-5
An f32 NumPy run of the same recurrence sits at <= 9.4e-7 (3 steps) and
<= 8.3e-6 (3k + 10 steps, k <= 33) from the FP64 reference on this data, and
at 3e-8 relative on a 4-epoch loss; every test prints its measured maximum.
"""

import ctypes
import pickle

import numpy as np
import pandas as pd
import pytest

import ials_cg_reference as cgref
import ials_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NU, NI, REG = cgref.NU, cgref.NI, cgref.REG
ZERO_USER, EMPTY_USER = cgref.ZERO_USER, cgref.EMPTY_USER
TOL = 2e-4


@pytest.fixture(scope="module")
def sweep_data():
    return cgref.sweep_data()


def _err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


def _close(a, b, tol, what):
    err = _err(a, b)
    print(f"{what}: max rel diff {err:.3e}")
    assert err <= tol, f"{what}: max rel diff {err:.3e} > {tol:.0e}"


def _engine(data, k, P, Q):
    from matrix_factorization.engine import ImplicitALS, SGDEngine

    u, i, r = data
    eng = SGDEngine(u, i, r, NU, NI, k, "linear", "float32", DEV, global_mean=0.0,
                    min_rating=0, max_rating=1)
    eng.load_params(P, Q, np.zeros(NU), np.zeros(NI))
    return eng, ImplicitALS(eng)


# ------------------------------------------------------------ half-sweeps
@pytest.mark.parametrize("alpha", [0.0, 40.0])
@pytest.mark.parametrize("k", [1, 3, 20, 32, 33, 64, 65, 100, 128])
def test_half_sweeps_match_cg_reference(sweep_data, k, alpha):
    u, i, r = sweep_data
    P, Q = cgref.start_rows(k)
    eng, als = _engine(sweep_data, k, P, Q)
    als.sweep_users(alpha, REG, cg_steps=3)
    Pg, Qg, bug, big = eng.params_numpy()
    P_ref = cgref.half_sweep(u, i, r, Q, NU, alpha, REG, P, 3)
    P_f32 = cgref.half_sweep(u, i, r, Q, NU, alpha, REG, P, 3, np.float32)
    assert np.all(np.isfinite(Pg))
    assert np.array_equal(Pg[EMPTY_USER], P[EMPTY_USER].astype(np.float64))   # row kept
    assert np.array_equal(Qg, Q.astype(np.float64))          # the fixed side untouched
    assert np.all(bug == 0) and np.all(big == 0)
    print(f"k={k} alpha={alpha}: f32 NumPy vs FP64 {_err(P_f32, P_ref):.3e}")
    _close(Pg, P_ref, TOL, f"user half-sweep cg3 k={k} alpha={alpha}")
    # three steps are not the solve (beyond k = 3): the zero-strength user
    # moves towards 0, it is not set to it
    assert np.any(Pg[ZERO_USER] != 0) or k <= 3
    # item half-sweep from the GPU's user side
    als.sweep_items(alpha, REG, cg_steps=3)
    Pg2, Qg2, bug, big = eng.params_numpy()
    assert np.array_equal(Pg2, Pg) and np.all(np.isfinite(Qg2))
    assert np.all(bug == 0) and np.all(big == 0)
    Q_ref = cgref.half_sweep(i, u, r, Pg, NI, alpha, REG, Q, 3)
    _close(Qg2, Q_ref, TOL, f"item half-sweep cg3 k={k} alpha={alpha}")


@pytest.mark.parametrize("k", [8, 33])
def test_many_steps_converge_to_the_direct_solve(sweep_data, k):
    u, i, r = sweep_data
    P, Q = cgref.start_rows(k)
    eng, als = _engine(sweep_data, k, P, Q)
    als.sweep_users(40.0, REG, cg_steps=3 * k + 10)
    Pg = eng.params_numpy()[0]
    want = ref.half_sweep(u, i, r, Q, NU, 40.0, REG, X=P)
    assert np.all(np.isfinite(Pg))
    _close(Pg, want, TOL, f"cg{3 * k + 10} vs direct k={k}")
    print(f"k={k}: zero-strength user max |x| {np.max(np.abs(Pg[ZERO_USER])):.3e}")
    assert np.all(want[ZERO_USER] == 0) and np.max(np.abs(Pg[ZERO_USER])) <= TOL
    assert np.array_equal(Pg[EMPTY_USER], P[EMPTY_USER].astype(np.float64))


def test_rank_one_stops_and_equals_the_direct_solve(sweep_data):
    """k = 1: the first step is the solve; the other twelve run into the rs
    rule (or act on a rounding-level residual) without a 0 / 0."""
    u, i, r = sweep_data
    P, Q = cgref.start_rows(1)
    eng, als = _engine(sweep_data, 1, P, Q)
    als.sweep_users(40.0, REG, cg_steps=13)
    Pg = eng.params_numpy()[0]
    assert np.all(np.isfinite(Pg))
    _close(Pg, ref.half_sweep(u, i, r, Q, NU, 40.0, REG, X=P), TOL, "cg13 vs direct k=1")


def test_warm_start_is_read(sweep_data):
    """From the (f32-rounded) direct solution three steps have nothing left to
    do; from any other start they would be far from it (the half-sweep test)."""
    u, i, r = sweep_data
    k = 64
    P, Q = cgref.start_rows(k)
    sol = ref.half_sweep(u, i, r, Q, NU, 40.0, REG, X=P).astype(np.float32)
    eng, als = _engine(sweep_data, k, sol, Q)
    als.sweep_users(40.0, REG, cg_steps=3)
    Pg = eng.params_numpy()[0]
    _close(Pg, sol, TOL, "cg3 from the direct solution k=64")
    cold = cgref.half_sweep(u, i, r, Q, NU, 40.0, REG, P, 3)
    print(f"cg3 from the random start is {_err(cold, sol):.3e} from the solution")
    assert _err(cold, sol) > 10 * TOL            # the start matters at three steps


def test_same_input_same_bits(sweep_data):
    k = 100
    P, Q = cgref.start_rows(k)
    out = []
    for _ in range(2):
        eng, als = _engine(sweep_data, k, P, Q)
        als.sweep_users(40.0, REG, cg_steps=3)
        als.sweep_items(40.0, REG, cg_steps=3)
        Pg, Qg, _, _ = eng.params_numpy()
        out.append((Pg, Qg))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert not np.array_equal(out[0][0], P.astype(np.float64))


def test_zero_entities_is_ok():
    import torch

    from matrix_factorization import _lib

    st = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    assert _lib.call("mf_ials_sweep_cg", None, None, None, 0, None, None, None, 8, 0, 40.0, 0.1,
                     3, st) == 0
    torch.cuda.synchronize()


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
    hp = dict(n_factors=48, n_epochs=4, alpha=40, reg=0.05, verbose=0)
    np.random.seed(9)
    m = ImplicitALSMF(solver="cg", cg_steps=3, **hp).fit(X, pd.Series(r))
    np.random.seed(9)
    d = ImplicitALSMF(**hp).fit(X, pd.Series(r))
    return m, d, X, r


def test_fit_matches_cg_reference(fitted):
    import oracle

    m, d, X, r = fitted
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
        P = cgref.half_sweep(uu, ii, rr, Q, len(uids), 40.0, 0.05, P, 3)
        Q = cgref.half_sweep(ii, uu, rr, P, len(iids), 40.0, 0.05, Q, 3)
        losses.append(ref.loss(uu, ii, rr, P, Q, 40.0, 0.05))
    got, want = np.array(m.train_loss), np.array(losses)
    print("train_loss cg3", got.tolist(), "reference", want.tolist(),
          "rel diff", (np.abs(got - want) / want).tolist(), "direct", d.train_loss)
    assert len(got) == 4 and np.max(np.abs(got - want) / want) <= 1e-5
    assert all(b < a for a, b in zip(got, got[1:]))
    # three steps from a random start are not the exact solve
    assert abs(got[0] - d.train_loss[0]) > 1e-3 * d.train_loss[0]
    assert m.solver == "cg" and m.cg_steps == 3 and d.solver == "direct"
    assert m.global_mean == 0.0 and np.all(m.user_biases == 0) and np.all(m.item_biases == 0)
    print(f"fitted rows after 4 epochs: users {_err(m.user_features, P):.3e} "
          f"items {_err(m.item_features, Q):.3e}")
    pairs = X.iloc[:200]
    pred = np.asarray(m.predict(pairs, bound_ratings=False))
    ui = np.array([m.user_id_map[x] for x in pairs["user_id"]])
    ij = np.array([m.item_id_map[x] for x in pairs["item_id"]])
    # an f32 sum of k products: within k 2^-24 sum |x_j y_j| of the exact one
    xy = m.user_features[ui] * m.item_features[ij]
    assert np.all(np.abs(pred - xy.sum(axis=1)) <= 48 * 2.0 ** -24 * np.abs(xy).sum(axis=1))
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.solver == "cg" and m2.cg_steps == 3 and m2.train_loss == m.train_loss


def test_update_users_folds_in_from_the_redrawn_rows():
    from matrix_factorization import ImplicitALSMF

    u, i, r = _pairs(6, 300, 200, 9000)
    X = pd.DataFrame({"user_id": u, "item_id": i})
    np.random.seed(1)
    m = ImplicitALSMF(n_factors=16, n_epochs=2, alpha=40, reg=0.1, verbose=0, solver="cg",
                      cg_steps=3).fit(X, pd.Series(r))
    Q, P = m.item_features.copy(), m.user_features.copy()
    sel = X["user_id"].isin([3, 4])
    Xn = X[sel].copy()
    Xn.loc[Xn["user_id"] == 4, "user_id"] = 10_000          # a new user
    rn = pd.Series(r[sel.to_numpy()], index=Xn.index)
    # the re-drawn / new rows: the same update without a sweep, same RNG state
    m0, m1 = pickle.loads(pickle.dumps(m)), pickle.loads(pickle.dumps(m))
    np.random.seed(21)
    m0.update_users(Xn, rn, n_epochs=0)
    start = m0.user_features
    np.random.seed(21)
    m.update_users(Xn, rn, n_epochs=1)
    assert np.array_equal(m.item_features, Q) and np.all(m.item_biases == 0)
    others = [m.user_id_map[x] for x in m.user_id_map if x not in (3, 10_000)]
    assert np.array_equal(m.user_features[others], P[others])
    assert np.array_equal(start[others], P[others])
    assert m.user_features.shape[0] == P.shape[0] + 1 and m.user_id_map[10_000] == P.shape[0]
    assert len(m.train_loss) == 1 and np.isfinite(m.train_loss[0])
    uu = np.array([m.user_id_map[x] for x in Xn["user_id"]])
    ii = np.array([m.item_id_map[x] for x in Xn["item_id"]])
    want = cgref.half_sweep(uu, ii, rn.to_numpy(), Q, P.shape[0] + 1, 40.0, 0.1, start, 3)
    direct = ref.half_sweep(uu, ii, rn.to_numpy(), Q, P.shape[0] + 1, 40.0, 0.1, X=start)
    assert not np.array_equal(start[m.user_id_map[3]], P[m.user_id_map[3]])   # re-drawn
    for user in (3, 10_000):
        x = m.user_id_map[user]
        _close(m.user_features[x], want[x], TOL, f"fold-in user {user} cg3")
        print(f"fold-in user {user}: cg3 is {_err(want[x], direct[x]):.3e} from the solve")
    # a second fold-in epoch refines instead of repeating: three more steps
    # from the first epoch's rows, so each user's quadratic x^T A x / 2 - b^T x
    # goes further down (after one epoch the rows are still ~0.9 from the
    # solve, above).  The rows are also printed against three FP64 steps from
    # the GPU's own first-epoch rows (the same bits: the kernel is
    # deterministic); this close to the solve a restarted CG amplifies the f32
    # rounding of its first residual by |A| |x| / |res|, so that figure is a
    # measurement, not a bar.
    np.random.seed(21)
    m1.update_users(Xn, rn, n_epochs=2)
    assert len(m1.train_loss) == 2 and np.all(np.isfinite(m1.train_loss))
    want2 = cgref.half_sweep(uu, ii, rn.to_numpy(), Q, P.shape[0] + 1, 40.0, 0.1,
                             m.user_features, 3)
    rows = {m.user_id_map[user]: user for user in (3, 10_000)}
    for e, A, b in cgref.systems(uu, ii, rn.to_numpy(), Q, P.shape[0] + 1, 40.0, 0.1):
        q = [0.5 * x @ A @ x - b @ x for x in (start[e], m.user_features[e], m1.user_features[e])]
        print(f"fold-in user {rows[e]}: quadratic {q[0]:.6f} -> {q[1]:.6f} -> {q[2]:.6f}; "
              f"two epochs vs FP64 steps from the first: {_err(m1.user_features[e], want2[e]):.3e}")
        assert q[2] < q[1] < q[0]
        rows.pop(e)
    assert not rows
