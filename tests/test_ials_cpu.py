"""CPU tests of implicit-feedback ALS: the NumPy reference pins the model, the
C ABI validates its arguments before any device work, the estimator validates
before any RNG draw.  No GPU."""

import ctypes

import numpy as np
import pandas as pd
import pytest

import ials_reference as ref

MF_OK, MF_ERR_INVALID, MF_F32, MF_F64 = 0, 1, 0, 1


def _data(seed, nu, ni, nnz, k):
    rs = np.random.RandomState(seed)
    keys = rs.choice(nu * ni, nnz, replace=False)
    u, i = keys // ni, keys % ni
    r = rs.randint(0, 6, nnz).astype(np.float64)
    return u, i, r, rs.normal(0, 0.3, (nu, k)), rs.normal(0, 0.3, (ni, k))


# ------------------------------------------------------------ reference pin
def test_half_sweep_zeroes_the_gradient_of_the_dense_loss():
    nu, ni, k, alpha, reg = 7, 5, 3, 40.0, 0.1
    u, i, r, P, Q = _data(0, nu, ni, 17, k)
    X = ref.half_sweep(u, i, r, Q, nu, alpha, reg, X=P)
    C = np.ones((nu, ni))
    T = np.zeros((nu, ni))
    C[u, i] = 1 + alpha * r
    T[u, i] = r > 0
    seen = np.bincount(u, minlength=nu) > 0
    grad = -2 * (C * (T - X @ Q.T)) @ Q + 2 * reg * X
    assert np.max(np.abs(grad[seen])) <= 1e-10
    assert np.array_equal(X[~seen], P[~seen])          # empty lists are left as given
    # the item side the same way
    Y = ref.half_sweep(i, u, r, X, ni, alpha, reg, X=Q)
    seen = np.bincount(i, minlength=ni) > 0
    grad = -2 * (C * (T - X @ Y.T)).T @ X + 2 * reg * Y
    assert np.max(np.abs(grad[seen])) <= 1e-10


def test_loss_identity_and_descent():
    nu, ni, k, alpha, reg = 120, 90, 16, 40.0, 0.1
    u, i, r, P, Q = _data(1, nu, ni, 2500, k)
    a, b = ref.loss(u, i, r, P, Q, alpha, reg), ref.loss_dense(u, i, r, P, Q, alpha, reg)
    assert abs(a - b) <= 1e-9 * abs(b)
    # every entity has observations here, so each half-sweep is the exact
    # minimiser over its side: the loss cannot increase
    assert np.bincount(u, minlength=nu).min() > 0 and np.bincount(i, minlength=ni).min() > 0
    losses = [b]
    for _ in range(4):
        P = ref.half_sweep(u, i, r, Q, nu, alpha, reg, X=P)
        losses.append(ref.loss(u, i, r, P, Q, alpha, reg))
        Q = ref.half_sweep(i, u, r, P, ni, alpha, reg, X=Q)
        losses.append(ref.loss(u, i, r, P, Q, alpha, reg))
    assert len(losses) == 9
    assert all(y <= x * (1 + 1e-12) for x, y in zip(losses, losses[1:])), losses
    assert abs(losses[-1] - ref.loss_dense(u, i, r, P, Q, alpha, reg)) <= 1e-9 * losses[-1]


# ---------------------------------------------------------------------- ABI
_PTR = ctypes.c_void_p(4096)         # non-NULL, never dereferenced: validation comes first


def _sweep(lib, **kw):
    a = dict(entity_ptr=_PTR, other_ids=_PTR, strengths=_PTR, n_entities=3, other_features=_PTR,
             gram=_PTR, features=_PTR, n_factors=8, dtype=MF_F32, alpha=40.0, reg=0.1)
    a.update(kw)
    return lib.mf_ials_sweep(a["entity_ptr"], a["other_ids"], a["strengths"], a["n_entities"],
                             a["other_features"], a["gram"], a["features"], a["n_factors"],
                             a["dtype"], a["alpha"], a["reg"], None)


def _gramian(lib, **kw):
    a = dict(features=_PTR, n_rows=10, n_factors=8, dtype=MF_F32, workspace=_PTR, gram=_PTR)
    a.update(kw)
    return lib.mf_gramian(a["features"], a["n_rows"], a["n_factors"], a["dtype"], a["workspace"],
                          a["gram"], None)


@pytest.mark.parametrize("bad,name", [
    (dict(dtype=MF_F64), "dtype"), (dict(n_factors=0), "n_factors"),
    (dict(n_factors=129), "n_factors"), (dict(alpha=-1.0), "alpha"),
    (dict(alpha=float("nan")), "alpha"), (dict(alpha=float("inf")), "alpha"),
    (dict(reg=0.0), "reg"), (dict(reg=-0.5), "reg"), (dict(reg=float("nan")), "reg"),
    (dict(reg=float("inf")), "reg"), (dict(n_entities=-1), "n_entities"),
    (dict(entity_ptr=None), "entity_ptr"), (dict(other_ids=None), "other_ids"),
    (dict(strengths=None), "strengths"), (dict(other_features=None), "other_features"),
    (dict(gram=None), "gram"), (dict(features=None), "features")])
def test_ials_sweep_rejects_invalid_arguments(bad, name):
    from matrix_factorization import _lib

    assert _sweep(_lib.load(), **bad) == MF_ERR_INVALID
    err = _lib.last_error()
    assert "mf_ials_sweep" in err and name in err


@pytest.mark.parametrize("bad,name", [
    (dict(dtype=MF_F64), "dtype"), (dict(n_factors=0), "n_factors"),
    (dict(n_factors=129), "n_factors"), (dict(n_rows=-1), "n_rows"),
    (dict(features=None), "features"), (dict(workspace=None), "workspace"),
    (dict(gram=None), "gram"), (dict(gram=None, n_rows=0), "gram")])
def test_gramian_rejects_invalid_arguments(bad, name):
    from matrix_factorization import _lib

    assert _gramian(_lib.load(), **bad) == MF_ERR_INVALID
    err = _lib.last_error()
    assert "mf_gramian" in err and name in err


def test_zero_sizes_are_ok_without_a_device():
    # (mf_gramian with n_rows == 0 writes k * k zeros to device memory: its
    # MF_OK is checked with the GPU tests)
    from matrix_factorization import _lib

    lib = _lib.load()
    assert _sweep(lib, n_entities=0) == MF_OK
    assert _sweep(lib, n_entities=0, entity_ptr=None, features=None) == MF_OK
    assert lib.mf_gramian_workspace_bytes(0, 64) == 0
    assert lib.mf_gramian_workspace_bytes(10, 0) == 0
    assert lib.mf_gramian_workspace_bytes(10, 129) == 0
    # one slab of 1024 rows; 1, 3 and 10 upper 32 x 32 tiles of f32
    assert lib.mf_gramian_workspace_bytes(1024, 32) == 4096
    assert lib.mf_gramian_workspace_bytes(1025, 33) == 2 * 3 * 4096
    assert lib.mf_gramian_workspace_bytes(1, 128) == 10 * 4096
    assert lib.mf_abi_version() == 1


# ---------------------------------------------------------------- estimator
def test_estimator_validates_before_any_rng_draw():
    from sklearn.base import clone

    from matrix_factorization import ImplicitALSMF

    with pytest.raises(ValueError, match="alpha"):
        ImplicitALSMF(alpha=-1)
    with pytest.raises(ValueError, match="reg"):
        ImplicitALSMF(reg=0)
    m = ImplicitALSMF(n_factors=8, alpha=12.5, reg=0.3, verbose=0)
    c = clone(m)
    assert c.alpha == 12.5 and c.get_params() == m.get_params()
    assert m.get_params()["alpha"] == 12.5 and "lr" not in m.get_params()
    assert m.kernel == "linear" and m.dtype == "float32"
    X = pd.DataFrame({"user_id": [1, 1, 2, 3], "item_id": [5, 6, 5, 7]})
    for bad in ([1.0, -2.0, 0.0, 3.0], [1.0, float("nan"), 0.0, 3.0],
                [1.0, float("inf"), 0.0, 3.0]):
        np.random.seed(11)
        before = np.random.get_state()
        with pytest.raises(ValueError, match="strengths"):
            m.fit(X, pd.Series(bad))
        after = np.random.get_state()
        assert before[0] == after[0] and np.array_equal(before[1], after[1])
        assert before[2:] == after[2:]
