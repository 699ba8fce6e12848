"""CPU tests of the conjugate-gradient solver of implicit-feedback ALS: the
NumPy reference of the recurrence (tests/ials_cg_reference.py) is pinned
against the dense solve of tests/ials_reference.py, mf_ials_sweep_cg validates
its arguments before any device work, ImplicitALSMF validates solver / cg_steps
before any RNG draw, and pickles written before the solver choice load with
the exact solve.  No GPU."""

import ctypes
import warnings

import numpy as np
import pandas as pd
import pytest

import ials_cg_reference as cgref
import ials_reference as ref

MF_OK, MF_ERR_INVALID, MF_F32, MF_F64 = 0, 1, 0, 1


@pytest.fixture(scope="module")
def sweep_data():
    return cgref.sweep_data()


# ------------------------------------------------------------ reference pin
@pytest.mark.parametrize("alpha", [0.0, 40.0])
@pytest.mark.parametrize("k", [1, 3, 8, 33])
def test_reference_converges_to_the_dense_solve(sweep_data, k, alpha):
    """CG on a k x k SPD system ends after k steps in exact arithmetic; 3k + 10
    steps in FP64 reach the dense solve to 1e-9 (measured <= 5e-14)."""
    u, i, r = sweep_data
    P, Q = cgref.start_rows(k)
    got = cgref.half_sweep(u, i, r, Q, cgref.NU, alpha, cgref.REG, P, 3 * k + 10)
    want = ref.half_sweep(u, i, r, Q, cgref.NU, alpha, cgref.REG, X=P)
    err = np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))
    print(f"k={k} alpha={alpha}: FP64 CG at {3 * k + 10} steps vs dense solve {err:.3e}")
    assert err <= 1e-9
    assert np.array_equal(got[cgref.EMPTY_USER], P[cgref.EMPTY_USER].astype(np.float64))
    assert np.all(np.isfinite(got))


@pytest.mark.parametrize("alpha", [0.0, 40.0])
@pytest.mark.parametrize("k", [1, 3, 8, 33])
def test_no_step_increases_the_quadratic(sweep_data, k, alpha):
    """A CG step minimises q(x) = x^T A x / 2 - b^T x along p, so q cannot go
    up.  The slack is FP64 rounding: evaluating q costs at most gamma_(2k+2)
    S(x), S(x) = |x|^T |A| |x| + |b|^T |x|, and the recurrence's residual
    drifts from b - A x by rounding errors proportional to the LARGEST iterate
    so far, one lot per step (so once x has converged towards 0 the steps are
    no longer exact line minimisations at the scale of the current q): the
    bound is gamma_(2k+2) x (steps so far + 2) x max S over the iterates so
    far.  Against q(x_0) of order 10 that is 1e-12 at most."""
    u, i, r = sweep_data
    P, Q = cgref.start_rows(k)
    n = 0
    for e, A, b in cgref.systems(u, i, r, Q, cgref.NU, alpha, cgref.REG):
        trace = []
        cgref.cg(A, b, P[e].astype(np.float64), 3 * k + 10, trace=trace)
        q = [0.5 * x @ A @ x - b @ x for x in trace]
        s = [np.abs(x) @ np.abs(A) @ np.abs(x) + np.abs(b) @ np.abs(x) for x in trace]
        for t in range(len(q) - 1):
            slack = (2 * k + 2) * 2.0 ** -52 * (t + 3) * max(s[:t + 2])
            assert q[t + 1] <= q[t] + slack, (e, t, q[t], q[t + 1])
        n += 1
    assert n == cgref.NU - 1                       # every user but the empty one


def test_rank_one_stops_by_the_residual_rule(sweep_data):
    """k = 1: the first step is the exact solve, the residual drops to rounding
    level and the rs rule ends the recurrence well before its 13 steps -- no
    0 / 0, every value finite."""
    u, i, r = sweep_data
    P, Q = cgref.start_rows(1)
    for dtype in (np.float64, np.float32):
        for e, A, b in cgref.systems(u, i, r, Q, cgref.NU, 40.0, cgref.REG):
            x, done = cgref.cg(A, b, P[e], 13, dtype)
            assert done < 13 and np.all(np.isfinite(x)), (dtype, e, done, x)
            if e == cgref.ZERO_USER:
                assert np.all(b == 0)


def test_f32_recurrence_sizes_the_gpu_bars(sweep_data):
    """What an f32 implementation of the same recurrence reaches against the
    FP64 reference on this data (printed; the GPU tests' bar is 2e-4)."""
    u, i, r = sweep_data
    worst = 0.0
    for k in (1, 3, 20, 33):
        P, Q = cgref.start_rows(k)
        a = cgref.half_sweep(u, i, r, Q, cgref.NU, 40.0, cgref.REG, P, 3, np.float32)
        b = cgref.half_sweep(u, i, r, Q, cgref.NU, 40.0, cgref.REG, P, 3)
        worst = max(worst, np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
    print(f"f32 NumPy CG at 3 steps vs FP64: {worst:.3e}")
    assert worst <= 2e-5                            # a tenth of the GPU bar


# ---------------------------------------------------------------------- ABI
_PTR = ctypes.c_void_p(4096)         # non-NULL, never dereferenced: validation comes first


def _sweep_cg(lib, **kw):
    a = dict(entity_ptr=_PTR, other_ids=_PTR, strengths=_PTR, n_entities=3, other_features=_PTR,
             gram=_PTR, features=_PTR, n_factors=8, dtype=MF_F32, alpha=40.0, reg=0.1, cg_steps=3)
    a.update(kw)
    return lib.mf_ials_sweep_cg(a["entity_ptr"], a["other_ids"], a["strengths"], a["n_entities"],
                                a["other_features"], a["gram"], a["features"], a["n_factors"],
                                a["dtype"], a["alpha"], a["reg"], a["cg_steps"], None)


@pytest.mark.parametrize("bad,name", [
    (dict(cg_steps=0), "cg_steps"), (dict(cg_steps=-1), "cg_steps"),
    (dict(cg_steps=1025), "cg_steps"),
    (dict(dtype=MF_F64), "dtype"), (dict(n_factors=0), "n_factors"),
    (dict(n_factors=129), "n_factors"), (dict(alpha=-1.0), "alpha"),
    (dict(alpha=float("nan")), "alpha"), (dict(alpha=float("inf")), "alpha"),
    (dict(reg=0.0), "reg"), (dict(reg=-0.5), "reg"), (dict(reg=float("nan")), "reg"),
    (dict(reg=float("inf")), "reg"), (dict(n_entities=-1), "n_entities"),
    (dict(entity_ptr=None), "entity_ptr"), (dict(other_ids=None), "other_ids"),
    (dict(strengths=None), "strengths"), (dict(other_features=None), "other_features"),
    (dict(gram=None), "gram"), (dict(features=None), "features")])
def test_ials_sweep_cg_rejects_invalid_arguments(bad, name):
    from matrix_factorization import _lib

    assert _sweep_cg(_lib.load(), **bad) == MF_ERR_INVALID
    err = _lib.last_error()
    assert "mf_ials_sweep_cg" in err and name in err


def test_zero_entities_are_ok_without_a_device():
    from matrix_factorization import _lib

    lib = _lib.load()
    assert _sweep_cg(lib, n_entities=0) == MF_OK
    assert _sweep_cg(lib, n_entities=0, entity_ptr=None, features=None) == MF_OK
    assert _sweep_cg(lib, n_entities=0, cg_steps=1) == MF_OK
    assert _sweep_cg(lib, n_entities=0, cg_steps=1024) == MF_OK
    assert _sweep_cg(lib, n_entities=0, cg_steps=0) == MF_ERR_INVALID   # checked all the same
    assert lib.mf_abi_version() == 1


# ---------------------------------------------------------------- estimator
def test_estimator_validates_solver_before_any_rng_draw():
    from sklearn.base import clone

    from matrix_factorization import ImplicitALSMF

    with pytest.raises(ValueError, match="solver"):
        ImplicitALSMF(solver="qr")
    for bad in (0, 2.5, 1025, -1, True, "3"):
        with pytest.raises(ValueError, match="cg_steps"):
            ImplicitALSMF(cg_steps=bad)
    d = ImplicitALSMF(n_factors=8, verbose=0)
    assert d.solver == "direct" and d.cg_steps == 3
    assert ImplicitALSMF(solver="cg", cg_steps=np.int64(1024)).cg_steps == 1024
    m = ImplicitALSMF(n_factors=8, verbose=0, solver="cg", cg_steps=5)
    c = clone(m)
    assert c.solver == "cg" and c.cg_steps == 5 and c.get_params() == m.get_params()
    assert m.get_params()["solver"] == "cg" and m.get_params()["cg_steps"] == 5
    assert "solver='cg'" in repr(m) and "cg_steps=5" in repr(m)
    X = pd.DataFrame({"user_id": [1, 1, 2, 3], "item_id": [5, 6, 5, 7]})
    y = pd.Series([1.0, 2.0, 0.0, 3.0])
    for attr, bad, match in (("solver", "qr", "solver"), ("cg_steps", 0, "cg_steps"),
                             ("cg_steps", 2.5, "cg_steps")):
        m = ImplicitALSMF(n_factors=8, verbose=0, solver="cg")
        setattr(m, attr, bad)
        for call in (lambda: m.fit(X, y), lambda: m.update_users(X, y)):
            np.random.seed(11)
            before = np.random.get_state()
            with pytest.raises(ValueError, match=match):
                call()
            after = np.random.get_state()
            assert before[0] == after[0] and np.array_equal(before[1], after[1])
            assert before[2:] == after[2:]


def test_pickles_from_before_the_solver_choice_load_as_direct():
    from matrix_factorization import ImplicitALSMF

    m = ImplicitALSMF(n_factors=8, alpha=12.5, verbose=0, solver="cg", cg_steps=7)
    state = m.__getstate__()
    assert state["solver"] == "cg" and state["cg_steps"] == 7
    del state["solver"], state["cg_steps"]
    old = ImplicitALSMF.__new__(ImplicitALSMF)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)    # no HIP device on this host
        old.__setstate__(state)
        new = ImplicitALSMF.__new__(ImplicitALSMF)
        new.__setstate__(m.__getstate__())
    assert old.solver == "direct" and old.cg_steps == 3 and old.alpha == 12.5
    assert old.dtype == "float32" and old.schedule == "exact"   # KernelMF's table still applies
    assert new.solver == "cg" and new.cg_steps == 7
    old._check_hyper()
