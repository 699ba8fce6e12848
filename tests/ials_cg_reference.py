"""NumPy restatement of the conjugate-gradient half-sweep of implicit-feedback
ALS (mf_ials_sweep_cg, ImplicitALSMF(solver="cg")); the model is
tests/ials_reference.py's.

Per entity e with a non-empty list, A = G + sum_n alpha r_n z_n z_n^T + reg I,
b = sum_{n: r_n > 0} (1 + alpha r_n) z_n and x = e's current row:

    res = b - A x;  p = res;  rs = res . res
    repeat steps times:
        if not (rs > 1e-30): stop
        Ap = A p;  a = rs / (p . Ap)
        x += a p;  res -= a Ap;  rs' = res . res
        p = res + (rs' / rs) p;  rs = rs'

``dtype`` float64 is the reference; float32 runs the same recurrence in f32
(from f32 A, b, x) and only sizes what an f32 implementation can be expected
to reach.
"""

import numpy as np

RS_STOP = 1e-30

# ---- the half-sweep data of the CG tests (tests/test_gpu_ials.py's generator
# restated): 14000 random pairs over users 0..398, then users 390..396 with
# lists of exactly 1, 63, 64, 65, 128, 129 and 250 items (chunk boundaries of
# the kernel), user 397 with all-zero strengths, user 399 without any pair
NU, NI = 400, 260
EXACT = {390: 1, 391: 63, 392: 64, 393: 65, 394: 128, 395: 129, 396: 250}
ZERO_USER, EMPTY_USER = 397, 399
REG = 0.1


def sweep_data():
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
    u, i, r = u[p].astype(np.int32), i[p].astype(np.int32), r[p]
    deg = np.bincount(u, minlength=NU)
    assert all(deg[user] == d for user, d in EXACT.items()) and deg[EMPTY_USER] == 0
    assert 0.10 < np.mean(r == 0) < 0.22 and deg[:390].min() > 0
    return u, i, r


def start_rows(k):
    """Start rows of the swept side and the fixed side, rounded to f32."""
    rs = np.random.RandomState(100 + k)
    P = rs.normal(0, 0.3, (NU, k)).astype(np.float32)
    Q = rs.normal(0, 0.3, (NI, k)).astype(np.float32)
    return P, Q


def systems(ent, oth, r, Z, n_ent, alpha, reg):
    """(e, A, b) of every entity with a non-empty list, FP64."""
    ent = np.asarray(ent, np.int64)
    oth = np.asarray(oth, np.int64)
    r = np.asarray(r, np.float64)
    Z = np.asarray(Z, np.float64)
    k = Z.shape[1]
    G = Z.T @ Z
    order = np.argsort(ent, kind="stable")
    ptr = np.zeros(n_ent + 1, np.int64)
    np.cumsum(np.bincount(ent, minlength=n_ent), out=ptr[1:])
    for e in range(n_ent):
        idx = order[ptr[e]:ptr[e + 1]]
        if len(idx) == 0:
            continue
        z, re = Z[oth[idx]], r[idx]
        A = G + (z * (alpha * re)[:, None]).T @ z + reg * np.eye(k)
        b = ((1.0 + alpha * re) * (re > 0)) @ z
        yield e, A, b


def cg(A, b, x, steps, dtype=np.float64, trace=None):
    """``steps`` steps of the recurrence from ``x`` in ``dtype``; returns the
    iterate and the number of steps taken.  ``trace``: a list that receives
    the iterate before the first and after every step (FP64 copies)."""
    A = np.asarray(A, dtype)
    b = np.asarray(b, dtype)
    x = np.array(x, dtype)
    res = b - A @ x
    p = res.copy()
    rs = res @ res
    if trace is not None:
        trace.append(x.astype(np.float64))
    done = 0
    for _ in range(steps):
        if not rs > RS_STOP:
            break
        Ap = A @ p
        a = rs / (p @ Ap)
        x = x + a * p
        res = res - a * Ap
        rs2 = res @ res
        p = res + (rs2 / rs) * p
        rs = rs2
        done += 1
        if trace is not None:
            trace.append(x.astype(np.float64))
    return x, done


def half_sweep(ent, oth, r, Z, n_ent, alpha, reg, X, steps, dtype=np.float64):
    """Rows of the swept side after ``steps`` CG steps per entity from the
    rows of ``X``, the other side Z fixed.  Entities with an empty list keep
    their row of ``X``.  Returns FP64 whatever ``dtype``."""
    out = np.array(X, np.float64)
    for e, A, b in systems(ent, oth, r, Z, n_ent, alpha, reg):
        out[e] = cg(A, b, out[e], steps, dtype)[0]
    return out
