"""NumPy FP64 restatement of implicit-feedback ALS (Hu, Koren & Volinsky 2008)
for the tests of mf_gramian / mf_ials_sweep / ImplicitALSMF.

Strength r >= 0 on the observed pairs, confidence c = 1 + alpha r, preference
p = [r > 0]; every other pair has c = 1, p = 0:

    L = sum_{u,i} c_ui (p_ui - x_u . y_i)^2 + reg (|X|_F^2 + |Y|_F^2)
"""

import numpy as np


def half_sweep(ent, oth, r, Z, n_ent, alpha, reg, X=None):
    """Rows of the swept side, the other side Z fixed: per entity e with list
    I_e, (Z^T Z + sum_{n in I_e} alpha r_n z_n z_n^T + reg I) x_e =
    sum_{n in I_e, r_n > 0} (1 + alpha r_n) z_n by a dense solve.  Entities
    with an empty list keep their row of ``X`` (zeros without one)."""
    ent = np.asarray(ent, np.int64)
    oth = np.asarray(oth, np.int64)
    r = np.asarray(r, np.float64)
    Z = np.asarray(Z, np.float64)
    k = Z.shape[1]
    out = np.zeros((n_ent, k)) if X is None else np.array(X, np.float64)
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
        out[e] = np.linalg.solve(A, b)
    return out


def loss(u, i, r, P, Q, alpha, reg):
    """L by the identity (no dense pass):
    sum_obs [c (p - s)^2 - s^2] + <P^T P, Q^T Q>_F + reg (|P|_F^2 + |Q|_F^2)."""
    P = np.asarray(P, np.float64)
    Q = np.asarray(Q, np.float64)
    r = np.asarray(r, np.float64)
    s = np.einsum("nk,nk->n", P[u], Q[i])
    obs = np.sum((1.0 + alpha * r) * ((r > 0) - s) ** 2 - s * s)
    return obs + np.sum((P.T @ P) * (Q.T @ Q)) + reg * (np.sum(P * P) + np.sum(Q * Q))


def loss_dense(u, i, r, P, Q, alpha, reg):
    """L by the definition: every user x item pair (the pairs are distinct)."""
    P = np.asarray(P, np.float64)
    Q = np.asarray(Q, np.float64)
    C = np.ones((P.shape[0], Q.shape[0]))
    T = np.zeros_like(C)
    r = np.asarray(r, np.float64)
    C[u, i] = 1.0 + alpha * r
    T[u, i] = r > 0
    S = P @ Q.T
    return np.sum(C * (T - S) ** 2) + reg * (np.sum(P * P) + np.sum(Q * Q))
