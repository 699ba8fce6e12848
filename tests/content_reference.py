"""NumPy FP64 restatement of ContentBasedRecommender's arithmetic
(include/mf_hip.h, "Content-based"; matrix_factorization/content_based.py).

    F       n_items x d: row i is the first feature row whose item id is i, a
            zero row (has_features[i] = False) without one
    P_u     with w = rating - min_rating over the user's pairs whose item has
            features, in the order of the pairs: sum w F_i / sum w when
            sum w > 0, else the undivided sum, zeros without such a pair
    S[a,b]  F_a . F_b / (|F_a| |F_b|), 0 where either norm is 0

Scorings: "reference" mean(P_u) (the global mean for an id of -1 and when
d = 0), "cosine" cos(P_u, F_i) (0 for an id of -1), "neighbors"
cf_reference.predict with S in place of the rating similarity.
"""

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("genres", "embed")          # tools/make_content_fixture.py


def load_case(name):
    z = np.load(os.path.join(GOLDEN, f"content_{name}.npz"))
    return {k: z[k] for k in z.files}


def internal(case):
    """The fixture in internal ids: (u, i, r) training triples, (rows' item
    ids, -1 = unknown) of the feature frame, (tu, ti) test pairs."""
    upos = {u: n for n, u in enumerate(case["user_ids"].tolist())}
    ipos = {i: n for n, i in enumerate(case["item_ids"].tolist())}
    u = np.asarray([upos[x] for x in case["train_user"].tolist()])
    i = np.asarray([ipos[x] for x in case["train_item"].tolist()])
    fi = np.asarray([ipos.get(x, -1) for x in case["feat_item"].tolist()])
    tu = np.asarray([upos.get(x, -1) for x in case["test_user"].tolist()])
    ti = np.asarray([ipos.get(x, -1) for x in case["test_item"].tolist()])
    return u, i, case["train_rating"], fi, tu, ti


def feature_matrix(row_items, values, n_items):
    """(F, has_features) from the frame's rows: ``row_items`` are internal item
    ids (-1: dropped), the first row of an item counts."""
    values = np.asarray(values, dtype=np.float64)
    F = np.zeros((n_items, values.shape[1]))
    has = np.zeros(n_items, bool)
    for row, i in enumerate(row_items):
        if i >= 0 and not has[i]:
            F[i], has[i] = values[row], True
    return F, has


def first_rows(row_items):
    """Positions of the rows that are the first of their item: the rows of the
    reference's frame-ordered similarity that have a counterpart here."""
    _, pos = np.unique(np.asarray(row_items), return_index=True)
    return np.sort(pos)


def profiles(u, i, r, F, has, n_users, min_rating):
    P = np.zeros((n_users, F.shape[1]))
    wsum = np.zeros(n_users)
    for uu, ii, rr in zip(u, i, r):
        if has[ii]:
            w = rr - min_rating
            P[uu] += F[ii] * w
            wsum[uu] += w
    pos = wsum > 0
    P[pos] /= wsum[pos, None]
    return P


def unit_rows(X):
    """x / |x| per row in FP64, a zero row where the norm is 0."""
    X = np.asarray(X, dtype=np.float64)
    nrm = np.sqrt((X * X).sum(axis=1))
    out = np.zeros_like(X)
    np.divide(X, nrm[:, None], out=out, where=nrm[:, None] > 0)
    return out


def similarity(F):
    U = unit_rows(F)
    return U @ U.T


def similarity_bar(F, d=None):
    """Per-entry bound of the float32 MFMA similarity against ``similarity``:
    (d + 4) 2^-24 A with A = |F^| |F^|^T -- two input roundings, a d-term
    f32 chain, margin for a split k."""
    U = np.abs(unit_rows(F))
    return ((F.shape[1] if d is None else d) + 4) * 2.0 ** -24 * (U @ U.T)


def score_reference(P, u, i, global_mean, bound=None):
    u, i = np.asarray(u), np.asarray(i)
    known = (u >= 0) & (i >= 0)
    out = np.full(len(u), float(global_mean))
    if P.shape[1]:
        for p in np.flatnonzero(known):
            out[p] = np.mean(P[u[p]])
    if bound is not None:
        out = np.clip(out, bound[0], bound[1])
    return out


def score_cosine(P, F, u, i):
    """(FP64 cosine, sum |p^ f^|) per pair; 0 for an id of -1."""
    u, i = np.asarray(u), np.asarray(i)
    known = (u >= 0) & (i >= 0)
    Pn, Fn = unit_rows(P), unit_rows(F)
    a, b = Pn[np.where(known, u, 0)], Fn[np.where(known, i, 0)]
    cos = np.where(known, (a * b).sum(axis=1), 0.0)
    mag = np.where(known, np.abs(a * b).sum(axis=1), 0.0)
    return cos, mag
