"""NumPy restatement of the stored-neighbours (top-M) neighbourhood model
(include/mf_hip.h, "neighbourhood models"; tests/cf_reference.py is the dense
one).

N_M(a), the stored neighbours of entity a, are the first min(M, n - 1)
entities b != a under (S[a,b] descending with -0 tied to +0, b ascending) --
the order of the n_neighbors cut.  A prediction for target e and other o is
cf_reference.predict's with the candidates restricted to N_M(e): entities
outside it are no candidates (not "similarity 0").
"""

import numpy as np

import cf_reference as cfref


def neighbour_sets(S, M):
    """int32 [n, M]: row a holds N_M(a) by id ascending, -1 padding."""
    S = np.asarray(S)
    n = S.shape[0]
    out = np.full((n, M), -1, np.int32)
    for a in range(n):
        b = np.delete(np.arange(n), a)
        s = S[a, b].astype(np.float64) + 0.0             # -0 ties with +0
        keep = np.sort(b[np.lexsort((b, -s))][:M])
        out[a, :len(keep)] = keep
    return out


def predict_truncated(R, S, m, nbr_ids, ent, oth, n_neighbors, global_mean, bound=None):
    """FP64 predictions for the pairs (ent[p], oth[p]): cf_reference.select on
    R[:, o] zeroed outside N_M(e), then cf_reference.predict's sum."""
    out = np.empty(len(ent))
    n = R.shape[0]
    for p, (e, o) in enumerate(zip(ent, oth)):
        if e < 0 or o < 0:
            out[p] = global_mean
            continue
        inside = np.zeros(n, bool)
        ids = np.asarray(nbr_ids[e])
        inside[ids[ids >= 0]] = True
        col = np.where(inside, R[:, o], 0.0)
        row = np.asarray(S[e], dtype=np.float64)
        keep = np.sort(cfref.select(row, col, e, n_neighbors))
        s = row[keep]
        den = np.abs(s).sum()
        out[p] = m[e] + (s * (R[keep, o] - m[keep])).sum() / den if den > 0 else m[e]
    if bound is not None:
        out = np.clip(out, bound[0], bound[1])
    return out


def n_candidates(R, nbr_ids, e, o):
    """Candidates of the pair (e, o): (truncated model, dense model)."""
    cand = np.flatnonzero(R[:, o] > 0)
    cand = cand[cand != e]
    ids = np.asarray(nbr_ids[e])
    return int(np.isin(cand, ids[ids >= 0]).sum()), len(cand)
