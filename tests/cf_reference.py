"""NumPy FP64 restatement of the neighbourhood models' arithmetic (ItemItemCF /
UserUserCF; include/mf_hip.h, "neighbourhood models").

One model, roles swapped: ENTITIES are the items (ItemItemCF) or the users
(UserUserCF), OTHERS are the other side, n = n_others.  r_ao is the rating of
entity a by other o, 0 where there is none; every sum runs over the stored
entries.

    m_a    = (sum_o r_ao) / n
    w_a    = sqrt(max(sum_o r_ao^2 - n m_a^2, 0))
    S[a,b] = (sum_o r_ao r_bo - n m_a m_b) / (w_a w_b),   0 where w_a w_b = 0

Prediction for target e and other o: candidates are the b != e with r_bo > 0;
more than n_neighbors of them are cut to the n_neighbors first under
(S[e,b] descending, b ascending); pred = m_e + sum S (r_bo - m_b) / sum |S|,
m_e with no candidate or a zero denominator, global_mean for an id of -1.
"""

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the reference's own classes on two datasets (tools/make_cf_fixture.py)
CASES = [(d, c) for d in ("small", "medium") for c in ("itemitemcf", "userusercf")]


def load_case(data, cls):
    z = np.load(os.path.join(GOLDEN, f"cf_{data}_{cls}.npz"))
    return {k: z[k] for k in z.files}


def dense(ent, oth, r, n_entities, n_others):
    """(n_entities, n_others) FP64 matrix of the stored ratings, 0 elsewhere."""
    R = np.zeros((n_entities, n_others))
    R[np.asarray(ent), np.asarray(oth)] = np.asarray(r, dtype=np.float64)
    return R


def stats(R):
    n = R.shape[1]
    m = R.sum(axis=1) / n if n else np.zeros(R.shape[0])
    w = np.sqrt(np.maximum((R * R).sum(axis=1) - n * m * m, 0.0))
    return m, w


def similarity(R, m=None, w=None):
    if m is None:
        m, w = stats(R)
    n = R.shape[1]
    num = R @ R.T - n * np.outer(m, m)
    den = np.outer(w, w)
    S = np.zeros_like(num)
    np.divide(num, den, out=S, where=den > 0)
    return S


def select(S_row, R_col, e, n_neighbors):
    """Kept neighbour ids of target e for the other whose ratings are R_col."""
    cand = np.flatnonzero(R_col > 0)
    cand = cand[cand != e]
    if len(cand) > n_neighbors:
        s = S_row[cand] + 0.0                        # -0 ties with +0
        cand = cand[np.lexsort((cand, -s))][:n_neighbors]
    return cand


def cut_margin(S_row, R_col, e, n_neighbors):
    """n_neighbors-th minus (n_neighbors+1)-th similarity; inf without a cut."""
    cand = np.flatnonzero(R_col > 0)
    cand = cand[cand != e]
    if len(cand) <= n_neighbors:
        return np.inf
    s = np.sort(S_row[cand])[::-1]
    return float(s[n_neighbors - 1] - s[n_neighbors])


def predict(R, S, m, ent, oth, n_neighbors, global_mean, bound=None):
    """FP64 predictions for the pairs (ent[p], oth[p]); S may be the float32
    matrix of the GPU (it is read as FP64).  ``bound``: (min, max) or None."""
    out = np.empty(len(ent))
    for p, (e, o) in enumerate(zip(ent, oth)):
        if e < 0 or o < 0:
            out[p] = global_mean
            continue
        row = np.asarray(S[e], dtype=np.float64)
        keep = np.sort(select(row, R[:, o], e, n_neighbors))
        s = row[keep]
        den = np.abs(s).sum()
        out[p] = m[e] + (s * (R[keep, o] - m[keep])).sum() / den if den > 0 else m[e]
    if bound is not None:
        out = np.clip(out, bound[0], bound[1])
    return out
