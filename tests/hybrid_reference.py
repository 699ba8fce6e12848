"""NumPy restatement of HybridRecommender's arithmetic: the five steps of
mf_hybrid_rerank (include/mf_hip.h, "Hybrid") in float32 as written and with a
stable argsort, and the reference's profile, retrieval and per-user metrics
(project_template/pipeline/evaluate_hybrid.py:107-167) for the CPU comparison
with tests/golden/hybrid_small.npz (tools/make_hybrid_fixture.py)."""

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
ALPHAS = (0.0, 0.7, 1.0)


def load_fixture():
    return dict(np.load(os.path.join(GOLDEN, "hybrid_small.npz")))


# ---------------------------------------------------------------- the rerank
def minmax(x):
    """evaluate_hybrid.py:72-79 on a float32 array."""
    x = np.asarray(x, F32)
    if x.size == 0:
        return x
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = np.min(x), np.max(x)                    # NaN if any value is
        d = float(hi) - float(lo)
        if d < 1e-8:
            return np.zeros_like(x)
        return ((x - F32(lo)) / F32(d)).astype(F32)


def blend(model, sims, alpha):
    """alpha * minmax(model) + (1.0 - alpha) * minmax(sims) in float32, -0 as +0."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = F32(alpha) * minmax(model) + F32(1.0 - alpha) * minmax(sims)
        return (s + F32(0.0)).astype(F32)


def rerank_one(cand_rows, cand_sims, scores_of, n_rows, exclude, alpha):
    """One query: (rows, blended scores, model scores, similarities) of the
    kept candidates in output order.  ``scores_of(rows)`` gives the float32
    model scores; ``exclude`` is the set of dropped index rows."""
    cand_rows = np.asarray(cand_rows)
    keep = np.array([0 <= r < n_rows and int(r) not in exclude for r in cand_rows], bool)
    rows = cand_rows[keep].astype(np.int32)
    sims = np.asarray(cand_sims, F32)[keep]
    model = np.asarray(scores_of(rows), F32)
    score = blend(model, sims, alpha)
    order = np.argsort(-score, kind="stable")            # NaN last, ties in retrieval order
    return rows[order], score[order], model[order], sims[order]


def rerank(cand_rows, cand_sims, scores_of, n_rows, exclude, alpha, amount):
    """mf_hybrid_rerank's outputs for [n_query, n_cand] inputs: out_rows,
    out_scores, out_model, out_sims ([n_query, amount], padded with -1 / NaN)
    and out_n_cand.  ``scores_of(q, rows)``; ``exclude[q]``: a set of rows."""
    nq = len(cand_rows)
    o_rows = np.full((nq, amount), -1, np.int32)
    o_sc, o_mo, o_si = (np.full((nq, amount), np.nan, F32) for _ in range(3))
    o_m = np.zeros(nq, np.int32)
    for q in range(nq):
        r, sc, mo, si = rerank_one(cand_rows[q], cand_sims[q], lambda rows: scores_of(q, rows),
                                   n_rows, exclude[q], alpha)
        o_m[q] = len(r)
        n = min(amount, len(r))
        o_rows[q, :n], o_sc[q, :n], o_mo[q, :n], o_si[q, :n] = r[:n], sc[:n], mo[:n], si[:n]
    return o_rows, o_sc, o_mo, o_si, o_m


def same_bits(a, b):
    """float32 arrays equal bit for bit, any NaN matching any NaN."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and
                np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ------------------------------------------- the reference's first stage
def profile(E, rows):
    """evaluate_hybrid.py:125-130: float32 mean, FP64 norm, float32 result."""
    prof = E[np.asarray(rows)].mean(axis=0)
    norm = float(np.linalg.norm(prof))
    if norm > 0:
        prof = prof / norm
    return prof.astype(F32)


def retrieve(E, prof, candidate_k):
    """evaluate_hybrid.py:133-136: (rows, all similarities)."""
    sims = E @ prof
    ck = min(candidate_k, len(E))
    top = np.argpartition(-sims, kth=ck - 1)[:ck]
    return top[np.argsort(-sims[top])], sims


def stub_scores(fx, user, rows):
    """The fixture's recording stub: ((mu + b_i) + b_u) + p . q in FP64 for the
    user's position in fx["users"] and the items of the index rows."""
    codes = fx["index_codes"][np.asarray(rows, np.int64)]
    p, q = fx["user_factors"][user], fx["item_factors"][codes]
    return ((float(fx["global_mean"]) + fx["item_biases"][codes]) + fx["user_biases"][user]) \
        + q @ p


def split_of(fx, u):
    """User u's stored split: (item codes of the history in the reference's
    order, their index rows where they have one, held-out item codes)."""
    train = fx["train_codes"][fx["train_ptr"][u]:fx["train_ptr"][u + 1]]
    test = fx["test_codes"][fx["test_ptr"][u]:fx["test_ptr"][u + 1]]
    rows = fx["row_of"][train]
    return train, rows[rows >= 0], test


def ndcg_of_hits(hit):
    """evaluate_hybrid.py:37-45 on a 0/1 vector."""
    hit = np.asarray(hit, np.int32)
    if hit.size == 0:
        return 0.0
    disc = np.log2(np.arange(2, hit.size + 2))
    dcg = float(np.sum((2 ** hit - 1) / disc))
    idcg = float(np.sum((2 ** np.sort(hit)[::-1] - 1) / disc))
    return dcg / idcg if idcg > 0 else 0.0


def evaluate(fx, alpha, use_model, k, candidate_k, min_profile_items, detail=None):
    """evaluate_hybrid.py:107-167 on the fixture's stored split: (precision,
    recall, ndcg).  ``detail``: a dict that receives per evaluated user
    (position in fx["users"]) the kept rows in retrieval order, all
    similarities, the retrieved rows, and the output rows and scores."""
    E = fx["embeddings"]
    P, R, N = [], [], []
    for u in range(len(fx["users"])):
        train, prof_rows, test = split_of(fx, u)
        if len(train) == 0 or len(test) == 0 or len(prof_rows) < min_profile_items:
            continue
        top, sims = retrieve(E, profile(E, prof_rows), candidate_k)
        known = set(prof_rows.tolist())
        rows, score, _, _ = rerank_one(
            top, sims[top], (lambda r: stub_scores(fx, u, r)) if use_model
            else (lambda r: np.zeros(len(r), F32)), len(E), known, alpha)
        if len(rows) == 0:
            continue
        rec = rows[:min(k, len(rows))]
        hit = np.isin(fx["index_codes"][rec], test).astype(np.int32)
        P.append(float(hit.mean()))
        R.append(float(hit.sum() / max(1, len(set(test.tolist())))))
        N.append(ndcg_of_hits(hit))
        if detail is not None:
            keep = np.array([int(r) not in known for r in top], bool)
            detail[u] = dict(kept=top[keep], sims=sims, top=top, rows=rows, score=score)
    if not P:
        return 0.0, 0.0, 0.0
    return float(np.mean(P)), float(np.mean(R)), float(np.mean(N))
