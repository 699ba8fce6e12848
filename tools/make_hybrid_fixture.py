#!/usr/bin/env python3
"""Write tests/golden/hybrid_small.npz: the reference's hybrid evaluation
(project_template/pipeline/evaluate_hybrid.py::evaluate_hybrid), run unmodified
on the CPU.

    python tools/make_hybrid_fixture.py /path/to/reference/checkout

The model handed to ``evaluate_hybrid`` is a recording stub: its ``predict``
returns ((mu + b_i) + b_u) + p . q from fixed FP64 factor arrays and records
each call's user and candidate list.  The per-user train / test split is the
one ``_pick_test_items`` draws with the same seed; it is replayed here once,
stored, and never replayed by the tests.

The file holds data only:
  users, items                 external ids (strings), positions = codes
  rating_user, rating_item, rating   the ratings frame, as codes
  index_codes, row_of          the index: item code of each embedding row (three
                               items have none), and each code's row or -1
  embeddings                   float32 unit-norm rows, d = 24
  global_mean, user_biases, item_biases, user_factors, item_factors   the stub, rank 16
  train_ptr, train_codes       each user's history in the reference's order
  test_ptr, test_codes         each user's held-out items
  cand_user, cand_ptr, cand_rows   the recorded candidate lists (index rows)
  alphas, metrics              precision, recall, NDCG per alpha (with the stub)
  metrics_no_model             the same for model=None (alpha = 0.7)
  k, candidate_k, n_test, min_profile_items, positive_threshold, seed

Before anything is written two conditions are asserted:
 (a) the NumPy restatement (tests/hybrid_reference.py) on the stored split
     reproduces every metric to 1e-12 and every recorded candidate list exactly;
 (b) for every evaluated user the similarity gap between the last retrieved
     and the first non-retrieved row is >= 1e-4, and for each alpha (and for
     model=None) the smallest gap between adjacent blended scores among the
     best k + 1 is >= 1e-4 -- about 100 x the float32 rounding of a d = 24 dot
     product, so that an FP64 profile mean and another summation order cannot
     change an id; also (so that the kept list may be compared as a list) the
     smallest gap between adjacent retrieved similarities is >= 2e-6.
Condition (b) is a condition on the inputs.  Users that miss it are dropped
from the ratings one at a time, the first offender each round (a dropped user
changes the draws of the users after it only), until none is left; then users
are taken off the end down to 60.  The tool prints the achieved minima; the
committed file (56711 bytes, 60 users evaluated, restatement against the
reference 0.0e+00) was written with
    users kept 60 of 82; minimum gaps: retrieval cut 2.3e-04, blended scores
    1.3e-04, adjacent retrieved similarities 4.4e-06
"""

from __future__ import annotations

import argparse
import importlib
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import hybrid_reference as href  # noqa: E402

N_USERS, N_ITEMS, NNZ, D, RANK = 82, 150, 2400, 24, 16
K, CANDIDATE_K, N_TEST, MIN_PROFILE, THRESHOLD, SEED = 10, 40, 3, 2, 2.0, 42
KEEP_USERS = 60
GAP, GAP_ADJ = 1e-4, 2e-6


class RecordingStub:
    """``predict`` of a linear factor model over string ids, recording its calls."""

    def __init__(self, fx):
        self.fx = fx
        self.user_pos = {u: j for j, u in enumerate(fx["users"].tolist())}
        self.item_code = {i: j for j, i in enumerate(fx["items"].tolist())}
        self.calls = []

    def predict(self, X, bound_ratings=False):
        assert bound_ratings is False
        u = self.user_pos[X["user_id"].iloc[0]]
        assert (X["user_id"] == X["user_id"].iloc[0]).all()
        codes = np.asarray([self.item_code[i] for i in X["item_id"]], np.int64)
        rows = self.fx["row_of"][codes]
        assert (rows >= 0).all()
        self.calls.append((u, rows.astype(np.int32)))
        return href.stub_scores(self.fx, u, rows).tolist()


def synth(rs):
    keys = rs.choice(N_USERS * N_ITEMS, size=NNZ, replace=False)
    u, i = keys // N_ITEMS, keys % N_ITEMS
    raw = 3.0 + rs.normal(0, 1.2, NNZ)
    return u, i, np.clip(np.rint(raw * 2) / 2, 0.5, 5.0)


def frame(fx):
    return pd.DataFrame({"user_id": fx["users"][fx["rating_user"]],
                         "item_id": fx["items"][fx["rating_item"]],
                         "rating": fx["rating"]})


def replay_split(mod, fx):
    """The split evaluate_hybrid draws (evaluate_hybrid.py:96-117), stored as codes."""
    ratings = frame(fx)
    rng = np.random.RandomState(SEED)
    code = {i: j for j, i in enumerate(fx["items"].tolist())}
    tr, te = [], []
    users = ratings["user_id"].astype(str).unique()
    assert users.tolist() == fx["users"].tolist()
    for u in users:
        hist = ratings[ratings["user_id"].astype(str) == u].copy()
        hist["item_id"] = hist["item_id"].astype(str)
        hist["rating"] = pd.to_numeric(hist["rating"], errors="coerce").fillna(0.0)
        a, b = mod._pick_test_items(user_hist=hist, n_test=N_TEST,
                                    positive_threshold=THRESHOLD, rng=rng)
        tr.append(np.asarray([code[x] for x in a], np.int32))
        te.append(np.asarray([code[x] for x in b], np.int32))

    def csr(parts):
        ptr = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        return ptr, np.concatenate(parts).astype(np.int32)

    fx["train_ptr"], fx["train_codes"] = csr(tr)
    fx["test_ptr"], fx["test_codes"] = csr(te)


def margins(fx):
    """Per evaluated user the three gaps of condition (b): {user: (cut, blended, adjacent)}."""
    out = {}
    for alpha, use_model in [(a, True) for a in href.ALPHAS] + [(0.7, False)]:
        detail = {}
        href.evaluate(fx, alpha, use_model, K, CANDIDATE_K, MIN_PROFILE, detail)
        for u, d in detail.items():
            sims = d["sims"].astype(np.float64)
            rest = np.setdiff1d(np.arange(len(sims)), d["top"])
            cut = float(sims[d["top"]].min() - sims[rest].max()) if len(rest) else np.inf
            adj = float(np.min(-np.diff(sims[d["top"]]))) if len(d["top"]) > 1 else np.inf
            sc = d["score"][:K + 1].astype(np.float64)
            bl = float(np.min(-np.diff(sc))) if len(sc) > 1 else np.inf
            c0, b0, a0 = out.get(u, (np.inf, np.inf, np.inf))
            out[u] = (min(c0, cut), min(b0, bl), min(a0, adj))
    return out


def build(mod):
    rs = np.random.RandomState(SEED)
    ru, ri, rr = synth(rs)
    order = np.argsort(ru, kind="stable")               # users appear in code order
    ru, ri, rr = ru[order], ri[order], rr[order]
    E = rs.normal(0, 1, (N_ITEMS, D))
    index_codes = rs.permutation(N_ITEMS)[:N_ITEMS - 3].astype(np.int32)
    E = E[:len(index_codes)]
    E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float32)
    row_of = np.full(N_ITEMS, -1, np.int32)
    row_of[index_codes] = np.arange(len(index_codes), dtype=np.int32)
    base = dict(
        items=np.asarray([str(7 + 2 * j) for j in range(N_ITEMS)]),
        index_codes=index_codes, row_of=row_of, embeddings=E,
        global_mean=np.float64(3.1), item_biases=rs.normal(0, 0.3, N_ITEMS),
        item_factors=rs.normal(0, 0.4, (N_ITEMS, RANK)))
    all_bu, all_p = rs.normal(0, 0.3, N_USERS), rs.normal(0, 0.4, (N_USERS, RANK))
    alive = np.ones(N_USERS, bool)
    while True:
        ids = np.flatnonzero(alive)
        pos = np.full(N_USERS, -1)
        pos[ids] = np.arange(len(ids))
        keep = alive[ru]
        fx = dict(base, users=np.asarray([str(1000 + 3 * j) for j in ids]),
                  rating_user=pos[ru[keep]].astype(np.int32),
                  rating_item=ri[keep].astype(np.int32), rating=rr[keep],
                  user_biases=all_bu[ids], user_factors=all_p[ids])
        replay_split(mod, fx)
        m = margins(fx)
        bad = [u for u in sorted(m) if m[u][0] < GAP or m[u][1] < GAP or m[u][2] < GAP_ADJ]
        if bad:
            alive[ids[bad[0]]] = False
            continue
        if len(ids) > KEEP_USERS:                       # trim to the size wanted, from the end
            alive[ids[-1]] = False
            continue
        return fx, m


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("reference", help="path of the reference checkout")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "tests", "golden"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    mod = importlib.import_module("project_template.pipeline.evaluate_hybrid")
    assert os.path.realpath(mod.__file__).startswith(os.path.realpath(args.reference))
    fx, m = build(mod)
    ratings = frame(fx)
    item_ids = fx["items"][fx["index_codes"]].tolist()
    kw = dict(ratings=ratings, item_ids=item_ids, item_emb=fx["embeddings"], k=K,
              candidate_k=CANDIDATE_K, positive_threshold=THRESHOLD, n_test=N_TEST, seed=SEED,
              min_profile_items=MIN_PROFILE)
    metrics, calls = [], None
    for alpha in href.ALPHAS:
        stub = RecordingStub(fx)
        res = mod.evaluate_hybrid(model=stub, alpha=alpha, **kw)
        metrics.append([res.precision, res.recall, res.ndcg])
        assert calls is None or all(a[0] == b[0] and np.array_equal(a[1], b[1])
                                    for a, b in zip(calls, stub.calls))
        calls = stub.calls
    res = mod.evaluate_hybrid(model=None, alpha=0.7, **kw)
    no_model = [res.precision, res.recall, res.ndcg]
    # condition (a): the restatement is the reference
    worst = 0.0
    for alpha, want in zip(href.ALPHAS, metrics):
        detail = {}
        got = href.evaluate(fx, alpha, True, K, CANDIDATE_K, MIN_PROFILE, detail)
        worst = max(worst, max(abs(a - b) for a, b in zip(got, want)))
        assert sorted(detail) == [u for u, _ in calls]
        for u, rows in calls:
            assert np.array_equal(detail[u]["kept"], rows), u
    got = href.evaluate(fx, 0.7, False, K, CANDIDATE_K, MIN_PROFILE)
    worst = max(worst, max(abs(a - b) for a, b in zip(got, no_model)))
    assert worst <= 1e-12, worst
    # condition (b), as achieved
    cut, bl, adj = (min(v[j] for v in m.values()) for j in range(3))
    assert cut >= GAP and bl >= GAP and adj >= GAP_ADJ
    fx.update(cand_user=np.asarray([u for u, _ in calls], np.int32),
              cand_ptr=np.concatenate([[0], np.cumsum([len(r) for _, r in calls])]).astype(
                  np.int64),
              cand_rows=np.concatenate([r for _, r in calls]).astype(np.int32),
              alphas=np.asarray(href.ALPHAS), metrics=np.asarray(metrics),
              metrics_no_model=np.asarray(no_model), k=np.int64(K),
              candidate_k=np.int64(CANDIDATE_K), n_test=np.int64(N_TEST),
              min_profile_items=np.int64(MIN_PROFILE), positive_threshold=np.float64(THRESHOLD),
              seed=np.int64(SEED))
    path = os.path.normpath(os.path.join(args.out, "hybrid_small.npz"))
    np.savez_compressed(path, **fx)
    print(f"{path}: {os.path.getsize(path)} bytes; {len(calls)} users evaluated; restatement vs "
          f"reference: {worst:.1e}")
    print(f"users kept {len(fx['users'])} of {N_USERS}; minimum gaps: retrieval cut {cut:.1e}, "
          f"blended scores {bl:.1e}, adjacent retrieved similarities {adj:.1e}")
    print("metrics (precision, recall, ndcg):",
          {a: np.round(v, 4).tolist() for a, v in zip(href.ALPHAS, metrics)}, "no model:",
          np.round(no_model, 4).tolist())


if __name__ == "__main__":
    main()
