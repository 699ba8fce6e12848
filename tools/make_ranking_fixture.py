#!/usr/bin/env python3
"""Write tests/golden/ranking_eval.json: the reference's evaluate_topk
(project_template/pipeline/evaluate.py) run on a fixed score table.

    python tools/make_ranking_fixture.py /path/to/reference/checkout

The reference's loop asks a model for ``recommend(user, amount=k,
items_known=train_items)`` per user.  Here the model is a stub that ranks a
fixed score table (score descending, item id ascending: the package's tie
rule) and records the ``items_known`` it was given, so the file holds
everything a test needs to recompute the three numbers without the reference:
the score table, per case and evaluated user the known and held-out items,
k, and the reference's precision / recall / NDCG.  Data only, CPU only.
"""

from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np
import pandas as pd

N_USERS, N_ITEMS = 40, 60
KS = (1, 5, 10)
N_TESTS = (1, 3)
POSITIVE_THRESHOLD = 4.0


def load_evaluate(ref_root: str):
    """evaluate.py by path (it imports only its sibling ``common``), without
    running the package's __init__ files."""
    pdir = os.path.join(ref_root, "project_template", "pipeline")
    pkg = types.ModuleType("_ref_pipeline")
    pkg.__path__ = [pdir]
    sys.modules["_ref_pipeline"] = pkg
    mod = None
    for name in ("common", "evaluate"):
        spec = importlib.util.spec_from_file_location(f"_ref_pipeline.{name}",
                                                      os.path.join(pdir, f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
    return mod


class TableModel:
    """recommend() from a fixed score table; remembers what it was asked."""

    def __init__(self, scores: np.ndarray):
        self.scores = scores
        self.calls = []

    def recommend(self, user, amount=10, items_known=None, include_user=True, **_):
        known = [int(i) for i in (items_known or [])]
        self.calls.append((int(user), known))
        cand = np.setdiff1d(np.arange(self.scores.shape[1]), np.asarray(known, np.int64))
        s = self.scores[int(user), cand]
        order = np.lexsort((cand, -s))                  # score desc, then id asc
        top = cand[order][:amount]
        return pd.DataFrame({"item_id": top.tolist(), "rating_pred": s[order][:amount]})


def make_inputs(rng: np.random.RandomState):
    # one decimal: plenty of equal scores, so the tie rule matters
    scores = np.round(rng.uniform(0.0, 5.0, (N_USERS, N_ITEMS)), 1)
    rows = []
    for u in range(N_USERS):
        # users 0..3 have too little history for the larger n_test: skipped there
        n_hist = [1, 2, 3, 3][u] if u < 4 else int(rng.randint(5, 25))
        items = rng.choice(N_ITEMS, size=n_hist, replace=False)
        for i in items:
            rows.append((u, int(i), float(rng.randint(1, 6))))
    ratings = pd.DataFrame(rows, columns=["user_id", "item_id", "rating"])
    return scores, ratings


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("reference", help="path of the reference checkout")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                  "..", "tests", "golden", "ranking_eval.json"))
    args = ap.parse_args()
    ev = load_evaluate(args.reference)
    scores, ratings = make_inputs(np.random.RandomState(20261019))
    hist = {int(u): sorted(int(i) for i in g["item_id"]) for u, g in ratings.groupby("user_id")}
    cases = []
    for n_test in N_TESTS:
        for k in KS:
            model = TableModel(scores)
            seed = 100 * n_test + k
            res = ev.evaluate_topk(ratings=ratings, model=model, k=k,
                                   positive_threshold=POSITIVE_THRESHOLD, n_test=n_test,
                                   seed=seed)
            users = [{"user": u, "known": known,
                      "test": sorted(set(hist[u]) - set(known))} for u, known in model.calls]
            assert all(len(x["test"]) == n_test for x in users)
            cases.append({"k": k, "n_test": n_test, "seed": seed, "users": users,
                          "skipped_users": sorted(set(hist) - {x["user"] for x in users}),
                          "precision": res.precision, "recall": res.recall, "ndcg": res.ndcg})
    out = {"n_users": N_USERS, "n_items": N_ITEMS, "positive_threshold": POSITIVE_THRESHOLD,
           "scores": scores.tolist(), "cases": cases}
    with open(args.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(f"{os.path.normpath(args.out)}: {len(cases)} cases, "
          f"{[len(c['users']) for c in cases]} evaluated users")


if __name__ == "__main__":
    main()
