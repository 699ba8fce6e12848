#!/usr/bin/env python3
"""Write tests/golden/cf_*.npz: the reference's ItemItemCF / UserUserCF
(matrix_factorization/collaborative_filtering.py), run unmodified on the CPU.

    python tools/make_cf_fixture.py /path/to/reference/checkout

The reference package imports numba at its top; where numba is not
importable, a throw-away ``numba`` module whose ``njit`` is the identity is put
ahead of it on sys.path (as tests/golden/make_golden.py describes).  The
neighbourhood models themselves use only pandas and scikit-learn.

The reference's ``fit`` trains on ratings permuted against their pairs (it
shuffles X, then assigns ``y.values`` positionally).  So the fixture stores as
its TRAINING INPUT the triples each reference model actually trained on, read
back from its ``user_item_matrix`` and id maps: a model fitted on those
triples as given is the model the reference's numbers belong to.

Per case (two datasets x two models) the file holds
  train_user, train_item, train_rating   the triples, external ids
  user_ids, item_ids                     external ids in the reference's internal order
  similarity, means                      the reference's, in that order (float64)
  test_user, test_item                   400 held-out pairs (target not rated by the other)
  pred, pred_bounded                     the reference's predictions for them
  margin, den                            per pair: the reference's cut margin (n_neighbors-th
                                         minus (n_neighbors+1)-th candidate similarity, inf
                                         without a cut) and its denominator sum |S|
  n_neighbors, min_rating, max_rating, global_mean
Data only, CPU only.
"""

from __future__ import annotations

import argparse
import os
import sys
import tempfile

import numpy as np
import pandas as pd

N_TEST = 400
MARGIN_MIN, DEN_MIN, EXCLUDED_MAX = 1e-5, 0.05, 0.02
DATASETS = {
    # name: (n_users, n_items, n_ratings, n_neighbors, n_zero_ratings, min_rating, seed)
    "small": (60, 80, 1500, 5, 0, 0.5, 11),
    "medium": (200, 150, 6000, 10, 12, 0.0, 12),
}


def import_reference(ref_root: str):
    try:
        import numba  # noqa: F401
    except Exception:
        shim = tempfile.mkdtemp(prefix="nbshim_")
        os.makedirs(os.path.join(shim, "numba"))
        with open(os.path.join(shim, "numba", "__init__.py"), "w") as f:
            f.write("def njit(*a, **k):\n"
                    "    if a and callable(a[0]) and not k:\n"
                    "        return a[0]\n"
                    "    return lambda f: f\n")
        sys.path.insert(0, shim)
    sys.path.insert(0, ref_root)
    import matrix_factorization as ref

    assert os.path.realpath(ref.__file__).startswith(os.path.realpath(ref_root)), ref.__file__
    return ref


def synth(n_users, n_items, nnz, n_zero, seed, rank=4):
    """Unique pairs, half-integer ratings 0.5..5 from a low-rank signal, and
    ``n_zero`` ratings of exactly 0; external ids offset and non-contiguous."""
    rs = np.random.RandomState(seed)
    keys = rs.choice(n_users * n_items, size=nnz, replace=False)
    u, i = keys // n_items, keys % n_items
    U = rs.normal(0, 0.7, (n_users, rank))
    V = rs.normal(0, 0.7, (n_items, rank))
    raw = 3.0 + (U[u] * V[i]).sum(1) + rs.normal(0, 0.6, nnz)
    r = np.clip(np.rint(raw * 2) / 2, 0.5, 5.0)
    r[rs.choice(nnz, size=n_zero, replace=False)] = 0.0
    return pd.DataFrame({"user_id": 1000 + 3 * u, "item_id": 7 + 2 * i, "rating": r})


def run_case(ref, cls_name, data, n_neighbors, min_rating, seed):
    cls = getattr(ref, cls_name)
    item_side = cls_name == "ItemItemCF"
    np.random.seed(seed)
    model = cls(min_rating=min_rating, max_rating=5, n_neighbors=n_neighbors)
    model.fit(data[["user_id", "item_id"]], data["rating"])
    M = model.user_item_matrix.to_numpy(dtype=np.float64)          # users x items
    users = np.asarray(list(model.user_id_map.keys()))
    items = np.asarray(list(model.item_id_map.keys()))
    assert list(model.user_id_map.values()) == list(range(len(users)))
    assert list(model.item_id_map.values()) == list(range(len(items)))
    assert M.shape == (len(users), len(items))
    # the triples it trained on: the input's pairs, the matrix's values
    ui = np.asarray([model.user_id_map[u] for u in data["user_id"]])
    ii = np.asarray([model.item_id_map[i] for i in data["item_id"]])
    trained = M[ui, ii]
    support = np.zeros(M.shape, bool)
    support[ui, ii] = True
    assert not np.any(M[~support]), "ratings outside the input's support"
    S = np.asarray(model.item_similarity_matrix if item_side else model.user_similarity_matrix,
                   dtype=np.float64)
    means = np.asarray(model.item_mean_ratings if item_side else model.user_mean_ratings,
                       dtype=np.float64)
    # held-out pairs: the target is not among the other's ratings
    rs = np.random.RandomState(seed + 1000)
    free = np.flatnonzero(~support.ravel())
    pick = rs.choice(free, size=N_TEST, replace=False)
    tu, ti = pick // M.shape[1], pick % M.shape[1]
    X = pd.DataFrame({"user_id": users[tu], "item_id": items[ti]})
    pred = np.asarray(model.predict(X, bound_ratings=False), dtype=np.float64)
    pred_b = np.asarray(model.predict(X, bound_ratings=True), dtype=np.float64)
    # the reference's own candidates, cut margin and denominator per pair
    margin, den = np.empty(N_TEST), np.empty(N_TEST)
    for p in range(N_TEST):
        e, col = (ti[p], M[tu[p], :]) if item_side else (tu[p], M[:, ti[p]])
        s = np.sort(S[e][col > 0])[::-1]
        margin[p] = s[n_neighbors - 1] - s[n_neighbors] if len(s) > n_neighbors else np.inf
        den[p] = np.abs(s[:n_neighbors]).sum()
    excluded = (margin < MARGIN_MIN) | (den < DEN_MIN)
    assert excluded.mean() <= EXCLUDED_MAX, (cls_name, excluded.sum())
    return dict(train_user=data["user_id"].to_numpy(), train_item=data["item_id"].to_numpy(),
                train_rating=trained, user_ids=users, item_ids=items, similarity=S, means=means,
                test_user=users[tu], test_item=items[ti], pred=pred, pred_bounded=pred_b,
                margin=margin, den=den, n_neighbors=np.int64(n_neighbors),
                min_rating=np.float64(min_rating), max_rating=np.float64(5.0),
                global_mean=np.float64(model.global_mean)), int(excluded.sum()), float(den.min())


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("reference", help="path of the reference checkout")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                  "..", "tests", "golden"))
    args = ap.parse_args()
    ref = import_reference(args.reference)
    for name, (nu, ni, nnz, nn, nz, lo, seed) in DATASETS.items():
        data = synth(nu, ni, nnz, nz, seed)
        for cls_name in ("ItemItemCF", "UserUserCF"):
            case, n_ex, den_min = run_case(ref, cls_name, data, nn, lo, seed)
            path = os.path.normpath(os.path.join(args.out, f"cf_{name}_{cls_name.lower()}.npz"))
            np.savez_compressed(path, **case)
            print(f"{path}: {os.path.getsize(path)} bytes, {n_ex} of {N_TEST} pairs below the "
                  f"margin / denominator floors, smallest denominator {den_min:.3f}")


if __name__ == "__main__":
    main()
