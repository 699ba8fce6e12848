#!/usr/bin/env python3
"""Write tests/golden/content_{genres,embed}.npz: the reference's
ContentBasedRecommender (matrix_factorization/content_based.py), run unmodified
on the CPU.

    python tools/make_content_fixture.py /path/to/reference/checkout

The reference's ``fit`` trains on ratings permuted against their pairs (it
shuffles X, then assigns ``y.values`` positionally).  The fixture stores as its
TRAINING INPUT the triples the reference actually trained on, recovered by
replaying the shuffle: with the same ``np.random.seed``, ``sample(frac=1)`` on
a frame of the same length gives the reference's row order, and ``y.values``
lands on it positionally.  Before anything is written, the NumPy restatement
(tests/content_reference.py) on the replayed triples must reproduce the
reference's profiles.

Per case the file holds
  train_user, train_item, train_rating   the replayed triples, external ids, in
                                         the reference's (shuffled) row order
  feat_item, feat_values, feat_cols      the feature frame as given to ``fit``
  user_ids, item_ids                     external ids in the reference's internal order
  profiles                               the reference's user_profiles, n_users x d
  similarity, sim_item                   its item_similarity_matrix (frame-row order,
                                         duplicates included) and each row's internal item id
  test_user, test_item                   400 pairs, unknown ids among them
  pred, pred_bounded                     the reference's ``predict`` for them
  global_mean, min_rating, max_rating
The two cases: ``genres`` (60 users x 80 items, 1500 ratings, 19 binary
columns; a duplicated feature row, two unknown ids, an item without features
and an all-zero feature row) and ``embed`` (200 x 150, 6000 ratings, d = 24
Gaussian features, one item without features).  Data only, CPU only.
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import pandas as pd

from make_cf_fixture import import_reference, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import content_reference as cref  # noqa: E402

N_TEST = 400


def features(name, items, rs):
    """The feature frame of a case (external item ids)."""
    if name == "genres":
        vals = (rs.random_sample((len(items), 19)) < 0.18).astype(np.int64)
        ids = items.copy()
        vals[5] = 0                                          # an all-zero feature row
        keep = np.ones(len(items), bool)
        keep[11] = False                                     # an item without features
        ids, vals = ids[keep], vals[keep]
        # a duplicated row (another content: the first one counts) and two unknown ids
        ids = np.concatenate([ids[:30], [ids[3]], ids[30:], [999001, 999002]])
        extra = (rs.random_sample((3, 19)) < 0.5).astype(np.int64)
        vals = np.concatenate([vals[:30], extra[:1], vals[30:], extra[1:]])
        cols = [f"genre_{c:02d}" for c in range(19)]
    else:
        vals = rs.normal(0, 1, (len(items), 24))
        keep = np.ones(len(items), bool)
        keep[17] = False
        ids, vals = items[keep], vals[keep]
        cols = [f"e{c:02d}" for c in range(24)]
    frame = pd.DataFrame(vals, columns=cols)
    frame.insert(0, "item_id", ids)
    return frame


def run_case(ref, name, data, min_rating, seed):
    rs = np.random.RandomState(seed + 500)
    frame = features(name, np.sort(data["item_id"].unique()), rs)
    np.random.seed(seed)
    model = ref.ContentBasedRecommender(min_rating=min_rating, max_rating=5)
    model.fit(data[["user_id", "item_id"]], data["rating"], item_features=frame)
    # the shuffle, replayed: the pairs in sample(frac=1)'s order, y.values on them
    np.random.seed(seed)
    order = pd.DataFrame({"a": np.arange(len(data))}).sample(frac=1).index.to_numpy()
    tr_u = data["user_id"].to_numpy()[order]
    tr_i = data["item_id"].to_numpy()[order]
    tr_r = data["rating"].to_numpy(np.float64)
    users = np.asarray(list(model.user_id_map.keys()))
    items = np.asarray(list(model.item_id_map.keys()))
    assert list(model.user_id_map.values()) == list(range(len(users)))
    assert list(model.item_id_map.values()) == list(range(len(items)))
    assert np.array_equal(pd.unique(tr_u), users) and np.array_equal(pd.unique(tr_i), items)
    d = frame.shape[1] - 1
    P = np.stack([np.asarray(model.user_profiles[u], np.float64) for u in range(len(users))])
    S = np.asarray(model.item_similarity_matrix, np.float64)
    sim_item = model.item_features["item_id"].to_numpy(np.int64)
    assert P.shape == (len(users), d) and S.shape == (len(sim_item), len(sim_item))
    # the restatement on the replayed triples is the reference's model
    case = dict(train_user=tr_u, train_item=tr_i, train_rating=tr_r,
                feat_item=frame["item_id"].to_numpy(),
                feat_values=frame.drop(columns="item_id").to_numpy(np.float64),
                feat_cols=np.asarray(list(frame.columns[1:])), user_ids=users, item_ids=items)
    u, i, r, fi, _, _ = cref.internal(dict(case, test_user=users[:0], test_item=items[:0]))
    F, has = cref.feature_matrix(fi, case["feat_values"], len(items))
    dP = float(np.max(np.abs(cref.profiles(u, i, r, F, has, len(users), min_rating) - P)))
    # (an item's first frame row is the one that counts: a duplicate's row of
    # the reference's matrix has no counterpart)
    rows = cref.first_rows(sim_item)
    dS = float(np.max(np.abs(cref.similarity(F)[np.ix_(sim_item[rows], sim_item[rows])]
                             - S[np.ix_(rows, rows)])))
    assert dP <= 1e-12 and dS <= 1e-12, (name, dP, dS)
    # test pairs: known ids, and unknown users / items among them
    rs = np.random.RandomState(seed + 1000)
    tu = users[rs.randint(0, len(users), N_TEST)]
    ti = items[rs.randint(0, len(items), N_TEST)]
    tu[rs.choice(N_TEST, 12, replace=False)] = 999100
    ti[rs.choice(N_TEST, 12, replace=False)] = 999200
    X = pd.DataFrame({"user_id": tu, "item_id": ti})
    pred = np.asarray(model.predict(X, bound_ratings=False), np.float64)
    pred_b = np.asarray(model.predict(X, bound_ratings=True), np.float64)
    case.update(profiles=P, similarity=S, sim_item=sim_item, test_user=tu, test_item=ti,
                pred=pred, pred_bounded=pred_b, global_mean=np.float64(model.global_mean),
                min_rating=np.float64(min_rating), max_rating=np.float64(5.0))
    return case, dP, dS, int((~has).sum())


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("reference", help="path of the reference checkout")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                  "..", "tests", "golden"))
    args = ap.parse_args()
    ref = import_reference(args.reference)
    # the two datasets of tools/make_cf_fixture.py
    for name, (nu, ni, nnz, nz, lo, seed) in {"genres": (60, 80, 1500, 0, 0.5, 11),
                                              "embed": (200, 150, 6000, 12, 0.0, 12)}.items():
        data = synth(nu, ni, nnz, nz, seed)
        case, dP, dS, n_without = run_case(ref, name, data, lo, seed)
        path = os.path.normpath(os.path.join(args.out, f"content_{name}.npz"))
        np.savez_compressed(path, **case)
        print(f"{path}: {os.path.getsize(path)} bytes; restatement vs reference: profiles "
              f"{dP:.1e}, similarity {dS:.1e}; {n_without} items without features")


if __name__ == "__main__":
    main()
