#!/usr/bin/env python
"""Device-event timing of the neighbourhood models' all-items pass for 1024
query users: mf_cf_scores / mf_cf_topk / mf_cf_rank against mf_cf_predict over
the same explicit (user, item) pairs.

    python tools/bench_cf_topk.py --out profiles/cf_topk/bench_cf_topk.json

Legs (tools/bench_cf.py's synthetic half-integer ratings):
  c2_itemitem        100K users x 10K items, 5M ratings, uniform pairs
  mlsmall_itemitem   610 users x 9.7K items, 100K ratings, popularity-skewed
  mlsmall_useruser   the same ratings, users as the entities
(the 1024 queries of the 610-user legs are drawn with replacement).  Per leg,
in one process, median and min-max of --reps runs:
  predict_pairs   mf_cf_predict on the 1024 x n_items pairs (one workgroup a pair)
  scores          mf_cf_scores; user-user also with MF_CF_ROW_LDS=1 (scores_row_lds)
  topk            mf_cf_topk, amount 10, the users' training items excluded
  rank            mf_cf_rank, 20 random targets per user, the same exclusions
``scores`` must equal ``predict_pairs`` bit for bit; ``faster`` says whether
the two min-max ranges are disjoint with scores below.
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "matrix-factorization_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_cf import synth, timed  # noqa: E402
from matrix_factorization import _lib  # noqa: E402
from matrix_factorization.engine import _tp  # noqa: E402
from matrix_factorization.neighbours import NeighbourEngine  # noqa: E402

GM = 2.75


def leg(name, nu, ni, nnz, skew, entity, n_neighbors, n_query, amount, n_targets, tpb, reps,
        warmup, dev):
    u, i, r, _ = synth(nu, ni, nnz, skew, 77)
    item_side = entity == "item"
    ent, oth, ne, no = (i, u, ni, nu) if item_side else (u, i, nu, ni)
    eng = NeighbourEngine(ent, oth, r, ne, no, dev)
    eng.targets_per_block = tpb
    side = _lib.MF_CF_QUERY_OTHER if item_side else _lib.MF_CF_QUERY_ENTITY
    rs = np.random.RandomState(79)
    users = rs.choice(nu, n_query, replace=nu < n_query).astype(np.int32)
    model = eng._model_args(n_neighbors, GM)
    optr, oent, orr = eng.other_csr
    to = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).to(dev)  # noqa: E731

    # (a) the explicit pairs
    pu, pi = np.repeat(users, ni), np.tile(np.arange(ni, dtype=np.int32), n_query)
    d_e, d_o = (to(pi, np.int32), to(pu, np.int32)) if item_side else \
        (to(pu, np.int32), to(pi, np.int32))
    pairs = torch.empty(n_query * ni, dtype=torch.float64, device=dev)

    def do_pairs():
        _lib.call("mf_cf_predict", _tp(d_e), _tp(d_o), n_query * ni, _tp(optr), _tp(oent),
                  _tp(orr), _tp(eng.S), _tp(eng.mean), ne, no, _lib.MF_F32, n_neighbors, GM, 0.0,
                  5.0, 0, _tp(pairs), eng.stream)

    # (b) .. (d): training exclusions and random targets as device CSR
    d_q = to(users, np.int32)
    order = np.argsort(u, kind="stable")
    uptr = np.zeros(nu + 1, np.int64)
    np.cumsum(np.bincount(u, minlength=nu), out=uptr[1:])
    per = [i[order[uptr[x]:uptr[x + 1]]] for x in users]
    ex_ptr = to(np.concatenate([[0], np.cumsum([len(x) for x in per])]), np.int64)
    ex_items = to(np.concatenate(per), np.int32)
    tg_ptr = to(np.arange(n_query + 1) * n_targets, np.int64)
    tg_items = to(rs.randint(0, ni, n_query * n_targets), np.int32)
    dense = torch.empty((n_query, ni), dtype=torch.float64, device=dev)
    ws = torch.empty(_lib.load().mf_cf_topk_workspace_bytes(n_query, ni), dtype=torch.uint8,
                     device=dev)
    items = torch.empty((n_query, amount), dtype=torch.int32, device=dev)
    best = torch.empty((n_query, amount), dtype=torch.float64, device=dev)
    ranks = torch.empty(n_query * n_targets, dtype=torch.int32, device=dev)
    cands = torch.empty(n_query, dtype=torch.int32, device=dev)

    def do_scores():
        _lib.call("mf_cf_scores", _tp(d_q), n_query, side, *model, _tp(dense), eng.stream)

    def do_topk():
        _lib.call("mf_cf_topk", _tp(d_q), n_query, side, *model, _tp(ex_ptr), _tp(ex_items),
                  amount, _tp(ws), _tp(items), _tp(best), eng.stream)

    def do_rank():
        _lib.call("mf_cf_rank", _tp(d_q), n_query, side, *model, _tp(ex_ptr), _tp(ex_items),
                  _tp(tg_ptr), _tp(tg_items), _tp(ws), _tp(ranks), _tp(cands), eng.stream)

    deg = (optr[1:] - optr[:-1]).double()
    out = {"shape": {"users": nu, "items": ni, "ratings": nnz, "entities": entity + "s",
                     "n_neighbors": n_neighbors, "skewed": bool(skew), "queries": n_query,
                     "pairs": n_query * ni, "amount": amount, "targets_per_query": n_targets,
                     "targets_per_block": int(_lib.load().mf_cf_targets_per_block(ni, tpb)),
                     "mean_list_length": float(deg.mean()), "max_list_length": float(deg.max())}}
    os.environ["MF_CF_ROW_LDS"] = "0"
    out["predict_pairs"] = timed(do_pairs, reps, warmup)
    out["scores"] = timed(do_scores, reps, warmup)
    if not torch.equal(dense.view(torch.int64).flatten(), pairs.view(torch.int64)):
        raise RuntimeError("mf_cf_scores differs from mf_cf_predict on the same pairs")
    if not item_side:
        os.environ["MF_CF_ROW_LDS"] = "1"
        out["scores_row_lds"] = timed(do_scores, reps, warmup)
        os.environ["MF_CF_ROW_LDS"] = "0"
        if not torch.equal(dense.view(torch.int64).flatten(), pairs.view(torch.int64)):
            raise RuntimeError("mf_cf_scores with the row in LDS differs from mf_cf_predict")
    out["topk"] = timed(do_topk, reps, warmup)
    out["rank"] = timed(do_rank, reps, warmup)
    a, b = out["predict_pairs"], out["scores"]
    out["scores_vs_pairs"] = {"ratio_of_medians": a["median_ms"] / b["median_ms"],
                              "faster": bool(b["max_ms"] < a["min_ms"]),
                              "slower": bool(b["min_ms"] > a["max_ms"])}
    for k in ("predict_pairs", "scores"):
        out[k]["mpairs_per_s"] = n_query * ni / (out[k]["median_ms"] * 1e-3) / 1e6
    print(f"{name}: pairs {a['median_ms']:.3f} ms, scores {b['median_ms']:.3f} ms, topk "
          f"{out['topk']['median_ms']:.3f} ms, rank {out['rank']['median_ms']:.3f} ms",
          file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--legs", nargs="+",
                    default=["c2_itemitem", "mlsmall_itemitem", "mlsmall_useruser"])
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--amount", type=int, default=10)
    ap.add_argument("--targets", type=int, default=20)
    ap.add_argument("--targets-per-block", type=int, default=0,
                    help="targets a workgroup of k_cf_scores walks (0: the library's choice)")
    ap.add_argument("--n-neighbors", type=int, default=50)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cf_topk.py needs a HIP device")
    dev = torch.device("cuda:0")
    shapes = {"c2_itemitem": (100_000, 10_000, 5_000_000, False, "item"),
              "mlsmall_itemitem": (610, 9_700, 100_000, True, "item"),
              "mlsmall_useruser": (610, 9_700, 100_000, True, "user")}
    res = {"device": torch.cuda.get_device_name(0)}
    for name in a.legs:
        res[name] = leg(name, *shapes[name], a.n_neighbors, a.queries, a.amount, a.targets,
                        a.targets_per_block, a.reps, a.warmup, dev)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
