#!/usr/bin/env python
"""Device-event timing of the stored-neighbours (top-M) neighbourhood model
against the dense one (tools/bench_cf.py times the dense model alone).

    python tools/bench_cf_truncated.py --out profiles/cf_truncated/bench.json

Legs (bench_cf.py's synthetic C2 ratings: 100K users x 10K items, 5M ratings,
half-integers 0.5..5, n_neighbors = 50):
  c2_itemitem   10K entities, M in {64, 256}: mf_cf_neighbours against
                mf_cf_similarity in the same run, mf_cf_predict_nbr of 10^6
                held-out pairs against mf_cf_predict, mf_cf_scores_nbr for
                1024 users against mf_cf_scores, and the RMSE of the truncated
                predictions against the dense ones on those pairs
  c2_useruser   100K entities, which the dense model refuses at the default
                budget, M = 256: build time and device bytes
Every number is the median of --reps launches between device events.  Each leg
runs in a child process of its own under a time limit (--leg-timeout); a leg
that fails or runs out of time ends the run.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {"c2_itemitem": ("item", [64, 256]), "c2_useruser": ("user", [256])}
NU, NI, NNZ = 100_000, 10_000, 5_000_000


def run_leg(name, a):
    import numpy as np
    import torch

    sys.path.insert(0, os.path.join(ROOT, "matrix-factorization_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_cf import held_out, synth, timed
    from matrix_factorization import _lib
    from matrix_factorization.engine import _tp
    from matrix_factorization.neighbours import (DEFAULT_MAX_SIMILARITY_BYTES, NeighbourEngine,
                                                 neighbour_bytes, similarity_bytes)

    if not torch.cuda.is_available():
        raise SystemExit("bench_cf_truncated.py needs a HIP device")
    dev = torch.device("cuda:0")
    entity, Ms = LEGS[name]
    u, i, r, keys = synth(NU, NI, NNZ, False, 77)
    ent, oth, ne, no = (i, u, NI, NU) if entity == "item" else (u, i, NU, NI)
    nn = a.n_neighbors
    out = {"shape": {"users": NU, "items": NI, "ratings": NNZ, "entities": entity + "s",
                     "n_entities": ne, "n_neighbors": nn},
           "dense_similarity_bytes": similarity_bytes(ne),
           "dense_fits_default_budget": similarity_bytes(ne) <= DEFAULT_MAX_SIMILARITY_BYTES}
    dense = None
    if out["dense_fits_default_budget"]:
        dense = NeighbourEngine(ent, oth, r, ne, no, dev)
        eptr, eoth, er = dense.entity_csr
        optr, oent, orr = dense.other_csr
        S2 = torch.empty_like(dense.S)
        out["dense"] = {"similarity": timed(lambda: _lib.call(
            "mf_cf_similarity", _tp(eptr), _tp(eoth), _tp(er), _tp(optr), _tp(oent), _tp(orr), ne,
            no, _lib.MF_F32, _tp(dense.mean), _tp(dense.norm), 0, _tp(S2), dense.stream),
            a.reps, a.warmup)}
        del S2
        pu, pi = held_out(NU, NI, keys, a.pairs, 78)
        pe, po = (pi, pu) if entity == "item" else (pu, pi)
        d_e, d_o = torch.from_numpy(pe).to(dev), torch.from_numpy(po).to(dev)
        res = torch.empty(a.pairs, dtype=torch.float64, device=dev)
        side = _lib.MF_CF_QUERY_OTHER if entity == "item" else _lib.MF_CF_QUERY_ENTITY
        d_q = torch.arange(a.queries, dtype=torch.int32, device=dev)
        sc = torch.empty((a.queries, dense.n_targets(side)), dtype=torch.float64, device=dev)

        def predict_and_scores(eng):
            lists = (_tp(eng.other_csr[0]), _tp(eng.other_csr[1]), _tp(eng.other_csr[2]))
            tail = (_tp(eng.mean), ne, no, _lib.MF_F32, nn)
            p = timed(lambda: _lib.call(
                eng._fn("mf_cf_predict"), _tp(d_e), _tp(d_o), a.pairs, *lists, *eng._sim_args(),
                *tail, 2.75, 0.0, 5.0, 1, _tp(res), eng.stream), a.reps, a.warmup)
            pred = res.cpu().numpy()
            s = timed(lambda: _lib.call(
                eng._fn("mf_cf_scores"), _tp(d_q), a.queries, side, *lists, *eng._sim_args(),
                *tail, 2.75, 0, _tp(sc), eng.stream), a.reps, a.warmup)
            p["pairs"], s["queries"], s["targets"] = a.pairs, a.queries, int(sc.shape[1])
            return p, s, pred

        out["dense"]["predict"], out["dense"]["scores"], dense_pred = predict_and_scores(dense)
        dense.S = None                                # the truncated engines need no dense matrix
        torch.cuda.empty_cache()
    for M in Ms:
        eng = NeighbourEngine(ent, oth, r, ne, no, dev, stored_neighbors=M)
        eptr, eoth, er = eng.entity_csr
        optr, oent, orr = eng.other_csr
        lists_b, ws_b = neighbour_bytes(ne, M)
        ws = torch.empty(ws_b, dtype=torch.uint8, device=dev)
        ids2, sims2 = torch.empty_like(eng.nbr_ids), torch.empty_like(eng.nbr_sims)
        leg = {"stored_bytes": lists_b, "workspace_bytes": ws_b,
               "build": timed(lambda: _lib.call(
                   "mf_cf_neighbours", _tp(eptr), _tp(eoth), _tp(er), _tp(optr), _tp(oent),
                   _tp(orr), ne, no, _lib.MF_F32, _tp(eng.mean), _tp(eng.norm), 0, M, _tp(ws),
                   _tp(ids2), _tp(sims2), eng.stream), a.reps, a.warmup)}
        if not (torch.equal(ids2, eng.nbr_ids) and torch.equal(sims2, eng.nbr_sims)):
            raise RuntimeError("mf_cf_neighbours: two runs differ")
        del ws, ids2, sims2
        if dense is not None:
            leg["build"]["over_dense_similarity"] = (leg["build"]["median_ms"]
                                                     / out["dense"]["similarity"]["median_ms"])
            leg["predict"], leg["scores"], pred = predict_and_scores(eng)
            for k in ("predict", "scores"):
                leg[k]["over_dense"] = leg[k]["median_ms"] / out["dense"][k]["median_ms"]
            leg["rmse_against_dense"] = float(np.sqrt(np.mean((pred - dense_pred) ** 2)))
            leg["pairs_changed"] = float(np.mean(pred != dense_pred))
        out[f"M{M}"] = leg
        print(f"{name} M={M}: build {leg['build']['median_ms']:.3f} ms", file=sys.stderr)
        del eng
        torch.cuda.empty_cache()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--legs", nargs="+", default=list(LEGS))
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)   # the child's one leg
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--n-neighbors", type=int, default=50)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--leg-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.leg:
        return run_leg(a.leg, a)
    res = {}
    for name in a.legs:                               # a fresh process per leg, under its own limit
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--pairs", str(a.pairs),
               "--queries", str(a.queries), "--n-neighbors", str(a.n_neighbors), "--reps",
               str(a.reps), "--warmup", str(a.warmup)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.leg_timeout, check=True)
        res[name] = json.loads(done.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
