#!/usr/bin/env python
"""Device-event timing of the neighbourhood models' kernels: fit (mf_cf_stats +
mf_cf_similarity) and predict (mf_cf_predict) of 10^6 held-out pairs.

    python tools/bench_cf.py --out profiles/cf/bench_cf.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_cf.py --reps 3

Legs (synthetic ratings, half-integers 0.5..5):
  c2_itemitem        100K users x 10K items, 5M ratings, uniform pairs
  mlsmall_itemitem   610 users x 9.7K items, 100K ratings, popularity-skewed
  mlsmall_useruser   the same ratings, users as the entities
The similarity kernel is set against two floors: its own multiply-add count
sum_o deg(o)^2 -- each one an 8-B LDS read and an 8-B LDS write, so the LDS
array's 256 B/clk/CU bounds it -- and the n_entities^2 float32 store at the
measured HBM copy rate.  ``engine_build_ms`` is the wall time of building the
device state from host triples (upload, two device sorts, both kernels).
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "matrix-factorization_amd"))

from matrix_factorization import _lib  # noqa: E402
from matrix_factorization.engine import _tp  # noqa: E402
from matrix_factorization.neighbours import NeighbourEngine  # noqa: E402

HBM_BYTES_PER_S = 6.29e12          # measured float4 copy rate of the MI355X
LDS_BYTES_PER_S = 256 * 256 * 2.4e9   # 256 B/clk/CU x 256 CUs x 2.4 GHz


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]),
            "spread": float((a[-1] - a[0]) / np.median(a)), "reps": len(a)}


def synth(nu, ni, nnz, skew, seed):
    rs = np.random.RandomState(seed)
    if skew:
        pu = 1.0 / np.arange(1, nu + 1) ** 0.8
        pi = 1.0 / np.arange(1, ni + 1) ** 0.9
        pu, pi = pu / pu.sum(), pi / pi.sum()
    keys = np.empty(0, np.int64)
    while len(keys) < nnz:
        m = 2 * (nnz - len(keys)) + 1024
        u = rs.choice(nu, m, p=pu) if skew else rs.randint(0, nu, m)
        i = rs.choice(ni, m, p=pi) if skew else rs.randint(0, ni, m)
        keys = np.unique(np.concatenate([keys, u.astype(np.int64) * ni + i]))
        if len(keys) > nnz:
            keys = rs.permutation(keys)[:nnz]
    r = rs.randint(1, 11, nnz) / 2.0
    return (keys // ni).astype(np.int32), (keys % ni).astype(np.int32), r, np.sort(keys)


def held_out(nu, ni, keys, n, seed):
    rs = np.random.RandomState(seed)
    out = np.empty(0, np.int64)
    while len(out) < n:
        c = rs.randint(0, nu * ni, 2 * (n - len(out)) + 1024).astype(np.int64)
        pos = np.minimum(np.searchsorted(keys, c), len(keys) - 1)
        out = np.concatenate([out, c[keys[pos] != c]])
    out = out[:n]
    return (out // ni).astype(np.int32), (out % ni).astype(np.int32)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return stats(ms)


def leg(name, nu, ni, nnz, skew, entity, n_neighbors, n_pairs, reps, warmup, dev):
    u, i, r, keys = synth(nu, ni, nnz, skew, 77)
    ent, oth, ne, no = (i, u, ni, nu) if entity == "item" else (u, i, nu, ni)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng = NeighbourEngine(ent, oth, r, ne, no, dev)
    eng.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    eptr, eoth, er = eng.entity_csr
    optr, oent, orr = eng.other_csr
    deg = (optr[1:] - optr[:-1]).double()
    macs = float((deg * deg).sum())
    S2 = torch.empty_like(eng.S)

    def do_stats():
        _lib.call("mf_cf_stats", _tp(eptr), _tp(er), ne, no, _lib.MF_F32, _tp(eng.mean),
                  _tp(eng.norm), eng.stream)

    def do_sim():
        _lib.call("mf_cf_similarity", _tp(eptr), _tp(eoth), _tp(er), _tp(optr), _tp(oent),
                  _tp(orr), ne, no, _lib.MF_F32, _tp(eng.mean), _tp(eng.norm), 0, _tp(S2),
                  eng.stream)

    out = {"shape": {"users": nu, "items": ni, "ratings": nnz, "entities": entity + "s",
                     "n_neighbors": n_neighbors, "skewed": bool(skew)},
           "engine_build_ms": build_ms, "similarity_bytes": 4 * ne * ne,
           "pass_cols": int(_lib.load().mf_cf_pass_cols(ne, 0)),
           "stats": timed(do_stats, reps, warmup), "similarity": timed(do_sim, reps, warmup)}
    if not torch.equal(S2, eng.S):
        raise RuntimeError("mf_cf_similarity: two runs differ")
    sim_s = out["similarity"]["median_ms"] * 1e-3
    out["similarity"].update({
        "multiply_adds": macs, "gmac_per_s": macs / sim_s / 1e9,
        "lds_floor_ms": macs * 16 / LDS_BYTES_PER_S * 1e3,
        "store_floor_ms": 4.0 * ne * ne / HBM_BYTES_PER_S * 1e3,
        "store_gb_per_s": 4.0 * ne * ne / sim_s / 1e9})
    pu, pi = held_out(nu, ni, keys, n_pairs, 78)
    pe, po = (pi, pu) if entity == "item" else (pu, pi)
    d_e = torch.from_numpy(pe).to(dev)
    d_o = torch.from_numpy(po).to(dev)
    res = torch.empty(n_pairs, dtype=torch.float64, device=dev)

    def do_pred():
        _lib.call("mf_cf_predict", _tp(d_e), _tp(d_o), n_pairs, _tp(optr), _tp(oent), _tp(orr),
                  _tp(eng.S), _tp(eng.mean), ne, no, _lib.MF_F32, n_neighbors, 2.75, 0.0, 5.0, 1,
                  _tp(res), eng.stream)

    out["predict"] = timed(do_pred, reps, warmup)
    out["predict"]["pairs"] = n_pairs
    out["predict"]["mpairs_per_s"] = n_pairs / (out["predict"]["median_ms"] * 1e-3) / 1e6
    lens = deg[d_o.long()]
    out["predict"]["mean_list_length"] = float(lens.mean())
    out["predict"]["max_list_length"] = float(lens.max())
    out["predict"]["fraction_cut"] = float((lens > n_neighbors).double().mean())
    t0 = time.perf_counter()
    host = eng.predict(pe, po, n_neighbors, 2.75, 0.0, 5.0, True)
    out["predict"]["engine_predict_wall_ms"] = (time.perf_counter() - t0) * 1e3
    if not np.array_equal(host, res.cpu().numpy()) or not np.all(np.isfinite(host)):
        raise RuntimeError("mf_cf_predict: the chunked call differs from the single launch")
    print(f"{name}: similarity {out['similarity']['median_ms']:.3f} ms, predict "
          f"{out['predict']['median_ms']:.3f} ms", file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--legs", nargs="+",
                    default=["c2_itemitem", "mlsmall_itemitem", "mlsmall_useruser"])
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--n-neighbors", type=int, default=50)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cf.py needs a HIP device")
    dev = torch.device("cuda:0")
    shapes = {"c2_itemitem": (100_000, 10_000, 5_000_000, False, "item"),
              "mlsmall_itemitem": (610, 9_700, 100_000, True, "item"),
              "mlsmall_useruser": (610, 9_700, 100_000, True, "user")}
    res = {"device": torch.cuda.get_device_name(0),
           "floors": {"hbm_bytes_per_s": HBM_BYTES_PER_S, "lds_bytes_per_s": LDS_BYTES_PER_S}}
    for name in a.legs:
        res[name] = leg(name, *shapes[name], a.n_neighbors, a.pairs, a.reps, a.warmup, dev)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
