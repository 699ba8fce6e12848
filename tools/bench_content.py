#!/usr/bin/env python
"""Device-event timing of the content-based model's kernels: the profile build
(mf_content_profiles), row normalisation (mf_content_normalize), the feature
cosine (mf_content_similarity), predict of 10^6 pairs in each scoring and
top-10 for 1024 users in the two ranking scorings.

    python tools/bench_content.py --out profiles/content/bench_content.json

Legs (synthetic ratings, half-integers 0.5..5):
  mlsmall   610 users x 9.7K items, 100K ratings, popularity-skewed, d = 19 binary columns
  c2        100K users x 10K items, 5M ratings, uniform pairs, d = 384 Gaussian features
The similarity's TFLOP/s count the full 2 n^2 d (the kernel computes the tiles
on or above the diagonal only).  For context only: the same similarity by
``torch.matmul`` on the normalised rows, and scikit-learn's ``cosine_similarity``
on the host at the small shape.
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

from bench_cf import held_out, synth, timed  # noqa: E402
from matrix_factorization import _lib  # noqa: E402
from matrix_factorization.content_based import ContentEngine  # noqa: E402
from matrix_factorization.device_model import DeviceModel, _tp  # noqa: E402
from matrix_factorization.neighbours import NeighbourEngine  # noqa: E402


def leg(name, nu, ni, nnz, skew, d, binary, n_neighbors, n_pairs, n_query, reps, warmup, dev):
    u, i, r, keys = synth(nu, ni, nnz, skew, 77)
    rs = np.random.RandomState(5)
    F = (rs.random_sample((ni, d)) < 0.15).astype(np.float64) if binary else rs.normal(0, 1, (ni, d))
    has = np.ones(ni, bool)
    has[rs.choice(ni, ni // 100, replace=False)] = False
    F[~has] = 0.0
    eng = ContentEngine(F, has, dev)
    out = {"shape": {"users": nu, "items": ni, "ratings": nnz, "d": d, "skewed": bool(skew)}}

    # profiles: the CSR once, then the kernel alone
    order = np.argsort(u, kind="stable")
    ptr = np.zeros(nu + 1, np.int64)
    np.cumsum(np.bincount(u, minlength=nu), out=ptr[1:])
    d_ptr = torch.from_numpy(ptr).to(dev)
    d_it = torch.from_numpy(i[order].astype(np.int32)).to(dev)
    d_w = torch.from_numpy(r[order] - 0.5).to(dev)
    P = torch.empty((nu, d), dtype=torch.float64, device=dev)

    def do_profiles():
        _lib.call("mf_content_profiles", _tp(d_ptr), _tp(d_it), _tp(d_w), _tp(eng.F), _tp(eng.has),
                  nu, ni, d, _lib.MF_F64, _tp(P), eng.stream)

    out["profiles"] = timed(do_profiles, reps, warmup)
    read = 8.0 * nnz * d + 12.0 * nnz * ((d + 63) // 64)
    out["profiles"]["gathered_gb_per_s"] = read / (out["profiles"]["median_ms"] * 1e-3) / 1e9
    if not torch.equal(P, eng.profiles(u, i, r - 0.5, nu)):
        raise RuntimeError("mf_content_profiles: two runs differ")

    dpad = (d + 3) // 4 * 4
    out["normalize_items"] = timed(lambda: eng.normalize(eng.F, dpad), reps, warmup)
    out["normalize_profiles"] = timed(lambda: eng.normalize(P, dpad), reps, warmup)
    Qn, Pn = eng.normalize(eng.F, dpad), eng.normalize(P, dpad)
    S = torch.empty((ni, ni), dtype=torch.float32, device=dev)

    def do_sim():
        _lib.call("mf_content_similarity", _tp(Qn), ni, dpad, _lib.MF_F32, _tp(S), eng.stream)

    out["similarity"] = timed(do_sim, reps, warmup)
    flop = 2.0 * ni * ni * d
    out["similarity"]["tflop_per_s_full_n2d"] = flop / (out["similarity"]["median_ms"] * 1e-3) / 1e12
    out["similarity"]["store_gb_per_s"] = 4.0 * ni * ni / (out["similarity"]["median_ms"] * 1e-3) / 1e9
    try:
        out["similarity_torch_matmul"] = timed(lambda: torch.matmul(Qn, Qn.T), reps, warmup)
        out["similarity_torch_matmul"]["max_abs_diff"] = float(
            (torch.matmul(Qn, Qn.T) - S).abs().max())
    except RuntimeError as e:                              # context only: no vendor BLAS, no figure
        out["similarity_torch_matmul"] = {"error": str(e).splitlines()[0]}
    if ni * ni * d <= 1e10:                                # the small shape only
        from sklearn.metrics.pairwise import cosine_similarity

        t0 = time.perf_counter()
        cosine_similarity(F)
        out["similarity_sklearn_host_ms"] = (time.perf_counter() - t0) * 1e3

    # predict of n_pairs held-out pairs and top-10 for n_query users, per scoring
    pu, pi = held_out(nu, ni, keys, n_pairs, 78)
    queries = np.random.RandomState(6).choice(nu, n_query, replace=False).astype(np.int32)
    pm = P.cpu().numpy().mean(axis=1)
    t0 = time.perf_counter()
    np.clip(pm[pu], 0.5, 5.0)
    out["predict_reference_host_ms"] = (time.perf_counter() - t0) * 1e3

    cos = DeviceModel(nu, ni, dpad, "linear", "float32", dev, min_rating=0.5, max_rating=5.0,
                      global_mean=0.0)
    cos.load_params(Pn, Qn, np.zeros(nu), np.zeros(ni))
    d_u, d_i = torch.from_numpy(pu).to(dev), torch.from_numpy(pi).to(dev)
    res32 = torch.empty(n_pairs, dtype=torch.float32, device=dev)

    def do_cos():
        _lib.call("mf_predict", _tp(d_u), _tp(d_i), n_pairs, 0.0, _tp(cos.bu), _tp(cos.bi),
                  _tp(cos.P), _tp(cos.Q), cos.k, cos.kcode, cos.dcode, 0.0, 0.5, 5.0, 0,
                  _tp(res32), cos.stream)

    out["predict_cosine"] = timed(do_cos, reps, warmup)
    q = cos.topk_prepare(queries, 10)

    def do_cos_topk():
        cos.topk_launch(q)
        cos.topk_finish(q)

    out["topk_cosine"] = timed(do_cos_topk, reps, warmup)
    out["topk_cosine"]["mfma_filter"] = bool(q["mm"])

    nbr = NeighbourEngine(i, u, r, ni, nu, dev, similarity=S)
    optr, oent, orr = nbr.other_csr
    res64 = torch.empty(n_pairs, dtype=torch.float64, device=dev)

    def do_nbr():
        _lib.call("mf_cf_predict", _tp(d_i), _tp(d_u), n_pairs, _tp(optr), _tp(oent), _tp(orr),
                  _tp(nbr.S), _tp(nbr.mean), ni, nu, _lib.MF_F32, n_neighbors, 2.75, 0.5, 5.0, 1,
                  _tp(res64), nbr.stream)

    out["predict_neighbors"] = timed(do_nbr, reps, warmup)
    out["topk_neighbors_wall"] = timed(
        lambda: nbr.topk(queries, _lib.MF_CF_QUERY_OTHER, n_neighbors, 2.75, 10), max(reps // 3, 1), 1)
    for key in ("predict_cosine", "predict_neighbors"):
        out[key]["mpairs_per_s"] = n_pairs / (out[key]["median_ms"] * 1e-3) / 1e6
    for key in ("topk_cosine", "topk_neighbors_wall"):
        out[key]["queries"] = n_query
    print(f"{name}: profiles {out['profiles']['median_ms']:.3f} ms, similarity "
          f"{out['similarity']['median_ms']:.3f} ms "
          f"({out['similarity']['tflop_per_s_full_n2d']:.1f} TFLOP/s)", file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--legs", nargs="+", default=["mlsmall", "c2"])
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--n-neighbors", type=int, default=50)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_content.py needs a HIP device")
    dev = torch.device("cuda:0")
    shapes = {"mlsmall": (610, 9_700, 100_000, True, 19, True),
              "c2": (100_000, 10_000, 5_000_000, False, 384, False)}
    res = {"device": torch.cuda.get_device_name(0)}
    for name in a.legs:
        res[name] = leg(name, *shapes[name], a.n_neighbors, a.pairs, min(a.queries, shapes[name][0]),
                        a.reps, a.warmup, dev)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
