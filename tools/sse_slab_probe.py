#!/usr/bin/env python
"""Time the item-stationary training-SSE pass (mf_sse_slab, k_sse_slab) alone
at one shape over user super-windows per phase (W), waves per workgroup,
register sets (user rows issued sets - 1 steps ahead) and LDS row padding, and
print each form's SSE relative to the default pass (k_sse_lean) of the same
engine.

Usage: python tools/sse_slab_probe.py [--dtype float64] [--shape c3]
           [--json out.json] W:waves:sets[:pad] ...
(shapes: c3 = 1M x 100K, 100M ratings; c3_shard2 / 4 / 8 = its N = 2 / 4 / 8
user shards; c2 = 100K x 10K, 5M ratings, rank 32)"""

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "matrix-factorization_amd"))

import numpy as np
import torch

import bench
from matrix_factorization.engine import SGDEngine

SHAPES = {"c3": (1_000_000, 100_000, 100_000_000, 64),
          "c3_shard2": (500_000, 100_000, 50_000_000, 64),
          "c3_shard4": (250_000, 100_000, 25_000_000, 64),
          "c3_shard8": (125_000, 100_000, 12_500_000, 64),
          "c2": (100_000, 10_000, 5_000_000, 32)}


def timed(eng, reps):
    for _ in range(3):
        eng.sse_async(0)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for s in range(reps):
        eng.sse_async(s)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps, eng.sse_values(1)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--shape", default="c3", choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("forms", nargs="*", default=["4:8:2"])
    args = ap.parse_args()
    nu, ni, nnz, k = SHAPES[args.shape]
    u, i, r = bench.synth(nu, ni, nnz)
    dt = args.dtype
    os.environ["MF_SSE_SLAB"] = "0"
    eng = SGDEngine(u, i, r, nu, ni, k, "linear", dt, "cuda:0",
                    global_mean=float(r.mean()), min_rating=1, max_rating=5)
    rs = np.random.RandomState(0)
    eng.load_params(rs.normal(0, 0.1, (nu, k)).astype(dt),
                    rs.normal(0, 0.1, (ni, k)).astype(dt),
                    rs.normal(0, 0.1, nu).astype(dt), rs.normal(0, 0.1, ni).astype(dt))
    ms, ref = timed(eng, args.reps)
    rows = [dict(shape=args.shape, dtype=dt, form="lean", sse_ms=round(ms, 4), rel=0.0)]
    print(f"shape={args.shape} dtype={dt} form=lean sse_ms={ms:.3f} sse={ref:.10f}", flush=True)
    os.environ["MF_SSE_SLAB"] = "1"
    built = None
    for f in args.forms:
        p = [int(x) for x in f.split(":")]
        w, waves, sets, pad = p[0], p[1], p[2], (p[3] if len(p) > 3 else 0)
        os.environ["MF_SSE_SLAB_W"] = str(w)
        os.environ["MF_SSE_SLAB_PAD"] = str(pad)
        os.environ["MF_SSE_SLAB_WAVES"] = str(waves)
        os.environ["MF_SSE_SLAB_SETS"] = str(sets)
        if built != (w, pad):
            eng._build_eval()
            built = (w, pad)
        ms, sse = timed(eng, args.reps)
        attrs = (ctypes.c_int32 * 3)()           # (no launch: the kernel's registers)
        eng._sse_slab(eng.P, eng.Q, eng.bu, eng.bi, eng.ws,
                      ctypes.c_void_p(eng.sse_buf.data_ptr()), eng.stream, attrs=attrs)
        sl = eng.slab
        rows.append(dict(shape=args.shape, dtype=dt, form=f, windows=w, waves=waves, sets=sets,
                         pad=pad, groups=sl["groups"], phases=sl["phases"], lds=sl["lds"],
                         regs=attrs[0],
                         sse_ms=round(ms, 4), rel=abs(sse - ref) / ref))
        print(f"shape={args.shape} dtype={dt} form={f} groups={sl['groups']} "
              f"phases={sl['phases']} lds={sl['lds']} regs={attrs[0]} sse_ms={ms:.3f} sse={sse:.10f} "
              f"rel_to_lean={abs(sse - ref) / ref:.2e}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
