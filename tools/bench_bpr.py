#!/usr/bin/env python
"""Where one BPR epoch's time goes, part by part, at the C2 shape (100K users
x 10K items, 5M positives at uniform pairs, k = 32, float32).

    python tools/bench_bpr.py --out profiles/bpr/bench_bpr.json

Parts of engine.BPR.epoch, each timed over ``--reps`` epochs after ``--warmup``:
  shuffle    np.random.shuffle of the visit order + the seed draw   (host clock)
  sample     visit-order upload, device gather + mf_bpr_sample      (device events)
  readback   the triples (u, i, j) to the host                      (host clock, synchronises)
  levels     mf_sched_levels3                                       (host clock)
  upload     the schedule to the device                             (host clock + synchronise)
  launches   mf_bpr_epoch: one launch per level                     (device events; the host's
             enqueue time beside it)
  stats      loss and accuracy from z_out with torch                (device events)
  epoch      all of it, wall clock to a final synchronise
One leg per ``--chunks`` value (mf_sched_levels3's n_chunks: 0 = by size, 1 =
the greedy levels): more chunks build the levels on more threads but give more
levels, hence more launches.
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

from matrix_factorization.engine import BPR, SGDEngine  # noqa: E402


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]),
            "reps": len(a)}


def synth(nu, ni, nnz, seed):
    rs = np.random.RandomState(seed)
    keys = np.empty(0, np.int64)
    while len(keys) < nnz:
        m = 2 * (nnz - len(keys)) + 1024
        keys = np.unique(np.concatenate([keys, rs.randint(0, nu * ni, m).astype(np.int64)]))
        if len(keys) > nnz:
            keys = rs.permutation(keys)[:nnz]
    return (keys // ni).astype(np.int32), (keys % ni).astype(np.int32), np.ones(nnz)


class DeviceTimer:
    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.b = torch.cuda.Event(enable_timing=True)
        self.a.record()
        return self

    def __exit__(self, *exc):
        self.b.record()

    def ms(self):
        self.b.synchronize()
        return self.a.elapsed_time(self.b)


def one_epoch(bpr, lr, reg, n_chunks, t):
    """BPR.epoch's steps with a clock around each; appends to the lists of t."""
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    c = time.perf_counter()
    seed = bpr.draw()
    t["shuffle"].append((time.perf_counter() - c) * 1e3)
    with DeviceTimer() as d:
        bpr.sample(seed)
    t["sample"].append(d.ms())
    c = time.perf_counter()
    triples = bpr.readback()
    t["readback"].append((time.perf_counter() - c) * 1e3)
    c = time.perf_counter()
    sched, offs = bpr.levels(triples, True, True, n_chunks)
    t["levels"].append((time.perf_counter() - c) * 1e3)
    c = time.perf_counter()
    kept = bpr.upload(sched)
    torch.cuda.synchronize()
    t["upload"].append((time.perf_counter() - c) * 1e3)
    c = time.perf_counter()
    with DeviceTimer() as d:
        bpr.run_levels(offs, lr, reg, True, True)
        t["enqueue"].append((time.perf_counter() - c) * 1e3)
    t["launches"].append(d.ms())
    with DeviceTimer() as d:
        loss, acc = bpr.stats_async(kept)
    t["stats"].append(d.ms())
    torch.cuda.synchronize()
    t["epoch"].append((time.perf_counter() - w0) * 1e3)
    return kept, len(offs) - 1, float(loss.item()), float(acc.item())


def leg(eng, P, Q, n_chunks, lr, reg, reps, warmup):
    eng.load_params(P, Q, np.zeros(eng.n_users), np.zeros(eng.n_items))
    bpr = BPR(eng)
    np.random.seed(1)
    t = {k: [] for k in ("shuffle", "sample", "readback", "levels", "upload", "enqueue",
                         "launches", "stats", "epoch")}
    for _ in range(warmup):
        one_epoch(bpr, lr, reg, n_chunks, {k: [] for k in t})
    runs = [one_epoch(bpr, lr, reg, n_chunks, t) for _ in range(reps)]
    out = {k: stats(v) for k, v in t.items()}
    kept = [r[0] for r in runs]
    levels = [r[1] for r in runs]
    out.update({"n_chunks": n_chunks, "positives": bpr.n, "kept": kept, "n_levels": levels,
                "triples_per_level": float(np.mean(kept) / np.mean(levels)),
                "us_per_launch": out["launches"]["median_ms"] * 1e3 / float(np.mean(levels)),
                "mtriples_per_s_launches":
                    float(np.mean(kept)) / (out["launches"]["median_ms"] * 1e-3) / 1e6,
                "mtriples_per_s_epoch":
                    float(np.mean(kept)) / (out["epoch"]["median_ms"] * 1e-3) / 1e6,
                "loss": [r[2] for r in runs], "accuracy": [r[3] for r in runs]})
    print(f"n_chunks={n_chunks}: epoch {out['epoch']['median_ms']:.1f} ms, launches "
          f"{out['launches']['median_ms']:.1f} ms over {levels[-1]} levels", file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", type=int, nargs=3, default=[100_000, 10_000, 5_000_000],
                    metavar=("USERS", "ITEMS", "POSITIVES"))
    ap.add_argument("--factors", type=int, default=32)
    ap.add_argument("--dtype", default="float32")
    ap.add_argument("--chunks", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nu, ni, nnz = a.shape
    u, i, r = synth(nu, ni, nnz, 77)
    rs = np.random.RandomState(5)
    P = rs.normal(0, 0.1, (nu, a.factors))
    Q = rs.normal(0, 0.1, (ni, a.factors))
    if not torch.cuda.is_available():
        raise SystemExit("bench_bpr.py needs a HIP device")
    eng = SGDEngine(u, i, r, nu, ni, a.factors, "linear", a.dtype, "cuda:0", global_mean=0.0,
                    eval_order=False)
    res = {"device": torch.cuda.get_device_name(0),
           "shape": {"users": nu, "items": ni, "positives": nnz, "n_factors": a.factors,
                     "dtype": a.dtype},
           "legs": [leg(eng, P, Q, c, 0.05, 0.01, a.reps, a.warmup) for c in a.chunks]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
