#!/usr/bin/env python
"""Probe: C3 FP64 sweep alone, RMSE pass alone (full / capped grid), and the
capped pass released beside a resident sweep ("beside
mode").  Usage: python tools/sse_beside_probe.py [--out FILE] [--reps N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "matrix-factorization_amd"))

import torch  # noqa: E402

import bench  # noqa: E402
from matrix_factorization.engine import SGDEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="sse_beside_probe.json")
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--workload", default="c3", choices=sorted(bench.WORKLOADS))
ARGS = ap.parse_args()
WL, REPS = ARGS.workload, ARGS.reps


def log(m):
    print(f"[probe {time.strftime('%H:%M:%S')}] {m}", flush=True)


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    nu, ni, nnz, k, kernel, _ = bench.WORKLOADS[WL]
    u, i, r = bench.synth(nu, ni, nnz)
    mu = float(np.mean(r, dtype=np.float64))
    rs = np.random.RandomState(7)
    P0 = rs.normal(0.0, 0.1, (nu, k)).astype(np.float32).astype(np.float64)
    Q0 = rs.normal(0.0, 0.1, (ni, k)).astype(np.float32).astype(np.float64)
    log("data ready")
    eng = SGDEngine(u, i, r, nu, ni, k, kernel, "float64", dev, gamma=1.0 / k,
                    min_rating=1.0, max_rating=5.0, global_mean=mu)
    plan = eng.prepare_strata()
    eng.load_params(P=P0, Q=Q0, bu=np.zeros(nu), bi=np.zeros(ni))
    eng._ensure_sse_slots(256)
    cus = eng._cus()
    log(f"engine ready: B={plan.B} classes={plan.classes} cus={cus}")
    main_s = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(dev)
    snap = [torch.empty_like(t) for t in (eng.P, eng.Q, eng.bu, eng.bi)]
    ws2 = torch.empty_like(eng.ws)
    ep = [0]

    def sweep():
        e = ep[0]
        ep[0] += 1
        eng.epoch_strata(bench.strata_seq(e, plan), bench.strata_rot(e), 0.01, 0.02)

    def E():
        return torch.cuda.Event(enable_timing=True)

    def take_snapshot():
        for d, s in zip(snap, (eng.P, eng.Q, eng.bu, eng.bi)):
            d.copy_(s)

    for _ in range(4):
        sweep()
        eng.sse_async(0)
    torch.cuda.synchronize()
    if eng.strata_failed():
        raise SystemExit("sweep failed in warm-up")
    res = {"workload": WL, "cus": cus, "reps": REPS}

    def stats(x):
        x = sorted(x)
        return {"min": x[0], "median": x[len(x) // 2], "max": x[-1], "all": x}

    # sweep alone
    t = []
    for _ in range(REPS):
        a, b = E(), E()
        a.record()
        sweep()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    res["sweep_alone_ms"] = stats(t)
    log(f"sweep alone {res['sweep_alone_ms']}")

    # snapshot alone
    t = []
    for _ in range(REPS):
        a, b = E(), E()
        a.record()
        take_snapshot()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    res["snapshot_ms"] = stats(t)
    log(f"snapshot {res['snapshot_ms']}")

    out = {}
    # pass alone: full grid, live parameters
    t = []
    for _ in range(REPS):
        a, b = E(), E()
        a.record()
        eng.sse_async(1)
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    out["pass_full_ms"] = stats(t)
    # pass alone: capped grid, snapshot
    take_snapshot()
    for cap in (cus, 2 * cus):
        t = []
        for _ in range(REPS):
            a, b = E(), E()
            a.record()
            eng.sse_from(2, *snap, ws2, main_s, max_blocks=cap)
            b.record()
            torch.cuda.synchronize()
            t.append(a.elapsed_time(b))
        out[f"pass_capped{cap}_ms"] = stats(t)
    torch.cuda.synchronize()
    v_full, v_cap = eng.sse_buf[1].item(), eng.sse_buf[2].item()
    # together: snapshot, sweep enqueued, host waits, capped pass on the side stream
    for wait_ms in (2.0, 0.0):
        tot, swp, pas, snp = [], [], [], []
        for _ in range(REPS):
            torch.cuda.synchronize()
            e0, e1, e2, e3, s0, s1 = E(), E(), E(), E(), E(), E()
            e0.record()
            take_snapshot()
            e1.record()
            side.wait_event(e1)
            sweep()
            e2.record()
            if wait_ms:
                t0 = time.perf_counter()
                while (time.perf_counter() - t0) * 1e3 < wait_ms:
                    pass
            s0.record(side)
            eng.sse_from(3, *snap, ws2, side, max_blocks=cus)
            s1.record(side)
            main_s.wait_event(s1)
            e3.record()
            torch.cuda.synchronize()
            tot.append(e0.elapsed_time(e3))
            snp.append(e0.elapsed_time(e1))
            swp.append(e1.elapsed_time(e2))
            pas.append(s0.elapsed_time(s1))
        out[f"together_wait{wait_ms:g}ms"] = {
            "total_ms": stats(tot), "snapshot_ms": stats(snp), "sweep_ms": stats(swp),
            "pass_ms": stats(pas)}
    out["sse_full"] = v_full
    out["sse_capped"] = v_cap
    res["pass"] = out
    log(f"pass: {json.dumps(out)}")
    if eng.strata_failed():
        raise SystemExit("a sweep gave up waiting")
    with open(ARGS.out, "w") as f:
        json.dump(res, f, indent=1)
    log("done")


if __name__ == "__main__":
    main()
