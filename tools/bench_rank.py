#!/usr/bin/env python
"""Device-event timing of exact ranking (mf_rank) beside the exact top-k
(mf_topk, amount 10) on the same inputs, in one process, alternating.

    python tools/bench_rank.py --out profiles/rank/bench_rank.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_rank.py --reps 3

Default shape is the top-k bench shape: 10K query users x 100K items at rank
64, float32, linear kernel, ~100 excluded items per user; mf_rank with one
target per user and with 20.  Gscores/s counts n_query x n_items scores per
call.  Before timing, the items mf_topk returns are ranked by mf_rank and
must come back at their positions.
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "matrix-factorization_amd"))

from matrix_factorization import _lib  # noqa: E402

MF_F32, MF_LINEAR = 0, 0


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]),
            "spread": float((a[-1] - a[0]) / np.median(a)), "reps": len(a)}


def run(nq, nu, ni, k, n_ex, targets, amount, reps, warmup, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    mk = lambda n: (torch.randn((n, k), device=dev, generator=g) * 0.1).contiguous()  # noqa: E731
    P, Q = mk(nu), mk(ni)
    bu = torch.randn(nu, device=dev, generator=g) * 0.1
    bi = torch.randn(ni, device=dev, generator=g) * 0.1
    users = torch.randperm(nu, device=dev, generator=g)[:nq].to(torch.int32).contiguous()
    ex_items = torch.sort(torch.randint(0, ni, (nq, n_ex), device=dev, generator=g), dim=1)[0]
    ex_items = ex_items.to(torch.int32).contiguous()
    ex_ptr = torch.arange(nq + 1, device=dev, dtype=torch.int64) * n_ex
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    model = (3.5, vp(bu), vp(bi), vp(P), vp(Q), ni, k, MF_LINEAR, MF_F32, 0.0, 1.0, 5.0)

    def rank_leg(t):
        items = torch.randint(0, ni, (nq, t), device=dev, generator=g).to(torch.int32).contiguous()
        ptr = torch.arange(nq + 1, device=dev, dtype=torch.int64) * t
        ws = torch.empty(max(lib.mf_rank_workspace_bytes(nq, nq * t, ni), 16),
                         dtype=torch.uint8, device=dev)
        out = torch.empty(nq * t, dtype=torch.int32, device=dev)
        cand = torch.empty(nq, dtype=torch.int32, device=dev)

        def go():
            _lib.call("mf_rank", vp(users), nq, *model, vp(ex_ptr), vp(ex_items), vp(ptr),
                      vp(items), vp(ws), vp(out), vp(cand), st)
        go.keep = (items, ptr, ws, out, cand)
        return go

    tk_ws = torch.empty(max(lib.mf_topk_workspace_bytes(nq, ni, amount), 8), dtype=torch.uint8,
                        device=dev)
    tk_items = torch.empty((nq, amount), dtype=torch.int32, device=dev)
    tk_scores = torch.empty((nq, amount), dtype=torch.float32, device=dev)

    def topk():
        _lib.call("mf_topk", vp(users), nq, *model, vp(ex_ptr), vp(ex_items), amount, vp(tk_ws),
                  vp(tk_items), vp(tk_scores), st)

    # the two must agree: the item at position p of a top-k list has rank p
    topk()
    ptr = torch.arange(nq + 1, device=dev, dtype=torch.int64) * amount
    ws = torch.empty(lib.mf_rank_workspace_bytes(nq, nq * amount, ni), dtype=torch.uint8,
                     device=dev)
    got = torch.empty(nq * amount, dtype=torch.int32, device=dev)
    cand = torch.empty(nq, dtype=torch.int32, device=dev)
    _lib.call("mf_rank", vp(users), nq, *model, vp(ex_ptr), vp(ex_items), vp(ptr), vp(tk_items),
              vp(ws), vp(got), vp(cand), st)
    want = torch.arange(amount, device=dev, dtype=torch.int32).repeat(nq)
    if not bool((got == want).all()):
        raise RuntimeError("mf_rank disagrees with mf_topk's order")
    if int(cand.max()) > ni or int(cand.min()) < ni - n_ex:
        raise RuntimeError("mf_rank: candidate counts out of range")

    steps = [(f"rank_t{t}", rank_leg(t)) for t in targets] + [(f"topk_exact_a{amount}", topk)]
    for _ in range(warmup):
        for _, fn in steps:
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in steps}
    for _ in range(reps):                       # alternating: one of each per round
        evs = []
        for name, fn in steps:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs.append((name, a, b))
        torch.cuda.synchronize()
        for name, a, b in evs:
            ms[name].append(a.elapsed_time(b))
    out = {name: stats(v) for name, v in ms.items()}
    for name in out:
        out[name]["gscores_per_s"] = nq * ni / (out[name]["median_ms"] * 1e-3) / 1e9
    tk = out[f"topk_exact_a{amount}"]["median_ms"]
    for t in targets:
        out[f"rank_t{t}_over_topk"] = out[f"rank_t{t}"]["median_ms"] / tk
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--query", type=int, default=10_000)
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--exclusions", type=int, default=100)
    ap.add_argument("--targets", type=int, nargs="+", default=[1, 20])
    ap.add_argument("--amount", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank.py needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"shape": {"query_users": a.query, "users": a.users, "items": a.items, "rank": a.rank,
                     "exclusions_per_user": a.exclusions, "dtype": "float32", "kernel": "linear"},
           "device": torch.cuda.get_device_name(0)}
    res.update(run(a.query, a.users, a.items, a.rank, a.exclusions, a.targets, a.amount, a.reps,
                   a.warmup, dev))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
