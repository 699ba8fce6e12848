#!/usr/bin/env python
"""Device-event timing of the implicit-ALS kernels (mf_gramian, mf_ials_sweep,
mf_ials_sweep_cg at --cg-steps steps) beside the explicit factor ALS
(mf_als_sweep) on the same CSR lists, in one process, alternating; the explicit
sweep also on its 4-wave kernel (MF_ALS_KERNEL=block: k_als_solve, the layout
k_ials_solve shares).  The CG rows warm-start from buffers of their own, so the
other rows see the inputs they saw before those rows existed.

    python tools/bench_ials.py --out profiles/ials/bench_ials_cg.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_ials.py --reps 3

Default shape is BASELINE config 5's: 1M users x 100K items, 100M pairs
(uniform random, drawn on the device), ranks 128 and 64.  TFLOP/s counts
2 nnz k^2 per half-sweep (the full Gramian a dense formulation would form; the
kernels compute the upper tiles only).
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


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def csr(ent, oth, r, m):
    order = torch.sort(ent, stable=True)[1]
    ptr = torch.zeros(m + 1, dtype=torch.int64, device=ent.device)
    ptr[1:] = torch.cumsum(torch.bincount(ent, minlength=m), 0)
    return ptr, oth[order].to(torch.int32).contiguous(), r[order].contiguous()


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]),
            "reps": len(a)}


def run(k, nu, ni, nnz, reps, warmup, alpha, reg, dev, cg_steps=3):
    g = torch.Generator(device=dev)
    g.manual_seed(1234 + k)
    u = torch.randint(0, nu, (nnz,), device=dev, generator=g)
    i = torch.randint(0, ni, (nnz,), device=dev, generator=g)
    r = torch.randint(0, 6, (nnz,), device=dev, generator=g).to(torch.float32)
    ucsr = csr(u, i, r, nu)
    icsr = csr(i, u, r, ni)
    del u, i, r
    mk = lambda n: (torch.randn((n, k), device=dev, generator=g) * 0.1).contiguous()  # noqa: E731
    P, Q, P2, Q2 = mk(nu), mk(ni), mk(nu), mk(ni)
    P3, Q3 = mk(nu), mk(ni)                     # the CG rows' warm starts / results
    bu, bi = torch.zeros(nu, device=dev), torch.zeros(ni, device=dev)
    lib = _lib.load()
    ws = torch.empty(max(lib.mf_gramian_workspace_bytes(nu, k), 4) // 4, device=dev)
    G = torch.empty((k, k), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def gram_items():
        _lib.call("mf_gramian", vp(Q), ni, k, 0, vp(ws), vp(G), st)

    def gram_users():
        _lib.call("mf_gramian", vp(P), nu, k, 0, vp(ws), vp(G), st)

    def ials_users():        # G = Q^T Q from the gram_items() just before
        _lib.call("mf_ials_sweep", vp(ucsr[0]), vp(ucsr[1]), vp(ucsr[2]), nu, vp(Q), vp(G),
                  vp(P), k, 0, alpha, reg, st)

    def ials_items():        # G = P^T P from the gram_users() just before
        _lib.call("mf_ials_sweep", vp(icsr[0]), vp(icsr[1]), vp(icsr[2]), ni, vp(P), vp(G),
                  vp(Q), k, 0, alpha, reg, st)

    def cg_users():          # same G and fixed side as ials_users, rows in P3
        _lib.call("mf_ials_sweep_cg", vp(ucsr[0]), vp(ucsr[1]), vp(ucsr[2]), nu, vp(Q), vp(G),
                  vp(P3), k, 0, alpha, reg, cg_steps, st)

    def cg_items():          # same G and fixed side as ials_items, rows in Q3
        _lib.call("mf_ials_sweep_cg", vp(icsr[0]), vp(icsr[1]), vp(icsr[2]), ni, vp(P), vp(G),
                  vp(Q3), k, 0, alpha, reg, cg_steps, st)

    def als_users():
        _lib.call("mf_als_sweep", vp(ucsr[0]), vp(ucsr[1]), vp(ucsr[2]), nu, 2.5, vp(bi),
                  vp(Q2), vp(bu), vp(P2), k, 0, reg, st)

    def als_items():
        _lib.call("mf_als_sweep", vp(icsr[0]), vp(icsr[1]), vp(icsr[2]), ni, 2.5, vp(bu),
                  vp(P2), vp(bi), vp(Q2), k, 0, reg, st)

    def block(fn):           # the explicit sweep on k_als_solve, k_ials_solve's layout
        def go():
            os.environ["MF_ALS_KERNEL"] = "block"
            try:
                fn()
            finally:
                del os.environ["MF_ALS_KERNEL"]
        return go

    steps = [("gramian_items", gram_items), ("ials_users", ials_users),
             ("ials_cg_users", cg_users),
             ("gramian_users", gram_users), ("ials_items", ials_items),
             ("ials_cg_items", cg_items),
             ("als_users", als_users), ("als_items", als_items),
             ("als_block_users", block(als_users)), ("als_block_items", block(als_items))]
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
    if not all(bool(torch.isfinite(t).all()) for t in (P, Q, P3, Q3)):
        raise RuntimeError("non-finite factors after the timed sweeps")
    out = {name: stats(v) for name, v in ms.items()}
    flop = 2.0 * nnz * k * k
    for name in ("ials_users", "ials_items", "ials_cg_users", "ials_cg_items", "als_users",
                 "als_items", "als_block_users", "als_block_items"):
        out[name]["tflops"] = flop / (out[name]["median_ms"] * 1e-3) / 1e12
    imp = sum(out[n]["median_ms"] for n in ("gramian_items", "ials_users", "gramian_users",
                                            "ials_items"))
    exp = out["als_users"]["median_ms"] + out["als_items"]["median_ms"]
    out["implicit_epoch_ms"] = imp
    out["explicit_epoch_ms"] = exp
    out["implicit_over_explicit"] = imp / exp
    cg = sum(out[n]["median_ms"] for n in ("gramian_items", "ials_cg_users", "gramian_users",
                                           "ials_cg_items"))
    out["cg_steps"] = cg_steps
    out["implicit_cg_epoch_ms"] = cg
    out["implicit_cg_over_explicit"] = cg / exp
    out["implicit_cg_over_direct"] = cg / imp
    out["explicit_block_epoch_ms"] = (out["als_block_users"]["median_ms"]
                                      + out["als_block_items"]["median_ms"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--ranks", type=int, nargs="+", default=[128, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alpha", type=float, default=40.0)
    ap.add_argument("--reg", type=float, default=0.1)
    ap.add_argument("--cg-steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ials.py needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"shape": {"users": a.users, "items": a.items, "pairs": a.pairs},
           "alpha": a.alpha, "reg": a.reg, "device": torch.cuda.get_device_name(0), "ranks": {}}
    for k in a.ranks:
        res["ranks"][str(k)] = run(k, a.users, a.items, a.pairs, a.reps, a.warmup, a.alpha,
                                   a.reg, dev, a.cg_steps)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
