#!/usr/bin/env python
"""Device-event timing of the hybrid recommendation path, leg by leg, in one
process, alternating: the query users' profiles (mf_content_profiles +
mf_content_normalize), the retrieval (mf_topk, amount = candidate_k), the fused
second stage (mf_hybrid_rerank), and beside it the composition a user could
already write from existing parts -- mf_predict on the flattened (user,
candidate) pairs plus torch masking, min / max, blend and sort.

    python tools/bench_hybrid.py --out profiles/hybrid/bench_hybrid.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_hybrid.py --reps 3

Default shape: 100K users x 10K items, d = 384 float32 unit-norm embeddings, a
rank-64 float32 linear model, 50 history items per user, 1024 query users,
candidate_k 200 and 1000, amount 10.  Before timing, the composition's ids must
equal mf_hybrid_rerank's.
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

MF_F32, MF_F64, MF_LINEAR = 0, 1, 0


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]),
            "spread": float((a[-1] - a[0]) / np.median(a)), "reps": len(a)}


def run(nq, nu, ni, d, k, n_hist, cks, amount, alpha, reps, warmup, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    E = torch.randn((ni, d), device=dev, generator=g)
    E = (E / E.norm(dim=1, keepdim=True)).contiguous()
    E64 = E.double().contiguous()
    has = torch.ones(ni, dtype=torch.uint8, device=dev)
    P = (torch.randn((nu, k), device=dev, generator=g) * 0.1).contiguous()
    Q = (torch.randn((ni, k), device=dev, generator=g) * 0.1).contiguous()
    bu = torch.randn(nu, device=dev, generator=g) * 0.1
    bi = torch.randn(ni, device=dev, generator=g) * 0.1
    users = torch.randperm(nu, device=dev, generator=g)[:nq].to(torch.int32).contiguous()
    hist = torch.sort(torch.randint(0, ni, (nq, n_hist), device=dev, generator=g), dim=1)[0]
    hist = hist.to(torch.int32).contiguous()
    h_ptr = torch.arange(nq + 1, device=dev, dtype=torch.int64) * n_hist
    ones = torch.ones(nq * n_hist, dtype=torch.float64, device=dev)
    model = (3.5, vp(bu), vp(bi), vp(P), vp(Q), ni, k, MF_LINEAR, MF_F32, 0.0, 1.0, 5.0)

    prof64 = torch.empty((nq, d), dtype=torch.float64, device=dev)
    prof = torch.empty((nq, d), dtype=torch.float32, device=dev)
    qid = torch.arange(nq, device=dev, dtype=torch.int32)
    zq, zi = torch.zeros(nq, device=dev), torch.zeros(ni, device=dev)

    def profiles():
        _lib.call("mf_content_profiles", vp(h_ptr), vp(hist), vp(ones), vp(E64), vp(has), nq, ni, d,
                  MF_F64, vp(prof64), st)
        _lib.call("mf_content_normalize", vp(prof64), nq, d, 0, MF_F64, vp(prof), st)

    profiles()
    ex_keys = torch.arange(nq, device=dev, dtype=torch.int64)[:, None] * ni + hist.long()
    ex_keys = ex_keys.flatten()
    a32 = torch.tensor(alpha, dtype=torch.float32, device=dev)
    b32 = torch.tensor(1.0 - alpha, dtype=torch.float32, device=dev)
    out = {}
    for ck in cks:
        ws = torch.empty(max(lib.mf_topk_workspace_bytes(nq, ni, ck), 8), dtype=torch.uint8,
                         device=dev)
        rows = torch.empty((nq, ck), dtype=torch.int32, device=dev)
        sims = torch.empty((nq, ck), dtype=torch.float32, device=dev)

        def retrieve():
            _lib.call("mf_topk", vp(qid), nq, 0.0, vp(zq), vp(zi), vp(prof), vp(E), ni, d,
                      MF_LINEAR, MF_F32, 0.0, 0.0, 1.0, None, None, ck, vp(ws), vp(rows),
                      vp(sims), st)

        o_rows = torch.empty((nq, amount), dtype=torch.int32, device=dev)
        o_sc = torch.empty((nq, amount), dtype=torch.float32, device=dev)
        o_m = torch.empty(nq, dtype=torch.int32, device=dev)

        def rerank():
            _lib.call("mf_hybrid_rerank", vp(users), nq, vp(rows), vp(sims), ck, None, ni, *model,
                      vp(h_ptr), vp(hist), alpha, amount, None, vp(o_rows), vp(o_sc), None, None,
                      vp(o_m), st)

        pu = users.repeat_interleave(ck).contiguous()
        pred = torch.empty(nq * ck, dtype=torch.float32, device=dev)
        qbase = torch.arange(nq, device=dev, dtype=torch.int64)[:, None] * ni
        inf = torch.tensor(float("inf"), device=dev)
        comp = {}

        def minmax(x, keep):
            lo = torch.where(keep, x, inf).amin(dim=1, keepdim=True)
            hi = torch.where(keep, x, -inf).amax(dim=1, keepdim=True)
            dd = hi.double() - lo.double()
            return torch.where(dd < 1e-8, torch.zeros_like(x), (x - lo) / dd.float())

        def composition():
            _lib.call("mf_predict", vp(pu), vp(rows), nq * ck, *model[:5], *model[6:], 0,
                      vp(pred), st)                          # the model without n_items
            keys = qbase + rows.long()
            at = torch.searchsorted(ex_keys, keys.flatten()).clamp(max=len(ex_keys) - 1)
            keep = (ex_keys[at].view(nq, ck) != keys) & (rows >= 0)
            score = a32 * minmax(pred.view(nq, ck), keep) + b32 * minmax(sims, keep)
            score = torch.where(keep, score, -inf)
            order = torch.sort(score, dim=1, descending=True, stable=True).indices[:, :amount]
            ids = torch.gather(rows, 1, order)
            comp["ids"] = torch.where(torch.gather(keep, 1, order), ids, torch.full_like(ids, -1))

        retrieve()
        rerank()
        composition()
        torch.cuda.synchronize()
        same = bool((comp["ids"] == o_rows).all())
        if not same:
            frac = float((comp["ids"] == o_rows).float().mean())
            raise RuntimeError(f"candidate_k={ck}: the composition's ids differ from "
                               f"mf_hybrid_rerank's ({frac:.6f} equal)")
        steps = [("profiles", profiles), ("retrieve_topk", retrieve), ("rerank_fused", rerank),
                 ("rerank_composition", composition)]
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
        res = {name: stats(v) for name, v in ms.items()}
        call = sum(res[n]["median_ms"] for n in ("profiles", "retrieve_topk", "rerank_fused"))
        res["call_ms"] = call
        res["share_of_call"] = {n: res[n]["median_ms"] / call
                                for n in ("profiles", "retrieve_topk", "rerank_fused")}
        res["composition_over_fused"] = (res["rerank_composition"]["median_ms"]
                                         / res["rerank_fused"]["median_ms"])
        res["ids_equal"] = same
        res["kept_mean"] = float(o_m.float().mean())
        out[f"candidate_k_{ck}"] = res
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--query", type=int, default=1024)
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--items", type=int, default=10_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--history", type=int, default=50)
    ap.add_argument("--candidate-k", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--amount", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hybrid.py needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"shape": {"query_users": a.query, "users": a.users, "items": a.items, "dim": a.dim,
                     "rank": a.rank, "history_per_user": a.history, "amount": a.amount,
                     "alpha": a.alpha, "dtype": "float32", "kernel": "linear"},
           "device": torch.cuda.get_device_name(0)}
    res.update(run(a.query, a.users, a.items, a.dim, a.rank, a.history, a.candidate_k, a.amount,
                   a.alpha, a.reps, a.warmup, dev))
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
