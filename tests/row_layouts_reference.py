"""The row layouts of ``dispatch_rows`` (csrc/mf_rows.hpp), the ranks that
reach each of them, and the float32 yardstick of the FP32 kernels.

``dispatch_rows`` picks one of 16 layouts (W, GS, V) per dtype; WV = 4 (float)
/ 2 (double) values per 16-B access:

    k > 0, k % WV == 0, k / WV <= 256; kvp = k / WV rounded up to a power of 2
      kvp   1        2        4        8        16        32        64        128       256
      W,GS,V (WV,1,1) (WV,2,1) (WV,4,1) (WV,8,1) (WV,16,1) (WV,16,2) (WV,16,4) (WV,16,8) (WV,16,16)
    every other k (0, k not a multiple of WV, FP64 k > 512); kp = kpad_of(k)
      kp    16       32       64       128      256      512      1024
      W,GS,V (1,16,1) (1,32,1) (1,64,1) (1,64,2) (1,64,4) (1,64,8) (1,64,16)

The tables are pinned to the sources by test_gpu_row_layouts.py
(``test_layout_tables_match_sources``), the NumPy sweep to ``oracle.sgd_pass``
(``test_numpy_sweep_in_fp64_is_the_oracle``).  Shared by
test_gpu_row_layouts.py (k_sgd_batch, the SSE passes, the read kernels) and
test_gpu_strata_layouts.py (the strata sweep in every launch form).
"""

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)

# ---------------------------------------------------------------- layouts
ROWS_WIDE = {1: (1, 1), 2: (2, 1), 4: (4, 1), 8: (8, 1), 16: (16, 1), 32: (16, 2),
             64: (16, 4), 128: (16, 8), 256: (16, 16)}              # kvp -> (GS, V)
ROWS_SCALAR = {16: (16, 1), 32: (32, 1), 64: (64, 1), 128: (64, 2), 256: (64, 4),
               512: (64, 8), 1024: (64, 16)}                        # kpad -> (GS, V)
WV = {"float32": 4, "float64": 2}


def kpad_of(k):
    kp = 16
    while kp < k:
        kp <<= 1
    return kp


def rows_layout(dtype, k):
    """(W, GS, V) of dispatch_rows."""
    wv = WV[dtype]
    if k > 0 and k % wv == 0 and k // wv <= 256:
        kvp = 1
        while kvp < k // wv:
            kvp <<= 1
        return (wv,) + ROWS_WIDE[kvp]
    return (1,) + ROWS_SCALAR[kpad_of(k)]


def all_rows_layouts(dtype):
    return ({(WV[dtype],) + v for v in ROWS_WIDE.values()} |
            {(1,) + v for v in ROWS_SCALAR.values()})


W1_RANKS = [1, 3, 17, 33, 101, 129, 257, 513, 1023]
# the full-width rank of every W > 1 layout, then a tail rank of each one that
# can have a tail (kvp >= 4), then the W = 1 ranks (all of them tails but FP64
# 1024); 0 = biases only
SGD_RANKS = {
    "float32": [0, 4, 8, 16, 32, 64, 128, 256, 512, 1024,
                12, 20, 40, 100, 132, 260, 516] + W1_RANKS,
    "float64": [0, 2, 4, 8, 16, 32, 64, 128, 256, 512,
                6, 10, 18, 34, 100, 130, 260] + W1_RANKS + [1024],
}


def layout_representatives(dtype):
    """One rank per layout of dispatch_rows: the last of SGD_RANKS that takes
    it with a tail, else the last that takes it."""
    best = {}
    for k in SGD_RANKS[dtype]:
        w, gs, v = lay = rows_layout(dtype, k)
        tail = 0 < k < w * gs * v
        if lay not in best or tail >= best[lay][0]:
            best[lay] = (tail, k)
    return sorted(k for _, k in best.values())


def maxabs(a):
    return float(np.max(np.abs(a))) if a.size else 0.0


# ------------------------------------------- NumPy restatement (any dtype)
def numpy_sgd_sweep(u, i, r, mu, bu, bi, P, Q, kernel, gamma, lr, reg, lo, hi, order, dtype,
                    update_user=True, update_item=True):
    """One sequential sweep over ``order`` in ``dtype`` arithmetic: the
    reference's per-rating bodies (kernels.py:108-327) in its expression
    order, as csrc/mf_rows.hpp restates them in sgd_error / sgd_bias /
    sgd_rows, every operation rounded on its own (no fused multiply-add),
    ``np.exp`` of ``dtype``.  Returns new (P, Q, b_u, b_i) as float64."""
    T = np.dtype(dtype).type
    P, Q, bu, bi = (np.array(a, dtype=T) for a in (P, Q, bu, bi))
    r = np.asarray(r, T)
    mu, gamma, lr, reg = T(mu), T(gamma), T(lr), T(reg)
    a, c = T(lo), T(hi - lo)
    one, two = T(1), T(2)
    for j in order:
        x, y = u[j], i[j]
        p, q = P[x].copy(), Q[y].copy()
        if kernel == "rbf":
            df = p - q
            E = np.exp((-gamma) * np.sum(df * df, dtype=T))
            e = (a + c * E) - r[j]
            d = (two * E) * gamma
            if update_user:
                P[x] = p - lr * (e * (d * (q - p)) + reg * p)
            if update_item:
                Q[y] = q - lr * (e * (d * (p - q)) + reg * q)
            continue
        ub, ib = bu[x], bi[y]
        dot = np.sum(p * q, dtype=T)
        if kernel == "linear":
            e = (((mu + ib) + ub) + dot) - r[j]
            if update_user:
                bu[x] = ub - lr * (e + reg * ub)
                P[x] = p - lr * (e * q + reg * p)
            if update_item:
                bi[y] = ib - lr * (e + reg * ib)
                Q[y] = q - lr * (e * p + reg * q)
        else:
            lin = ((mu + ub) + ib) + dot
            ex = np.exp(-lin)
            sg = one / (one + ex)
            e = (a + c * sg) - r[j]
            d = (sg * sg) * ex
            if update_user:
                bu[x] = ub - lr * (e * d + reg * ub)
                P[x] = p - lr * (e * (q * d) + reg * p)
            if update_item:
                bi[y] = ib - lr * (e * d + reg * ib)
                Q[y] = q - lr * (e * (p * d) + reg * q)
    return tuple(np.asarray(a, np.float64) for a in (P, Q, bu, bi))


# ------------------------------------------------------- the FP32 bound
def assert_fp32_close(tag, got, n32, ref, m, figure=None):
    """max|gpu - ref| <= m d32 + 4 eps32 max|ref| per array of (P, Q, b_u,
    b_i), d32 = max|n32 - ref| (the float32 NumPy sweep's deviation from the
    FP64 oracle ``ref``), and m d32 <= 1e-4 max|ref| (the bound is not
    vacuous).  ``figure``: called with one line of figures per array, before
    anything is asserted.  Returns the per-array (d32, max|gpu - ref|, max|ref|)."""
    bad, out = [], []
    for name, g, n, rf in zip(("P", "Q", "bu", "bi"), got, n32, ref):
        assert g.shape == rf.shape
        d32, dev, scale = maxabs(n - rf), maxabs(g - rf), maxabs(rf)
        ratio = dev / d32 if d32 > 0 else (0.0 if dev == 0 else float("inf"))
        if figure is not None:
            figure(f"ROWLAYOUT {tag} {name} d32={d32:.3e} gpu={dev:.3e} ratio={ratio:.3f} "
                   f"scale={scale:.3e}")
        out.append((d32, dev, scale))
        assert m * d32 <= 1e-4 * scale, f"{name}: vacuous bound, d32 = {d32:.3e}"
        if not dev <= m * d32 + 4 * EPS32 * scale:
            bad.append(f"{name}: max |diff| {dev:.3e} > {m} * {d32:.3e} + 4 eps32 * {scale:.3g}")
    assert not bad, "; ".join(bad)
    return out
