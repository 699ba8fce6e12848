"""Every row layout of the KernelMF hot kernels, one kernel family at a time.

``dispatch_rows`` (csrc/mf_rows.hpp) picks one of 16 layouts (W, GS, V) per
dtype for k_sgd_batch / k_sse_lean / k_sse_stream, ``dispatch``
(csrc/mf_dispatch.hpp) one of 7 layouts (GS, V) per dtype for the predict,
top-k and rank kernels.  The tables, restated below and checked against the
two sources by ``test_layout_tables_match_sources``:

  dispatch_rows, WV = 4 (float) / 2 (double) values per 16-B access
    k > 0, k % WV == 0, k / WV <= 256; kvp = k / WV rounded up to a power of 2
      kvp   1        2        4        8        16        32        64        128       256
      W,GS,V (WV,1,1) (WV,2,1) (WV,4,1) (WV,8,1) (WV,16,1) (WV,16,2) (WV,16,4) (WV,16,8) (WV,16,16)
    every other k (0, k not a multiple of WV, FP64 k > 512); kp = kpad_of(k)
      kp    16       32       64       128      256      512      1024
      W,GS,V (1,16,1) (1,32,1) (1,64,1) (1,64,2) (1,64,4) (1,64,8) (1,64,16)
  dispatch (both dtypes); kp = kpad_of(k)
      kp    16     32     64     128    256    512    1024
      GS,V  (16,1) (32,1) (64,1) (64,2) (64,4) (64,8) (64,16)

One rank per layout at its full width, a second one where the layout can
have a tail (k < GS V W; (WV,1,1) and (WV,2,1) cannot).  Rank 100 is a
multiple of 4 and of 2, so it is a tail rank of (4,16,2) / (2,16,4), not of
the W = 1 branch; 101 covers (1,64,2).

The engine level on purpose: ``SGDEngine`` directly, a few thousand ratings,
so a failure names one layout of one kernel.  The strata sweep in every
layout and launch form, and the strata planner with its LDS budgets at wide
ranks, are covered the same way by tests/test_gpu_strata_layouts.py; the
layout tables, the NumPy float32 sweep and the FP32 bound used by both files
live in tests/row_layouts_reference.py.  Follow-up, not covered by either:
``KernelMF.fit()`` itself at ranks > 128.

FP32 bounds (checks 2 to 4).  The FP32 kernels are compared value by value
with the FP64 oracle run on the FP32-rounded inputs.  The tolerance is a
measured unit, not a constant: ``d32`` is the deviation from the same oracle
of a plain NumPy float32 evaluation of the same operation (unfused, ``np.exp``
in float32, the reference's expression order), per array.  The GPU must stay
within ``M * d32 + 4 * eps32 * max|ref|``.  M was chosen once, by this rule:
the smallest power of two that is at least twice the largest GPU / d32 ratio
of the linear SGD cases (there only the FMA contraction and the order of the
dot product's sum differ from NumPy).  That ratio is 1.43, so M = 4.

Observed on an MI355X (78 SGD cases, 4 arrays each; 84 predict runs); ratio =
max|gpu - ref| / d32, the largest over all ranks and arrays:

  kernel    SGD ratio (median)   d32 of P, Q        predict ratio   d32 of predict
  linear    1.43 (1.00)          3.2e-8 .. 1.9e-7   1.09            <= 4.3e-7
  sigmoid   1.63 (1.00)          3.4e-8 .. 2.3e-7   1.00            <= 5.9e-7
  rbf       1.18 (1.00)          3.3e-8 .. 2.0e-7   0.65            <= 7.0e-7

d32 / max|ref| is at most 8.1e-7 in the SGD cases, so M * d32 stays below
3.3e-6 of the parameter scale (asserted below 1e-4 in every case: the bound
is never vacuous).  A median of 1.00 says what dominates both deviations: the
rounding of each stored value to float32, not the arithmetic in between.

For the training RMSE the unit is the deviation of one aggregate number, in
which the per-rating roundings cancel (d32 between 0 and 1.4e-8 by chance),
so a ratio means nothing there and the 4 eps32 RMSE term (about 7e-7) carries
the bound; the GPU's RMSE was within 4.8e-9 (linear), 1.2e-8 (sigmoid) and
2.0e-8 (rbf) of the oracle's, k_sse_lean and k_sse_stream alike.  The two
passes agree with each other to 1e-12 in FP64 and, in FP32, wherever W = 1 or
V = 1 (the same bits per rating); in the FP32 layouts (4,16,2) .. (4,16,16)
they associate a lane's part of the dot product differently and their RMSEs
differ by 6e-11 .. 8e-10.
"""

import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from row_layouts_reference import (EPS32, ROWS_SCALAR, ROWS_WIDE, SGD_RANKS, WV,  # noqa: F401
                                   W1_RANKS, all_rows_layouts, assert_fp32_close, kpad_of,
                                   layout_representatives, numpy_sgd_sweep, rows_layout)
from row_layouts_reference import maxabs as _maxabs

gpu = pytest.mark.gpu

KERNELS = ("linear", "sigmoid", "rbf")
LR, REG, LO, HI = 0.01, 0.02, 1.0, 5.0
M = 4          # see the module docstring

# ---------------------------------------------------------------- layouts
READ_TABLE = dict(ROWS_SCALAR)                                      # dispatch: kpad -> (GS, V)


def read_layout(k):
    """(GS, V) of dispatch."""
    return READ_TABLE[kpad_of(k)]


# every read layout at its full width and at a tail rank
READ_RANKS = [12, 16, 20, 32, 40, 64, 100, 128, 200, 256, 300, 512, 1000, 1024]
# one tail rank per W: the frozen-side runs
FROZEN_RANKS = {"float32": [132, 1023], "float64": [260, 1023]}
MM_RANKS = [12, 16, 20, 32, 40, 64]        # mf_topk_mm_supported: FP32, linear, these of READ_RANKS


# ------------------------------------------------------------------ data
def _shape(k):
    return (120, 60, 2500) if k > 128 else (300, 120, 6000)


@functools.lru_cache(maxsize=None)
def _ratings(wide):
    """Ratings 1..5 in colour-major order (what prepare_colored stores), the
    colour offsets, one permutation of the colours and the visit order it
    serialises to.  Shared by every case of a shape; never modified."""
    from matrix_factorization.engine import sched_color

    nu, ni, nnz = _shape(1024 if wide else 1)
    rs = np.random.RandomState(11 if wide else 3)
    keys = rs.choice(nu * ni, nnz, replace=False)
    u0 = (keys // ni).astype(np.int32)
    i0 = (keys % ni).astype(np.int32)
    r0 = rs.randint(1, 6, nnz).astype(np.float64)
    sched, offs = sched_color(u0, i0, nu, ni)
    nb = len(offs) - 1
    seq = rs.permutation(nb).astype(np.int32)
    order = np.concatenate([np.arange(offs[b], offs[b + 1]) for b in seq]).astype(np.int64)
    out = dict(nu=nu, ni=ni, u0=u0, i0=i0, r0=r0, u=u0[sched], i=i0[sched], r=r0[sched],
               offs=offs, seq=seq, order=order, mu=float(r0.mean()))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _params(nu, ni, k, dtype, seed):
    """P, Q ~ N(0, 0.1) sqrt(64 / max(k, 64)), biases ~ N(0, 0.05); rounded
    through float32 for the FP32 cases (float64 arrays either way)."""
    rs = np.random.RandomState(seed)
    sc = np.sqrt(64.0 / max(k, 64))
    out = [rs.normal(0, 0.1, (nu, k)) * sc, rs.normal(0, 0.1, (ni, k)) * sc,
           rs.normal(0, 0.05, nu), rs.normal(0, 0.05, ni)]
    if dtype == "float32":
        out = [a.astype(np.float32).astype(np.float64) for a in out]
    return out


def _hyp(k):
    return dict(gamma=1.0 / k if k else 1.0, min_rating=LO, max_rating=HI)


def _figure(line):
    """The measured figures behind the docstring's table: printed only when
    MF_ROW_LAYOUT_FIGURES is set (then run with -s)."""
    if os.environ.get("MF_ROW_LAYOUT_FIGURES"):
        print(line)


# ------------------------------------------- NumPy restatements (any dtype)
def numpy_predict(u, i, mu, bu, bi, P, Q, kernel, gamma, lo, hi, dtype, bound=False):
    """predict_one (kernels.py:21-105) for id pairs in ``dtype`` arithmetic
    (-1: zero row, zero bias); float64 result."""
    T = np.dtype(dtype).type
    u, i = np.asarray(u, np.int64), np.asarray(i, np.int64)
    P, Q, bu, bi = (np.asarray(a, T) for a in (P, Q, bu, bi))
    uk, ik = u >= 0, i >= 0
    p = np.where(uk[:, None], P[np.maximum(u, 0)], T(0))
    q = np.where(ik[:, None], Q[np.maximum(i, 0)], T(0))
    ub = np.where(uk, bu[np.maximum(u, 0)], T(0))
    ib = np.where(ik, bi[np.maximum(i, 0)], T(0))
    mu, gamma, a, c = T(mu), T(gamma), T(lo), T(hi - lo)
    if kernel == "rbf":
        df = p - q
        pred = a + c * np.exp((-gamma) * np.sum(df * df, axis=1, dtype=T))
    else:
        dot = np.sum(p * q, axis=1, dtype=T)
        if kernel == "linear":
            pred = ((mu + ib) + ub) + dot
        else:
            pred = a + c * (T(1) / (T(1) + np.exp(-(((mu + ub) + ib) + dot))))
    assert pred.dtype == T
    if bound:
        pred = np.clip(pred, T(lo), T(hi))
    return pred.astype(np.float64)


def numpy_rmse(u, i, r, mu, bu, bi, P, Q, kernel, gamma, lo, hi, dtype):
    """Training RMSE with the per-rating error in ``dtype`` arithmetic,
    squared and accumulated in float64."""
    T = np.dtype(dtype).type
    pred = numpy_predict(u, i, mu, bu, bi, P, Q, kernel, gamma, lo, hi, dtype).astype(T)
    err = (np.asarray(r, T) - pred).astype(np.float64)
    return float(np.sqrt(np.sum(err * err) / len(err)))


# ------------------------------------------------------------- CPU tests
def test_layout_tables_match_sources():
    """The Python tables above are the case labels of the two C++ tables."""
    csrc = os.path.join(ROOT, "matrix-factorization_amd", "csrc")
    rows = open(os.path.join(csrc, "mf_rows.hpp")).read()
    body = rows[rows.index("int dispatch_rows("):rows.index("#undef MF_K3")]
    assert "k > 0 && k % WV == 0 && k / WV <= 256" in body
    assert "constexpr int WV = 16 / (int)sizeof(T);" in body
    cases = re.findall(r"case (\d+): MF_K3\((WV|\d+), (\d+), (\d+)\)", body)
    wide = {int(c): (int(gs), int(v)) for c, w, gs, v in cases if w == "WV"}
    scalar = {int(c): (int(gs), int(v)) for c, w, gs, v in cases if w == "1"}
    assert len(cases) == len(wide) + len(scalar) == 16
    assert wide == ROWS_WIDE and scalar == ROWS_SCALAR
    disp = open(os.path.join(csrc, "mf_dispatch.hpp")).read()
    read = {int(kp): (int(gs), int(v))
            for kp, gs, v in re.findall(r"MF_KCASE\(T, (\d+), (\d+), (\d+)\)", disp)}
    assert read == READ_TABLE
    common = open(os.path.join(csrc, "mf_common.hpp")).read()
    assert re.search(r"inline int kpad_of\(int k\) \{\s*int kp = 16;\s*while \(kp < k\) kp <<= 1;",
                     common)
    assert "constexpr int kMaxFactors = 1024;" in common


def test_rank_lists_cover_every_layout():
    """Every (W, GS, V) of dispatch_rows and every (GS, V) of dispatch is
    reached for both dtypes, and every layout that can have a tail is also
    reached at a tail rank (k < GS V W)."""
    for dtype in ("float32", "float64"):
        ranks = SGD_RANKS[dtype]
        assert len(set(ranks)) == len(ranks) and 0 in ranks and max(ranks) == 1024
        hit = {rows_layout(dtype, k) for k in ranks}
        want = all_rows_layouts(dtype)
        assert len(want) == 16 and hit == want, sorted(want - hit)
        tails = {rows_layout(dtype, k) for k in ranks
                 if 0 < k < int(np.prod(rows_layout(dtype, k)))}
        # (WV,1,1) and (WV,2,1) are entered at k = WV and 2 WV only: no tail
        can_tail = {lay for lay in want if lay[0] == 1 or lay[1] * lay[2] >= 4}
        assert tails == can_tail, sorted(can_tail - tails)
        full = {rows_layout(dtype, k) for k in ranks
                if k == int(np.prod(rows_layout(dtype, k)))}
        assert full >= {lay for lay in want if lay[0] > 1}
        reps = layout_representatives(dtype)
        assert {rows_layout(dtype, k) for k in reps} == want and len(reps) == 16
        for k in FROZEN_RANKS[dtype]:
            assert k in ranks and 0 < k < int(np.prod(rows_layout(dtype, k)))
        assert {rows_layout(dtype, k)[0] for k in FROZEN_RANKS[dtype]} == {WV[dtype], 1}
    assert rows_layout("float64", 1024) == (1, 64, 16)       # k / WV > 256
    assert rows_layout("float32", 100) == (4, 16, 2) and rows_layout("float64", 100) == (2, 16, 4)
    assert rows_layout("float32", 0) == rows_layout("float64", 0) == (1, 16, 1)
    assert {read_layout(k) for k in READ_RANKS} == set(READ_TABLE.values())
    assert {read_layout(k) for k in READ_RANKS if k < kpad_of(k)} == set(READ_TABLE.values())


def _oracle_epoch(d, start, kernel, k, update_user=True, update_item=True):
    import oracle

    P, Q, bu, bi = (a.copy() for a in start)
    oracle.sgd_pass(d["u"], d["i"], d["r"], d["mu"], bu, bi, P, Q, kernel=kernel, lr=LR,
                    reg=REG, order=d["order"], update_user=update_user,
                    update_item=update_item, **_hyp(k))
    return P, Q, bu, bi


def _numpy_epoch(d, start, kernel, k, dtype, update_user=True, update_item=True):
    P, Q, bu, bi = start
    return numpy_sgd_sweep(d["u"], d["i"], d["r"], d["mu"], bu, bi, P, Q, kernel,
                           _hyp(k)["gamma"], LR, REG, LO, HI, d["order"], dtype,
                           update_user, update_item)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k,uu,ui", [(0, True, True), (6, True, True), (33, True, False),
                                     (260, False, True)])
def test_numpy_sweep_in_fp64_is_the_oracle(kernel, k, uu, ui):
    """The restated sweep is the reference's operation: in float64 it equals
    oracle.sgd_pass (the two differ in the order of the dot product's sum
    only)."""
    d = _ratings(k > 128)
    start = _params(d["nu"], d["ni"], k, "float64", 100 + k)
    ref = _oracle_epoch(d, start, kernel, k, uu, ui)
    got = _numpy_epoch(d, start, kernel, k, "float64", uu, ui)
    for g, rf in zip(got, ref):
        assert g.shape == rf.shape and _maxabs(g - rf) <= 1e-12
    if kernel != "rbf" or k:
        assert any(_maxabs(rf - s) > 1e-4 for rf, s in zip(ref, start))     # it did move


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k", [12, 132, 1023])
def test_float32_unit_is_small_and_not_zero(kernel, k):
    """d32, the unit of the FP32 bounds: the float32 sweep differs from the
    FP64 oracle (it is a float32 computation) by far less than 1e-4 / M of
    the parameters' size (the bound is not vacuous)."""
    d = _ratings(k > 128)
    start = _params(d["nu"], d["ni"], k, "float32", 100 + k)
    ref = _oracle_epoch(d, start, kernel, k)
    n32 = _numpy_epoch(d, start, kernel, k, "float32")
    for name, n, rf in zip("PQ", n32, ref):
        d32 = _maxabs(n - rf)
        assert 0 < d32 and M * d32 < 1e-4 * _maxabs(rf), (name, d32)


# ------------------------------------------------------------- GPU tests
@pytest.fixture(scope="module")
def mf():
    import matrix_factorization

    matrix_factorization._lib.load()
    return matrix_factorization


def _sgd_engine(d, start, kernel, k, dtype):
    from matrix_factorization.engine import SGDEngine

    eng = SGDEngine(d["u0"].copy(), d["i0"].copy(), d["r0"].copy(), d["nu"], d["ni"], k,
                    kernel, dtype, "cuda:0", global_mean=d["mu"], **_hyp(k))
    eng.load_params(*start)
    nb = eng.prepare_colored()
    assert nb == len(d["seq"]) and np.array_equal(eng.colored, d["offs"])
    assert np.array_equal(eng.u_host, d["u"]) and np.array_equal(eng.i_host, d["i"])
    return eng


def _gpu_epoch(d, start, kernel, k, dtype, update_user=True, update_item=True):
    eng = _sgd_engine(d, start, kernel, k, dtype)
    eng.epoch_colored(d["seq"], lr=LR, reg=REG, update_user=update_user,
                      update_item=update_item)
    return eng.params_numpy()


def _assert_fp64_close(got, ref):
    for name, g, rf in zip(("P", "Q", "bu", "bi"), got, ref):
        assert g.shape == rf.shape
        err, scale = _maxabs(g - rf), max(1.0, _maxabs(rf))
        assert err <= 1e-11 * scale, f"{name}: max |diff| {err:.3e} > 1e-11 * {scale:.3g}"


_assert_fp32_close = functools.partial(assert_fp32_close, m=M, figure=_figure)


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k", SGD_RANKS["float64"])
def test_sgd_batch_fp64_equals_oracle(mf, kernel, k):
    """Check 1: one coloured epoch of k_sgd_batch<double> in every layout
    against oracle.sgd_pass in the serialised colour order."""
    d = _ratings(k > 128)
    start = _params(d["nu"], d["ni"], k, "float64", 100 + k)
    got = _gpu_epoch(d, start, kernel, k, "float64")
    _assert_fp64_close(got, _oracle_epoch(d, start, kernel, k))


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k", SGD_RANKS["float32"])
def test_sgd_batch_fp32_value_by_value(mf, kernel, k):
    """Check 2: k_sgd_batch<float> (fast_exp, v_rcp_f32, fused multiply-adds)
    in every layout, value by value against the FP64 oracle on the
    FP32-rounded start, within M float32-NumPy units."""
    d = _ratings(k > 128)
    start = _params(d["nu"], d["ni"], k, "float32", 100 + k)
    ref = _oracle_epoch(d, start, kernel, k)
    n32 = _numpy_epoch(d, start, kernel, k, "float32")
    got = _gpu_epoch(d, start, kernel, k, "float32")
    _assert_fp32_close(f"sgd32 {kernel} k={k}", got, n32, ref)


@gpu
@pytest.mark.parametrize("side", ["user", "item"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype,k", [(t, k) for t in ("float64", "float32")
                                     for k in FROZEN_RANKS[t]])
def test_sgd_batch_frozen_side_is_untouched(mf, dtype, k, kernel, side):
    """update_user=False / update_item=False at a tail rank of each W: the
    frozen side keeps its input bits, the other side is the oracle's."""
    uu, ui = side != "user", side != "item"
    d = _ratings(k > 128)
    start = _params(d["nu"], d["ni"], k, dtype, 100 + k)
    got = _gpu_epoch(d, start, kernel, k, dtype, uu, ui)
    frozen = (0, 2) if side == "user" else (1, 3)
    for j in frozen:
        assert np.array_equal(got[j], start[j])
    ref = _oracle_epoch(d, start, kernel, k, uu, ui)
    for j in frozen:
        assert np.array_equal(ref[j], start[j])
    if dtype == "float64":
        _assert_fp64_close(got, ref)
    else:
        n32 = _numpy_epoch(d, start, kernel, k, "float32", uu, ui)
        _assert_fp32_close(f"frozen-{side} {kernel} k={k}", got, n32, ref)


def _sse_case(d, kernel, k, dtype):
    """(engine with the start parameters loaded, oracle RMSE, float32-NumPy
    unit of the RMSE or None)."""
    import oracle
    from matrix_factorization.engine import SGDEngine

    start = _params(d["nu"], d["ni"], k, dtype, 200 + k)
    P, Q, bu, bi = start
    eng = SGDEngine(d["u0"].copy(), d["i0"].copy(), d["r0"].copy(), d["nu"], d["ni"], k,
                    kernel, dtype, "cuda:0", global_mean=d["mu"], **_hyp(k))
    eng.load_params(*start)
    assert eng.slab is None and eng.eval_offs is not None
    ro = oracle.rmse(d["u0"], d["i0"], d["r0"], d["mu"], bu, bi, P, Q, kernel=kernel, **_hyp(k))
    d32 = None
    if dtype == "float32":
        d32 = abs(numpy_rmse(d["u0"], d["i0"], d["r0"], d["mu"], bu, bi, P, Q, kernel,
                             _hyp(k)["gamma"], LO, HI, "float32") - ro)
    return eng, ro, d32


def _gpu_rmse(eng):
    eng.sse_async(0)
    return eng.rmse_values(1)[0]


def _assert_rmse(tag, got, ro, d32):
    if d32 is None:
        assert abs(got - ro) < 1e-12, f"{tag}: |diff| {abs(got - ro):.3e}"
        return
    _figure(f"ROWLAYOUT {tag} d32={d32:.3e} gpu={abs(got - ro):.3e} rmse={ro:.6f}")
    assert M * d32 <= 1e-4 * ro
    assert abs(got - ro) <= M * d32 + 4 * EPS32 * ro, \
        f"{tag}: |diff| {abs(got - ro):.3e} > {M} * {d32:.3e} + 4 eps32 * {ro:.3g}"


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype,k", [(t, k) for t in ("float64", "float32")
                                     for k in SGD_RANKS[t]])
def test_training_sse_equals_oracle(mf, dtype, k, kernel, monkeypatch):
    """Check 3: k_sse_lean in every layout against oracle.rmse."""
    monkeypatch.delenv("MF_SSE_VARIANT", raising=False)
    eng, ro, d32 = _sse_case(_ratings(k > 128), kernel, k, dtype)
    _assert_rmse(f"sse-lean {dtype} {kernel} k={k}", _gpu_rmse(eng), ro, d32)


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype,k", [(t, k) for t in ("float64", "float32")
                                     for k in layout_representatives(t)])
def test_training_sse_stream_variant(mf, dtype, k, kernel, monkeypatch):
    """Check 3, MF_SSE_VARIANT=1: k_sse_stream at one rank per layout (the
    tail rank where there is one) against oracle.rmse and against
    k_sse_lean."""
    monkeypatch.delenv("MF_SSE_VARIANT", raising=False)
    eng, ro, d32 = _sse_case(_ratings(k > 128), kernel, k, dtype)
    lean = _gpu_rmse(eng)
    monkeypatch.setenv("MF_SSE_VARIANT", "1")
    stream = _gpu_rmse(eng)
    _assert_rmse(f"sse-stream {dtype} {kernel} k={k}", stream, ro, d32)
    # Both passes square and add the ratings' errors in float64, in different
    # orders.  With W = 1 or V = 1 they form each error with the same
    # operations (the same bits, in either dtype), so they differ by the order
    # of a float64 sum only.  With W > 1 and V > 1 a lane's part of the dot
    # product is associated differently (k_sse_lean: vector by vector, then
    # the vector sums; k_sse_stream: one chain), a float32 effect in FP32:
    # there the issue's measured-unit bound holds between the two as well.
    w, _, v = rows_layout(dtype, k)
    gap = abs(stream - lean)
    _figure(f"ROWLAYOUT sse-gap {dtype} {kernel} k={k} gap={gap:.3e}")
    if d32 is None or w == 1 or v == 1:
        assert gap < 1e-12, f"|stream - lean| = {gap:.3e}"
    else:
        assert gap <= M * d32 + 4 * EPS32 * ro, f"|stream - lean| = {gap:.3e}"


# ----------------------------------------------------------- read layouts
READ_NU, READ_NI = 90, 150


def _read_engine(kernel, k, dtype):
    from matrix_factorization.device_model import DeviceModel

    start = _params(READ_NU, READ_NI, k, dtype, 300 + k)
    P, Q, bu, bi = start
    Q[5], bi[5] = Q[3], bi[3]                    # an exact tie for every user
    Q[149], bi[149] = Q[70], bi[70]
    eng = DeviceModel(READ_NU, READ_NI, k, kernel, dtype, "cuda:0", global_mean=3.4, **_hyp(k))
    eng.load_params(*start)
    return eng, start


def _all_scores(eng, users):
    u = np.repeat(np.asarray(users, np.int32), READ_NI)
    i = np.tile(np.arange(READ_NI, dtype=np.int32), len(users))
    return eng.predict(u, i, False).reshape(len(users), READ_NI)


def _read_users():
    users = np.random.RandomState(5).choice(READ_NU, 40, replace=False).astype(np.int32)
    users[7] = -1                                # unknown user: zero row, zero bias
    return users


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k", READ_RANKS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_predict_topk_rank(mf, dtype, k, kernel):
    """Check 4: the predict kernel against oracle.predict; the exact top-k
    and the rank kernel against a stable sort of predict's own scores."""
    import oracle
    import ranking_reference as rr

    eng, (P, Q, bu, bi) = _read_engine(kernel, k, dtype)
    rs = np.random.RandomState(k)
    u = rs.randint(0, READ_NU, 500).astype(np.int32)
    i = rs.randint(0, READ_NI, 500).astype(np.int32)
    u[::97] = -1
    i[::89] = -1
    for bound in (True, False):
        got = eng.predict(u, i, bound)
        ref = oracle.predict(u, i, 3.4, bu, bi, P, Q, kernel=kernel, bound=bound, **_hyp(k))
        dev = _maxabs(got - ref)
        if dtype == "float64":
            assert dev <= 1e-12, f"bound={bound}: max |diff| {dev:.3e}"
            continue
        n32 = numpy_predict(u, i, 3.4, bu, bi, P, Q, kernel, _hyp(k)["gamma"], LO, HI,
                            "float32", bound)
        d32, scale = _maxabs(n32 - ref), _maxabs(ref)
        _figure(f"ROWLAYOUT predict32 {kernel} k={k} bound={int(bound)} d32={d32:.3e} "
              f"gpu={dev:.3e} ratio={dev / d32 if d32 else 0.0:.3f}")
        assert M * d32 <= 1e-4 * scale
        assert dev <= M * d32 + 4 * EPS32 * scale, \
            f"bound={bound}: max |diff| {dev:.3e} > {M} * {d32:.3e} + 4 eps32 * {scale:.3g}"

    users = _read_users()
    scores = _all_scores(eng, users)
    eng.topk_mfma = False                        # the exact path
    for amount in (10, 65):                      # fused; above kFusedMaxAmount = 64: two-stage
        ids, sc = eng.topk(users, amount)
        for q in range(len(users)):
            order = np.argsort(~rr.order_key(scores[q]), kind="stable")[:amount]
            assert ids[q].tolist() == order.tolist(), f"amount {amount}, user slot {q}"
            assert np.array_equal(sc[q], scores[q][order]), f"amount {amount}, user slot {q}"
    tp = np.arange(len(users) + 1, dtype=np.int64) * 3
    ti = rs.randint(0, READ_NI, 3 * len(users)).astype(np.int32)
    ti[:4] = [3, 5, 70, 149]                     # the tied pairs
    ranks, ncand = eng.rank(users, tp, ti)
    want_r, want_c = rr.ranks_from_scores(scores, tp, ti)
    assert np.array_equal(ncand, want_c) and np.array_equal(ranks, want_r)


@gpu
@pytest.mark.parametrize("k", MM_RANKS)
def test_topk_mfma_filter_equals_exact(mf, k, monkeypatch):
    """Check 4, where mf_topk_mm_supported says yes: the MFMA candidate
    filter returns the exact path's ids and scores."""
    monkeypatch.delenv("MF_TOPK_MFMA", raising=False)
    eng, _ = _read_engine("linear", k, "float32")
    users = _read_users()
    q = eng.topk_prepare(users, 10)
    assert q["mm"], "the MFMA filter should take this case"
    eng.topk_launch(q)
    assert not eng.topk_finish(q), "the filter overflowed: exact would be compared with exact"
    assert q["mm"]
    mi, ms = q["items"].cpu().numpy(), q["scores"].cpu().numpy()
    eng.topk_launch(q, exact=True)
    assert np.array_equal(mi, q["items"].cpu().numpy())
    assert np.array_equal(ms, q["scores"].cpu().numpy())


def test_topk_mfma_cases_left_out():
    """The MFMA comparison leaves out exactly the cases mf_topk_mm_supported
    refuses: everything of check 4 but FP32 linear at ranks up to 64."""
    from matrix_factorization import _lib

    lib = _lib.load()
    yes = {(dt, kn, k) for dt in ("float32", "float64") for kn in KERNELS for k in READ_RANKS
           if lib.mf_topk_mm_supported(k, _lib.KERNEL_CODES[kn],
                                       _lib.MF_F32 if dt == "float32" else _lib.MF_F64, 10)}
    assert yes == {("float32", "linear", k) for k in MM_RANKS}
