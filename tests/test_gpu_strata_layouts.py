"""Every row layout of the stratified sweep (csrc/mf_strata.hpp), in every
launch form.

The strata kernels are compiled for the 16 layouts (W, GS, V) per dtype of
``dispatch_rows`` (tests/row_layouts_reference.py restates the table), times
the launch forms: one launch per stratum (k_sgd_strata), the persistent epoch
(k_sgd_strata_epoch) at depth 1 and 2, with and without user-range classes,
the stream form (k_sgd_strata_stream, KB = 2 / 4), the 8-wave kernels and the
narrow 4-wave kernels (which run (GS/2, 2V)).  tests/test_gpu_strata.py checks
the schedules at ranks up to 100 (FP64) / 64 (FP32); this file walks the
layouts: ``SGD_RANKS`` without 0, every layout at its full width and at a tail
rank, at the engine level (``SGDEngine``), on a few thousand ratings, so a
failure names one layout of one kernel.

The checks, as the tests' docstrings number them:

  1  (CPU) the rank lists cover every layout, full and tail; the slot and form
     tables restated here equal mf_strata_slots_waves; the shapes meet the
     preconditions the GPU tests rely on (host planner only)
  2  FP64, every layout: per-stratum launches against oracle.sgd_pass in
     plan.serial_order; rank 0 is refused by name
  3  FP32, every layout: the same runs value by value (the bound below)
  4  FP32 bits against k_sgd_batch (epoch_exact) in the same serial order
  5  every launch form at every layout where it exists, bit for bit against
     per-stratum launches, the three kernels each
  6  the planner left to choose everything at wide ranks, where it must raise
     B until the LDS image fits

Shapes.  Dense: 240 users x 48 items, 3000 ratings, B = 3 (item ranges of at
most 17 items: the FP64 image at rank 1024 is 140 048 B of the 160 KiB).  Its
plans forward user rows from t-1, from t-2 only, and leave slots idle, in
every layout (``test_shapes_meet_their_preconditions``).  Sparse: the same
users and items, 170 ratings, B = 4, C = 3: blocks of 0 to 4 steps, one of
the 48 empty and 47 shorter than the stream form's 4-step lookahead (1200
ratings leave none empty; the count was lowered with the host planner).

Which test covers which instantiation family (all per layout unless noted):

  k_sgd_strata (one launch per stratum), 16 waves
      test_per_stratum_fp64_equals_oracle, test_per_stratum_fp32_value_by_value
  k_sgd_strata, 16 and 8 waves, FP32 bits against k_sgd_batch
      test_fp32_strata_bits_equal_the_batch_kernel
  k_sgd_strata_epoch, depth 1 and 2, one class, 16 and 8 waves
      test_persistent_forms_equal_per_stratum_launches
  k_sgd_strata / k_sgd_strata_epoch, 4 narrow waves
      test_narrow_form
  k_sgd_strata_epoch with classes (CLS = true), depth 1 and 2
      test_user_range_classes (dense), test_user_range_classes_sparse
  k_sgd_strata_stream, KB = 2 (V <= 2: the layouts it exists for), 16 / 8 waves
      test_stream_form (dense), test_stream_form_sparse
  k_sgd_strata_stream, KB = 4
      test_stream_form_four_bias_loads_per_thread
  MF_FLAG_L2_HANDOFF, item phases, delta-out (one wide rank each)
      test_l2_handoff_wide_rank, test_item_phases_and_delta_out_wide_tail
  the planner (choose_strata_blocks raising B, classes, regroupings)
      test_planner_raises_blocks_until_the_image_fits

FP64 bars, unchanged from test_gpu_strata.py: parameters within 1e-11 *
max(1, |value|), training RMSE within 1e-12 of oracle.rmse.

FP32, value by value.  Every element of P, Q, b_u, b_i against the FP64
oracle run on the FP32-rounded start in the same serial order, within
``M * d32 + 4 * eps32 * max|ref|``: d32 is the deviation from that oracle of
the NumPy float32 sweep (row_layouts_reference.numpy_sgd_sweep) in that same
order, per array; M the smallest power of two that is at least twice the
largest ratio max|gpu - ref| / d32 of the linear-kernel cases (the lane-group
summation order differs from NumPy's, and per layout).  M * d32 < 1e-4 of the
parameter scale is asserted in every case.

Observed on an MI355X (the 75 per-stratum cases of check 3, then all 109
FP32 value-compared cases: narrow, sparse, stream, phases, planner; 4 arrays each);
ratio = max|gpu - ref| / d32, the largest over all ranks and arrays:

  kernel    per-stratum ratio (median)   d32 of P, Q        all FP32 cases (median)
  linear    1.892 (1.00)                 4.0e-8 .. 2.1e-7   1.892 (1.00)
  sigmoid   1.428 (1.00)                 3.9e-8 .. 3.7e-7   1.428 (1.00)
  rbf       1.160 (1.00)                 3.4e-8 .. 3.6e-7   1.160 (1.00)

The largest linear ratio is 1.892 (rank 101, b_i), twice that 3.78, so M = 4,
the M of test_gpu_row_layouts.py.  d32 / max|ref| is at most 1.14e-6, so
M * d32 stays below 4.6e-6 of the parameter scale.

Check 4 (``test_fp32_strata_bits_equal_the_batch_kernel``) is bitwise in all
16 FP32 layouts, at the full and the tail rank of each, in the 16-wave form
and in the 8-wave form of the eight layouts that have one, linear and sigmoid:
no layout is left to check 3 alone.  The narrow form associates the dot
product differently by design ((GS/2, 2V): mf_strata.hpp, StrataRun::run) and
is held to check 3's bound instead (largest ratio 1.41).

What the file sees: four deliberately wrong FP32 builds of mf_strata.hpp
(values only, none kept), one run each -- failing GPU cases of this file (of
430), median excess of P / Q over the FP32 bound where values are compared,
failing cases of test_gpu_strata.py (of 51); counted while each launch-form
case ran linear and one of sigmoid / rbf (all three now: no fewer fail):

  pprev2 ignored in step2 (the stale gathered row)     60   13 000x (2 arrays)   14
  h.reg dropped on a tail row's last vector            103  3300x                none
  tail q select returns the clamped value, not 0       18   580x (rbf only)      none
  sigmoid derivative halved on lane 1 of a group       63   2200x                4

Wall time of this file on an MI355X: 17 s (433 cases).
"""

import functools
import os

import numpy as np
import pytest

from row_layouts_reference import (SGD_RANKS, WV, all_rows_layouts, assert_fp32_close,
                                   layout_representatives, maxabs, numpy_sgd_sweep,
                                   rows_layout)

gpu = pytest.mark.gpu

KERNELS = ("linear", "sigmoid", "rbf")
LR, REG, LO, HI = 0.01, 0.02, 1.0, 5.0
M = 4          # see the module docstring
TS = {"float32": 4, "float64": 8}
STRATA_ENV = ("MF_STRATA_DEEP", "MF_STRATA_STREAM", "MF_STRATA_L2", "MF_STRATA_WAVES",
              "MF_STRATA_CLASSES", "MF_STRATA_PHASES", "MF_STRATA_REGROUP", "MF_STRATA_ORDER",
              "MF_STRATA_PERSISTENT", "MF_STRATA_COOP", "MF_STRATA_EARLY", "MF_SSE_BESIDE")

# name -> (users, items, ratings, seed of the ids and ratings)
SHAPES = {
    "dense": (240, 48, 3000, 7),
    "sparse": (240, 48, 170, 7),
    "kb4-8": (3000, 40, 6000, 8),         # B = 1, C = 2: 1500 users per range
    "kb4-16": (6000, 40, 9000, 9),        # 3000 users per range
    "l2": (480, 96, 6000, 10),
    "planner": (2000, 400, 20000, 11),        # B starts at 4: slabs of 100 items
    "planner-items": (2000, 1400, 20000, 12),    # ... of 350 items (for FP32 rank 132)
}
# check 6: (dtype, rank, kernel, shape); at B = 4 none of the images fits the LDS
PLANNER_CASES = [("float64", 260, "linear", "planner"), ("float64", 516, "sigmoid", "planner"),
                 ("float32", 132, "sigmoid", "planner-items"),
                 ("float32", 1023, "linear", "planner")]
PLANNER_B0 = 4
DENSE_B = 3
SPARSE_B, SPARSE_C = 4, 3


# ------------------------------------------------------- ranks and forms
def is_tail(dtype, k):
    w, gs, v = rows_layout(dtype, k)
    return 0 < k < w * gs * v


RANKS = {t: [k for k in SGD_RANKS[t] if k] for t in ("float32", "float64")}
# one full-width rank (where the layout has one in the lists) and one tail
# rank (where it can have a tail) per layout
FORM_RANKS = {t: sorted({k for k in RANKS[t] if not is_tail(t, k)} |
                        set(layout_representatives(t))) for t in RANKS}
# one tail rank per W
W_TAIL_RANKS = {"float32": [132, 1023], "float64": [260, 1023]}


def strata_group_slots(dtype, w, gs, v):
    """mf_strata.hpp:strata_group_slots: two rating slots per lane group while
    a lane's share of a row is small, else one."""
    ts = TS[dtype]
    return 2 if 64 // gs < 8 and w * v * ts <= (32 if ts == 4 else 16) else 1


def strata_slots(dtype, w, gs, v, nw=16):
    return nw * strata_group_slots(dtype, w, gs, v) * (64 // gs)


def strata_has_8_waves(dtype, v):
    return v == 1 or (dtype == "float64" and v == 2)


def strata_has_narrow(dtype, w, gs, v):
    if dtype != "float32" or not strata_has_8_waves(dtype, v) or gs < 2:
        return False
    return strata_slots(dtype, w, gs // 2, 2 * v, 4) == strata_slots(dtype, w, gs, v, 8)


def form_slots(dtype, k, waves):
    """Slots per step of the ``waves``-wave strata kernels of rank k, 0 where
    that form does not exist (StrataSlots in mf_strata.hpp)."""
    w, gs, v = rows_layout(dtype, k)
    if waves == 16:
        return strata_slots(dtype, w, gs, v, 16)
    if waves == 8 and strata_has_8_waves(dtype, v):
        return strata_slots(dtype, w, gs, v, 8)
    if waves == 4 and strata_has_narrow(dtype, w, gs, v):
        return strata_slots(dtype, w, gs // 2, 2 * v, 4)
    return 0


def _wave_cases(waves_of):
    """(dtype, k, waves) over FORM_RANKS; every case runs the three kernels."""
    return [(t, k, wv) for t in ("float64", "float32") for k in FORM_RANKS[t]
            for wv in waves_of(t, k)]


WAVE_CASES = _wave_cases(lambda t, k: [wv for wv in (16, 8) if form_slots(t, k, wv)])
NARROW_CASES = _wave_cases(lambda t, k: [4] if form_slots(t, k, 4) else [])
STREAM_CASES = [c for c in WAVE_CASES if rows_layout(c[0], c[1])[2] <= 2]


# ------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def _ratings(shape):
    """Distinct (user, item) pairs with ratings 1..5; shared, never modified."""
    nu, ni, nnz, seed = SHAPES[shape]
    rs = np.random.RandomState(seed)
    keys = rs.choice(nu * ni, nnz, replace=False)
    u = (keys // ni).astype(np.int32)
    i = (keys % ni).astype(np.int32)
    r = rs.randint(1, 6, nnz).astype(np.float64)
    out = dict(nu=nu, ni=ni, u=u, i=i, r=r, mu=float(r.mean()))
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
    for a in out:
        a.setflags(write=False)
    return out


def _hyp(k):
    return dict(gamma=1.0 / k if k else 1.0, min_rating=LO, max_rating=HI)


def _figure(line):
    """The measured figures behind the docstring's table: printed only when
    MF_STRATA_LAYOUT_FIGURES is set (then run with -s)."""
    if os.environ.get("MF_STRATA_LAYOUT_FIGURES"):
        print(line.replace("ROWLAYOUT", "STRATALAYOUT"))


def _draws(B, C, n_epochs):
    """(stratum order, rotation seed) of each epoch."""
    from matrix_factorization.engine import stratum_order

    return [(stratum_order(np.random.RandomState(40 + ep), B, "random", C), 9000 + 17 * ep)
            for ep in range(n_epochs)]


def _dcode(dtype):
    from matrix_factorization import _lib

    return _lib.MF_F32 if dtype == "float32" else _lib.MF_F64


@functools.lru_cache(maxsize=None)
def _host_plan(shape, dtype, k, B, C=1, waves=16):
    """The plan prepare_strata(n_blocks=B, waves=waves, classes=C) builds
    (SGDEngine._build_plan), from the host planner alone: no GPU."""
    from matrix_factorization import _lib
    from matrix_factorization.engine import (StrataPlan, balanced_bounds, sched_strata_pick,
                                             strata_slots as lib_slots)

    d = _ratings(shape)
    lib = _lib.load()
    ub = balanced_bounds(d["u"], d["nu"], C * B)
    ib = balanced_bounds(d["i"], d["ni"], B)
    if (lib.mf_strata_lds_bytes(int(np.diff(ib).max()), int(np.diff(ub).max()), k, _dcode(dtype))
            > lib.mf_strata_lds_limit()):
        ib = balanced_bounds(d["i"], d["ni"], B, False)
    ns = lib_slots(k, _dcode(dtype), waves)
    assert ns > 0
    sched, bstep, _ = sched_strata_pick(d["u"], d["i"], d["nu"], d["ni"], B, ub, ib,
                                        [(ns, waves)], C, 0.0)
    plan = StrataPlan(B, ns, ub, ib, bstep, sched, C)
    plan.narrow = waves == 4
    return plan


def _same_plan(a, b):
    return (a.B == b.B and a.NS == b.NS and a.classes == b.classes and a.narrow == b.narrow
            and all(np.array_equal(getattr(a, f), getattr(b, f))
                    for f in ("ubnd", "ibnd", "bstep", "sched")))


def _oracle_epochs(d, start, kernel, k, orders, item_flags):
    import oracle

    P, Q, bu, bi = (a.copy() for a in start)
    for order, ui in zip(orders, item_flags):
        oracle.sgd_pass(d["u"], d["i"], d["r"], d["mu"], bu, bi, P, Q, kernel=kernel, lr=LR,
                        reg=REG, order=order, update_item=ui, **_hyp(k))
    return P, Q, bu, bi


def _numpy_epochs(d, start, kernel, k, orders, item_flags):
    cur = start
    for order, ui in zip(orders, item_flags):
        cur = numpy_sgd_sweep(d["u"], d["i"], d["r"], d["mu"], cur[2], cur[3], cur[0], cur[1],
                              kernel, _hyp(k)["gamma"], LR, REG, LO, HI, order, "float32",
                              True, ui)
    return cur


def _reference(shape, dtype, k, kernel, B, C, waves, item_flags):
    """The epochs ``item_flags`` (update_item of each) of the plan (B, C,
    waves) in the serial order of ``_draws``: the start parameters, the FP64
    oracle's result and, for float32, the NumPy float32 sweep's."""
    d = _ratings(shape)
    plan = _host_plan(shape, dtype, k, B, C, waves)
    start = _params(d["nu"], d["ni"], k, dtype, 100 + k)
    draws = _draws(B, C, len(item_flags))
    orders = [plan.serial_order(seq, seed) for seq, seed in draws]
    for o in orders:
        assert np.array_equal(np.sort(o), np.arange(len(d["u"])))
    ref = _oracle_epochs(d, start, kernel, k, orders, item_flags)
    n32 = _numpy_epochs(d, start, kernel, k, orders, item_flags) if dtype == "float32" else None
    return dict(plan=plan, start=start, draws=draws, orders=orders, ref=ref, n32=n32)


# ------------------------------------------------------------- CPU tests
def test_rank_lists_cover_every_strata_layout():
    """The rank lists reach every (W, GS, V) of dispatch_rows per dtype, every
    layout that can have a tail once full (where a full-width rank takes it)
    and once with a tail; FORM_RANKS keeps one of each."""
    for dtype in ("float32", "float64"):
        want = all_rows_layouts(dtype)
        for ranks in (RANKS[dtype], FORM_RANKS[dtype]):
            assert 0 not in ranks and max(ranks) == 1024
            assert {rows_layout(dtype, k) for k in ranks} == want and len(want) == 16
            tails = {rows_layout(dtype, k) for k in ranks if is_tail(dtype, k)}
            # (WV,1,1) and (WV,2,1) are entered at k = WV and 2 WV only: no tail
            assert tails == {lay for lay in want if lay[0] == 1 or lay[1] * lay[2] >= 4}
            full = {rows_layout(dtype, k) for k in ranks if not is_tail(dtype, k)}
            assert full >= {lay for lay in want if lay[0] > 1}
        for k in W_TAIL_RANKS[dtype]:
            assert k in FORM_RANKS[dtype] and is_tail(dtype, k)
        assert {rows_layout(dtype, k)[0] for k in W_TAIL_RANKS[dtype]} == {WV[dtype], 1}
    assert rows_layout("float64", 1024) == (1, 64, 16) and not is_tail("float64", 1024)
    # what tests/test_gpu_strata.py's ranks leave out, by layout
    old = {"float64": [7, 8, 16, 20, 32, 64, 100], "float32": [16, 20, 32, 64]}
    for dtype, n_new in (("float64", 10), ("float32", 13)):
        assert len(all_rows_layouts(dtype) - {rows_layout(dtype, k) for k in old[dtype]}) == n_new


def test_form_tables_match_the_library():
    """strata_group_slots / strata_slots / strata_has_8_waves /
    strata_has_narrow restated above give mf_strata_slots_waves for every rank
    of the lists: the slot counts, and no kernel where the form does not exist."""
    from matrix_factorization import _lib

    lib = _lib.load()
    seen = set()
    for dtype in ("float32", "float64"):
        for k in RANKS[dtype]:
            for waves in (16, 8, 4):
                got = int(lib.mf_strata_slots_waves(k, _dcode(dtype), waves))
                assert max(got, 0) == form_slots(dtype, k, waves), (dtype, k, waves, got)
                assert got > 0 or got == -1
                seen.add((dtype, waves, got > 0))
        # S = 2 up to (1,64,8) in FP32 (Rows::p[2][8]) / (1,64,2) in FP64, then 1
        v2 = 8 if dtype == "float32" else 2
        assert strata_group_slots(dtype, 1, 64, v2) == 2
        assert strata_group_slots(dtype, 1, 64, 2 * v2) == 1
    # every form exists somewhere and is missing somewhere, but 16 waves
    # (always there) and the FP64 narrow form (never)
    assert len(seen) == 9 and ("float64", 4, True) not in seen
    narrow = [k for k in RANKS["float32"] if form_slots("float32", k, 4)]
    assert narrow == [8, 16, 32, 12, 20, 17, 33]
    assert form_slots("float32", 64, 8) == 64 and form_slots("float32", 64, 16) == 128
    assert form_slots("float64", 64, 8) and not form_slots("float64", 100, 8)


def _plan_figures(plan, users):
    """Slot-steps that forward their user row from the step before, from two
    steps before only, and idle slot-steps, in the plan's own step order."""
    f1 = f2 = idle = 0
    for blk in range(len(plan.bstep) - 1):
        st0, st1 = int(plan.bstep[blk]), int(plan.bstep[blk + 1])
        if st1 == st0:
            continue
        g = plan.sched[st0 * plan.NS:st1 * plan.NS].reshape(st1 - st0, plan.NS)
        idle += int((g < 0).sum())
        usr = np.where(g >= 0, users[np.maximum(g, 0)], -1)
        a = (usr[1:] >= 0) & (usr[1:] == usr[:-1])
        f1 += int(a.sum())
        if len(usr) > 2:
            f2 += int(((usr[2:] >= 0) & (usr[2:] == usr[:-2]) & ~a[1:]).sum())
    return f1, f2, idle


def _sparse_steps(plan):
    steps = np.diff(plan.bstep)
    return steps.min() == 0 and (steps < 4).mean() > 0.5


def test_shapes_meet_their_preconditions():
    """What the GPU tests below rely on, checked with the host planner alone:
    the dense shape's image fits the LDS at every rank, and its plans forward
    rows from t-1, from t-2 only, and have idle slots, at every slot count and
    with C = 1 and 2; the sparse shape has empty blocks and mostly blocks
    shorter than 4 steps; the KB = 4 shapes' user ranges need 4 bias loads per
    thread."""
    from matrix_factorization import _lib

    lib = _lib.load()
    limit = lib.mf_strata_lds_limit()
    assert limit == 160 * 1024
    users = _ratings("dense")["u"]
    seen_ns = set()
    for dtype in ("float64", "float32"):
        for k in RANKS[dtype]:
            for waves in (16, 8, 4):
                if not form_slots(dtype, k, waves):
                    continue
                for C in (1, 2):
                    plan = _host_plan("dense", dtype, k, DENSE_B, C, waves)
                    assert plan.NS == form_slots(dtype, k, waves)
                    need = lib.mf_strata_lds_bytes(plan.max_items, plan.max_users, k,
                                                   _dcode(dtype))
                    assert need <= limit, (dtype, k, need)
                    if (plan.NS, C) in seen_ns:
                        continue
                    seen_ns.add((plan.NS, C))
                    f1, f2, idle = _plan_figures(plan, users)
                    assert f1 > 0 and f2 > 0 and idle > 0, (plan.NS, C, f1, f2, idle)
                    assert plan.max_items <= 17 and plan.max_users <= (81 if C == 1 else 41)
    assert {ns for ns, _ in seen_ns} >= {16, 32, 64, 128, 256, 1024}
    assert lib.mf_strata_lds_bytes(17, 81, 1024, _dcode("float64")) == 140048
    for dtype, k in (("float32", 1023), ("float64", 260), ("float32", 64), ("float64", 20)):
        for waves in (16, 8):
            if form_slots(dtype, k, waves):
                assert _sparse_steps(_host_plan("sparse", dtype, k, SPARSE_B, SPARSE_C, waves))
    for shape, waves in (("kb4-8", 8), ("kb4-16", 16)):
        plan = _host_plan(shape, "float32", 64, 1, 2, waves)
        assert 2 * waves * 64 < plan.max_users <= 4 * waves * 64
    for dtype, k, _, shape in PLANNER_CASES:
        assert _planner_image_at_b0(shape, dtype, k) > limit


def _planner_image_at_b0(shape, dtype, k):
    """LDS bytes of the default plan (B = sqrt(n / 1024) = 4, one class) of a
    planner shape: the smaller of the two item cuts choose_strata_blocks tries."""
    from matrix_factorization import _lib
    from matrix_factorization.engine import balanced_bounds

    d = _ratings(shape)
    assert int(np.sqrt(len(d["u"]) / 1024.0)) == PLANNER_B0
    users = int(np.diff(balanced_bounds(d["u"], d["nu"], PLANNER_B0)).max())
    return min(int(_lib.load().mf_strata_lds_bytes(
        int(np.diff(balanced_bounds(d["i"], d["ni"], PLANNER_B0, by)).max()), users, k,
        _dcode(dtype))) for by in (True, False))


# ------------------------------------------------------------- GPU tests
@pytest.fixture(scope="module")
def mf():
    import matrix_factorization

    matrix_factorization._lib.load()
    return matrix_factorization


@pytest.fixture(autouse=True)
def _no_strata_env(monkeypatch):
    """The forms are chosen by the tests, not by the environment."""
    for name in STRATA_ENV:
        monkeypatch.delenv(name, raising=False)


def _engine(shape, dtype, k, kernel, start=None):
    from matrix_factorization.engine import SGDEngine

    d = _ratings(shape)
    if start is None:
        start = _params(d["nu"], d["ni"], k, dtype, 100 + k)
    eng = SGDEngine(d["u"].copy(), d["i"].copy(), d["r"].copy(), d["nu"], d["ni"], k, kernel,
                    dtype, "cuda:0", global_mean=d["mu"], **_hyp(k))
    eng.load_params(*(a.copy() for a in start))
    eng.strata_regroup = 1
    return eng


def _run(shape, dtype, k, kernel, B, C=1, waves=16, item_flags=(True, True), persistent=False,
         deep=None, stream=None, expect=None):
    """The epochs of ``_draws`` on a fresh engine; (engine, plan, parameters).
    Every epoch is one launch when ``persistent``, else C * B."""
    eng = _engine(shape, dtype, k, kernel)
    eng.strata_deep_pipe, eng.strata_stream = deep, stream
    plan = eng.prepare_strata(n_blocks=B, waves=waves, classes=C)
    assert _same_plan(plan, _host_plan(shape, dtype, k, B, C, waves))
    if expect is not None:
        expect(eng, plan)
    for (seq, seed), ui in zip(_draws(B, C, len(item_flags)), item_flags):
        _, n_launch = eng.epoch_strata(seq, seed, lr=LR, reg=REG, update_item=ui,
                                       persistent=persistent, timing=True)
        assert n_launch == (1 if persistent else C * B)
    eng.check_strata()
    return eng, plan, eng.params_numpy()


def _assert_same_bits(got, want, what):
    for name, a, b in zip(("P", "Q", "bu", "bi"), got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), \
            f"{what}: {name} differs in {int((a != b).sum())} values, max {maxabs(a - b):.3e}"


def _assert_fp64_close(got, ref):
    for name, g, rf in zip(("P", "Q", "bu", "bi"), got, ref):
        assert g.shape == rf.shape
        err, scale = maxabs(g - rf), max(1.0, maxabs(rf))
        assert err <= 1e-11 * scale, f"{name}: max |diff| {err:.3e} > 1e-11 * {scale:.3g}"


def _assert_oracle(tag, dtype, got, rf):
    """FP64: the project's bars; FP32: the measured-unit bound."""
    if dtype == "float64":
        _assert_fp64_close(got, rf["ref"])
    else:
        assert_fp32_close(tag, got, rf["n32"], rf["ref"], m=M, figure=_figure)


def _two_epochs(dtype, k):
    return (True, not is_tail(dtype, k))


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k", RANKS["float64"])
def test_per_stratum_fp64_equals_oracle(mf, kernel, k):
    """Check 2: k_sgd_strata<double> in every layout, two epochs (the second
    with the items frozen at the tail ranks), against oracle.sgd_pass in
    plan.serial_order; parameters and the training RMSE."""
    import oracle

    flags = _two_epochs("float64", k)
    rf = _reference("dense", "float64", k, kernel, DENSE_B, 1, 16, flags)
    eng, _, got = _run("dense", "float64", k, kernel, DENSE_B, item_flags=flags)
    _assert_fp64_close(got, rf["ref"])
    d = _ratings("dense")
    P, Q, bu, bi = rf["ref"]
    ro = oracle.rmse(d["u"], d["i"], d["r"], d["mu"], bu, bi, P, Q, kernel=kernel, **_hyp(k))
    eng.sse_async(0)
    assert abs(eng.rmse_values(1)[0] - ro) < 1e-12


@gpu
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_rank_zero_is_refused_by_name(mf, dtype):
    """The strata schedule has no biases-only form: prepare_strata() refuses
    rank 0 with a message that says so (its one-time launcher call,
    MF_FLAG_PREPARE) and keeps no plan, so an epoch after it is refused as
    well; nothing is applied."""
    from matrix_factorization._lib import MFLibraryError

    eng = _engine("dense", dtype, 0, "linear")
    before = eng.params_numpy()
    with pytest.raises(MFLibraryError, match="the strata schedule needs n_factors >= 1"):
        eng.prepare_strata(n_blocks=DENSE_B, waves=16)
    assert eng.strata is None
    with pytest.raises(RuntimeError, match="call prepare_strata\\(\\) first"):
        eng.epoch_strata(None, 1, lr=LR, reg=REG)
    _assert_same_bits(eng.params_numpy(), before, "after the refusal")
    assert maxabs(before[2]) > 0 and maxabs(before[3]) > 0


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k", RANKS["float32"])
def test_per_stratum_fp32_value_by_value(mf, kernel, k):
    """Check 3: k_sgd_strata<float> in every layout, the same two epochs,
    every value of P, Q, b_u, b_i against the FP64 oracle on the FP32-rounded
    start, within M float32-NumPy units."""
    flags = _two_epochs("float32", k)
    rf = _reference("dense", "float32", k, kernel, DENSE_B, 1, 16, flags)
    _, _, got = _run("dense", "float32", k, kernel, DENSE_B, item_flags=flags)
    assert_fp32_close(f"strata32 {kernel} k={k}", got, rf["n32"], rf["ref"], m=M, figure=_figure)


@gpu
@pytest.mark.parametrize("kernel", ["linear", "sigmoid"])
@pytest.mark.parametrize("k,waves", [(k, wv) for t, k, wv in WAVE_CASES if t == "float32"])
def test_fp32_strata_bits_equal_the_batch_kernel(mf, k, waves, kernel):
    """Check 4: strata_block and k_sgd_batch call the same per-rating routines
    at the same (W, GS, V) (lane_partial, group_sum, sgd_error, sgd_rows), and
    a strata step is a conflict-free batch: the FP32 result of the 16- and
    8-wave forms has the bits of epoch_exact in plan.serial_order."""
    flags = _two_epochs("float32", k)
    _, plan, got = _run("dense", "float32", k, kernel, DENSE_B, waves=waves, item_flags=flags)
    eng = _engine("dense", "float32", k, kernel)
    for (seq, seed), ui in zip(_draws(DENSE_B, 1, len(flags)), flags):
        eng.epoch_exact(plan.serial_order(seq, seed), LR, REG, update_item=ui)
    _assert_same_bits(got, eng.params_numpy(), "strata vs k_sgd_batch")


@gpu
@pytest.mark.parametrize("dtype,k,waves", WAVE_CASES)
def test_persistent_forms_equal_per_stratum_launches(mf, dtype, k, waves):
    """Check 5: the persistent epoch at depth 1 and at depth 2
    (strata_deep_pipe) is bit-identical to one launch per stratum, 16 waves at
    every layout and 8 waves wherever that kernel exists; three epochs, the
    last with the items frozen."""
    flags = (True, True, False)
    for kernel in KERNELS:
        _, _, base = _run("dense", dtype, k, kernel, DENSE_B, waves=waves, item_flags=flags)
        for deep in (False, True):
            _, _, got = _run("dense", dtype, k, kernel, DENSE_B, waves=waves, item_flags=flags,
                             persistent=True, deep=deep)
            _assert_same_bits(got, base, f"{kernel}, depth {1 + deep}")


@gpu
@pytest.mark.parametrize("k", [k for _, k, _ in NARROW_CASES])
def test_narrow_form(mf, k):
    """Check 5: the narrow 4-wave kernels (the 8-wave plan on lane groups half
    as wide, (GS/2, 2V)) wherever strata_has_narrow holds: persistent ==
    per-stratum bits, and check 3's bound against the oracle."""
    flags = (True, True, False)
    for kernel in KERNELS:
        rf = _reference("dense", "float32", k, kernel, DENSE_B, 1, 4, flags)
        _, plan, base = _run("dense", "float32", k, kernel, DENSE_B, waves=4, item_flags=flags)
        assert plan.narrow and plan.NS == form_slots("float32", k, 8)
        _, _, got = _run("dense", "float32", k, kernel, DENSE_B, waves=4, item_flags=flags,
                         persistent=True)
        _assert_same_bits(got, base, kernel)
        assert_fp32_close(f"narrow32 {kernel} k={k}", base, rf["n32"], rf["ref"], m=M,
                          figure=_figure)


def _classes_case(shape, dtype, k, kernel, B, C):
    flags = (True, True, False)
    _, plan, base = _run(shape, dtype, k, kernel, B, C, item_flags=flags)
    assert plan.classes == C and plan.n_strata == C * B
    for deep in (False, True):
        _, _, got = _run(shape, dtype, k, kernel, B, C, item_flags=flags, persistent=True,
                         deep=deep, stream=False)
        _assert_same_bits(got, base, f"{kernel}, depth {1 + deep}")
    return plan, base


@gpu
@pytest.mark.parametrize("dtype,k", [(t, k) for t, k, wv in WAVE_CASES if wv == 16])
def test_user_range_classes(mf, dtype, k):
    """Check 5: C = 2 user-range classes (k_sgd_strata_epoch<..., CLS = true>)
    at every layout, depth 1 and 2, one launch per epoch, bit-identical to the
    per-stratum launches; those are the oracle's sweep (FP64 bars)."""
    for kernel in KERNELS:
        _, base = _classes_case("dense", dtype, k, kernel, DENSE_B, 2)
        if dtype == "float64":
            rf = _reference("dense", dtype, k, kernel, DENSE_B, 2, 16, (True, True, False))
            _assert_fp64_close(base, rf["ref"])


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dtype,k", [(t, k) for t in W_TAIL_RANKS for k in W_TAIL_RANKS[t]])
def test_user_range_classes_sparse(mf, dtype, k, kernel):
    """Check 5: B = 4, C = 3 on the sparse shape (empty blocks, most blocks
    under 4 steps) at one tail rank per W: persistent == per-stratum bits, and
    the oracle's sweep."""
    plan, base = _classes_case("sparse", dtype, k, kernel, SPARSE_B, SPARSE_C)
    assert _sparse_steps(plan)
    rf = _reference("sparse", dtype, k, kernel, SPARSE_B, SPARSE_C, 16, (True, True, False))
    _assert_oracle(f"sparse32 {kernel} k={k}", dtype, base, rf)


def _stream_lds_bytes(dtype, max_items, cap, k, th, n_seq):
    """mf_strata.hpp:strata_stream_lds_bytes."""
    tb = TS[dtype] * (max_items * k + max_items + 2 * cap + th)
    return (tb + 15) // 16 * 16 + 16 * n_seq


def _expect_stream(dtype, k, waves, kb):
    """The launcher takes the stream kernel with KB = ``kb`` bias loads per
    thread: the plan's largest user range is in that window, and the kernel it
    reports has the stream form's LDS image (larger than the per-block
    form's by two bias slices, a word per thread and the geometry table)."""
    from matrix_factorization import _lib

    def check(eng, plan):
        th = waves * 64
        lo, hi = (0, 2 * th) if kb == 2 else (2 * th, 4 * th)
        assert lo < plan.max_users <= hi, (plan.max_users, th)
        slds = _stream_lds_bytes(dtype, plan.max_items, plan.max_users, k, th, plan.n_strata)
        plain = int(_lib.load().mf_strata_lds_bytes(plan.max_items, plan.max_users, k,
                                                    _dcode(dtype)))
        assert plain + 64 < slds <= 160 * 1024
        _, nw, lds = eng.strata_kernel_attrs(plan)
        assert nw == waves and slds <= lds < slds + 64, (nw, lds, slds, plain)
    return check


def _stream_case(monkeypatch, shape, dtype, k, kernel, B, C, waves, kb):
    flags = (True, True, False)
    _, plan, base = _run(shape, dtype, k, kernel, B, C, waves=waves, item_flags=flags)
    monkeypatch.setenv("MF_STRATA_DEEP", "1")
    monkeypatch.setenv("MF_STRATA_STREAM", "1")
    _, _, got = _run(shape, dtype, k, kernel, B, C, waves=waves, item_flags=flags,
                     persistent=True, expect=_expect_stream(dtype, k, waves, kb))
    monkeypatch.delenv("MF_STRATA_DEEP")
    monkeypatch.delenv("MF_STRATA_STREAM")
    _assert_same_bits(got, base, f"{kernel}, stream")
    return plan, base


@gpu
@pytest.mark.parametrize("dtype,k,waves", STREAM_CASES)
def test_stream_form(mf, dtype, k, waves, monkeypatch):
    """Check 5: k_sgd_strata_stream<..., KB = 2> (MF_STRATA_DEEP=1,
    MF_STRATA_STREAM=1, C = 2) at every layout it is compiled for (V <= 2),
    16 and 8 waves: bit-identical to the per-stratum launches."""
    for kernel in KERNELS:
        _stream_case(monkeypatch, "dense", dtype, k, kernel, DENSE_B, 2, waves, 2)


@gpu
@pytest.mark.parametrize("dtype,k,waves,kernel", [
    ("float32", 64, 8, "linear"), ("float32", 100, 16, "sigmoid"),
    ("float64", 20, 8, "sigmoid"), ("float64", 33, 16, "linear")])
def test_stream_form_sparse(mf, dtype, k, waves, kernel, monkeypatch):
    """Check 5: the stream form over empty blocks and blocks shorter than its
    4-step lookahead (B = 4, C = 3): per-stratum bits, the oracle's sweep."""
    plan, base = _stream_case(monkeypatch, "sparse", dtype, k, kernel, SPARSE_B, SPARSE_C,
                              waves, 2)
    assert _sparse_steps(plan)
    rf = _reference("sparse", dtype, k, kernel, SPARSE_B, SPARSE_C, waves, (True, True, False))
    _assert_oracle(f"stream-sparse32 {kernel} k={k}", dtype, base, rf)


@gpu
@pytest.mark.parametrize("dtype,k,waves,kernel", [
    ("float32", 64, 8, "linear"), ("float32", 20, 16, "sigmoid"),
    ("float64", 20, 8, "sigmoid"), ("float64", 64, 16, "linear")])
def test_stream_form_four_bias_loads_per_thread(mf, dtype, k, waves, kernel, monkeypatch):
    """Check 5: k_sgd_strata_stream<..., KB = 4>, chosen when the largest user
    range is in (2 TH, 4 TH] (TH = 64 waves threads): B = 1, C = 2 over 3000
    (8 waves) / 6000 (16 waves) users x 40 items.  Per-stratum bits, and the
    oracle's sweep."""
    shape = f"kb4-{waves}"
    _, base = _stream_case(monkeypatch, shape, dtype, k, kernel, 1, 2, waves, 4)
    rf = _reference(shape, dtype, k, kernel, 1, 2, waves, (True, True, False))
    _assert_oracle(f"stream-kb4-32 {kernel} k={k}", dtype, base, rf)


@gpu
@pytest.mark.parametrize("dtype,k", [("float32", 256), ("float64", 128)])
def test_l2_handoff_wide_rank(mf, dtype, k, monkeypatch):
    """Check 5: MF_FLAG_L2_HANDOFF (MF_STRATA_L2=1, the XCD-class stratum
    order, B = 16) at a wide rank whose rows are whole 128-B lines (1 KiB):
    the launcher turned it on (every workgroup published its XCC id) and the
    epoch is bit-identical to one launch per stratum."""
    import torch

    from matrix_factorization.engine import stratum_order

    B = 16
    monkeypatch.setenv("MF_STRATA_L2", "1")
    out = []
    for persistent in (True, False):
        eng = _engine("l2", dtype, k, "linear")
        eng.prepare_strata(n_blocks=B, waves=16)
        for ep in range(3):
            seq = stratum_order(np.random.RandomState(ep), B, "xcd")
            assert len(set((seq[:2] % 8).tolist())) == 1          # an XCD-class order
            _, n_launch = eng.epoch_strata(seq, 3000 + ep, lr=LR, reg=REG, update_item=ep != 2,
                                           persistent=persistent, timing=True)
            assert n_launch == (1 if persistent else B)
        eng.check_strata()
        if persistent:
            torch.cuda.synchronize()
            tags = eng._strata_ws.cpu().numpy().view(np.int32)[B + 1: 2 * B + 1]
            assert np.all(tags >> 4 == tags[0] >> 4) and tags[0] >> 4 > 0
            assert len(set((tags & 0xF).tolist())) == 8
        out.append(eng.params_numpy())
    _assert_same_bits(out[0], out[1], "L2 hand-off")


@gpu
@pytest.mark.parametrize("dtype,k,kernel", [("float32", 132, "linear"),
                                            ("float64", 260, "sigmoid")])
def test_item_phases_and_delta_out_wide_tail(mf, dtype, k, kernel):
    """Check 5: PhasedStrata (two item phases) and the delta-out form at a
    wide tail rank: persistent == per-stratum bits, the oracle's sweep in
    plan.serial_order, and delta-out leaves Q / b_i untouched with the same
    update in the deltas (as test_item_phases_equal_serialized_oracle)."""
    import torch

    from matrix_factorization.engine import PhasedStrata

    d = _ratings("dense")
    B, n_ph = DENSE_B, 2
    flags = (True, True)
    draws = _draws(B, 1, 2)
    start = _params(d["nu"], d["ni"], k, dtype, 100 + k)
    out = []
    for persistent in (True, False):
        eng = _engine("dense", dtype, k, kernel)
        plan = eng.prepare_strata(n_blocks=B, waves=16, phases=n_ph)
        assert isinstance(plan, PhasedStrata) and len(plan.phases) == n_ph and plan.B == B
        for seq, seed in draws:
            _, n_launch = eng.epoch_strata(seq, seed, lr=LR, reg=REG, persistent=persistent,
                                           timing=True)
            assert n_launch == (n_ph if persistent else n_ph * B)
        eng.check_strata()
        out.append(eng.params_numpy())
    _assert_same_bits(out[0], out[1], "item phases")
    orders = [plan.serial_order(seq, seed) for seq, seed in draws]
    ref = _oracle_epochs(d, start, kernel, k, orders, flags)
    if dtype == "float64":
        _assert_fp64_close(out[0], ref)
    else:
        n32 = _numpy_epochs(d, start, kernel, k, orders, flags)
        assert_fp32_close(f"phases32 {kernel} k={k}", out[0], n32, ref, m=M, figure=_figure)
    # delta-out: the replica stays, the deltas carry the epoch's item update
    eng = _engine("dense", dtype, k, kernel)
    eng.prepare_strata(n_blocks=B, waves=16, phases=n_ph)
    dq, dbi = torch.zeros_like(eng.Q), torch.zeros_like(eng.bi)
    seq, seed = draws[0]
    eng.epoch_strata(seq, seed, lr=LR, reg=REG, delta=(dq, dbi))
    eng.check_strata()
    Pd, Qd, bud, bid = eng.params_numpy()
    assert np.array_equal(Qd, start[1].astype(eng.ndt))
    assert np.array_equal(bid, start[3].astype(eng.ndt))
    one = _engine("dense", dtype, k, kernel)
    one.prepare_strata(n_blocks=B, waves=16, phases=n_ph)
    one.epoch_strata(seq, seed, lr=LR, reg=REG)
    Pr, Qr, bur, bir = one.params_numpy()
    assert np.array_equal(Pd, Pr) and np.array_equal(bud, bur)
    # delta = fl(new - old): old + delta is the new value to one rounding
    eps = float(np.finfo(eng.ndt).eps)
    assert maxabs(Qd.astype(np.float64) + dq.cpu().numpy() - Qr) <= 2 * eps * maxabs(Qr)
    assert maxabs(bid.astype(np.float64) + dbi.cpu().numpy() - bir) <= 2 * eps * maxabs(bir)
    assert maxabs(dq.cpu().numpy()) > 1e-4


@gpu
@pytest.mark.parametrize("dtype,k,kernel,shape", PLANNER_CASES)
def test_planner_raises_blocks_until_the_image_fits(mf, dtype, k, kernel, shape):
    """Check 6: fit_epochs(..., "strata") with prepare_strata() left to choose
    everything.  20 000 ratings start at B = 4, whose slabs (100 items; 350 for
    FP32 rank 132) exceed the LDS in all four cases, so choose_strata_blocks
    must raise B; the fit is the oracle's sweep in engine.serial_order of the
    replayed draws."""
    from matrix_factorization import _lib
    from matrix_factorization.engine import fit_epochs, stratum_order

    d = _ratings(shape)
    lib = _lib.load()
    limit = lib.mf_strata_lds_limit()
    assert _planner_image_at_b0(shape, dtype, k) > limit
    start = _params(d["nu"], d["ni"], k, dtype, 100 + k)
    eng = _engine(shape, dtype, k, kernel, start)
    eng.strata_regroup = "auto"
    np.random.seed(k)
    rmse = fit_epochs(eng, 3, "strata", LR, REG)
    eng.check_strata()
    plan = eng.strata
    assert plan.B > PLANNER_B0
    assert lib.mf_strata_lds_bytes(plan.max_items, plan.max_users, k, _dcode(dtype)) <= limit
    if kernel == "linear":
        assert plan.classes == 4 and len(eng._regroups) == 1  # the automatic choices
    np.random.seed(k)
    orders = []
    for _ in range(3):
        seq = stratum_order(np.random, plan)
        seed = int(np.random.randint(0, 2**31 - 1))
        orders.append(eng.serial_order(seq, seed))
        assert np.array_equal(np.sort(orders[-1]), np.arange(len(d["u"])))
    flags = (True, True, True)
    ref = _oracle_epochs(d, start, kernel, k, orders, flags)
    got = eng.params_numpy()
    if dtype == "float64":
        import oracle

        _assert_fp64_close(got, ref)
        P, Q, bu, bi = ref
        ro = oracle.rmse(d["u"], d["i"], d["r"], d["mu"], bu, bi, P, Q, kernel=kernel, **_hyp(k))
        assert abs(rmse[-1] - ro) < 1e-12
    else:
        n32 = _numpy_epochs(d, start, kernel, k, orders, flags)
        assert_fp32_close(f"planner32 {kernel} k={k}", got, n32, ref, m=M, figure=_figure)
