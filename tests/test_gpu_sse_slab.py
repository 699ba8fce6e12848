"""The item-stationary training-RMSE pass (mf_sse_slab, k_sse_slab: item rows
in LDS, user rows gathered; MF_SSE_SLAB=1) against the default pass
(k_sse_lean) and the FP64 oracle.  Per rating the arithmetic is the default
pass's; the FP64 sums differ only in accumulation order, so the two passes
agree to 1e-12 relative and with the oracle to 1e-9 relative (the tolerances
of test_gpu_sse.py), and bit for bit where every product and sum is exact."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(64, 20000, 4000, 600000),
          (64, 300, 5000, 200000),        # fewer users than lanes' worth per window
          (20, 5000, 3000, 300000)]       # row tails


@functools.lru_cache(maxsize=None)
def _data(k, nu, ni, nnz):
    rs = np.random.RandomState(k + nu)
    keys = rs.choice(nu * ni, nnz, replace=False)
    u = (keys // ni).astype(np.int32)
    i = (keys % ni).astype(np.int32)
    r = rs.randint(1, 6, nnz).astype(np.float32)
    P = rs.normal(0, 0.3, (nu, k)).astype(np.float32)
    Q = rs.normal(0, 0.3, (ni, k)).astype(np.float32)
    bu = rs.normal(0, 0.1, nu).astype(np.float32)
    bi = rs.normal(0, 0.1, ni).astype(np.float32)
    for a in (u, i, r, P, Q, bu, bi):
        a.setflags(write=False)
    return u, i, r, P, Q, bu, bi


@functools.lru_cache(maxsize=None)
def _oracle_sse(k, nu, ni, nnz, kernel):
    import oracle

    u, i, r, P, Q, bu, bi = _data(k, nu, ni, nnz)
    rbf = kernel == "rbf"
    return oracle.sse(u, i, r.astype(np.float64), float(r.mean()),
                      np.zeros(nu) if rbf else bu.astype(np.float64),
                      np.zeros(ni) if rbf else bi.astype(np.float64), P.astype(np.float64),
                      Q.astype(np.float64), kernel=kernel, gamma=1.0 / k, min_rating=1,
                      max_rating=5)


def _slab_env(monkeypatch, on, windows=None, lds=None):
    monkeypatch.setenv("MF_SSE_SLAB", "1" if on else "0")
    for name, v in (("MF_SSE_SLAB_W", windows), ("MF_SSE_SLAB_LDS", lds)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    for name in ("MF_SSE_SLAB_PAD", "MF_SSE_SLAB_WAVES", "MF_SSE_SLAB_SETS", "MF_SSE_BESIDE",
                 "MF_SSE_VARIANT"):
        monkeypatch.delenv(name, raising=False)


def _engine(u, i, r, P, Q, bu, bi, nu, ni, kernel, dtype, mean=None):
    from matrix_factorization.engine import SGDEngine

    k = P.shape[1]
    eng = SGDEngine(u, i, r.astype(dtype), nu, ni, k, kernel, dtype, "cuda:0", gamma=1.0 / k,
                    global_mean=float(r.mean()) if mean is None else mean, min_rating=1,
                    max_rating=5)
    eng.load_params(P.astype(dtype), Q.astype(dtype), bu.astype(dtype), bi.astype(dtype))
    return eng


def _sse(eng, slot=0):
    eng.sse_async(slot)
    return eng.sse_values(slot + 1)[slot]


def _small_budget(eng, ni, k, dtype):
    """An LDS budget that makes the item groups at least 1.5 x the workgroup
    count, i.e. two phases or more."""
    size = 4 if dtype == "float32" else 8
    return (k + 1) * size * max(1, ni // (eng._cus() + eng._cus() // 2))


# the sigmoid and rbf cases in FP64: an FP32 exp rounds each prediction to
# ~6e-8 relative, so no FP32 pass (the default one included) can meet the
# oracle to 1e-9 there
CASES = [(s, dt, "linear") for s in SHAPES for dt in ("float64", "float32")] + \
        [(SHAPES[0], "float64", "sigmoid"), (SHAPES[2], "float64", "rbf")]


@pytest.mark.parametrize("shape,dtype,kernel", CASES)
def test_slab_pass_agrees_with_default_and_oracle(shape, dtype, kernel, monkeypatch):
    k, nu, ni, nnz = shape
    u, i, r, P, Q, bu, bi = _data(*shape)
    if kernel == "rbf":                                  # (rbf has no biases)
        bu, bi = np.zeros_like(bu), np.zeros_like(bi)
    _slab_env(monkeypatch, False)
    eng = _engine(u, i, r, P, Q, bu, bi, nu, ni, kernel, dtype)
    assert eng.slab is None
    base = _sse(eng)
    ref = _oracle_sse(*shape, kernel)
    print(f"default pass {base!r} oracle {ref!r} rel {abs(base - ref) / ref:.3e}")
    assert abs(base - ref) <= 1e-9 * ref
    for windows, small in ((1, False), (5, True), (1, True), (5, False)):
        _slab_env(monkeypatch, True, windows, _small_budget(eng, ni, k, dtype) if small else None)
        eng._build_eval()
        assert eng.slab is not None and eng.slab["windows"] == windows
        if small:
            assert eng.slab["groups"] >= 2 * eng._cus() and eng.slab["phases"] >= 2
        got = _sse(eng, 1)
        print(f"W={windows} groups={eng.slab['groups']} phases={eng.slab['phases']} slab {got!r} "
              f"rel to default {abs(got - base) / base:.3e} to oracle {abs(got - ref) / ref:.3e}")
        assert abs(got - base) <= 1e-12 * base, (got, base)
        assert abs(got - ref) <= 1e-9 * ref, (got, ref)


def _exact_data(nu, ni, nnz, k, seed, items=None):
    """Parameters in {-1, -0.5, 0, 0.5, 1}, biases multiples of 0.25, integer
    ratings: every product, error and partial sum is exact in FP32 and FP64."""
    rs = np.random.RandomState(seed)
    keys = rs.choice(nu * ni, nnz, replace=False)
    u = (keys // ni).astype(np.int32)
    i = (keys % ni).astype(np.int32)
    if items is not None:
        i = items[i % len(items)].astype(np.int32)
    r = rs.randint(1, 6, nnz).astype(np.float32)
    P = (rs.randint(-2, 3, (nu, k)) * 0.5).astype(np.float32)
    Q = (rs.randint(-2, 3, (ni, k)) * 0.5).astype(np.float32)
    bu = (rs.randint(-4, 5, nu) * 0.25).astype(np.float32)
    bi = (rs.randint(-4, 5, ni) * 0.25).astype(np.float32)
    return u, i, r, P, Q, bu, bi


def _exact_check(monkeypatch, dtype, nu, ni, nnz, k, windows, small, items=None, seed=3):
    import oracle

    u, i, r, P, Q, bu, bi = _exact_data(nu, ni, nnz, k, seed, items)
    _slab_env(monkeypatch, False)
    eng = _engine(u, i, r, P, Q, bu, bi, nu, ni, "linear", dtype, mean=3.0)
    base = _sse(eng)
    ref = oracle.sse(u, i, r.astype(np.float64), 3.0, bu.astype(np.float64),
                     bi.astype(np.float64), P.astype(np.float64), Q.astype(np.float64))
    _slab_env(monkeypatch, True, windows, _small_budget(eng, ni, k, dtype) if small else None)
    eng._build_eval()
    assert eng.slab is not None
    got = _sse(eng, 1)
    print(f"slab {got!r} default {base!r} oracle {ref!r} groups={eng.slab['groups']}")
    assert got == base == ref, (got, base, ref)
    return eng


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("k,nu,ni,nnz,windows,small",
                         [(64, 20000, 4000, 600000, 5, True), (20, 5000, 3000, 300000, 1, False)])
def test_slab_pass_exact_sums_are_bit_equal(dtype, k, nu, ni, nnz, windows, small, monkeypatch):
    """Catches a dropped or doubled rating that a 1e-12 tolerance could hide."""
    _exact_check(monkeypatch, dtype, nu, ni, nnz, k, windows, small)


@pytest.mark.parametrize("name,nu,ni,nnz,windows,small,items", [
    # only every 16th item is rated: item groups (and cells) with no ratings
    ("empty_groups", 3000, 4000, 60000, 5, True, np.arange(0, 4000, 16)),
    # few ratings against 512 groups x 7 windows: most (group, window) cells are empty
    ("empty_cells", 5000, 4099, 900, 7, True, None),
    # n_items not divisible by the group count (a prime)
    ("ni_not_divisible", 4000, 4099, 200000, 5, True, None),
    # fewer items than workgroups
    ("ni_100", 20000, 100, 300000, 5, False, None),
    # fewer users than windows
    ("nu_below_windows", 3, 5000, 9000, 5, False, None),
    # every rating on one item
    ("one_item", 30000, 3000, 20000, 5, True, np.array([1234])),
])
def test_slab_pass_edge_cases(name, nu, ni, nnz, windows, small, items, monkeypatch):
    if name == "one_item":
        # distinct users for the one item
        nnz = min(nnz, nu)
    eng = _exact_check(monkeypatch, "float64", nu, ni, nnz, 24, windows, small, items,
                       seed=len(name))
    if name == "ni_100":
        assert eng.slab["items"] == 1 and eng.slab["groups"] >= 100


def test_slab_pass_is_deterministic_and_read_only(monkeypatch):
    k, nu, ni, nnz = SHAPES[0]
    u, i, r, P, Q, bu, bi = _data(*SHAPES[0])
    _slab_env(monkeypatch, True, 5)
    eng = _engine(u, i, r, P, Q, bu, bi, nu, ni, "linear", "float32")
    assert eng.slab is not None
    a, b = _sse(eng, 0), _sse(eng, 1)
    assert a == b
    for t, h in ((eng.P, P), (eng.Q, Q), (eng.bu, bu), (eng.bi, bi)):
        assert np.array_equal(t.cpu().numpy().reshape(h.shape), h)


def test_slab_selection(monkeypatch):
    """With the environment unset a C2-sized and a tiny engine keep the
    default pass; MF_SSE_SLAB=0 is today's pass bit for bit."""
    from matrix_factorization.engine import SGDEngine, sse_slab_selected

    for name in ("MF_SSE_SLAB", "MF_SSE_BESIDE"):
        monkeypatch.delenv(name, raising=False)
    assert not sse_slab_selected("float32", 5_000_000, 100_000, 10_000, 32)       # C2
    assert not sse_slab_selected("float64", 5_000_000, 100_000, 10_000, 32)
    assert not sse_slab_selected("float64", 12_500_000, 125_000, 100_000, 64)     # c3_shard8
    assert not sse_slab_selected("float64", 1000, 50, 40, 8)
    k, nu, ni, nnz = SHAPES[2]
    u, i, r, P, Q, bu, bi = _data(*SHAPES[2])
    eng = _engine(u, i, r, P, Q, bu, bi, nu, ni, "linear", "float64")
    assert eng.slab is None and eng.eval_offs is not None
    unset = _sse(eng)
    rs = np.random.RandomState(0)
    nc = 5_000_000
    uc = rs.randint(0, 100_000, nc).astype(np.int32)
    ic = rs.randint(0, 10_000, nc).astype(np.int32)
    c2 = SGDEngine(uc, ic, np.ones(nc, np.float32), 100_000, 10_000, 32, "sigmoid", "float32",
                   "cuda:0")
    assert c2.slab is None and c2.eval_offs is not None
    monkeypatch.setenv("MF_SSE_SLAB", "0")
    eng0 = _engine(u, i, r, P, Q, bu, bi, nu, ni, "linear", "float64")
    assert eng0.slab is None
    assert np.array_equal(eng0.eval_offs, eng.eval_offs)
    assert np.array_equal(eng0.eu.cpu().numpy(), eng.eu.cpu().numpy())
    assert _sse(eng0) == unset
    monkeypatch.setenv("MF_SSE_SLAB", "1")
    monkeypatch.setenv("MF_SSE_BESIDE", "1")
    eng1 = _engine(u, i, r, P, Q, bu, bi, nu, ni, "linear", "float64")
    assert eng1.slab is not None and not eng1.beside_active
