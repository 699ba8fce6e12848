"""GPU tests of DeviceModel built directly (no ratings, no SGDEngine): its
predict against the CPU oracle, its top-k and rank against the NumPy
restatement of tests/test_gpu_rank.py, exclusion CSRs that do not start at 0,
and that the serving paths of the estimators hold a DeviceModel and no
training state.

Predict bounds: the rule of tests/test_gpu_row_layouts.py (its module
docstring), the suite's only predict-against-oracle tolerance.  FP64: 1e-12.
FP32: inputs rounded through float32, the GPU within M d32 + 4 eps32 max|ref|
of the FP64 oracle, d32 being the deviation of a plain NumPy float32
evaluation from the same oracle.  Everything else here is exact."""

import pickle

import numpy as np
import pandas as pd
import pytest

import ranking_reference as rr
from row_layouts_reference import EPS32, maxabs
from test_gpu_rank import check, csr, scores_of
from test_gpu_row_layouts import M, numpy_predict

pytestmark = pytest.mark.gpu

NU, NI, NQ = 60, 80, 7
MU, GAMMA, LO, HI = 3.5, 0.7, 1.0, 5.0


def make_model(kernel, k, dtype, seed=0):
    from matrix_factorization.device_model import DeviceModel

    rs = np.random.RandomState(1000 * seed + 10 * k + len(kernel))
    params = [rs.normal(0, 0.3, (NU, k)), rs.normal(0, 0.3, (NI, k)), rs.normal(0, 0.1, NU),
              rs.normal(0, 0.1, NI)]
    if dtype == "float32":
        params = [a.astype(np.float32).astype(np.float64) for a in params]
    m = DeviceModel(NU, NI, k, kernel, dtype, "cuda:0", gamma=GAMMA, min_rating=LO,
                    max_rating=HI, global_mean=MU)
    if kernel == "bias":
        m.load_params(bu=params[2], bi=params[3])
    else:
        m.load_params(*params)
    return m, params


def queries(seed):
    """7 query users (one unknown), targets and unsorted exclusion lists with
    repeats and out-of-range ids; one target is excluded itself."""
    rs = np.random.RandomState(seed)
    users = rs.choice(NU, NQ, replace=False).astype(np.int32)
    users[4] = -1
    tgt = [rs.randint(0, NI, rs.randint(0, 5)).tolist() for _ in range(NQ)]
    tgt[2] = [7, 7, NI, -1, 30]
    ex = [rs.randint(-2, NI + 2, rs.randint(0, 6)).tolist() for _ in range(NQ)]
    ex[2].append(30)
    ex[5] = []
    return users, tgt, ex


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("k", [8, 33])
@pytest.mark.parametrize("kernel", ["linear", "sigmoid", "rbf"])
def test_scoring_matches_the_references(kernel, k, dtype):
    import oracle

    m, (P, Q, bu, bi) = make_model(kernel, k, dtype)
    rs = np.random.RandomState(k)
    u = rs.randint(0, NU, 300).astype(np.int32)
    i = rs.randint(0, NI, 300).astype(np.int32)
    u[::41] = -1
    i[::37] = -1
    for bound in (True, False):
        got = m.predict(u, i, bound)
        ref = oracle.predict(u, i, MU, bu, bi, P, Q, kernel=kernel, gamma=GAMMA, min_rating=LO,
                             max_rating=HI, bound=bound)
        dev = maxabs(got - ref)
        if dtype == "float64":
            print(f"DEVICEMODEL predict64 {kernel} k={k} bound={int(bound)} gpu={dev:.3e}")
            assert dev <= 1e-12, f"bound={bound}: max |diff| {dev:.3e}"
            continue
        n32 = numpy_predict(u, i, MU, bu, bi, P, Q, kernel, GAMMA, LO, HI, "float32", bound)
        d32, scale = maxabs(n32 - ref), maxabs(ref)
        print(f"DEVICEMODEL predict32 {kernel} k={k} bound={int(bound)} d32={d32:.3e} "
              f"gpu={dev:.3e}")
        assert M * d32 <= 1e-4 * scale
        assert dev <= M * d32 + 4 * EPS32 * scale, \
            f"bound={bound}: max |diff| {dev:.3e} > {M} * {d32:.3e} + 4 eps32 * {scale:.3g}"

    users, tgt, ex = queries(k)
    ep, ei = csr(ex)
    scores = scores_of(m, users)
    m.topk_mfma = False                          # the exact path: fused, then two-stage
    for amount in (10, 65):
        ids, sc = m.topk(users, amount, ep, ei)
        assert ids.shape == sc.shape == (NQ, amount)
        for q in range(NQ):
            gone = {x for x in ex[q] if 0 <= x < NI}
            order = [j for j in np.argsort(~rr.order_key(scores[q]), kind="stable")
                     if j not in gone][:amount]          # at least 74 candidates remain
            assert ids[q].tolist() == order, f"amount {amount}, query {q}"
            assert np.array_equal(sc[q], scores[q][order]), f"amount {amount}, query {q}"
    ranks, _ = check(m, users, tgt, ex)
    assert ranks[ranks >= 0].size and (ranks == -1).sum() >= 3
    check(m, users, tgt)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_bias_model_predicts_and_refuses_ranking(dtype):
    m, (_, _, bu, bi) = make_model("bias", 0, dtype)
    assert m.bias_only and m.P is None and m.Q is None
    rs = np.random.RandomState(3)
    u = rs.randint(-1, NU, 200).astype(np.int32)
    i = rs.randint(-1, NI, 200).astype(np.int32)
    raw = MU + np.where(u >= 0, bu[u], 0.0) + np.where(i >= 0, bi[i], 0.0)
    # FP32: two additions of values below HI, each rounded by at most eps32 / 2 of it;
    # 4 eps32 max|ref| is the suite's FP32 term (tests/row_layouts_reference.py)
    tol = 1e-12 if dtype == "float64" else 4 * EPS32 * HI
    assert maxabs(m.predict(u, i, False) - raw) <= tol
    assert maxabs(m.predict(u, i, True) - np.clip(raw, LO, HI)) <= tol
    with pytest.raises(NotImplementedError):
        m.topk(np.zeros(1, np.int32), 3)
    with pytest.raises(NotImplementedError):
        m.rank(np.zeros(1, np.int32), np.array([0, 1]), np.zeros(1, np.int32))


@pytest.mark.parametrize("mfma", ["1", "0"])
def test_offset_exclusions_equal_the_rebased_csr(mfma, monkeypatch):
    """An ex_ptr that starts at 3 (three leading junk items, two trailing)
    gives the arrays of the same CSR rebased by hand, bit for bit."""
    monkeypatch.setenv("MF_TOPK_MFMA", mfma)
    m, _ = make_model("linear", 8, "float32")
    users, _, ex = queries(5)
    for q, best in enumerate(np.argmax(scores_of(m, users), axis=1)):
        ex[q].append(int(best))                  # every list changes its user's result
    ptr, items = csr(ex)
    off_items = np.concatenate([[1, 2, 3], items, [4, 5]]).astype(np.int32)
    assert bool(m.topk_prepare(users, 10, ptr + 3, off_items)["mm"]) == (mfma == "1")
    for amount in (10, 65):
        want = m.topk(users, amount, ptr, items)
        got = m.topk(users, amount, ptr + 3, off_items)
        assert np.array_equal(got[0], want[0])
        assert np.array_equal(got[1], want[1], equal_nan=True)
        assert not np.array_equal(want[0], m.topk(users, amount)[0])     # the lists matter
    tp, ti = csr([[1, 2]] * NQ)
    want, got = m.rank(users, tp, ti, ptr, items), m.rank(users, tp, ti, ptr + 3, off_items)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


TRAINING_STATE = ("ws", "sse_buf", "eu", "strata")


def small_frame(seed=4):
    rs = np.random.RandomState(seed)
    pairs = np.unique(np.stack([rs.randint(0, NU, 900), rs.randint(0, NI, 900)], 1), axis=0)
    X = pd.DataFrame({"user_id": pairs[:, 0] + 100, "item_id": pairs[:, 1] + 500})
    y = pd.Series(rs.randint(1, 6, len(X)).astype(np.float64))
    feats = pd.DataFrame(rs.normal(0, 1, (NI, 6)), columns=[f"f{j}" for j in range(6)])
    feats.insert(0, "item_id", np.arange(NI) + 500)
    return X, y, feats


def test_a_bare_model_holds_no_training_state():
    from matrix_factorization.device_model import DeviceModel
    from matrix_factorization.engine import SGDEngine

    m, _ = make_model("linear", 8, "float32")
    assert type(m) is DeviceModel
    for name in TRAINING_STATE:
        assert not hasattr(m, name), name
    eng = SGDEngine(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), NU, NI, 8,
                    "linear", "float32", "cuda:0")
    for name in TRAINING_STATE:
        assert hasattr(eng, name), name


def test_serving_paths_hold_a_device_model():
    from matrix_factorization import ContentBasedRecommender, HybridRecommender, KernelMF
    from matrix_factorization.device_model import DeviceModel
    from matrix_factorization.engine import SGDEngine

    X, y, feats = small_frame()
    cb = ContentBasedRecommender(scoring="cosine").fit(X, y, item_features=feats)
    assert type(cb._ranking_backend()) is DeviceModel
    hy = HybridRecommender(model=None, candidate_k=20).fit(X, feats)
    assert type(hy._retrieval_engine()) is DeviceModel
    np.random.seed(2)
    mf = KernelMF(n_factors=8, n_epochs=2, verbose=0).fit(X, y)
    assert type(mf._predictor()) is SGDEngine            # the training engine is kept
    loaded = pickle.loads(pickle.dumps(mf))
    assert type(loaded._predictor()) is DeviceModel
    for name in TRAINING_STATE:
        assert not hasattr(loaded._predictor(), name), name
    assert loaded.predict(X) == mf.predict(X)
