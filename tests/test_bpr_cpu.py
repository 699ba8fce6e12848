"""CPU tests of BPR's host side: mf_sched_levels3 against the NumPy reference
(tests/bpr_reference.py) and the reference itself (gradient, sampler
properties, learning on the planted set).  No GPU: the library loads without a
device."""

import ctypes

import numpy as np
import pytest

import bpr_reference as ref


# ---------------------------------------------------------------- helpers
def levels3(tu, ti, tj, n_users, n_items, use_user=True, use_item=True, n_chunks=1):
    from matrix_factorization.engine import sched_levels3

    return sched_levels3(tu, ti, tj, n_users, n_items, use_user, use_item, n_chunks)


@pytest.fixture(scope="module")
def data():
    u, i, r = ref.make_dataset()
    pu, pi = ref.positives(u, i, r)
    ptr, ids = ref.user_lists(pu, pi, ref.N_USERS)
    return dict(u=u, i=i, r=r, pu=pu, pi=pi, ptr=ptr, ids=ids)


@pytest.fixture(scope="module")
def triples(data):
    """One epoch's triples in visit order (skipped ones included)."""
    rs = np.random.RandomState(3)
    order = rs.permutation(len(data["pu"])).astype(np.int32)
    return ref.epoch_triples(order, data["pu"], data["pi"], data["ptr"], data["ids"],
                             ref.N_ITEMS, ref.SEEDS[0])


def check_schedule(tu, ti, tj, sched, offs, use_user=True, use_item=True):
    """Conflict-free levels whose order respects the visit order of every row."""
    keep = np.flatnonzero(tj >= 0)
    assert sorted(sched.tolist()) == keep.tolist()              # each kept triple once
    assert offs[0] == 0 and offs[-1] == len(sched) and np.all(np.diff(offs) >= 0)
    level_of = np.zeros(len(tu), np.int64)
    for L in range(len(offs) - 1):
        pos = sched[offs[L]:offs[L + 1]]
        assert np.all(np.diff(pos) > 0)                          # a level is in visit order
        level_of[pos] = L + 1
        if use_user:
            assert len(set(tu[pos].tolist())) == len(pos)
        if use_item:
            items = np.concatenate([ti[pos], tj[pos]])           # both roles together
            assert len(set(items.tolist())) == len(items)
    last_u, last_i = {}, {}
    for t in keep:
        rows = ([("u", tu[t])] if use_user else []) + \
               ([("i", ti[t]), ("i", tj[t])] if use_item else [])
        for kind, x in rows:
            tab = last_u if kind == "u" else last_i
            assert level_of[t] > tab.get(x, 0)                   # above every earlier sharer
        for kind, x in rows:
            (last_u if kind == "u" else last_i)[x] = level_of[t]


# --------------------------------------------------------- mf_sched_levels3
def test_levels3_one_chunk_is_the_greedy_schedule(triples):
    tu, ti, tj = triples
    sched, offs = levels3(tu, ti, tj, ref.N_USERS, ref.N_ITEMS)
    rs, ro = ref.greedy_levels(tu, ti, tj, ref.N_USERS, ref.N_ITEMS)
    assert np.array_equal(sched, rs) and np.array_equal(offs, ro)
    check_schedule(tu, ti, tj, sched, offs)
    assert np.any(tj < 0)                                        # the set has skipped triples
    # the depth is at least the largest degree of a row among the kept triples
    keep = tj >= 0
    deg_u = np.bincount(tu[keep]).max()
    deg_i = np.bincount(np.concatenate([ti[keep], tj[keep]])).max()
    assert len(offs) - 1 >= max(deg_u, deg_i)


@pytest.mark.parametrize("n_chunks", [2, 4, 7])
def test_levels3_chunks_are_valid_exact_schedules(triples, n_chunks):
    tu, ti, tj = triples
    sched, offs = levels3(tu, ti, tj, ref.N_USERS, ref.N_ITEMS, n_chunks=n_chunks)
    check_schedule(tu, ti, tj, sched, offs)
    g_sched, g_offs = levels3(tu, ti, tj, ref.N_USERS, ref.N_ITEMS, n_chunks=1)
    assert len(offs) >= len(g_offs)
    # chunk c's kept triples fill their own contiguous range, in chunk order
    n = len(tu)
    bounds = [n * c // n_chunks for c in range(n_chunks + 1)]
    chunk_of = np.searchsorted(bounds, sched, side="right") - 1
    assert np.all(np.diff(chunk_of) >= 0)


def test_levels3_item_in_both_roles_conflicts():
    # item 1 is the negative of triple 0 and the positive of triple 1
    tu = np.array([0, 1, 2], np.int32)
    ti = np.array([0, 1, 3], np.int32)
    tj = np.array([1, 2, 4], np.int32)
    sched, offs = levels3(tu, ti, tj, 3, 5)
    assert offs.tolist() == [0, 2, 3] and sched.tolist() == [0, 2, 1]


def test_levels3_drops_skipped_triples():
    tu = np.array([0, 0, 1, 1], np.int32)
    ti = np.array([0, 1, 0, 2], np.int32)
    tj = np.array([3, -1, -1, 3], np.int32)
    sched, offs = levels3(tu, ti, tj, 2, 4)
    assert sched.tolist() == [0, 3] and offs.tolist() == [0, 1, 2]
    # a skipped triple does not raise its rows' levels: all skipped -> no level
    sched, offs = levels3(tu, ti, np.full(4, -1, np.int32), 2, 4)
    assert len(sched) == 0 and offs.tolist() == [0]


def test_levels3_frozen_items_level_by_user_only(triples):
    tu, ti, tj = triples
    sched, offs = levels3(tu, ti, tj, ref.N_USERS, ref.N_ITEMS, use_item=False)
    rs, ro = ref.greedy_levels(tu, ti, tj, ref.N_USERS, ref.N_ITEMS, use_item=False)
    assert np.array_equal(sched, rs) and np.array_equal(offs, ro)
    check_schedule(tu, ti, tj, sched, offs, use_item=False)
    keep = tj >= 0
    assert len(offs) - 1 == np.bincount(tu[keep]).max()          # the largest user degree


@pytest.mark.parametrize("bad", [
    dict(u=5), dict(u=-1), dict(i=9), dict(i=-1), dict(j=9), dict(j=-2), dict(j="i"),
])
def test_levels3_rejects_bad_ids(bad):
    from matrix_factorization import _lib

    tu = np.array([0, 1], np.int32)
    ti = np.array([0, 1], np.int32)
    tj = np.array([2, 3], np.int32)
    if "u" in bad:
        tu[1] = bad["u"]
    if "i" in bad:
        ti[1] = bad["i"]
    if "j" in bad:
        tj[1] = ti[1] if bad["j"] == "i" else bad["j"]
    with pytest.raises(_lib.MFLibraryError, match="triple 1"):
        levels3(tu, ti, tj, 5, 9)


def test_levels3_empty_and_bad_arguments():
    from matrix_factorization import _lib

    e = np.zeros(0, np.int32)
    sched, offs = levels3(e, e, e, 0, 0)
    assert len(sched) == 0 and offs.tolist() == [0]
    lib = _lib.load()
    nl, kept = ctypes.c_int32(), ctypes.c_int64()
    offs = np.zeros(4, np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.mf_sched_levels3(None, None, None, -1, 1, 1, 1, 1, 1, None, p(offs), 4,
                                ctypes.byref(nl), ctypes.byref(kept)) == 1
    # a level table too small for the levels: MF_ERR_CAPACITY
    tu = np.zeros(3, np.int32)
    ti = np.array([0, 1, 2], np.int32)
    tj = np.array([3, 3, 3], np.int32)
    out = np.zeros(3, np.int32)
    assert lib.mf_sched_levels3(p(tu), p(ti), p(tj), 3, 1, 4, 1, 1, 1, p(out), p(offs), 2,
                                ctypes.byref(nl), ctypes.byref(kept)) == _lib.MF_ERR_CAPACITY


# ------------------------------------------------------------ the reference
def test_reference_update_is_the_gradient_of_its_objective():
    """(new - old) / lr equals a central finite-difference gradient of the
    per-triple objective to 1e-6 relative."""
    rs = np.random.RandomState(11)
    k, lr, reg, h = 6, 0.05, 0.03, 1e-5
    x, yi, yj = rs.normal(0, 0.7, (3, k))
    bi, bj = rs.normal(0, 0.5, 2)
    _, nx, nyi, nyj, nbi, nbj = ref.step(x, yi, yj, bi, bj, lr, reg)
    got = np.concatenate([(nx - x) / lr, (nyi - yi) / lr, (nyj - yj) / lr,
                          [(nbi - bi) / lr, (nbj - bj) / lr]])
    theta = np.concatenate([x, yi, yj, [bi, bj]])

    def f(th):
        return ref.objective(th[:k], th[k:2 * k], th[2 * k:3 * k], th[3 * k], th[3 * k + 1], reg)

    fd = np.zeros_like(theta)
    for c in range(len(theta)):
        e = np.zeros_like(theta)
        e[c] = h
        fd[c] = (f(theta + e) - f(theta - e)) / (2 * h)
    assert np.max(np.abs(got - fd)) <= 1e-6 * np.max(np.abs(fd))


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_sampler_properties(data, seed):
    pu, pi, ptr, ids = data["pu"], data["pi"], data["ptr"], data["ids"]
    rs = np.random.RandomState(5)
    order = rs.permutation(len(pu)).astype(np.int32)
    tu, ti, tj = ref.epoch_triples(order, pu, pi, ptr, ids, ref.N_ITEMS, seed)
    pos = set(zip(pu.tolist(), pi.tolist()))
    keep = tj >= 0
    assert np.all(tj[keep] < ref.N_ITEMS)
    assert not any((u, j) in pos for u, j in zip(tu[keep].tolist(), tj[keep].tolist()))
    assert np.all(tj != ti)
    # r = 0 observations count as unobserved: they may be drawn
    # deterministic in (seed, t): the same call again, and a prefix of the
    # visit order gives the same integers at the same positions
    again = ref.sample_negatives(order, pu, pi, ptr, ids, ref.N_ITEMS, seed)
    assert np.array_equal(again, tj)
    half = ref.sample_negatives(order[:1000], pu, pi, ptr, ids, ref.N_ITEMS, seed)
    assert np.array_equal(half, tj[:1000])
    other = ref.sample_negatives(order, pu, pi, ptr, ids, ref.N_ITEMS, seed ^ 1)
    assert not np.array_equal(other, tj)
    # the condition the GPU tests rest on: skips only for the saturated users
    assert set(tu[~keep].tolist()) <= {ref.U_ALL, ref.U_ALMOST}
    assert np.all(tj[tu == ref.U_ALL] == -1)
    assert np.mean(tj[tu == ref.U_ALMOST] == -1) > 0.5
    assert not np.any(np.isin(tu, [ref.U_ZERO, ref.U_EMPTY]))


def test_dataset_shape(data):
    pu, pi = data["pu"], data["pi"]
    assert 2500 <= len(pu) <= 3500
    deg = np.bincount(pu, minlength=ref.N_USERS)
    assert deg[:ref.U_ALL].max() <= ref.N_ITEMS // 2
    assert deg[ref.U_ALL] == 200 and deg[ref.U_ALMOST] == 199
    assert deg[ref.U_ZERO] == 0 and deg[ref.U_EMPTY] == 0
    assert np.sum(data["u"] == ref.U_ZERO) == 5 and np.sum(data["u"] == ref.U_EMPTY) == 0
    ipop = np.sort(np.bincount(pi[pu < ref.U_ALL], minlength=ref.N_ITEMS))[::-1]
    assert ipop[:20].sum() > 3 * ipop[-20:].sum()                # skewed popularity


def test_reference_learns_on_the_planted_set(data):
    rs = np.random.RandomState(2)
    k = 8
    P = rs.normal(0, 0.1, (ref.N_USERS, k))
    Q = rs.normal(0, 0.1, (ref.N_ITEMS, k))
    b = np.zeros(ref.N_ITEMS)
    state = np.random.get_state()
    try:
        np.random.seed(4)
        _, _, _, loss, acc = ref.run_epochs(data["pu"], data["pi"], ref.N_USERS, ref.N_ITEMS,
                                            P, Q, b, 5, 0.05, 0.01)
    finally:
        np.random.set_state(state)
    # the loss falls epoch by epoch; the accuracy is a count over ~2600 freshly
    # sampled triples (+-0.01 of sampling noise per epoch once it has
    # saturated), so it is held to "higher after 5 epochs than after the first"
    assert all(b < a for a, b in zip(loss, loss[1:])), loss
    assert acc[-1] > acc[0], acc
    assert loss[0] < np.log(2)                # z starts near 0: softplus(0) = ln 2
