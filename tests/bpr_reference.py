"""NumPy restatement of BPRMF's contract (include/mf_hip.h, "BPR"): the
counter-based negative sampler, the greedy exact levels of triples, the
sequential sweep and the loss -- plus the small planted data set the BPR tests
share.  Not a test module; imported by test_bpr_cpu.py and test_gpu_bpr.py.
"""

import numpy as np

N_USERS, N_ITEMS = 300, 200
U_ALL, U_ALMOST, U_ZERO, U_EMPTY = 296, 297, 298, 299    # the planted users
SEEDS = (0x0123456789ABCDEF, 42, 2 ** 64 - 59)           # sampler seeds of the tests

_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
_POS = np.uint64(0x9E3779B97F4A7C15)
_TRY = np.uint64(0xD1B54A32D192ED03)
ATTEMPTS = 16


def mix(x):
    """splitmix64's finaliser on a uint64 array (wrap-around arithmetic)."""
    x = x ^ (x >> np.uint64(30))
    x = x * _M1
    x = x ^ (x >> np.uint64(27))
    x = x * _M2
    return x ^ (x >> np.uint64(31))


def user_lists(pu, pi, n_users):
    """(ptr int64, ids int32): each user's positive items, ascending."""
    order = np.lexsort((pi, pu))
    ptr = np.zeros(n_users + 1, np.int64)
    np.cumsum(np.bincount(pu, minlength=n_users), out=ptr[1:])
    return ptr, np.ascontiguousarray(pi[order], np.int32)


def sample_negatives(visit, pu, pi, ptr, ids, n_items, seed):
    """neg[t] for every visit position t: the first of 16 candidates
    j(a) = ((mix(mix(seed + (t+1) POS) + (a+1) TRY) >> 32) * n_items) >> 32
    that is neither the triple's positive nor in its user's list; else -1."""
    n = len(visit)
    u = np.asarray(pu)[visit].astype(np.int64)
    i = np.asarray(pi)[visit].astype(np.int64)
    # the lists as one sorted key array: a binary search per candidate
    owner = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    keys = owner * n_items + ids.astype(np.int64)
    out = np.full(n, -1, np.int32)
    open_ = np.ones(n, bool)
    with np.errstate(over="ignore"):
        t1 = np.arange(1, n + 1, dtype=np.uint64)
        base = mix(np.uint64(seed) + t1 * _POS)
        for a in range(ATTEMPTS):
            h = mix(base + np.uint64(a + 1) * _TRY)
            j = (((h >> np.uint64(32)) * np.uint64(n_items)) >> np.uint64(32)).astype(np.int64)
            key = u * n_items + j
            at = np.searchsorted(keys, key)
            member = (at < len(keys)) & (keys[np.minimum(at, len(keys) - 1)] == key) \
                if len(keys) else np.zeros(n, bool)
            ok = open_ & (j != i) & ~member
            out[ok] = j[ok]
            open_ &= ~ok
    return out


def greedy_levels(tu, ti, tj, n_users, n_items, use_user=True, use_item=True):
    """(kept visit positions grouped by level, level offsets): level(t) = 1 +
    max(last level of u, of i, of j), one table for both item roles; j = -1
    dropped."""
    lu = np.zeros(n_users, np.int64)
    li = np.zeros(n_items, np.int64)
    lvl = np.zeros(len(tu), np.int64)
    for t in range(len(tu)):
        u, i, j = tu[t], ti[t], tj[t]
        if j < 0:
            continue
        L = 0
        if use_user:
            L = lu[u]
        if use_item:
            L = max(L, li[i], li[j])
        L += 1
        if use_user:
            lu[u] = L
        if use_item:
            li[i] = li[j] = L
        lvl[t] = L
    kept = np.flatnonzero(lvl > 0)
    nl = int(lvl.max()) if len(lvl) else 0
    sched = kept[np.argsort(lvl[kept], kind="stable")].astype(np.int32)
    offs = np.zeros(nl + 1, np.int64)
    np.cumsum(np.bincount(lvl[kept], minlength=nl + 1)[1:], out=offs[1:])
    return sched, offs


def step(x, yi, yj, bi, bj, lr, reg):
    """One triple's update from the values before it: (z, x', yi', yj', bi',
    bj'), in the dtype of the inputs, in the header's expression order."""
    one = x.dtype.type(1)
    d = yi - yj
    z = x.dot(d) + (bi - bj)
    with np.errstate(over="ignore"):
        g = one / (one + np.exp(z))
    return (z, x + lr * (g * d - reg * x), yi + lr * (g * x - reg * yi),
            yj + lr * (-g * x - reg * yj), bi + lr * (g - reg * bi), bj + lr * (-g - reg * bj))


def sweep(P, Q, b, triples, lr, reg, dtype=np.float64, update_user=True, update_item=True):
    """The sequential sweep over kept triples (u, i, j) in visit order.
    Returns (P, Q, b, z) -- new arrays of ``dtype``; z[t] is triple t's
    pre-update z."""
    dt = np.dtype(dtype).type
    P, Q, b = (np.array(a, dtype=dt) for a in (P, Q, b))
    lr, reg = dt(lr), dt(reg)
    tu, ti, tj = triples
    z = np.zeros(len(tu), dt)
    for t in range(len(tu)):
        u, i, j = tu[t], ti[t], tj[t]
        z[t], x, yi, yj, bi, bj = step(P[u].copy(), Q[i].copy(), Q[j].copy(), b[i], b[j], lr, reg)
        if update_user:
            P[u] = x
        if update_item:
            Q[i], Q[j], b[i], b[j] = yi, yj, bi, bj
    return P, Q, b, z


def objective(x, yi, yj, bi, bj, reg):
    """ln sigmoid(z) - reg/2 (|x|^2 + |yi|^2 + |yj|^2 + bi^2 + bj^2)."""
    z = x.dot(yi - yj) + (bi - bj)
    return -np.logaddexp(0.0, -z) - 0.5 * reg * (x.dot(x) + yi.dot(yi) + yj.dot(yj)
                                                 + bi * bi + bj * bj)


def loss_auc(z):
    """(mean softplus(-z), mean [z > 0]) in FP64; NaN without triples."""
    z = np.asarray(z, np.float64)
    if len(z) == 0:
        return float("nan"), float("nan")
    return float(np.mean(np.logaddexp(0.0, -z))), float(np.mean(z > 0))


def epoch_triples(order, pu, pi, ptr, ids, n_items, seed):
    """The epoch's triples in visit order, skipped ones included (j = -1)."""
    neg = sample_negatives(order, pu, pi, ptr, ids, n_items, seed)
    return np.asarray(pu)[order], np.asarray(pi)[order], neg


def kept(triples):
    keep = triples[2] >= 0
    return tuple(a[keep] for a in triples)


def run_epochs(pu, pi, n_users, n_items, P, Q, b, n_epochs, lr, reg, dtype=np.float64,
               update_item=True):
    """BPR.epoch's loop on the global RandomState: per epoch np.random.shuffle
    of the (persistent) visit order, then one uint64 seed.  Returns (P, Q, b,
    losses, accuracies)."""
    ptr, ids = user_lists(pu, pi, n_users)
    order = np.arange(len(pu), dtype=np.int32)
    losses, accs = [], []
    for _ in range(n_epochs):
        np.random.shuffle(order)
        seed = int(np.random.randint(0, 2 ** 64, dtype=np.uint64))
        tr = kept(epoch_triples(order, pu, pi, ptr, ids, n_items, seed))
        P, Q, b, z = sweep(P, Q, b, tr, lr, reg, dtype, True, update_item)
        lo, ac = loss_auc(z)
        losses.append(lo)
        accs.append(ac)
    return P, Q, b, losses, accs


def make_dataset(seed=7):
    """(u, i, r): 300 users x 200 items, ~3000 positives with skewed item
    popularity.  Users 0..295 hold at most half of the items (and a few r = 0
    observations, which count as unobserved); U_ALL holds all 200 items,
    U_ALMOST 199 of them, U_ZERO only r = 0 observations, U_EMPTY nothing."""
    rs = np.random.RandomState(seed)
    pop = 1.0 / (np.arange(N_ITEMS) + 1.0) ** 0.8
    pop /= pop.sum()
    us, its, rr = [], [], []
    for u in range(U_ALL):
        deg = min(1 + rs.poisson(7.5), N_ITEMS // 2)
        items = rs.choice(N_ITEMS, deg, replace=False, p=pop)
        us += [u] * deg
        its += list(items)
        rr += list(rs.randint(1, 6, deg).astype(np.float64))
        if u % 3 == 0:                                   # an observed pair of strength 0
            free = np.setdiff1d(np.arange(N_ITEMS), items)
            us.append(u)
            its.append(int(rs.choice(free)))
            rr.append(0.0)
    us += [U_ALL] * N_ITEMS
    its += list(range(N_ITEMS))
    rr += [1.0] * N_ITEMS
    hole = 57
    us += [U_ALMOST] * (N_ITEMS - 1)
    its += [x for x in range(N_ITEMS) if x != hole]
    rr += [2.0] * (N_ITEMS - 1)
    us += [U_ZERO] * 5
    its += [3, 50, 99, 120, 199]
    rr += [0.0] * 5
    p = rs.permutation(len(us))
    return (np.asarray(us, np.int32)[p], np.asarray(its, np.int32)[p],
            np.asarray(rr, np.float64)[p])


LR, REG = 0.05, 0.01


def epoch_case(k, seed=SEEDS[0]):
    """The fixed one-epoch case of the tests at rank k: visit order, triples
    (skipped included) and initial parameters on the planted set."""
    u, i, r = make_dataset()
    pu, pi = positives(u, i, r)
    ptr, ids = user_lists(pu, pi, N_USERS)
    order = np.random.RandomState(3).permutation(len(pu)).astype(np.int32)
    rs = np.random.RandomState(100 + k)
    P = rs.normal(0, 0.1, (N_USERS, k))
    Q = rs.normal(0, 0.1, (N_ITEMS, k))
    b = rs.normal(0, 0.1, N_ITEMS)
    return dict(u=u, i=i, r=r, pu=pu, pi=pi, ptr=ptr, ids=ids, order=order, P=P, Q=Q, b=b,
                triples=epoch_triples(order, pu, pi, ptr, ids, N_ITEMS, seed))


def positives(u, i, r):
    keep = r > 0
    return np.ascontiguousarray(u[keep]), np.ascontiguousarray(i[keep])
