// mf_rank.hip -- exact rank of held-out items among a user's candidates:
// out_rank[t] = number of candidate items that come before target t in
// mf_topk's order (score descending, item id ascending, NaN last).  Every
// top-k metric (precision / recall / NDCG / MAP / MRR at any k) and AUC is a
// function of these ranks, so no list is selected and no score is stored.
//
// Pass 1 (k_rank_targets): a wave per query scores the query's targets
//   (mf_score.hpp: mf_predict's value) and writes (order key, item id) per target; a target
//   out of range or in the query's exclusion list gets the never-counted
//   sentinel and rank -1.  out_candidates[q] starts at n_items.
// Pass 2 (k_rank_count): workgroup (user block x, item split y).  The rows of
//   NU users stay in registers, the four waves stream the split's item rows.
//   Lane l of a lane group holds target seg * GS + l of each user, so a score
//   (bit-identical in the GS lanes of its group after group_sum) meets GS
//   targets in one compare per user; each lane counts the items that come
//   before its target.  Exclusions are ignored here.  A user with more than
//   GS targets takes further passes over the split (segments).  Counts of the
//   groups are summed by shuffles, those of waves and splits by integer
//   atomics: order-independent, so the result does not depend on the grid.
// Pass 3 (k_rank_exclude): a workgroup per query scores the query's distinct
//   in-range excluded items once more and takes them out again: -1 on every
//   target they came before, -1 on out_candidates.  ~100 excluded items
//   against 10^5 scored ones per user: cheaper than a list search per score.
#include <algorithm>

#include "mf_score.hpp"
#include "mf_order.hpp"

namespace mf {

struct RankTarget { uint64_t key; int32_t id; int32_t pad; };     // workspace entry
// a target nothing comes before: order_key never yields this key, and no id is below -1
constexpr uint64_t kRankNoKey = ~0ull;

template <typename T>
struct RankArgs {
    ModelView<T> m;
    const int32_t* users; int32_t nq, n_splits;
    const int64_t* ex_ptr; const int32_t* ex_items;
    const int64_t* tg_ptr; const int32_t* tg_items;
    RankTarget* tg;
    int32_t* out_rank; int32_t* out_cand;
};

// users per workgroup of k_rank_count: 16 while a row is one register per lane
template <typename T, int V>
constexpr int rank_users() {
    constexpr int words = V * (int)(sizeof(T) / 4);
    return words >= 8 ? 2 : 16 / words;
}

// query qy's row and bias; past the last query: a zero row, a zero bias
template <typename T, int GS, int V, int KERN>
__device__ __forceinline__ void rank_user(const RankArgs<T>& A, int qy, int l, T (&p)[V], T& bu) {
    load_user<T, GS, V, KERN>(A.m, qy < A.nq ? A.users[qy] : -1, l, p, bu);
}

// the pair's score (mf_score.hpp) as mf_topk's order key, in every lane of the group
template <typename T, int GS, int V, int KERN>
__device__ __forceinline__ uint64_t rank_key(const Hyper<T>& h, const T (&p)[V], T bu,
                                             const T (&q)[V], T bi) {
    return order_key((double)score_pair<T, GS, V, KERN>(h, p, bu, q, bi));
}

// per-lane counts of one lane group -> their sum over the wave's groups (in every lane)
template <int GS>
__device__ __forceinline__ int groups_sum(int c) {
#pragma unroll
    for (int o = GS; o < kWave; o <<= 1) c += __shfl_xor(c, o, kWave);
    return c;
}

template <typename T, int GS, int V, int KERN>
__global__ __launch_bounds__(kBlock) void k_rank_targets(RankArgs<T> A) {
    constexpr int R = kWave / GS;
    const int lane = threadIdx.x & (kWave - 1);
    const int g = lane / GS, l = lane % GS;
    const int64_t wq = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    if (wq >= A.nq) return;                              // wave-uniform
    const int qy = (int)wq;
    T p[V], bu;
    rank_user<T, GS, V, KERN>(A, qy, l, p, bu);
    if (lane == 0) A.out_cand[qy] = A.m.n_items;
    const int64_t t0 = A.tg_ptr[qy], t1 = A.tg_ptr[qy + 1];
    const int64_t xlo = A.ex_ptr ? A.ex_ptr[qy] : 0, xhi = A.ex_ptr ? A.ex_ptr[qy + 1] : 0;
    for (int64_t tb = t0; tb < t1; tb += R) {
        const int64_t t = tb + g;
        const bool have = t < t1;
        const int32_t it = have ? A.tg_items[t] : -1;
        const bool ok = have && it >= 0 && it < A.m.n_items &&
                        !in_sorted(A.ex_items, xlo, xhi, it);
        T q[V], bi;
        load_item<T, GS, V, KERN>(A.m, it, ok, l, q, bi);
        const uint64_t key = rank_key<T, GS, V, KERN>(A.m.h, p, bu, q, bi);
        if (have && l == 0) {
            RankTarget r;
            r.key = ok ? key : kRankNoKey;
            r.id = ok ? it : -1;
            r.pad = 0;
            A.tg[t] = r;
            A.out_rank[t] = ok ? 0 : -1;
        }
    }
}

template <typename T, int GS, int V, int KERN>
__global__ __launch_bounds__(kBlock) void k_rank_count(RankArgs<T> A) {
    constexpr int NU = rank_users<T, V>();
    constexpr int R = kWave / GS;
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int g = lane / GS, l = lane % GS;
    const int64_t q0 = (int64_t)blockIdx.x * NU;
    const int split = blockIdx.y;
    const int64_t span = ((int64_t)A.m.n_items + A.n_splits - 1) / A.n_splits;
    const int64_t ibeg = min((int64_t)A.m.n_items, span * split);
    const int64_t iend = min((int64_t)A.m.n_items, span * (split + 1));
    T p[NU][V], bu[NU];
    int64_t t0[NU];
    int tn[NU];
    int nseg = 0;                                        // workgroup-uniform
#pragma unroll
    for (int x = 0; x < NU; ++x) {
        const int64_t qy = q0 + x;
        const bool uq = qy < A.nq;
        rank_user<T, GS, V, KERN>(A, uq ? (int)qy : A.nq, l, p[x], bu[x]);
        t0[x] = uq ? A.tg_ptr[qy] : 0;
        tn[x] = uq ? (int)(A.tg_ptr[qy + 1] - t0[x]) : 0;
        nseg = max(nseg, (tn[x] + GS - 1) / GS);
    }
    for (int seg = 0; seg < nseg; ++seg) {
        uint64_t tk[NU];
        int32_t ti[NU];
        int cnt[NU];
        const int j = seg * GS + l;                      // this lane's target of every user
#pragma unroll
        for (int x = 0; x < NU; ++x) {
            tk[x] = kRankNoKey;
            ti[x] = -1;
            cnt[x] = 0;
            if (j < tn[x]) {
                const RankTarget r = A.tg[t0[x] + j];
                tk[x] = r.key;
                ti[x] = r.id;
            }
        }
        for (int64_t ib = ibeg + wv * R; ib < iend; ib += kWavesPerBlock * R) {
            const int64_t it = ib + g;
            const bool have = it < iend;
            T q[V], bi;
            load_item<T, GS, V, KERN>(A.m, it, have, l, q, bi);
#pragma unroll
            for (int x = 0; x < NU; ++x) {
                const uint64_t key = rank_key<T, GS, V, KERN>(A.m.h, p[x], bu[x], q, bi);
                cnt[x] += (have && cand_before(key, (int32_t)it, tk[x], ti[x])) ? 1 : 0;
            }
        }
#pragma unroll
        for (int x = 0; x < NU; ++x) {
            const int c = groups_sum<GS>(cnt[x]);
            if (g == 0 && ti[x] >= 0 && c != 0) atomicAdd(&A.out_rank[t0[x] + j], c);
        }
    }
}

template <typename T, int GS, int V, int KERN>
__global__ __launch_bounds__(kBlock) void k_rank_exclude(RankArgs<T> A) {
    constexpr int R = kWave / GS;
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int g = lane / GS, l = lane % GS;
    const int qy = blockIdx.x;
    const int64_t xlo = A.ex_ptr[qy], xhi = A.ex_ptr[qy + 1];
    if (xlo >= xhi) return;
    T p[V], bu;
    rank_user<T, GS, V, KERN>(A, qy, l, p, bu);
    const int64_t t0 = A.tg_ptr[qy];
    const int tn = (int)(A.tg_ptr[qy + 1] - t0);
    const int nseg = max(1, (tn + GS - 1) / GS);         // segment 0 also counts the candidates
    for (int seg = 0; seg < nseg; ++seg) {
        const int j = seg * GS + l;
        const bool ht = j < tn;
        uint64_t tk = kRankNoKey;
        int32_t ti = -1;
        if (ht) {
            const RankTarget r = A.tg[t0 + j];
            tk = r.key;
            ti = r.id;
        }
        int cnt = 0, nex = 0;
        for (int64_t xb = xlo + wv * R; xb < xhi; xb += kWavesPerBlock * R) {
            const int64_t x = xb + g;
            const bool have = x < xhi;
            const int32_t it = have ? A.ex_items[x] : -1;
            // in range, and the first of its duplicates in the sorted list
            const bool ok = have && it >= 0 && it < A.m.n_items &&
                            (x == xlo || A.ex_items[x - 1] != it);
            nex += (ok && l == 0) ? 1 : 0;
            if (tn > 0) {                                // workgroup-uniform
                T q[V], bi;
                load_item<T, GS, V, KERN>(A.m, it, ok, l, q, bi);
                const uint64_t key = rank_key<T, GS, V, KERN>(A.m.h, p, bu, q, bi);
                cnt += (ok && cand_before(key, it, tk, ti)) ? 1 : 0;
            }
        }
        const int c = groups_sum<GS>(cnt);
        if (g == 0 && ti >= 0 && c != 0) atomicSub(&A.out_rank[t0 + j], c);
        if (seg == 0) {
            nex = wave_sum(nex);
            if (lane == 0 && nex != 0) atomicSub(&A.out_cand[qy], nex);
        }
    }
}

// item splits of k_rank_count: enough workgroups to fill the chip several
// times over, at least 1024 items per split
static int rank_splits(int64_t user_blocks, int32_t n_items) {
    int64_t s = (2048 + user_blocks - 1) / std::max<int64_t>(1, user_blocks);
    s = std::min<int64_t>(s, n_items / 1024);
    s = std::min<int64_t>(s, 1024);
    return (int)std::max<int64_t>(1, s);
}

struct RankLaunch {
    const int32_t* users; int32_t nq; Model m;
    const int64_t* ex_ptr; const int32_t* ex_items;
    const int64_t* tg_ptr; const int32_t* tg_items;
    void* ws; int32_t* out_rank; int32_t* out_cand;
    hipStream_t stream;

    template <typename T, int GS, int V, int KERN>
    int run() {
        RankArgs<T> a;
        a.m = m.view<T>(); a.users = users; a.nq = nq;
        const bool ex = ex_ptr && ex_items;
        a.ex_ptr = ex ? ex_ptr : nullptr; a.ex_items = ex ? ex_items : nullptr;
        a.tg_ptr = tg_ptr; a.tg_items = tg_items; a.tg = (RankTarget*)ws;
        a.out_rank = out_rank; a.out_cand = out_cand;
        constexpr int NU = rank_users<T, V>();
        const int64_t ub = ((int64_t)nq + NU - 1) / NU;
        a.n_splits = rank_splits(ub, m.n_items);
        const unsigned bq = (unsigned)(((int64_t)nq + kWavesPerBlock - 1) / kWavesPerBlock);
        hipLaunchKernelGGL((k_rank_targets<T, GS, V, KERN>), dim3(bq), dim3(kBlock), 0, stream, a);
        if (m.n_items > 0)
            hipLaunchKernelGGL((k_rank_count<T, GS, V, KERN>),
                               dim3((unsigned)ub, (unsigned)a.n_splits), dim3(kBlock), 0, stream, a);
        if (ex)
            hipLaunchKernelGGL((k_rank_exclude<T, GS, V, KERN>), dim3((unsigned)nq), dim3(kBlock),
                               0, stream, a);
        MF_HIP_CHECK(hipGetLastError());
        return MF_OK;
    }
};

void touch_rank(hipStream_t s) { hipLaunchKernelGGL(k_touch<10>, dim3(1), dim3(64), 0, s); }

}  // namespace mf

#include "mf_dispatch.hpp"

using namespace mf;

extern "C" size_t mf_rank_workspace_bytes(int32_t n_query, int64_t n_targets, int32_t n_items) {
    (void)n_items;
    if (n_query <= 0 || n_targets <= 0) return 0;
    return sizeof(RankTarget) * (size_t)n_targets;
}

extern "C" int mf_rank(const int32_t* query_users, int32_t n_query, double global_mean,
                       const void* user_biases, const void* item_biases,
                       const void* user_features, const void* item_features, int32_t n_items,
                       int32_t n_factors, int32_t kernel, int32_t dtype, double gamma,
                       double min_rating, double max_rating, const int64_t* exclude_ptr,
                       const int32_t* exclude_items, const int64_t* target_ptr,
                       const int32_t* target_items, void* workspace, int32_t* out_rank,
                       int32_t* out_candidates, void* stream) {
    if (check_model("mf_rank", dtype, n_factors, kernel) != MF_OK) return MF_ERR_INVALID;
    if (n_query < 0) {
        set_error("mf_rank: n_query=%d (must be >= 0)", n_query);
        return MF_ERR_INVALID;
    }
    if (n_items < 0) {
        set_error("mf_rank: n_items=%d (must be >= 0)", n_items);
        return MF_ERR_INVALID;
    }
    if (n_query == 0) return MF_OK;
    const void* need[] = {query_users, target_ptr, target_items, workspace, out_rank,
                          out_candidates};
    const char* names[] = {"query_users", "target_ptr", "target_items", "workspace", "out_rank",
                           "out_candidates"};
    if (null_arg("mf_rank", need, names, 6)) return MF_ERR_INVALID;
    RankLaunch L{query_users, n_query,
                 {global_mean, user_biases, item_biases, user_features, item_features, n_items,
                  n_factors, gamma, min_rating, max_rating},
                 exclude_ptr, exclude_items, target_ptr, target_items, workspace, out_rank,
                 out_candidates, (hipStream_t)stream};
    return dispatch("mf_rank", dtype, n_factors, kernel, L);
}
