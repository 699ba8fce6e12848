// mf_bpr.hip -- Bayesian personalised ranking (Rendle et al. 2009) by
// exact-order SGD (include/mf_hip.h, "BPR"):
//   mf_bpr_sample -> k_bpr_sample  one negative item per visit position, a pure
//                                  function of (seed, position, attempt)
//   mf_bpr_epoch  -> k_bpr_batch   one conflict-free level of triple updates
//                                  (mf_sched_levels3; one launch per level)
//
// Compiled with -ffp-contract=off: the FP64 update rounds like the written
// expression; only the k-long dot product follows the group's DPP order.
#include <algorithm>
#include <type_traits>

#include "mf_rows.hpp"
#include "mf_dispatch.hpp"

namespace mf {
namespace bpr {

constexpr int kAttempts = 16;
constexpr uint64_t kPosStep = 0x9e3779b97f4a7c15ull;      // per visit position
constexpr uint64_t kTryStep = 0xd1b54a32d192ed03ull;      // per attempt

__host__ __device__ inline uint64_t mix(uint64_t x) {      // splitmix64 finaliser
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

struct SampleArgs {
    const int32_t* order;       // nullable: visit position -> positive index
    const int32_t* pu;
    const int32_t* pi;
    const int64_t* ptr;
    const int32_t* ids;
    int32_t* neg;
    int64_t n;
    uint64_t seed;
    uint32_t n_items;
};

// One thread per visit position; no state, no atomics: the integers do not
// depend on the launch geometry.
__global__ __launch_bounds__(kBlock) void k_bpr_sample(SampleArgs A) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= A.n) return;
    const int64_t p = A.order ? (int64_t)A.order[t] : t;
    const int32_t u = A.pu[p], i = A.pi[p];
    const int64_t b = A.ptr[u], e = A.ptr[u + 1];
    const uint64_t base = mix(A.seed + (uint64_t)(t + 1) * kPosStep);
    int32_t out = -1;
    for (int a = 0; a < kAttempts; ++a) {
        const uint64_t h = mix(base + (uint64_t)(a + 1) * kTryStep);
        const int32_t j = (int32_t)(((h >> 32) * (uint64_t)A.n_items) >> 32);
        if (j == i) continue;
        int64_t lo = b, hi = e;                            // first entry >= j
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (A.ids[mid] < j) lo = mid + 1;
            else hi = mid;
        }
        if (lo < e && A.ids[lo] == j) continue;
        out = j;
        break;
    }
    A.neg[t] = out;
}

template <typename T>
struct BatchArgs {
    const int32_t* u;
    const int32_t* i;
    const int32_t* j;
    const int32_t* order;   // nullable: schedule position -> triple index
    T* P;
    T* Q;
    T* Bi;
    T* z;                   // per schedule position: the pre-update z
    int64_t off;            // first schedule position of this level
    int64_t n;              // triples in this level
    int32_t k;
    int32_t upd_user;
    int32_t upd_item;
    T lr, reg;
};

// Triple slots per group: three rows of V values (2 registers each in FP64)
// per slot stay in registers.
template <typename T, int V>
struct Slots {
    static constexpr int S = V * (int)(sizeof(T) / 4) <= 2 ? 2 : 1;
};

// Wave w applies triples [w*RPW, (w+1)*RPW) of the level (RPW = S*R): lane t
// loads triple t and its two item biases, then per slot the group of GS lanes
// gathers x_u, y_i, y_j, reduces x_u.(y_i - y_j) on DPP and stores the three
// updated rows.  No two triples of a level share a row, and i != j inside a
// triple, so no slot reads another's write.
template <typename T, int GS, int V, int S>
__global__ __launch_bounds__(kBlock) void k_bpr_batch(BatchArgs<T> A) {
    constexpr int R = kWave / GS;
    constexpr int RPW = S * R;
    constexpr bool F32 = std::is_same<T, float>::value;
    static_assert(RPW <= kWave, "one lane per triple for the id loads");

    const int lane = threadIdx.x & (kWave - 1);
    const int g = lane / GS;
    const int l = lane % GS;
    const int64_t w0 = ((int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave) * RPW;
    if (w0 >= A.n) return;
    const int nw = (int)min((int64_t)RPW, A.n - w0);
    const int k = A.k;
    const T lr = A.lr, reg = A.reg;

    int tu, ti, tj;
    T tbi, tbj;
    {
        const int64_t pos = A.off + w0 + (lane < nw ? lane : 0);
        const int64_t t = A.order ? (int64_t)A.order[pos] : pos;
        tu = A.u[t];
        ti = A.i[t];
        tj = A.j[t];
        tbi = A.Bi[ti];
        tbj = A.Bi[tj >= 0 ? tj : ti];
    }

    int uu[S], ii[S], jj[S];
    bool have[S];
    T bi[S], bj[S];
#pragma unroll
    for (int x = 0; x < S; ++x) {
        const int idx = x * R + g;
        const int src = idx < nw ? idx : 0;
        uu[x] = take_i<GS>(tu, src);
        ii[x] = take_i<GS>(ti, src);
        jj[x] = take_i<GS>(tj, src);
        bi[x] = take_f<GS>(tbi, src);
        bj[x] = take_f<GS>(tbj, src);
        // (a skipped triple, j = -1, has no place in a schedule: no update)
        have[x] = idx < nw && jj[x] >= 0;
        if (jj[x] < 0) jj[x] = ii[x];
    }
    T xu[S][V], yi[S][V], yj[S][V];
    if (k > 0) {
        gather_rows<T, 1, GS, V, S, 0>(A.P, uu, k, k, l, xu);
        gather_rows<T, 1, GS, V, S, 0>(A.Q, ii, k, k, l, yi);
        gather_rows<T, 1, GS, V, S, 0>(A.Q, jj, k, k, l, yj);
    } else {
#pragma unroll
        for (int x = 0; x < S; ++x)
#pragma unroll
            for (int v = 0; v < V; ++v) xu[x][v] = yi[x][v] = yj[x][v] = (T)0;
    }

#pragma unroll
    for (int x = 0; x < S; ++x) {
        T d[V];
        T s = (T)0;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            d[v] = yi[x][v] - yj[x][v];
            if constexpr (F32) s = __builtin_fmaf(xu[x][v], d[v], s);
            else s = s + xu[x][v] * d[v];
        }
        s = group_sum<GS>(s);
        const T z = s + (bi[x] - bj[x]);
        T gr;
        if constexpr (F32) gr = __builtin_amdgcn_rcpf(1.0f + fast_exp(z));
        else gr = (T)1 / ((T)1 + dexp<T>(z));
        const bool lead = have[x] && l == 0;
        if (lead) A.z[A.off + w0 + x * R + g] = z;
        if (A.upd_item && lead) {
            if constexpr (F32) {
                A.Bi[ii[x]] = __builtin_fmaf(lr, __builtin_fmaf(-reg, bi[x], gr), bi[x]);
                A.Bi[jj[x]] = __builtin_fmaf(lr, __builtin_fmaf(-reg, bj[x], -gr), bj[x]);
            } else {
                A.Bi[ii[x]] = bi[x] + lr * (gr - reg * bi[x]);
                A.Bi[jj[x]] = bj[x] + lr * ((-gr) - reg * bj[x]);
            }
        }
        T* pw = A.P + (int64_t)uu[x] * k;
        T* qi = A.Q + (int64_t)ii[x] * k;
        T* qj = A.Q + (int64_t)jj[x] * k;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int f = v * GS + l;
            if (!(have[x] && f < k)) continue;
            const T a = xu[x][v], bI = yi[x][v], bJ = yj[x][v];
            T nx, ni, nj;
            if constexpr (F32) {
                nx = __builtin_fmaf(lr, __builtin_fmaf(gr, d[v], -(reg * a)), a);
                ni = __builtin_fmaf(lr, __builtin_fmaf(gr, a, -(reg * bI)), bI);
                nj = __builtin_fmaf(lr, __builtin_fmaf(-gr, a, -(reg * bJ)), bJ);
            } else {
                nx = a + lr * (gr * d[v] - reg * a);
                ni = bI + lr * (gr * a - reg * bI);
                nj = bJ + lr * ((-gr) * a - reg * bJ);
            }
            if (A.upd_user) pw[f] = nx;
            if (A.upd_item) {
                qi[f] = ni;
                qj[f] = nj;
            }
        }
    }
}

struct EpochLaunch {
    const int32_t* u; const int32_t* i; const int32_t* j; const int32_t* order;
    const int64_t* offs; const int32_t* seq; int32_t nl;       // nl = launches
    void* bi; void* P; void* Q; void* z; int32_t k;
    double lr, reg; int32_t uu, ui; hipStream_t stream;

    template <typename T, int GS, int V, int KERN>
    int run() {
        constexpr int S = Slots<T, V>::S;
        constexpr int RPW = S * (kWave / GS);
        BatchArgs<T> a;
        a.u = u; a.i = i; a.j = j; a.order = order;
        a.P = static_cast<T*>(P); a.Q = static_cast<T*>(Q); a.Bi = static_cast<T*>(bi);
        a.z = static_cast<T*>(z);
        a.k = k; a.upd_user = uu; a.upd_item = ui; a.lr = (T)lr; a.reg = (T)reg;
        for (int32_t s = 0; s < nl; ++s) {
            const int32_t b = seq ? seq[s] : s;
            a.off = offs[b];
            a.n = offs[b + 1] - offs[b];
            if (a.n <= 0) continue;
            const int64_t waves = (a.n + RPW - 1) / RPW;
            const dim3 grid((unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock));
            hipLaunchKernelGGL((k_bpr_batch<T, GS, V, S>), grid, dim3(kBlock), 0, stream, a);
        }
        MF_HIP_CHECK(hipGetLastError());
        return MF_OK;
    }
};

}  // namespace bpr
}  // namespace mf

using namespace mf;

// (no instantiation of k_bpr_batch spills: every rank the row dispatch takes)
extern "C" int32_t mf_bpr_max_factors(void) { return kMaxFactors; }

extern "C" int mf_bpr_sample(const int32_t* order, const int32_t* pos_users,
                             const int32_t* pos_items, int64_t n_pos, const int64_t* user_ptr,
                             const int32_t* user_items, int32_t n_users, int32_t n_items,
                             uint64_t seed, int32_t* neg_items, void* stream) {
    if (n_pos < 0 || n_pos >= ((int64_t)1 << 31)) {
        set_error("mf_bpr_sample: n_pos=%lld (must be in [0, 2^31))", (long long)n_pos);
        return MF_ERR_INVALID;
    }
    if (n_users < 0) {
        set_error("mf_bpr_sample: n_users=%d (must be >= 0)", n_users);
        return MF_ERR_INVALID;
    }
    if (n_items < 0) {
        set_error("mf_bpr_sample: n_items=%d (must be >= 0)", n_items);
        return MF_ERR_INVALID;
    }
    if (n_pos == 0) return MF_OK;
    if (n_users == 0 || n_items == 0) {
        set_error("mf_bpr_sample: n_users=%d, n_items=%d with n_pos=%lld positives", n_users,
                  n_items, (long long)n_pos);
        return MF_ERR_INVALID;
    }
    const void* need[] = {pos_users, pos_items, user_ptr, user_items, neg_items};
    const char* names[] = {"pos_users", "pos_items", "user_ptr", "user_items", "neg_items"};
    if (null_arg("mf_bpr_sample", need, names, 5)) return MF_ERR_INVALID;
    bpr::SampleArgs a{order, pos_users, pos_items, user_ptr, user_items, neg_items, n_pos, seed,
                      (uint32_t)n_items};
    hipLaunchKernelGGL(bpr::k_bpr_sample, dim3((unsigned)((n_pos + kBlock - 1) / kBlock)),
                       dim3(kBlock), 0, (hipStream_t)stream, a);
    MF_HIP_CHECK(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_bpr_epoch(const int32_t* user_ids, const int32_t* item_ids,
                            const int32_t* neg_items, int64_t n_triples, const int32_t* order,
                            const int64_t* batch_offsets, int32_t n_batches,
                            const int32_t* batch_seq, int32_t n_seq, void* item_biases,
                            void* user_features, void* item_features, int32_t n_users,
                            int32_t n_items, int32_t n_factors, int32_t dtype, double lr,
                            double reg, int32_t update_user_params, int32_t update_item_params,
                            void* z_out, void* stream) {
    if (dtype != MF_F32 && dtype != MF_F64) {
        set_error("mf_bpr_epoch: dtype=%d (unknown dtype code)", dtype);
        return MF_ERR_INVALID;
    }
    if (n_factors < 0 || n_factors > mf_bpr_max_factors()) {
        set_error("mf_bpr_epoch: n_factors=%d (must be in [0, %d])", n_factors,
                  mf_bpr_max_factors());
        return MF_ERR_INVALID;
    }
    if (n_triples < 0) {
        set_error("mf_bpr_epoch: n_triples=%lld (must be >= 0)", (long long)n_triples);
        return MF_ERR_INVALID;
    }
    if (n_batches < 0) {
        set_error("mf_bpr_epoch: n_batches=%d (must be >= 0)", n_batches);
        return MF_ERR_INVALID;
    }
    if (batch_seq && n_seq < 0) {
        set_error("mf_bpr_epoch: n_seq=%d (must be >= 0)", n_seq);
        return MF_ERR_INVALID;
    }
    if (n_users < 0) {
        set_error("mf_bpr_epoch: n_users=%d (must be >= 0)", n_users);
        return MF_ERR_INVALID;
    }
    if (n_items < 0) {
        set_error("mf_bpr_epoch: n_items=%d (must be >= 0)", n_items);
        return MF_ERR_INVALID;
    }
    const int32_t n_launch = batch_seq ? n_seq : n_batches;
    if (n_launch == 0 || n_triples == 0) return MF_OK;
    if (!batch_offsets) {
        set_error("mf_bpr_epoch: batch_offsets is NULL");
        return MF_ERR_INVALID;
    }
    for (int32_t b = 0; b < n_batches; ++b) {
        if (batch_offsets[b] < 0 || batch_offsets[b + 1] < batch_offsets[b] ||
            batch_offsets[b + 1] > n_triples) {
            set_error("mf_bpr_epoch: batch_offsets[%d..%d] = %lld..%lld invalid for "
                      "n_triples=%lld", b, b + 1, (long long)batch_offsets[b],
                      (long long)batch_offsets[b + 1], (long long)n_triples);
            return MF_ERR_INVALID;
        }
    }
    for (int32_t q = 0; batch_seq && q < n_seq; ++q) {
        if (batch_seq[q] < 0 || batch_seq[q] >= n_batches) {
            set_error("mf_bpr_epoch: batch_seq[%d] = %d out of range [0, %d)", q, batch_seq[q],
                      n_batches);
            return MF_ERR_INVALID;
        }
    }
    // (n_factors == 0: the bias-only model, no factor rows are touched)
    const void* need[] = {user_ids, item_ids, neg_items, item_biases, z_out, user_features,
                          item_features};
    const char* names[] = {"user_ids", "item_ids", "neg_items", "item_biases", "z_out",
                           "user_features", "item_features"};
    if (null_arg("mf_bpr_epoch", need, names, n_factors > 0 ? 7 : 5)) return MF_ERR_INVALID;
    bpr::EpochLaunch L{user_ids, item_ids, neg_items, order, batch_offsets, batch_seq, n_launch,
                       item_biases, user_features, item_features, z_out, n_factors, lr, reg,
                       update_user_params ? 1 : 0, update_item_params ? 1 : 0,
                       (hipStream_t)stream};
    return dispatch("mf_bpr_epoch", dtype, n_factors, MF_LINEAR, L);
}
