// mf_topk.hip -- batched recommend(): score every item for a set of users and
// keep the best `amount` per user (recommender_base.py:214-271 scores all
// candidate items with predict(bound_ratings=False) and sorts descending).
//
// amount <= 64 (recommend's default 10): k_topk_fused + k_topk_merge (below:
// scores never leave the chip).  Larger amounts, or MF_TOPK_TWO_STAGE=1:
// Stage 1 (k_topk_scores): one wave per (user, chunk of items); the user's
//   factor row stays in registers, item rows stream from HBM/L2; each score
//   becomes a 64-bit order-preserving key (1 = NaN); k_topk_exclude then
//   zeroes the keys of the excluded (user, item) pairs (CSR list).
// Stage 2 (k_topk_select): one workgroup per user: 8-pass radix select of
//   the amount-th key (LDS histograms), collect, bitonic sort in LDS by
//   (score desc, item id asc).
//
// This is the exact path (the C ABI's mf_topk).  The MFMA candidate filter
// that runs in front of it for the linear FP32 kernel (mf_topk_mm) is a unit
// of its own, mf_topk_mm.hip; what the two share is in mf_order.hpp.
#include <algorithm>
#include <climits>
#include <cstdlib>

#include "mf_score.hpp"
#include "mf_order.hpp"

namespace mf {

constexpr int kTopkMaxAmount = 2048;
constexpr int kTopkItemsPerWave = 256;

template <typename T>
struct TopkArgs {
    ModelView<T> m;
    const int32_t* users;
    uint64_t* keys;
};

template <typename T, int GS, int V, int KERN>
__global__ __launch_bounds__(kBlock) void k_topk_scores(TopkArgs<T> A) {
    constexpr int R = kWave / GS;
    const int lane = threadIdx.x & (kWave - 1);
    const int g = lane / GS, l = lane % GS;
    const int qy = blockIdx.y;
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const int64_t i0 = wave * kTopkItemsPerWave;
    if (i0 >= A.m.n_items) return;
    T p[V], bu;
    load_user<T, GS, V, KERN>(A.m, A.users[qy], l, p, bu);
    const int64_t iend = min((int64_t)A.m.n_items, i0 + kTopkItemsPerWave);
    uint64_t* keys = A.keys + (int64_t)qy * A.m.n_items;
    for (int64_t ib = i0; ib < iend; ib += R) {
        const int64_t it = ib + g;
        const bool have = it < iend;
        T q[V], bi;
        load_item<T, GS, V, KERN>(A.m, it, have, l, q, bi);
        const T pred = score_pair<T, GS, V, KERN>(A.m.h, p, bu, q, bi);
        if (have && l == 0) keys[it] = order_key((double)pred);
    }
}

// excluded (query, item) pairs: key 0, below every candidate.  One workgroup
// per query walks its CSR list (ids outside [0, n_items) are ignored).
__global__ __launch_bounds__(kBlock) void k_topk_exclude(uint64_t* __restrict__ keys,
                                                         int32_t n_items,
                                                         const int64_t* __restrict__ ptr,
                                                         const int32_t* __restrict__ items) {
    const int qy = blockIdx.x;
    for (int64_t x = ptr[qy] + threadIdx.x; x < ptr[qy + 1]; x += kBlock) {
        const int32_t it = items[x];
        if (it >= 0 && it < n_items) keys[(int64_t)qy * n_items + it] = 0ull;
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_topk_select(const uint64_t* __restrict__ all_keys,
                                                        int32_t n_items, int32_t amount,
                                                        int32_t a2, int32_t* out_items,
                                                        T* out_scores) {
    const int qy = blockIdx.x;
    const int tid = threadIdx.x;
    const uint64_t* K = all_keys + (int64_t)qy * n_items;
    __shared__ unsigned hist[256];
    __shared__ uint64_t s_key[kTopkMaxAmount];
    __shared__ int32_t s_idx[kTopkMaxAmount];
    __shared__ int s_cnt, s_rem, s_want, s_base;
    __shared__ uint64_t s_prefix, s_mask;
    __shared__ int wsum[kWavesPerBlock];

    // candidates
    int c = 0;
    for (int i = tid; i < n_items; i += kBlock) c += K[i] != 0ull;
    c = wave_sum(c);
    if ((tid & 63) == 0) wsum[tid / kWave] = c;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) t += wsum[w];
        s_want = t < amount ? t : amount;
        s_rem = s_want;
        s_prefix = 0ull;
        s_mask = 0ull;
        s_cnt = 0;
    }
    __syncthreads();
    const int want = s_want;
    if (want > 0) {
        for (int d = 7; d >= 0; --d) {
            for (int b = tid; b < 256; b += kBlock) hist[b] = 0u;
            __syncthreads();
            const uint64_t pre = s_prefix, msk = s_mask;
            for (int i = tid; i < n_items; i += kBlock) {
                const uint64_t kk = K[i];
                if (kk != 0ull && (kk & msk) == pre) atomicAdd(&hist[(kk >> (8 * d)) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                int cum = 0, sel = 0;
                for (int b = 255; b >= 0; --b) {
                    if (cum + (int)hist[b] >= s_rem) { sel = b; break; }
                    cum += (int)hist[b];
                }
                s_rem -= cum;
                s_prefix |= (uint64_t)sel << (8 * d);
                s_mask |= 0xffull << (8 * d);
            }
            __syncthreads();
        }
        const uint64_t thr = s_prefix;
        // every key above the threshold
        for (int i = tid; i < n_items; i += kBlock) {
            const uint64_t kk = K[i];
            if (kk > thr) {
                const int slot = atomicAdd(&s_cnt, 1);
                s_key[slot] = kk;
                s_idx[slot] = i;
            }
        }
        __syncthreads();
        // the s_rem lowest-id items whose key equals the threshold
        if (tid == 0) s_base = s_cnt;
        __syncthreads();
        for (int i0 = 0; i0 < n_items && s_rem > 0; i0 += kBlock) {
            const int i = i0 + tid;
            const bool m = i < n_items && K[i] == thr;
            const unsigned long long bal = __ballot(m);
            const int w = tid / kWave, ln = tid & 63;
            if (ln == 0) wsum[w] = __popcll(bal);
            __syncthreads();
            int before = 0;
            for (int x = 0; x < w; ++x) before += wsum[x];
            before += __popcll(bal & ((1ull << ln) - 1ull));
            if (m && before < s_rem) {
                s_key[s_base + before] = thr;
                s_idx[s_base + before] = i;
            }
            __syncthreads();
            if (tid == 0) {
                int tot = 0;
                for (int x = 0; x < kWavesPerBlock; ++x) tot += wsum[x];
                const int took = tot < s_rem ? tot : s_rem;
                s_base += took;
                s_rem -= took;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    // pad to a2 and bitonic-sort by (key desc, idx asc)
    for (int s = want + tid; s < a2; s += kBlock) { s_key[s] = 0ull; s_idx[s] = INT_MAX; }
    __syncthreads();
    for (int sz = 2; sz <= a2; sz <<= 1) {
        for (int st = sz >> 1; st > 0; st >>= 1) {
            for (int x = tid; x < a2; x += kBlock) {
                const int y = x ^ st;
                if (y > x) {
                    const bool desc = (x & sz) == 0;
                    const uint64_t kx = s_key[x], ky = s_key[y];
                    const int ix = s_idx[x], iy = s_idx[y];
                    // "x before y" in the final order
                    const bool xfirst = kx > ky || (kx == ky && ix < iy);
                    if (desc ? !xfirst : xfirst) {
                        s_key[x] = ky; s_key[y] = kx;
                        s_idx[x] = iy; s_idx[y] = ix;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int s = tid; s < amount; s += kBlock) {
        const bool ok = s < want;
        out_items[(int64_t)qy * amount + s] = ok ? s_idx[s] : -1;
        out_scores[(int64_t)qy * amount + s] =
            ok ? (T)key_score(s_key[s]) : (T)__longlong_as_double(0x7ff8000000000000LL);
    }
}

// ---------------------------------------------------------------- fused
// k_topk_fused: the same scores without materialising them.  Of mf_score.hpp
// it calls predict_one alone and keeps its own row loads, partial loop and
// loose FusedArgs fields (what load_user / load_item / score_pair do, written
// where it was): with GS = 64 its 16-user inner loop is wave-uniform and sits
// at the 106-SGPR limit, and through the helpers or with a ModelView member
// k_topk_fused<float, *, 1, MF_LINEAR> spilled 20 SGPRs for 14 / 14 / 17 and
// ran 1.25 % slower (profiles/score_share/README.md).
// Workgroup (split x, user block y) scores items [ibeg, iend) of its split
// against kFusedUsers users whose rows sit in registers; every wave walks
// one item at a time.  A score enters the user's LDS candidate list only if
// it beats the list's current threshold (the amount-th best so far, in the
// order (score desc, item id asc)); excluded items are looked up (binary
// search in the user's sorted CSR list) only for such candidates.  After
// every chunk of items a barrier; lists that grew past A2 + chunk are
// bitonic-sorted and cut to the best A2 (A2 = amount rounded up to a power
// of two), raising the threshold.  At the end each list is sorted and its
// best `amount` go to the split's partial output; k_topk_merge merges the
// splits per user.  Random scores settle the threshold after a few chunks,
// so almost every score costs its reduction and one compare.
constexpr int kFusedUsers = 16;          // users per workgroup (registers)
constexpr int kFusedItemsPerWave = 16;   // items per wave between barriers
constexpr int kFusedChunk = kWavesPerBlock * kFusedItemsPerWave;
constexpr int kFusedCap = 256;           // list capacity: A2 + 2 chunks <= 256

template <typename T>
struct FusedArgs {
    const int32_t* users; int32_t nq;
    const T* P; const T* Q; const T* Bu; const T* Bi;
    int32_t n_items, k, amount, a2, n_splits;
    Hyper<T> h;
    const int64_t* ex_ptr; const int32_t* ex_items;
    uint64_t* part_key; int32_t* part_id;           // [nq][n_splits][amount]
};

template <typename T, int GS, int V, int KERN>
__global__ __launch_bounds__(kBlock) void k_topk_fused(FusedArgs<T> A) {
    static_assert(GS == kWave || V == 1, "the scalar layout: one item per wave");
    __shared__ uint64_t s_key[kFusedUsers][kFusedCap];
    __shared__ int32_t s_id[kFusedUsers][kFusedCap];
    __shared__ int s_cnt[kFusedUsers];
    __shared__ uint64_t s_tk[kFusedUsers];
    __shared__ int32_t s_ti[kFusedUsers];
    constexpr int R = kWave / GS;                    // items per wave instruction
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const int g = lane / GS, l = lane % GS;
    const int split = blockIdx.x, q0 = blockIdx.y * kFusedUsers;
    const int k = A.k;
    const int64_t span = ((int64_t)A.n_items + A.n_splits - 1) / A.n_splits;
    const int ibeg = (int)min((int64_t)A.n_items, span * split);
    const int iend = (int)min((int64_t)A.n_items, span * (split + 1));
    if (tid < kFusedUsers) {
        s_cnt[tid] = 0;
        s_tk[tid] = 0ull;                            // below every candidate key (>= 1)
        s_ti[tid] = 0x7fffffff;
    }
    T p[kFusedUsers][V], bu[kFusedUsers];
#pragma unroll
    for (int x = 0; x < kFusedUsers; ++x) {
        const int qy = q0 + x;
        const int32_t uu = qy < A.nq ? A.users[qy] : -1;
        const bool uk = uu >= 0;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int f = l + v * GS;
            p[x][v] = (uk && f < k) ? A.P[(int64_t)uu * k + f] : (T)0;
        }
        bu[x] = (uk && KERN != MF_RBF) ? A.Bu[uu] : (T)0;
    }
    __syncthreads();
    for (int c0 = ibeg; c0 < iend; c0 += kFusedChunk) {
        // thresholds of this chunk (wave-uniform copies)
        uint64_t tk[kFusedUsers];
        int32_t ti[kFusedUsers];
#pragma unroll
        for (int x = 0; x < kFusedUsers; ++x) { tk[x] = s_tk[x]; ti[x] = s_ti[x]; }
        for (int j = 0; j < kFusedItemsPerWave; j += R) {
            const int it = c0 + wv * kFusedItemsPerWave + j + g;
            const bool have = it < iend;
            const T* qr = A.Q + (int64_t)(have ? it : 0) * k;
            T q[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int f = l + v * GS;
                q[v] = (have && f < k) ? qr[f] : (T)0;
            }
            const T bi = (have && KERN != MF_RBF) ? A.Bi[it] : (T)0;
#pragma unroll
            for (int x = 0; x < kFusedUsers; ++x) {
                T sc = (T)0;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    if constexpr (KERN == MF_RBF) {
                        const T d = p[x][v] - q[v];
                        sc = sc + d * d;
                    } else {
                        sc = sc + p[x][v] * q[v];
                    }
                }
                sc = group_sum<GS>(sc);
                const T pred = predict_one<T, KERN>(sc, bu[x], bi, A.h);
                const uint64_t key = order_key((double)pred);
                const int qy = q0 + x;
                if (have && l == 0 && qy < A.nq && cand_before(key, it, tk[x], ti[x]) &&
                    !excluded(A.ex_ptr, A.ex_items, qy, it)) {
                    const int slot = atomicAdd(&s_cnt[x], 1);
                    s_key[x][slot] = key;
                    s_id[x][slot] = it;
                }
            }
        }
        __syncthreads();
        // cut lists that can no longer take a full chunk
#pragma unroll 1
        for (int x = 0; x < kFusedUsers; ++x) {
            const int n = s_cnt[x];
            if (n <= A.a2 + kFusedChunk) continue;       // uniform: s_cnt read after the barrier
            int n2 = 1;
            while (n2 < n) n2 <<= 1;
            for (int y = n + tid; y < n2; y += kBlock) { s_key[x][y] = 0ull; s_id[x][y] = 0x7fffffff; }
            __syncthreads();
            cand_sort(s_key[x], s_id[x], n2, tid, kBlock);
            if (tid == 0) {
                s_cnt[x] = A.a2;
                s_tk[x] = s_key[x][A.amount - 1];        // the amount-th best so far
                s_ti[x] = s_id[x][A.amount - 1];
            }
            __syncthreads();
        }
    }
    // final: sort each list, write its best `amount` (padding: key 0, id -1)
#pragma unroll 1
    for (int x = 0; x < kFusedUsers; ++x) {
        const int qy = q0 + x;
        if (qy >= A.nq) break;                           // uniform
        const int n = s_cnt[x];
        int n2 = 1;
        while (n2 < max(n, A.a2)) n2 <<= 1;
        for (int y = n + tid; y < n2; y += kBlock) { s_key[x][y] = 0ull; s_id[x][y] = 0x7fffffff; }
        __syncthreads();
        cand_sort(s_key[x], s_id[x], n2, tid, kBlock);
        for (int y = tid; y < A.amount; y += kBlock) {
            const int64_t o = ((int64_t)qy * A.n_splits + split) * A.amount + y;
            const bool ok = y < n;
            A.part_key[o] = ok ? s_key[x][y] : 0ull;
            A.part_id[o] = ok ? s_id[x][y] : -1;
        }
        __syncthreads();
    }
}

// merge the n_splits partial lists of one user (a workgroup per user)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_topk_merge(const uint64_t* __restrict__ part_key,
                                                       const int32_t* __restrict__ part_id,
                                                       int32_t n_splits, int32_t amount,
                                                       int32_t* out_items, T* out_scores) {
    __shared__ uint64_t s_key[kFusedCap * 4];
    __shared__ int32_t s_id[kFusedCap * 4];
    const int qy = blockIdx.x, tid = threadIdx.x;
    const int n = n_splits * amount;                     // <= 4 * kFusedCap (launcher)
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int y = tid; y < n2; y += kBlock) {
        const bool ok = y < n;
        const int64_t o = (int64_t)qy * n + y;
        const int32_t id = ok ? part_id[o] : -1;
        s_key[y] = (ok && id >= 0) ? part_key[o] : 0ull;
        s_id[y] = (ok && id >= 0) ? id : 0x7fffffff;
    }
    __syncthreads();
    cand_sort(s_key, s_id, n2, tid, kBlock);
    for (int y = tid; y < amount; y += kBlock) {
        const bool ok = s_key[y] != 0ull;
        out_items[(int64_t)qy * amount + y] = ok ? s_id[y] : -1;
        out_scores[(int64_t)qy * amount + y] =
            ok ? (T)key_score(s_key[y]) : (T)__longlong_as_double(0x7ff8000000000000LL);
    }
}

// splits of the item range for the fused path: enough workgroups to fill the
// chip (~6 per CU), at least 512 items per split, n_splits * amount <= 1024
inline int topk_splits(int32_t nq, int32_t n_items, int32_t amount) {
    const int64_t blocks_q = ((int64_t)nq + kFusedUsers - 1) / kFusedUsers;
    int64_t s = (1536 + blocks_q - 1) / blocks_q;
    s = std::min<int64_t>(s, std::max<int64_t>(1, n_items / 512));
    s = std::min<int64_t>(s, 1024 / std::max(amount, 1));
    return (int)std::max<int64_t>(1, s);
}
inline bool topk_fused(int32_t amount) {
    const char* e = std::getenv("MF_TOPK_TWO_STAGE");
    return amount <= kFusedMaxAmount && !(e && std::atoi(e) == 1);
}

void topk_exclude_keys(uint64_t* keys, int32_t nq, int32_t n_items, const int64_t* ex_ptr,
                       const int32_t* ex_items, hipStream_t stream) {
    hipLaunchKernelGGL(k_topk_exclude, dim3((unsigned)nq), dim3(kBlock), 0, stream, keys, n_items,
                       ex_ptr, ex_items);
}

// Stage 2 of the two-stage path on an [nq x n_items] key matrix: the excluded
// pairs' keys are zeroed, then each row's best `amount` are selected and sorted
template <typename T>
inline void topk_from_keys(uint64_t* keys, int32_t nq, int32_t n_items, const int64_t* ex_ptr,
                           const int32_t* ex_items, int32_t amount, int32_t* out_items,
                           T* out_scores, hipStream_t stream) {
    if (ex_ptr && ex_items) topk_exclude_keys(keys, nq, n_items, ex_ptr, ex_items, stream);
    int a2 = 1;
    while (a2 < amount) a2 <<= 1;
    hipLaunchKernelGGL(k_topk_select<T>, dim3((unsigned)nq), dim3(kBlock), 0, stream,
                       (const uint64_t*)keys, n_items, amount, a2, out_items, out_scores);
}

struct TopkLaunch {
    const int32_t* users; int32_t nq; Model m;
    const int64_t* ex_ptr; const int32_t* ex_items; int32_t amount; void* ws; int32_t* out_items; void* out_scores;
    hipStream_t stream;

    template <typename T, int GS, int V, int KERN>
    int run() {
        const int32_t n_items = m.n_items;
        if (topk_fused(amount)) {
            FusedArgs<T> f;
            const ModelView<T> v = m.view<T>();
            f.users = users; f.nq = nq; f.P = v.P; f.Q = v.Q; f.Bu = v.Bu; f.Bi = v.Bi;
            f.n_items = n_items; f.k = v.k; f.h = v.h; f.amount = amount;
            int a2 = 1;
            while (a2 < amount) a2 <<= 1;
            f.a2 = a2;
            f.n_splits = topk_splits(nq, n_items, amount);
            f.ex_ptr = ex_items ? ex_ptr : nullptr; f.ex_items = ex_items;
            const size_t np = (size_t)nq * f.n_splits * amount;
            f.part_key = (uint64_t*)ws;
            f.part_id = (int32_t*)((uint64_t*)ws + np);
            const unsigned by = (unsigned)((nq + kFusedUsers - 1) / kFusedUsers);
            hipLaunchKernelGGL((k_topk_fused<T, GS, V, KERN>), dim3((unsigned)f.n_splits, by),
                               dim3(kBlock), 0, stream, f);
            hipLaunchKernelGGL(k_topk_merge<T>, dim3((unsigned)nq), dim3(kBlock), 0, stream,
                               (const uint64_t*)f.part_key, (const int32_t*)f.part_id, f.n_splits,
                               amount, out_items, (T*)out_scores);
            MF_HIP_CHECK(hipGetLastError());
            return MF_OK;
        }
        const TopkArgs<T> a{m.view<T>(), users, (uint64_t*)ws};
        const int64_t waves = ((int64_t)n_items + kTopkItemsPerWave - 1) / kTopkItemsPerWave;
        const unsigned bx = (unsigned)((waves + kWavesPerBlock - 1) / kWavesPerBlock);
        hipLaunchKernelGGL((k_topk_scores<T, GS, V, KERN>), dim3(bx, (unsigned)nq),
                           dim3(kBlock), 0, stream, a);
        topk_from_keys<T>(a.keys, nq, n_items, ex_ptr, ex_items, amount, out_items,
                          (T*)out_scores, stream);
        MF_HIP_CHECK(hipGetLastError());
        return MF_OK;
    }
};

void topk_select_f64(uint64_t* keys, int32_t nq, int32_t n_items, const int64_t* ex_ptr,
                     const int32_t* ex_items, int32_t amount, int32_t* out_items,
                     double* out_scores, hipStream_t stream) {
    topk_from_keys<double>(keys, nq, n_items, ex_ptr, ex_items, amount, out_items, out_scores,
                           stream);
}

void touch_topk(hipStream_t s) { hipLaunchKernelGGL(k_touch<6>, dim3(1), dim3(64), 0, s); }

}  // namespace mf

#include "mf_dispatch.hpp"

using namespace mf;

extern "C" size_t mf_topk_workspace_bytes(int32_t n_query, int32_t n_items, int32_t amount) {
    if (n_query <= 0 || n_items <= 0) return 0;
    if (topk_fused(amount))       // partial lists: n_query x splits x amount (key + id)
        return (sizeof(uint64_t) + sizeof(int32_t)) * (size_t)n_query *
               (size_t)topk_splits(n_query, n_items, amount) * (size_t)std::max(amount, 1);
    return sizeof(uint64_t) * (size_t)n_query * (size_t)n_items;
}

extern "C" int mf_topk(const int32_t* query_users, int32_t n_query, double global_mean,
                       const void* user_biases, const void* item_biases,
                       const void* user_features, const void* item_features, int32_t n_items,
                       int32_t n_factors, int32_t kernel, int32_t dtype, double gamma,
                       double min_rating, double max_rating, const int64_t* exclude_ptr,
                       const int32_t* exclude_items, int32_t amount, void* workspace, int32_t* out_items, void* out_scores,
                       void* stream) {
    if (n_query < 0 || n_items < 0 || amount < 0 || amount > kTopkMaxAmount) {
        set_error("mf_topk: need 0 <= amount <= %d and non-negative sizes", kTopkMaxAmount);
        return MF_ERR_INVALID;
    }
    if (n_query == 0 || amount == 0) return MF_OK;
    if (!workspace || !out_items || !out_scores || !query_users) {
        set_error("mf_topk: NULL buffer");
        return MF_ERR_INVALID;
    }
    if (n_items == 0) {
        // nothing to rank: every slot is padding
        set_error("mf_topk: n_items == 0");
        return MF_ERR_INVALID;
    }
    TopkLaunch L{query_users, n_query,
                 {global_mean, user_biases, item_biases, user_features, item_features, n_items,
                  n_factors, gamma, min_rating, max_rating},
                 exclude_ptr, exclude_items, amount, workspace, out_items, out_scores,
                 (hipStream_t)stream};
    return dispatch("mf_topk", dtype, n_factors, kernel, L);
}
