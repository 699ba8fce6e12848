// mf_order.hpp -- the ranking order shared by top-k (mf_topk.hip, its MFMA
// filter mf_topk_mm.hip) and exact
// ranking (mf_rank.hip): candidates go by score descending, then by item id
// ascending, with NaN below every number; and the sorted-list searches both
// use for the per-query exclusion CSR.
#pragma once

#include "mf_common.hpp"

namespace mf {

__device__ __forceinline__ uint64_t order_key(double s) {
    if (s != s) return 1ull;                       // NaN: below every number
    uint64_t b = (uint64_t)__double_as_longlong(s);
    return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_score(uint64_t k) {
    if (k <= 1ull) return __longlong_as_double(0x7ff8000000000000LL);
    uint64_t b = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// (key desc, id asc): does (ka, ia) come before (kb, ib)?
__device__ __forceinline__ bool cand_before(uint64_t ka, int32_t ia, uint64_t kb, int32_t ib) {
    return ka > kb || (ka == kb && ia < ib);
}

// The largest amount the fused exact path (k_topk_fused, mf_topk.hip) and the
// MFMA filter in front of it (mf_topk_mm.hip) take.
constexpr int kFusedMaxAmount = 64;

// bitonic sort of n (power of two) candidates in LDS by the whole workgroup
// subset `lanes` (threads t < lanes participate; all threads hit the barriers).
// k_topk_merge's order: k_topk_mm_merge sorts with it too, so the filter's
// output is the exact path's.
__device__ __forceinline__ void cand_sort(uint64_t* key, int32_t* id, int n, int t, int lanes) {
    for (int sz = 2; sz <= n; sz <<= 1) {
        for (int st = sz >> 1; st > 0; st >>= 1) {
            for (int x = t; x < n && t < lanes; x += lanes) {
                const int y = x ^ st;
                if (y > x) {
                    const bool desc = (x & sz) == 0;
                    const uint64_t kx = key[x], ky = key[y];
                    const int32_t ix = id[x], iy = id[y];
                    const bool xfirst = cand_before(kx, ix, ky, iy);
                    if (desc ? !xfirst : xfirst) {
                        key[x] = ky; key[y] = kx;
                        id[x] = iy; id[y] = ix;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// is `it` in the sorted id range items[lo, hi)?
__device__ __forceinline__ bool in_sorted(const int32_t* items, int64_t lo, int64_t hi, int32_t it) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t v = items[mid];
        if (v == it) return true;
        if (v < it) lo = mid + 1;
        else hi = mid;
    }
    return false;
}
// first position in the sorted items[lo, hi) whose id is >= it
__device__ __forceinline__ int64_t lower_pos(const int32_t* items, int64_t lo, int64_t hi,
                                             int32_t it) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (items[mid] < it) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool excluded(const int64_t* ptr, const int32_t* items, int qy,
                                         int32_t it) {
    if (!ptr) return false;
    int64_t lo = ptr[qy], hi = ptr[qy + 1];          // sorted ascending
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t v = items[mid];
        if (v == it) return true;
        if (v < it) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

// mf_topk.hip's stage 2 for any [nq x n_items] matrix of order keys (0 = no
// candidate), also used by mf_cf_topk.hip: topk_exclude_keys zeroes the keys
// of the CSR pairs (k_topk_exclude); topk_select_f64 does that (ex_ptr or
// ex_items null: not) and writes each row's best `amount` (<= 2048) by (key
// desc, id asc), padded with id -1 / NaN (k_topk_select<double>).  Both only
// enqueue.
void topk_exclude_keys(uint64_t* keys, int32_t nq, int32_t n_items, const int64_t* ex_ptr,
                       const int32_t* ex_items, hipStream_t stream);
void topk_select_f64(uint64_t* keys, int32_t nq, int32_t n_items, const int64_t* ex_ptr,
                     const int32_t* ex_items, int32_t amount, int32_t* out_items,
                     double* out_scores, hipStream_t stream);

}  // namespace mf
