// mf_cf.hpp -- what the neighbourhood kernels share (mf_cf.hip: one pair per
// workgroup; mf_cf_topk.hip: one query against every target): the total order
// at the n_neighbors cut, the exact radix select, the per-pair prediction of
// one wave, and the two sources of a target's similarities (the dense matrix,
// or the stored neighbour lists of the top-M model).
#pragma once

#include <cmath>

#include "mf_common.hpp"

namespace mf {
namespace cf {

constexpr int kKeysLds = 1024;               // longest list whose keys stay in LDS
constexpr int64_t kMaxGrid = 1 << 25;        // workgroups of one wave: 2^31 threads a launch
constexpr int kMaxStored = 4096;             // stored neighbours per entity: a row is <= 32 KiB
constexpr int kNbrSlots = 2048;              // k_cf_neighbours' workgroups = scratch rows: 8 per CU

// Total order at the cut: similarity descending, then entity id ascending.
// key = (monotone image of the float's bits) << 32 | ~id is larger for what
// comes first, distinct per candidate and never 0 (ids are < 2^31).
__device__ __forceinline__ uint64_t make_key(float s, int32_t id) {
    if (s == 0.f) s = 0.f;                            // -0 and +0 tie
    const uint32_t b = __float_as_uint(s);
    const uint32_t m = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)m << 32) | (uint32_t)~(uint32_t)id;
}
__device__ __forceinline__ float key_sim(uint64_t k) {
    const uint32_t m = (uint32_t)(k >> 32);
    return __uint_as_float((m & 0x80000000u) ? (m & 0x7fffffffu) : ~m);
}
__device__ __forceinline__ int32_t key_id(uint64_t k) { return (int32_t)~(uint32_t)k; }

// Where a target's similarities come from -- the one thing the dense and the
// stored-neighbours (top-M) model differ in.  sim.row(e).key(b) is candidate
// b's key for target e: make_key(S[e,b], b), or, with lists, 0 ("not a
// candidate") for a b outside N_M(e).
struct DenseRow {
    const float* s;                              // S[e, :]
    __device__ __forceinline__ uint64_t key(int32_t b) const { return make_key(s[b], b); }
};
struct DenseSim {
    static constexpr bool kLists = false;
    const float* S;
    int32_t n_entities;
    __device__ __forceinline__ DenseRow row(int32_t e) const {
        return DenseRow{S + (size_t)e * (size_t)n_entities};
    }
};
struct ListRow {
    const int32_t* ids;                          // n entries, ascending
    const float* sims;
    int32_t n;
    __device__ __forceinline__ uint64_t key(int32_t b) const {
        int32_t lo = 0, hi = n;
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (ids[mid] < b) lo = mid + 1; else hi = mid;
        }
        return (lo < n && ids[lo] == b) ? make_key(sims[lo], b) : 0;
    }
};
struct ListSim {
    static constexpr bool kLists = true;
    const int32_t* ids;                          // n_entities x n_stored, rows id-ascending
    const float* sims;
    int32_t n_stored, n_valid;                   // n_valid = min(n_stored, n_entities - 1): the
                                                 // rest of every row is padding (-1 / 0)
    __device__ __forceinline__ ListRow row(int32_t e) const {
        const size_t at = (size_t)e * (size_t)n_stored;
        return ListRow{ids + at, sims + at, n_valid};
    }
};
inline ListSim list_sim(const int32_t* ids, const void* sims, int32_t n_stored,
                        int32_t n_entities) {
    const int32_t most = n_entities > 0 ? n_entities - 1 : 0;
    return ListSim{ids, static_cast<const float*>(sims), n_stored,
                   n_stored < most ? n_stored : most};
}

// One wave: the want-th largest of the non-zero keys key_at(0 .. len), of which
// there are MORE than want (want >= 1) -- a radix select (256 integer bins per
// pass, most significant byte first, at most 8 passes; it stops at the pass
// whose bin is kept whole): exact for any len, linear in it.  Exactly `want`
// keys are >= the value returned.  bins (256) is this wave's LDS.
template <typename KeyAt, typename Sync>
__device__ __forceinline__ uint64_t select_cut(uint32_t* bins, int64_t len, uint32_t want,
                                               int lane, KeyAt key_at, Sync sync) {
    uint64_t prefix = 0;                          // the cut's bytes above the current one
    for (int sh = 56; sh >= 0; sh -= 8) {         // want: rank of the cut among keys matching prefix
        for (int c = lane; c < 256; c += kWave) bins[c] = 0;
        sync();
        for (int64_t j = lane; j < len; j += kWave) {
            const uint64_t k = key_at(j);
            if (k != 0 && (sh == 56 || (k >> (sh + 8)) == prefix))
                atomicAdd(&bins[(uint32_t)(k >> sh) & 255u], 1u);
        }
        sync();
        // lane l owns bins 4l .. 4l+3; suf = count in this lane's bins and above
        const uint32_t h0 = bins[4 * lane], h1 = bins[4 * lane + 1],
                       h2 = bins[4 * lane + 2], h3 = bins[4 * lane + 3];
        const uint32_t own = h0 + h1 + h2 + h3;
        uint32_t suf = own;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t v = __shfl_down(suf, d, kWave);
            if (lane + d < kWave) suf += v;
        }
        const unsigned long long has = __ballot(suf >= want);
        const int src = 63 - __builtin_clzll(has);            // has != 0: more keys than want
        uint32_t above = suf - own, digit;                    // counted above this lane
        if (above + h3 >= want) digit = 3;
        else if ((above += h3) + h2 >= want) digit = 2;
        else if ((above += h2) + h1 >= want) digit = 1;
        else { above += h1; digit = 0; }
        const uint32_t in_bin = digit == 3 ? h3 : digit == 2 ? h2 : digit == 1 ? h1 : h0;
        digit = (uint32_t)bcast_i32((int)(4 * lane + digit), src);
        want -= (uint32_t)bcast_i32((int)above, src);
        prefix = (prefix << 8) | digit;
        // the whole bin is kept: every key from its lowest up, and the bytes below
        // (as a rule the id's, once the similarity's have singled one key out) decide nothing
        if ((uint32_t)bcast_i32((int)in_bin, src) == want) {
            prefix <<= sh;
            break;
        }
        sync();
    }
    return prefix;
}

// One wave, one (entity e, other o) pair: the unclipped prediction, in every
// lane.  The list has `len` positions; build(j) is position j's key (0: not a
// candidate), dev(j, key) its r_bo - m_b as a double.  keys (kKeysLds) and bins
// (256) are this wave's LDS; the keys stay there for lists of up to kKeysLds
// entries and are rebuilt on every read for longer ones.  With more candidates
// than n_neighbors the n_neighbors-th largest key is found by select_cut:
// exact for any list length.  num and den are summed lane-strided over the
// list positions, then by the wave butterfly.  sync() orders this wave's LDS
// accesses: a workgroup barrier where the wave is the workgroup.
template <typename Build, typename Dev, typename Sync>
__device__ __forceinline__ double pair_predict(uint64_t* keys, uint32_t* bins, int64_t len,
                                               int32_t n_neighbors, int lane, double me,
                                               Build build, Dev dev, Sync sync) {
    const bool in_lds = len <= kKeysLds;
    uint32_t cnt = 0;
    for (int64_t j = lane; j < len; j += kWave) {
        const uint64_t k = build(j);
        if (in_lds) keys[j] = k;
        cnt += k != 0;
    }
    cnt = wave_sum(cnt);
    sync();
    auto key_at = [&](int64_t j) -> uint64_t { return in_lds ? keys[j] : build(j); };

    // keep every candidate (keys are >= 2^31) unless there are more than n_neighbors
    const uint64_t cut = cnt > (uint32_t)n_neighbors
                             ? select_cut(bins, len, (uint32_t)n_neighbors, lane, key_at, sync)
                             : 1;
    double num = 0.0, den = 0.0;
    for (int64_t j = lane; j < len; j += kWave) {
        const uint64_t k = key_at(j);
        if (k >= cut) {                           // k == 0 never is
            const double s = (double)key_sim(k);
            num = num + s * dev(j, k);
            den = den + fabs(s);
        }
    }
    num = wave_sum(num);
    den = wave_sum(den);
    return den > 0.0 ? me + num / den : me;
}

inline bool bad_n_stored(const char* fn, int32_t n_stored) {
    if (n_stored >= 1 && n_stored <= kMaxStored) return false;
    set_error("%s: n_stored=%d (must be in [1, %d])", fn, n_stored, kMaxStored);
    return true;
}

}  // namespace cf
}  // namespace mf
