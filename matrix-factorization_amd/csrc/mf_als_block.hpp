// mf_als_block.hpp -- the pieces shared by the least-squares kernels that give
// one workgroup of 4 waves to an entity: k_als_solve (mf_als.hip),
// k_ials_solve (mf_ials.hip) and k_ials_cg (mf_ials_cg.hip).
//
//   Tiles / tile_row     the upper 32 x 32 MFMA tiles of the symmetric Gramian
//                        (also k_als_wave's and k_gramian's enumeration)
//   weighted_gram_wave   the implicit kernels' chunk pipeline: the weighted
//                        Gramian sum w z z^T and the right-hand side sum cf z
//   check_ials_args      argument checks of the two implicit entry points
//
// The expression order in here is part of the contract: the kernels are
// checked bit for bit against earlier builds (tools/als_bits.py).
//
// The register-tiled elimination and the back substitution of k_als_solve and
// k_ials_solve are NOT in here, on purpose.  As __forceinline__ functions they
// are simplified on their own before they are inlined, and the kernels come
// out different: k_als_solve<2> went from 90 to 110 VGPRs (5 -> 4 waves per
// SIMD) and lost 7-10 % at rank 64 (profiles/als_block/).  The two copies
// differ only in the number of right-hand columns; a fix to one belongs in
// the other.
#pragma once

#include <cmath>
#include <cstdint>

#include "mf_common.hpp"

namespace mf {
namespace alsblk {

constexpr int kThreads = 256;
constexpr int kChunk = 64;           // other-side rows per LDS chunk (32 K-steps)
constexpr int kMaxFactors = 128;

using f32x16 = __attribute__((ext_vector_type(16))) float;

// Upper 32 x 32 tiles of a symmetric (32 NT)^2 matrix: column blocks
// J = 0..NT-1, row blocks I <= J.  In the 4-wave kernels tile q belongs to
// wave q % 4.
template <int NT>
struct Tiles {
    static constexpr int count = NT * (NT + 1) / 2;
    static constexpr int per_wave = (count + 3) / 4;
    static constexpr int I(int q) {
        for (int J = 0, n = 0; J < NT; ++J)
            for (int i = 0; i <= J; ++i, ++n)
                if (n == q) return i;
        return 0;
    }
    static constexpr int J(int q) {
        for (int J = 0, n = 0; J < NT; ++J)
            for (int i = 0; i <= J; ++i, ++n)
                if (n == q) return J;
        return 0;
    }
};

// row of accumulator register i in a 32 x 32 tile (lane half h); the column
// is lane & 31
__device__ __forceinline__ int tile_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// float4 column c4 of one row (k values, zero past k); vec: rows 16-byte aligned
__device__ __forceinline__ float4 load_row4(const float* row, int c4, int k, bool vec) {
    float4 v;
    const int c = 4 * c4;
    if (vec) {
        v = *reinterpret_cast<const float4*>(row + (c < k ? c : 0));
        if (c >= k) v = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        v.x = c + 0 < k ? row[c + 0] : 0.f;
        v.y = c + 1 < k ? row[c + 1] : 0.f;
        v.z = c + 2 < k ? row[c + 2] : 0.f;
        v.w = c + 3 < k ? row[c + 3] : 0.f;
    }
    return v;
}

inline int nt_of(int k) { return k <= 32 ? 1 : (k <= 64 ? 2 : 4); }   // 96 columns do not tile 256 lanes
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- the weighted Gramian of an observed list (implicit feedback) -------------

struct ListArgs {
    const int64_t* ptr;        // n_entities + 1
    const int32_t* other;      // other-side id per observation (CSR order)
    const float* r;            // strength per observation (CSR order)
    const float* oq;           // other-side factor rows (row-major, k)
    int32_t k;
    int32_t vec;               // oq rows 16-byte aligned
    float alpha;
};

// One K-step (two chunk rows) of wave WV: lane (r, h) holds row 2 s + h.  The
// A operand of every tile is the row scaled by w; the right-hand side of
// column block WV adds cf z (cf = (1 + w) [r > 0]).
template <int NT, int WV>
__device__ __forceinline__ void weighted_kstep(const float* zr, float w, float cf, int r,
                                               f32x16 (&acc)[Tiles<NT>::per_wave], float& fsum) {
    using TL = Tiles<NT>;
    float zv[NT], zw[NT];
#pragma unroll
    for (int I = 0; I < NT; ++I) {
        zv[I] = zr[32 * I + r];
        zw[I] = zv[I] * w;
    }
#pragma unroll
    for (int s = 0; s < TL::per_wave; ++s) {
        const int q = WV + 4 * s;
        if (q < TL::count)
            acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(zw[TL::I(q)], zv[TL::J(q)], acc[s],
                                                          0, 0, 0);
    }
    if constexpr (WV < NT) fsum = __builtin_fmaf(cf, zv[WV], fsum);
}

// The weighted Gramian of one entity on wave WV's tiles, into acc (zeroed
// here), and the right-hand sums of column block WV into fsum (lane (r, h):
// column 32 WV + r over the chunk rows of parity h).  Chunks of kChunk other-
// side rows are software-pipelined through registers: while the MFMAs consume
// chunk c from Zc, the rows of chunk c + 1 (ids loaded one chunk earlier) are
// in flight.  Thread t moves float4 column t % C4 of rows t / C4 + RPP w;
// thread t < kChunk also fetches the strength of chunk row t (w_n to wc, cf_n
// to cc).  Ends with a barrier: the caller may reuse Zc at once.
template <int NT, int WV>
__device__ __forceinline__ void weighted_gram_wave(const ListArgs& A, float* Zc, float* wc,
                                                   float* cc, int64_t p0, int64_t cnt, int lane,
                                                   f32x16 (&acc)[Tiles<NT>::per_wave],
                                                   float& fsum) {
    using TL = Tiles<NT>;
    constexpr int KP = NT * 32;
    constexpr int C4 = KP / 4;                    // float4 per row
    constexpr int RPP = kThreads / C4;            // rows per pass of the block
    constexpr int NW = kChunk / RPP;              // float4 per thread per chunk
    static_assert(kThreads % C4 == 0 && kChunk % RPP == 0, "chunk tiling");
    const int tid = threadIdx.x;
    const int c4 = tid % C4, n0 = tid / C4;
    const int k = A.k;
    const bool vec = A.vec != 0;
#pragma unroll
    for (int s = 0; s < TL::per_wave; ++s)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[s][i] = 0.f;
    const int r = lane & 31, h = lane >> 5;
    fsum = 0.f;

    auto load_ids = [&](int64_t c0, int (&ids)[NW], float& rr) __attribute__((always_inline)) {
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int64_t n = c0 + n0 + RPP * w;
            ids[w] = n < cnt ? A.other[p0 + n] : -1;
        }
        const int64_t nt = c0 + tid;
        rr = (tid < kChunk && nt < cnt) ? A.r[p0 + nt] : 0.f;
    };
    auto load_rows = [&](const int (&ids)[NW], float4 (&v)[NW]) __attribute__((always_inline)) {
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int id = ids[w] >= 0 ? ids[w] : 0;
            v[w] = load_row4(A.oq + (int64_t)id * k, c4, k, vec);
        }
    };

    int ids[NW];
    float rr;
    float4 v[NW];
    load_ids(0, ids, rr);
    load_rows(ids, v);
    float rr_cur = rr;
    load_ids(kChunk, ids, rr);                    // chunk 1's ids (may be empty)
    for (int64_t c0 = 0; c0 < cnt; c0 += kChunk) {
        const int m = (int)min((int64_t)kChunk, cnt - c0);
        __syncthreads();                          // previous chunk consumed
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const bool ok = c0 + n0 + RPP * w < cnt;
            *reinterpret_cast<float4*>(Zc + (n0 + RPP * w) * KP + 4 * c4) =
                ok ? v[w] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (tid < kChunk) {
            const float w = tid < m ? A.alpha * rr_cur : 0.f;
            wc[tid] = w;
            cc[tid] = (tid < m && rr_cur > 0.f) ? 1.f + w : 0.f;
        }
        __syncthreads();
        // next chunk: rows from the ids already loaded, then the ids after it
        const float rr_next = rr;
        load_rows(ids, v);
        load_ids(c0 + 2 * kChunk, ids, rr);
        rr_cur = rr_next;
        const int steps = (m + 1) >> 1;
        for (int s = 0; s < steps; ++s) {
            const int n = 2 * s + h;                  // rows past m are zero rows
            weighted_kstep<NT, WV>(Zc + n * KP, wc[n], cc[n], r, acc, fsum);
        }
    }
    __syncthreads();                              // Zc may be reused (as M) from here
}

// ---- argument checks of mf_ials_sweep / mf_ials_sweep_cg ------------------------
//
// fn names the entry point in the messages.  max_steps > 0: cg_steps must lie
// in [1, max_steps] (the direct solve passes 0 and has no such argument).
// With n_entities == 0 the pointers are not looked at.
inline int check_ials_args(const char* fn, const int64_t* entity_ptr, const int32_t* other_ids,
                           const void* strengths, int32_t n_entities, const void* other_features,
                           const void* gram, const void* features, int32_t n_factors,
                           int32_t dtype, double alpha, double reg, int32_t cg_steps,
                           int32_t max_steps) {
    if (dtype != MF_F32) {
        set_error("%s: dtype=%d (float32 only: f32-input MFMA)", fn, dtype);
        return MF_ERR_INVALID;
    }
    if (n_factors < 1 || n_factors > kMaxFactors) {
        set_error("%s: n_factors=%d (must be in [1, %d])", fn, n_factors, kMaxFactors);
        return MF_ERR_INVALID;
    }
    if (!std::isfinite(alpha) || alpha < 0) {
        set_error("%s: alpha=%g (must be finite and >= 0)", fn, alpha);
        return MF_ERR_INVALID;
    }
    if (!std::isfinite(reg) || reg <= 0) {
        set_error("%s: reg=%g (must be finite and > 0)", fn, reg);
        return MF_ERR_INVALID;
    }
    if (max_steps > 0 && (cg_steps < 1 || cg_steps > max_steps)) {
        set_error("%s: cg_steps=%d (must be in [1, %d])", fn, cg_steps, max_steps);
        return MF_ERR_INVALID;
    }
    if (n_entities < 0) {
        set_error("%s: n_entities=%d (must be >= 0)", fn, n_entities);
        return MF_ERR_INVALID;
    }
    if (n_entities == 0) return MF_OK;
    const void* need[] = {entity_ptr, other_ids, strengths, other_features, gram, features};
    const char* names[] = {"entity_ptr", "other_ids", "strengths", "other_features", "gram",
                           "features"};
    return null_arg(fn, need, names, 6) ? MF_ERR_INVALID : MF_OK;
}

}  // namespace alsblk
}  // namespace mf
