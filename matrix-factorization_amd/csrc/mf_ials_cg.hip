// mf_ials_cg.hip -- implicit-feedback ALS half-sweep by conjugate gradients
// (Takacs, Pilaszy & Tikk 2011), the inexact companion of mf_ials.hip's
// k_ials_solve.  For entity e with a non-empty list
//
//   A = G + sum_n w_n z_n z_n^T + reg I,   w_n = alpha r_n
//   b = sum_{n: r_n > 0} (1 + w_n) z_n,    x = e's current row (warm start)
//
//   res = b - A x;  p = res;  rs = res . res
//   repeat cg_steps times:
//       if not (rs > 1e-30): stop
//       Ap = A p;  a = rs / (p . Ap)
//       x += a p;  res -= a Ap;  rs' = res . res
//       p = res + (rs' / rs) p;  rs = rs'
//   write x
//
//   k_ials_cg   one workgroup (4 waves) per entity.  Phase 1 is k_ials_solve's
//      assembly (the weighted Gramian on MFMA with A operand = w_n z_n, the
//      right-hand side on the VALU beside it), so every list row is read once
//      per half-sweep however many steps follow; the tiles + G + reg I go to
//      LDS as M[KP][KP + 1], b to a vector beside it.  Phase 2 runs the
//      recurrence on M: 256 / KP threads per matrix row, x / res / p / Ap of
//      the row in registers, p also in LDS for the matvec, each dot one
//      workgroup reduction in a fixed order broadcast through LDS (every
//      thread branches on the same bits).  No atomics: the same input gives
//      the same bits.
//
// mf_ials.hip is untouched; the shared pieces (tile enumeration, chunk
// pipeline, dump) are restated here in namespace mf::ials_cg.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "mf_common.hpp"

namespace mf {
namespace ials_cg {

constexpr int kThreads = 256;
constexpr int kChunk = 64;           // rows per LDS chunk (32 K-steps)
constexpr int kMaxFactors = 128;
constexpr int kMaxSteps = 1024;
constexpr float kRsStop = 1e-30f;    // the recurrence stops once rs is not above this

using f32x16 = __attribute__((ext_vector_type(16))) float;

// Upper 32 x 32 tiles of a symmetric (32 NT)^2 matrix: column blocks
// J = 0..NT-1, row blocks I <= J; tile q belongs to wave q % 4 (the
// enumeration of mf_als.hip's AlsTiles).
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

struct CgArgs {
    const int64_t* ptr;        // n_entities + 1
    const int32_t* other;      // other-side id per observation (CSR order)
    const float* r;            // strength per observation (CSR order)
    const float* oq;           // other-side factor rows (row-major, k)
    const float* G;            // (k, k): oq^T oq over all rows
    float* feat;               // factor rows (n_entities x k): warm start, result
    int32_t k;
    int32_t vec;               // oq rows 16-byte aligned
    float alpha;
    float reg;
    int32_t steps;
};

// One K-step (two chunk rows) of wave WV: lane (r, h) holds row 2 s + h.  The
// A operand of every tile is the row scaled by w; the right-hand side of
// column block WV adds cf z (cf = (1 + w) [r > 0]).
template <int NT, int WV>
__device__ __forceinline__ void cg_kstep(const float* zr, float w, float cf, int r,
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

// Accumulator tiles + the matching tile of G (+ reg on the diagonal; padding
// dimensions k <= a < KP are decoupled: zero row and column, diagonal 1)
// -> M (row stride LD), an off-diagonal tile also transposed; the right-hand
// sums of column block WV -> bv.
template <int NT, int WV>
__device__ __forceinline__ void cg_dump(const CgArgs& A, float* M, float* bv, int LD, int lane,
                                        const f32x16 (&acc)[Tiles<NT>::per_wave], float fsum) {
    using TL = Tiles<NT>;
    const int col = lane & 31, h = lane >> 5;
    const int k = A.k;
#pragma unroll
    for (int s = 0; s < TL::per_wave; ++s) {
        const int q = WV + 4 * s;
        if (q >= TL::count) continue;
        const int I = TL::I(q), J = TL::J(q);
        const int c = 32 * J + col;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = 32 * I + tile_row(i, h);
            const float g = (row < k && c < k) ? A.G[row * k + c] : 0.f;
            float v = acc[s][i] + g;
            if (I == J && row == c) v = row < k ? v + A.reg : 1.f;
            M[row * LD + c] = v;
            if (I < J) M[c * LD + row] = v;
        }
    }
    if constexpr (WV < NT) {
        // rows h = 0 and h = 1 of every K-step: lanes r and r + 32
        fsum = fsum + __shfl_xor(fsum, 32, kWave);
        if (h == 0) bv[32 * WV + col] = fsum;
    }
}

// The weighted Gramian of one entity on wave WV's tiles: k_ials_solve's chunk
// pipeline (chunk c + 1's rows in registers, ids one chunk further ahead).
// Thread t < kChunk also fetches the strength of chunk row t.
template <int NT, int WV>
__device__ __forceinline__ void cg_gram_wave(const CgArgs& A, float* Zc, float* wc, float* cc,
                                             int64_t p0, int64_t cnt, int lane, float* M,
                                             float* bv, int LD) {
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
    f32x16 acc[TL::per_wave];
#pragma unroll
    for (int s = 0; s < TL::per_wave; ++s)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[s][i] = 0.f;
    const int r = lane & 31, h = lane >> 5;
    float fsum = 0.f;

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
            cg_kstep<NT, WV>(Zc + n * KP, wc[n], cc[n], r, acc, fsum);
        }
    }
    __syncthreads();                              // Zc is reused as M below
    cg_dump<NT, WV>(A, M, bv, LD, lane, acc, fsum);
}

// Floats of the region Zc / wc / cc and M share (a multiple of 4: the vectors
// behind it stay 16-byte aligned).
template <int NT>
constexpr int region_floats() {
    constexpr int KP = NT * 32;
    constexpr int m = KP * (KP + 1), z = kChunk * KP + 2 * kChunk;
    return ((m > z ? m : z) + 3) & ~3;
}

template <int NT>
__global__ __launch_bounds__(kThreads, 2) void k_ials_cg(CgArgs A) {
    constexpr int KP = NT * 32;
    constexpr int LD = KP + 1;                    // odd stride: row and column walks conflict-free
    constexpr int TPR = kThreads / KP;            // threads per matrix row: 8 / 4 / 2
    constexpr int CP = KP / TPR;                  // columns per thread: 4 / 16 / 64
    extern __shared__ __align__(16) float lds[];
    float* Zc = lds;                              // [kChunk][KP]   (assembly)
    float* wc = lds + kChunk * KP;                // [kChunk] w_n
    float* cc = wc + kChunk;                      // [kChunk] (1 + w_n) [r_n > 0]
    float* M = lds;                               // [KP][LD]       (CG)
    float* bv = lds + region_floats<NT>();        // [KP] right-hand side
    float* pv = bv + KP;                          // [KP] search direction
    float* red = pv + KP;                         // [2][4] per-wave partial dots

    const int e = blockIdx.x;
    const int64_t p0 = A.ptr[e], cnt = A.ptr[e + 1] - p0;
    if (cnt <= 0) return;                         // empty list: the row is kept
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wv = tid / kWave;
    const int k = A.k;

    // thread (row, sub) of phase 2 owns element `row` of x / res / p (every
    // sub holds the same bits); the warm start is in flight during phase 1
    const int row = tid / TPR, sub = tid % TPR;
    float* feat = A.feat + (int64_t)e * k;
    float x = row < k ? feat[row] : 0.f;

    switch (wv) {
        case 0: cg_gram_wave<NT, 0>(A, Zc, wc, cc, p0, cnt, lane, M, bv, LD); break;
        case 1: cg_gram_wave<NT, 1>(A, Zc, wc, cc, p0, cnt, lane, M, bv, LD); break;
        case 2: cg_gram_wave<NT, 2>(A, Zc, wc, cc, p0, cnt, lane, M, bv, LD); break;
        default: cg_gram_wave<NT, 3>(A, Zc, wc, cc, p0, cnt, lane, M, bv, LD); break;
    }

    // ---- CG on M.  Sub s of a row walks columns s CP .. s CP + CP - 1,
    // started `rot` columns in, so that the 32 lanes of one ds_read_b32 group
    // (32 / TPR consecutive rows x TPR subs; bank = (row + column) mod 32 at
    // the odd stride) hit 32 different banks; the lanes of one sub read the
    // same element of p (a broadcast).
    constexpr int rot_unit = NT == 4 ? 16 : (NT == 2 ? 8 : 0);
    const int rot = NT == 4 ? rot_unit * sub : (NT == 2 ? rot_unit * (sub >> 1) : 0);
    const float* Mrow = M + row * LD + sub * CP;
    const float* prow = pv + sub * CP;

    // (A v)[row] for the v in pv: four partial chains per thread (columns
    // j mod 4), summed in a fixed order, then the subs by an xor butterfly
    // (every sub ends with the same bits)
    auto matvec = [&]() __attribute__((always_inline)) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 4
        for (int j = 0; j < CP; j += 4) {
            const int j0 = (j + 0 + rot) & (CP - 1), j1 = (j + 1 + rot) & (CP - 1);
            const int j2 = (j + 2 + rot) & (CP - 1), j3 = (j + 3 + rot) & (CP - 1);
            s0 = s0 + Mrow[j0] * prow[j0];
            s1 = s1 + Mrow[j1] * prow[j1];
            s2 = s2 + Mrow[j2] * prow[j2];
            s3 = s3 + Mrow[j3] * prow[j3];
        }
        float s = (s0 + s1) + (s2 + s3);
#pragma unroll
        for (int o = 1; o < TPR; o <<= 1) s = s + __shfl_xor(s, o, kWave);
        return s;
    };
    // sum over the rows of v (one value per row, taken from sub 0): wave
    // butterfly, then the four waves in wave order; every thread reads the
    // same four partials, so the result is workgroup-uniform bit for bit
    auto block_dot = [&](float v, float* part) __attribute__((always_inline)) {
        v = sub == 0 ? v : 0.f;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) v = v + __shfl_xor(v, o, kWave);
        if (lane == 0) part[wv] = v;
        __syncthreads();
        return ((part[0] + part[1]) + part[2]) + part[3];
    };

    if (sub == 0) pv[row] = x;
    __syncthreads();                              // M, bv, pv = x complete
    float res = bv[row] - matvec();
    float p = res;
    float rs = block_dot(res * res, red + 4);
    for (int it = 0; it < A.steps; ++it) {
        if (!(rs > kRsStop)) break;               // uniform: rs is the same bits everywhere
        if (sub == 0) pv[row] = p;
        __syncthreads();
        const float ap = matvec();
        const float pap = block_dot(p * ap, red);
        const float a = rs / pap;
        x = x + a * p;
        res = res - a * ap;
        const float rs2 = block_dot(res * res, red + 4);
        p = res + (rs2 / rs) * p;
        rs = rs2;
    }
    if (sub == 0 && row < k) feat[row] = x;
}

template <int NT>
int cg_go(const CgArgs& a, int32_t n, hipStream_t stream) {
    constexpr int KP = NT * 32;
    const size_t lds = (size_t)(region_floats<NT>() + 2 * KP + 8) * sizeof(float);
    auto kfn = k_ials_cg<NT>;
    MF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kfn),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kfn, dim3((unsigned)n), dim3(kThreads), lds, stream, a);
    MF_HIP_CHECK(hipGetLastError());
    return MF_OK;
}

inline int nt_of(int k) { return k <= 32 ? 1 : (k <= 64 ? 2 : 4); }   // 96 columns do not tile 256 lanes
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace ials_cg

void touch_ials_cg(hipStream_t s) { hipLaunchKernelGGL(k_touch<9>, dim3(1), dim3(64), 0, s); }

}  // namespace mf

using namespace mf;

extern "C" int mf_ials_sweep_cg(const int64_t* entity_ptr, const int32_t* other_ids,
                                const void* strengths, int32_t n_entities,
                                const void* other_features, const void* gram, void* features,
                                int32_t n_factors, int32_t dtype, double alpha, double reg,
                                int32_t cg_steps, void* stream) {
    if (dtype != MF_F32) {
        set_error("mf_ials_sweep_cg: dtype=%d (float32 only: f32-input MFMA)", dtype);
        return MF_ERR_INVALID;
    }
    if (n_factors < 1 || n_factors > ials_cg::kMaxFactors) {
        set_error("mf_ials_sweep_cg: n_factors=%d (must be in [1, %d])", n_factors,
                  ials_cg::kMaxFactors);
        return MF_ERR_INVALID;
    }
    if (!std::isfinite(alpha) || alpha < 0) {
        set_error("mf_ials_sweep_cg: alpha=%g (must be finite and >= 0)", alpha);
        return MF_ERR_INVALID;
    }
    if (!std::isfinite(reg) || reg <= 0) {
        set_error("mf_ials_sweep_cg: reg=%g (must be finite and > 0)", reg);
        return MF_ERR_INVALID;
    }
    if (cg_steps < 1 || cg_steps > ials_cg::kMaxSteps) {
        set_error("mf_ials_sweep_cg: cg_steps=%d (must be in [1, %d])", cg_steps,
                  ials_cg::kMaxSteps);
        return MF_ERR_INVALID;
    }
    if (n_entities < 0) {
        set_error("mf_ials_sweep_cg: n_entities=%d (must be >= 0)", n_entities);
        return MF_ERR_INVALID;
    }
    if (n_entities == 0) return MF_OK;
    const void* need[] = {entity_ptr, other_ids, strengths, other_features, gram, features};
    const char* names[] = {"entity_ptr", "other_ids", "strengths", "other_features", "gram",
                           "features"};
    for (int i = 0; i < 6; ++i)
        if (!need[i]) {
            set_error("mf_ials_sweep_cg: %s is NULL", names[i]);
            return MF_ERR_INVALID;
        }
    ials_cg::CgArgs a;
    a.ptr = entity_ptr; a.other = other_ids; a.r = static_cast<const float*>(strengths);
    a.oq = static_cast<const float*>(other_features);
    a.G = static_cast<const float*>(gram);
    a.feat = static_cast<float*>(features);
    a.k = n_factors;
    a.vec = (n_factors % 4 == 0 && ials_cg::aligned16(other_features)) ? 1 : 0;
    a.alpha = (float)alpha; a.reg = (float)reg;
    a.steps = cg_steps;
    hipStream_t s = (hipStream_t)stream;
    switch (ials_cg::nt_of(n_factors)) {
        case 1: return ials_cg::cg_go<1>(a, n_entities, s);
        case 2: return ials_cg::cg_go<2>(a, n_entities, s);
        default: return ials_cg::cg_go<4>(a, n_entities, s);
    }
}
