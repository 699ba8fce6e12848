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
// The tile enumeration and the chunk pipeline of phase 1 are
// mf_als_block.hpp's, shared with k_ials_solve; the dump differs (it folds reg
// and the padding diagonal in and writes b to its own vector).
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "mf_als_block.hpp"
#include "mf_common.hpp"

namespace mf {
namespace ials_cg {

// the 4-wave layout's constants, tile enumeration and chunk pipeline
using alsblk::aligned16;
using alsblk::f32x16;
using alsblk::kChunk;
using alsblk::kThreads;
using alsblk::ListArgs;
using alsblk::nt_of;
using alsblk::tile_row;
using alsblk::Tiles;

constexpr int kMaxSteps = 1024;
constexpr float kRsStop = 1e-30f;    // the recurrence stops once rs is not above this

struct CgArgs : ListArgs {
    const float* G;            // (k, k): oq^T oq over all rows
    float* feat;               // factor rows (n_entities x k): warm start, result
    float reg;
    int32_t steps;
};

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

// The weighted Gramian of one entity on wave WV's tiles (the shared chunk
// pipeline), then the tiles to M and the right-hand side to bv.
template <int NT, int WV>
__device__ __forceinline__ void cg_gram_wave(const CgArgs& A, float* Zc, float* wc, float* cc,
                                             int64_t p0, int64_t cnt, int lane, float* M,
                                             float* bv, int LD) {
    f32x16 acc[Tiles<NT>::per_wave];
    float fsum;
    alsblk::weighted_gram_wave<NT, WV>(A, Zc, wc, cc, p0, cnt, lane, acc, fsum);
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

}  // namespace ials_cg

void touch_ials_cg(hipStream_t s) { hipLaunchKernelGGL(k_touch<9>, dim3(1), dim3(64), 0, s); }

}  // namespace mf

using namespace mf;

extern "C" int mf_ials_sweep_cg(const int64_t* entity_ptr, const int32_t* other_ids,
                                const void* strengths, int32_t n_entities,
                                const void* other_features, const void* gram, void* features,
                                int32_t n_factors, int32_t dtype, double alpha, double reg,
                                int32_t cg_steps, void* stream) {
    const int rc = alsblk::check_ials_args("mf_ials_sweep_cg", entity_ptr, other_ids, strengths,
                                           n_entities, other_features, gram, features, n_factors,
                                           dtype, alpha, reg, cg_steps, ials_cg::kMaxSteps);
    if (rc != MF_OK || n_entities == 0) return rc;
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
