// mf_ials.hip -- implicit-feedback ALS (Hu, Koren & Volinsky 2008: confidence-
// weighted least squares over ALL user x item pairs).  No reference
// counterpart.  With strengths r_n >= 0 on an entity's observed list,
// confidence c = 1 + alpha r, preference p = [r > 0], unobserved pairs c = 1,
// p = 0, the half-sweep of entity e against the other side's rows z is
//
//   (G + sum_n w_n z_n z_n^T + reg I) x_e = sum_{n: r_n > 0} (1 + w_n) z_n,
//   G = Z^T Z over ALL rows of the other side,  w_n = alpha r_n  (n in e's list)
//
// so the dense "every pair" term is one shared k x k Gramian and only the
// correction runs over the observed list.  Two kernels:
//
//   k_gramian + k_gramian_reduce   G = F^T F of a row-major (n, k) matrix.
//      Workgroups take slabs of kGramSlab rows, staged through LDS in chunks
//      of 64 rows and consumed by v_mfma_f32_32x32x2_f32 (upper 32 x 32 tiles,
//      mf_als_block.hpp's enumeration); each slab's raw accumulator tiles go to
//      the workspace and the second kernel sums the slabs in slab order in
//      FP64 (no float atomics: the same input gives the same bits).
//   k_ials_solve   one workgroup (4 waves) per entity, k_als_solve's layout:
//      the weighted Gramian on MFMA (A operand = w_n z_n, B operand = z_n),
//      the right-hand side on the VALU beside it, + G + reg I when the tiles
//      go to LDS, symmetric elimination without pivoting (the matrix is SPD:
//      w >= 0, reg > 0), back substitution on wave 0.  No bias border.
//      The tile enumeration and the chunk pipeline are mf_als_block.hpp's,
//      shared with k_ials_cg; the elimination and the back substitution are
//      k_als_solve's, restated here (mf_als_block.hpp says why).
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "mf_als_block.hpp"
#include "mf_common.hpp"

namespace mf {
namespace ials {

// the 4-wave layout's constants, tile enumeration and chunk pipeline
using alsblk::aligned16;
using alsblk::f32x16;
using alsblk::kChunk;
using alsblk::kMaxFactors;
using alsblk::kThreads;
using alsblk::ListArgs;
using alsblk::load_row4;
using alsblk::nt_of;
using alsblk::tile_row;
using alsblk::Tiles;

constexpr int kGramSlab = 1024;      // rows per workgroup of k_gramian
constexpr int kTileFloats = 32 * 32;

// ---- F^T F -------------------------------------------------------------------

struct GramArgs {
    const float* F;            // (n, k) row-major
    int64_t n;
    int32_t k;
    int32_t vec;               // rows 16-byte aligned (k % 4 == 0, aligned base)
    float* ws;                 // [n_slabs][Tiles::count][16][64] raw accumulators
    int32_t n_slabs;
    float* G;                  // (k, k)
};

// Wave WV's tiles over one slab.  Thread t moves float4 column t % C4 of rows
// t / C4 + RPP w of each chunk; chunk c + 1 is in registers while the MFMAs
// consume chunk c from LDS.
template <int NT, int WV>
__device__ __forceinline__ void gram_wave(const GramArgs& A, float* Zc, int64_t row0, int rows,
                                          int lane) {
    using TL = Tiles<NT>;
    constexpr int KP = NT * 32;
    constexpr int C4 = KP / 4;
    constexpr int RPP = kThreads / C4;
    constexpr int NW = kChunk / RPP;
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

    auto load_rows = [&](int c0, float4 (&v)[NW]) __attribute__((always_inline)) {
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int n = c0 + n0 + RPP * w;
            v[w] = n < rows ? load_row4(A.F + (row0 + n) * k, c4, k, vec)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    float4 v[NW];
    load_rows(0, v);
    for (int c0 = 0; c0 < rows; c0 += kChunk) {
        const int m = min(kChunk, rows - c0);
        __syncthreads();                          // previous chunk consumed
#pragma unroll
        for (int w = 0; w < NW; ++w)
            *reinterpret_cast<float4*>(Zc + (n0 + RPP * w) * KP + 4 * c4) = v[w];
        __syncthreads();
        load_rows(c0 + kChunk, v);                // rows past the slab: zeros, no load
        const int steps = (m + 1) >> 1;
        for (int s = 0; s < steps; ++s) {
            const float* zr = Zc + (2 * s + h) * KP;   // rows past m are zero rows
            float zv[NT];
#pragma unroll
            for (int I = 0; I < NT; ++I) zv[I] = zr[32 * I + r];
#pragma unroll
            for (int t = 0; t < TL::per_wave; ++t) {
                const int q = WV + 4 * t;
                if (q < TL::count)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(zv[TL::I(q)], zv[TL::J(q)],
                                                                  acc[t], 0, 0, 0);
            }
        }
    }
    // raw accumulators, register-major: coalesced over the lanes
    float* out = A.ws + (int64_t)blockIdx.x * TL::count * kTileFloats;
#pragma unroll
    for (int t = 0; t < TL::per_wave; ++t) {
        const int q = WV + 4 * t;
        if (q >= TL::count) continue;
#pragma unroll
        for (int i = 0; i < 16; ++i) out[q * kTileFloats + i * kWave + lane] = acc[t][i];
    }
}

template <int NT>
__global__ __launch_bounds__(kThreads, 2) void k_gramian(GramArgs A) {
    extern __shared__ __align__(16) float lds[];  // [kChunk][32 NT]
    const int64_t row0 = (int64_t)blockIdx.x * kGramSlab;
    const int rows = (int)min((int64_t)kGramSlab, A.n - row0);
    const int lane = threadIdx.x & (kWave - 1);
    switch (threadIdx.x / kWave) {
        case 0: gram_wave<NT, 0>(A, lds, row0, rows, lane); break;
        case 1: gram_wave<NT, 1>(A, lds, row0, rows, lane); break;
        case 2: gram_wave<NT, 2>(A, lds, row0, rows, lane); break;
        default: gram_wave<NT, 3>(A, lds, row0, rows, lane); break;
    }
}

// One thread per accumulator element of the upper tiles: the slabs summed in
// slab order in FP64, rounded once, written to both triangles.
template <int NT>
__global__ __launch_bounds__(kThreads) void k_gramian_reduce(GramArgs A) {
    using TL = Tiles<NT>;
    const int e = blockIdx.x * kThreads + threadIdx.x;       // < count * 1024
    if (e >= TL::count * kTileFloats) return;
    const int q = e / kTileFloats, i = (e % kTileFloats) / kWave, lane = e % kWave;
    int I = 0, J = 0;
#pragma unroll
    for (int qq = 0; qq < TL::count; ++qq)
        if (qq == q) { I = TL::I(qq); J = TL::J(qq); }
    const int row = 32 * I + tile_row(i, lane >> 5), col = 32 * J + (lane & 31);
    const int k = A.k;
    if (row >= k || col >= k) return;
    const float* p = A.ws + e;
    const int64_t stride = (int64_t)TL::count * kTileFloats;
    double s = 0.0;
    for (int b = 0; b < A.n_slabs; ++b) s += (double)p[b * stride];
    const float g = (float)s;
    A.G[row * k + col] = g;
    if (I < J) A.G[col * k + row] = g;
}

template <int NT>
int gram_go(const GramArgs& a, hipStream_t stream) {
    using TL = Tiles<NT>;
    const size_t lds = (size_t)kChunk * NT * 32 * sizeof(float);
    hipLaunchKernelGGL(k_gramian<NT>, dim3((unsigned)a.n_slabs), dim3(kThreads), lds, stream, a);
    MF_HIP_CHECK(hipGetLastError());
    const int blocks = (TL::count * kTileFloats + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(k_gramian_reduce<NT>, dim3(blocks), dim3(kThreads), 0, stream, a);
    MF_HIP_CHECK(hipGetLastError());
    return MF_OK;
}

inline int64_t slabs_of(int64_t n) { return (n + kGramSlab - 1) / kGramSlab; }
inline size_t gram_ws_bytes(int64_t n, int k) {
    const int nt = nt_of(k);
    return (size_t)slabs_of(n) * (size_t)(nt * (nt + 1) / 2) * kTileFloats * sizeof(float);
}

// ---- the per-entity solve ------------------------------------------------------

struct SolveArgs : ListArgs {
    const float* G;            // (k, k): oq^T oq over all rows
    float* feat;               // solved factor rows (n_entities x k)
    float reg;
};

// Accumulator tiles + the matching tile of G -> M (row stride LD), an
// off-diagonal tile also transposed; the right-hand sums of column block WV
// -> column KP.
template <int NT, int WV>
__device__ __forceinline__ void solve_dump(const SolveArgs& A, float* M, int LD, int lane,
                                           const f32x16 (&acc)[Tiles<NT>::per_wave],
                                           float fsum) {
    using TL = Tiles<NT>;
    constexpr int KP = NT * 32;
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
            const float v = acc[s][i] + g;
            M[row * LD + c] = v;
            if (I < J) M[c * LD + row] = v;
        }
    }
    if constexpr (WV < NT) {
        // rows h = 0 and h = 1 of every K-step: lanes r and r + 32
        fsum = fsum + __shfl_xor(fsum, 32, kWave);
        if (h == 0) M[(32 * WV + col) * LD + KP] = fsum;
    }
}

// The weighted Gramian of one entity on wave WV's tiles (the shared chunk
// pipeline), then the tiles to M.
template <int NT, int WV>
__device__ __forceinline__ void solve_gram_wave(const SolveArgs& A, float* Zc, float* wc,
                                                float* cc, int64_t p0, int64_t cnt, int lane,
                                                float* M, int LD) {
    f32x16 acc[Tiles<NT>::per_wave];
    float fsum;
    alsblk::weighted_gram_wave<NT, WV>(A, Zc, wc, cc, p0, cnt, lane, acc, fsum);
    solve_dump<NT, WV>(A, M, LD, lane, acc, fsum);
}

template <int NT>
__global__ __launch_bounds__(kThreads, 2) void k_ials_solve(SolveArgs A) {
    constexpr int KP = NT * 32;
    constexpr int LD = KP + 1;                    // odd stride: column reads conflict-free
    extern __shared__ __align__(16) float lds[];
    float* Zc = lds;                              // [kChunk][KP]   (Gramian phase)
    float* wc = lds + kChunk * KP;                // [kChunk] w_n
    float* cc = wc + kChunk;                      // [kChunk] (1 + w_n) [r_n > 0]
    float* M = lds;                               // [KP][LD]       (solve phase)

    const int e = blockIdx.x;
    const int64_t p0 = A.ptr[e], cnt = A.ptr[e + 1] - p0;
    if (cnt <= 0) return;                         // empty list: the row is kept
    const int lane = threadIdx.x & (kWave - 1);
    const int wv = threadIdx.x / kWave;
    const int k = A.k;

    switch (wv) {
        case 0: solve_gram_wave<NT, 0>(A, Zc, wc, cc, p0, cnt, lane, M, LD); break;
        case 1: solve_gram_wave<NT, 1>(A, Zc, wc, cc, p0, cnt, lane, M, LD); break;
        case 2: solve_gram_wave<NT, 2>(A, Zc, wc, cc, p0, cnt, lane, M, LD); break;
        default: solve_gram_wave<NT, 3>(A, Zc, wc, cc, p0, cnt, lane, M, LD); break;
    }
    __syncthreads();

    // ---- symmetric elimination, register-tiled as in k_als_solve: thread
    // (ty, tx) of a 16 x 16 grid holds rows ty + 16x and columns tx + 16y of
    // [A | f].  Pivots in groups of four, one barrier per group: the wave
    // holding rows j0..j0+3 publishes them to a double-buffered LDS block;
    // every thread eliminates the 4 x 4 diagonal block redundantly and applies
    // the rank-4 update to its trailing elements (multipliers of row a are the
    // pivot rows at column a, by symmetry).
    constexpr int RX = KP / 16;                   // rows per thread
    constexpr int CY = KP / 16 + 1;               // columns per thread (+ f)
    constexpr int CW = 16 * CY;                   // published row width
    __shared__ float rowbuf[2][4][CW];
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    float m[RX][CY];
#pragma unroll
    for (int x = 0; x < RX; ++x) {
        const int a = ty + 16 * x;
#pragma unroll
        for (int y = 0; y < CY; ++y) {
            const int b = tx + 16 * y;
            float v = b < KP + 1 ? M[a * LD + b] : 0.f;
            // + reg on the diagonal; padding dimensions (k <= a < KP) are
            // decoupled zero rows: pivot 1, solution 0
            if (a == b) v = a < k ? v + A.reg : 1.f;
            m[x][y] = v;
        }
    }
#pragma unroll
    for (int jb = 0; jb < RX; ++jb) {
#pragma clang loop unroll(disable)
        for (int jq = 0; jq < 4; ++jq) {
            const int j0 = 16 * jb + 4 * jq;
            float (*rb)[CW] = rowbuf[jq & 1];
            const bool owner = (ty >> 2) == jq;
            if (owner) {
#pragma unroll
                for (int y = jb; y < CY; ++y) rb[ty & 3][tx + 16 * y] = m[jb][y];
            }
            __syncthreads();
            float D[4][4], PR[4][CY], inv[4], f[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int c = 0; c < 4; ++c) D[r][c] = rb[r][j0 + c];
#pragma unroll
                for (int y = jb; y < CY; ++y) PR[r][y] = rb[r][tx + 16 * y];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                inv[r] = 1.f / D[r][r];
#pragma unroll
                for (int r2 = r + 1; r2 < 4; ++r2) {
                    f[r][r2] = D[r][r2] * inv[r];
#pragma unroll
                    for (int c = r2; c < 4; ++c)
                        D[r2][c] = __builtin_fmaf(-f[r][r2], D[r][c], D[r2][c]);
#pragma unroll
                    for (int y = jb; y < CY; ++y)
                        PR[r2][y] = __builtin_fmaf(-f[r][r2], PR[r][y], PR[r2][y]);
                }
            }
#pragma unroll
            for (int x = jb; x < RX; ++x) {
                const int a = ty + 16 * x;
                float pc[4], l4[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) pc[r] = rb[r][a];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int r2 = r + 1; r2 < 4; ++r2)
                        pc[r2] = __builtin_fmaf(-f[r][r2], pc[r], pc[r2]);
#pragma unroll
                for (int r = 0; r < 4; ++r) l4[r] = a > j0 + r ? pc[r] * inv[r] : 0.f;
#pragma unroll
                for (int y = jb; y < CY; ++y) {
                    const int b = tx + 16 * y;
                    float upd = m[x][y];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float lr = b > j0 + r ? l4[r] : 0.f;
                        upd = __builtin_fmaf(-lr, PR[r][y], upd);
                    }
                    m[x][y] = upd;
                }
            }
        }
    }
    // eliminated rows (D U | f') back to M for the back substitution
#pragma unroll
    for (int x = 0; x < RX; ++x)
#pragma unroll
        for (int y = 0; y < CY; ++y) {
            const int b = tx + 16 * y;
            if (b < KP + 1) M[(ty + 16 * x) * LD + b] = m[x][y];
        }
    __syncthreads();

    // ---- back substitution on wave 0: x = U^-1 D^-1 f'; lane L owns rows L
    // and L + 64; columns come from LDS in blocks of 8, one block ahead
    if (wv != 0) return;
    const int a0 = lane, a1 = lane + kWave;
    const bool v0 = a0 < KP, v1 = a1 < KP;
    const float d0 = v0 ? M[a0 * LD + a0] : 1.f, d1 = v1 ? M[a1 * LD + a1] : 1.f;
    const float i0 = 1.f / d0, i1 = 1.f / d1;
    const float w0 = (v0 ? M[a0 * LD + KP] : 0.f) * i0, w1 = (v1 ? M[a1 * LD + KP] : 0.f) * i1;
    float acc0 = 0.f, acc1 = 0.f, x0 = 0.f, x1 = 0.f;
    constexpr int BJ = 8;
    static_assert(KP % (2 * BJ) == 0, "back substitution blocks");
    float cA0[BJ], cA1[BJ], cB0[BJ], cB1[BJ];
    auto load_cols = [&](int jb, float (&c0)[BJ], float (&c1)[BJ]) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < BJ; ++u) {
            c0[u] = v0 ? M[a0 * LD + jb + u] : 0.f;
            c1[u] = v1 ? M[a1 * LD + jb + u] : 0.f;
        }
    };
    auto solve_cols = [&](int jb, const float (&c0)[BJ], const float (&c1)[BJ])
                          __attribute__((always_inline)) {
#pragma unroll
        for (int u = BJ - 1; u >= 0; --u) {
            const int j = jb + u;
            const float cand = j >= kWave ? (w1 - acc1) : (w0 - acc0);
            const float xj =
                __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cand), j & (kWave - 1)));
            if (lane == (j & (kWave - 1))) {
                if (j >= kWave) x1 = xj;
                else x0 = xj;
            }
            if (v0 && a0 < j) acc0 = acc0 + (c0[u] * i0) * xj;
            if (v1 && a1 < j) acc1 = acc1 + (c1[u] * i1) * xj;
        }
    };
    load_cols(KP - BJ, cA0, cA1);
    for (int jb = KP - BJ; jb >= 0; jb -= 2 * BJ) {
        load_cols(jb - BJ, cB0, cB1);             // jb - BJ >= 0: KP % (2 BJ) == 0
        solve_cols(jb, cA0, cA1);
        if (jb - 2 * BJ >= 0) load_cols(jb - 2 * BJ, cA0, cA1);
        solve_cols(jb - BJ, cB0, cB1);
    }
    float* out = A.feat + (int64_t)e * k;
    if (v0 && a0 < k) out[a0] = x0;
    if (v1 && a1 < k) out[a1] = x1;
}

template <int NT>
int solve_go(const SolveArgs& a, int32_t n, hipStream_t stream) {
    constexpr int KP = NT * 32;
    const size_t lds = std::max((size_t)KP * (KP + 1), (size_t)kChunk * KP + 2 * kChunk) *
                       sizeof(float);
    auto kfn = k_ials_solve<NT>;
    MF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kfn),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kfn, dim3((unsigned)n), dim3(kThreads), lds, stream, a);
    MF_HIP_CHECK(hipGetLastError());
    return MF_OK;
}

}  // namespace ials

void touch_ials(hipStream_t s) { hipLaunchKernelGGL(k_touch<8>, dim3(1), dim3(64), 0, s); }

}  // namespace mf

using namespace mf;

extern "C" size_t mf_gramian_workspace_bytes(int64_t n_rows, int32_t n_factors) {
    if (n_rows <= 0 || n_factors < 1 || n_factors > ials::kMaxFactors) return 0;
    return ials::gram_ws_bytes(n_rows, n_factors);
}

extern "C" int mf_gramian(const void* features, int64_t n_rows, int32_t n_factors, int32_t dtype,
                          void* workspace, void* gram, void* stream) {
    if (dtype != MF_F32) {
        set_error("mf_gramian: dtype=%d (float32 only: f32-input MFMA)", dtype);
        return MF_ERR_INVALID;
    }
    if (n_factors < 1 || n_factors > ials::kMaxFactors) {
        set_error("mf_gramian: n_factors=%d (must be in [1, %d])", n_factors, ials::kMaxFactors);
        return MF_ERR_INVALID;
    }
    if (n_rows < 0) {
        set_error("mf_gramian: n_rows=%lld (must be >= 0)", (long long)n_rows);
        return MF_ERR_INVALID;
    }
    if (ials::slabs_of(n_rows) > INT32_MAX) {
        set_error("mf_gramian: n_rows=%lld (too many slabs)", (long long)n_rows);
        return MF_ERR_INVALID;
    }
    if (!gram) {
        set_error("mf_gramian: gram is NULL");
        return MF_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    if (n_rows == 0) {
        MF_HIP_CHECK(hipMemsetAsync(gram, 0, (size_t)n_factors * n_factors * sizeof(float), s));
        return MF_OK;
    }
    if (!features) {
        set_error("mf_gramian: features is NULL");
        return MF_ERR_INVALID;
    }
    if (!workspace) {
        set_error("mf_gramian: workspace is NULL");
        return MF_ERR_INVALID;
    }
    ials::GramArgs a;
    a.F = static_cast<const float*>(features);
    a.n = n_rows; a.k = n_factors;
    a.vec = (n_factors % 4 == 0 && ials::aligned16(features)) ? 1 : 0;
    a.ws = static_cast<float*>(workspace);
    a.n_slabs = (int32_t)ials::slabs_of(n_rows);
    a.G = static_cast<float*>(gram);
    switch (ials::nt_of(n_factors)) {
        case 1: return ials::gram_go<1>(a, s);
        case 2: return ials::gram_go<2>(a, s);
        default: return ials::gram_go<4>(a, s);
    }
}

extern "C" int mf_ials_sweep(const int64_t* entity_ptr, const int32_t* other_ids,
                             const void* strengths, int32_t n_entities,
                             const void* other_features, const void* gram, void* features,
                             int32_t n_factors, int32_t dtype, double alpha, double reg,
                             void* stream) {
    const int rc = alsblk::check_ials_args("mf_ials_sweep", entity_ptr, other_ids, strengths,
                                           n_entities, other_features, gram, features, n_factors,
                                           dtype, alpha, reg, 0, 0);
    if (rc != MF_OK || n_entities == 0) return rc;
    ials::SolveArgs a;
    a.ptr = entity_ptr; a.other = other_ids; a.r = static_cast<const float*>(strengths);
    a.oq = static_cast<const float*>(other_features);
    a.G = static_cast<const float*>(gram);
    a.feat = static_cast<float*>(features);
    a.k = n_factors;
    a.vec = (n_factors % 4 == 0 && ials::aligned16(other_features)) ? 1 : 0;
    a.alpha = (float)alpha; a.reg = (float)reg;
    hipStream_t s = (hipStream_t)stream;
    switch (ials::nt_of(n_factors)) {
        case 1: return ials::solve_go<1>(a, n_entities, s);
        case 2: return ials::solve_go<2>(a, n_entities, s);
        default: return ials::solve_go<4>(a, n_entities, s);
    }
}
