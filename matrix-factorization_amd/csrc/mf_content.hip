// mf_content.hip -- ContentBasedRecommender (content_based.py): user profiles
// from item feature rows, row normalisation, and the item x item feature
// cosine on the f32-input MFMA.
//
//   mf_content_profiles    P_u = sum w F_i / sum w over the user's pairs whose
//                          item has features (FP64; lanes own feature columns,
//                          a group of lanes owns a user, no atomics)
//   mf_content_normalize   fl32(x / ||x||) per row, the norm in FP64
//   mf_content_similarity  S = X X^T of the normalised float32 rows, LDS-tiled
//                          on v_mfma_f32_32x32x2_f32; tiles on or above the
//                          diagonal only, each written to both places
#include "mf_common.hpp"
#include "mf_cf.hpp"

namespace mf {
namespace content {

// ------------------------------------------------------------------ profiles
// G lanes (a power of two, <= 64) own a user; lane s of the group owns the
// columns s, s + G, ...  Every lane walks its user's list once per column it
// owns and sums the weights itself, in list order: no cross-lane traffic, and
// the same inputs give the same bits.
__global__ void __launch_bounds__(kBlock)
k_content_profiles(const int64_t* __restrict__ uptr, const int32_t* __restrict__ items,
                   const double* __restrict__ w, const double* __restrict__ F,
                   const uint8_t* __restrict__ has, int32_t n_users, int32_t n_items, int32_t d,
                   int32_t G, double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t u = t / G;
    const int s = (int)(t % G);
    if (u >= n_users) return;
    const int64_t beg = uptr[u], end = uptr[u + 1];
    for (int c = s; c < d; c += G) {
        double acc = 0.0, wsum = 0.0;
        for (int64_t p = beg; p < end; ++p) {
            const int32_t i = items[p];
            if (i < 0 || i >= n_items || !has[i]) continue;
            const double wp = w[p];
            acc = acc + F[(int64_t)i * d + c] * wp;
            wsum = wsum + wp;
        }
        if (wsum > 0.0) acc = acc / wsum;
        out[u * d + c] = acc;
    }
}

// ----------------------------------------------------------------- normalise
// One wave per row; the sum of squares goes round the wave by xor butterfly,
// which leaves the same bits in every lane.
__global__ void __launch_bounds__(kBlock)
k_content_normalize(const double* __restrict__ x, int64_t n, int32_t d, int32_t stride,
                    float* __restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t row = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (row >= n) return;
    const double* xr = x + row * d;
    double ss = 0.0;
    for (int c = lane; c < d; c += kWave) ss = ss + xr[c] * xr[c];
    ss = wave_sum(ss);
    const double norm = sqrt(ss);
    float* o = out + row * stride;
    for (int c = lane; c < stride; c += kWave)
        o[c] = (c < d && norm > 0.0) ? (float)(xr[c] / norm) : 0.f;
}

// ---------------------------------------------------------------- similarity
// A workgroup of 4 waves owns a 128 x 128 tile of S; wave w owns the 64 x 64
// quarter (w >> 1, w & 1) as 2 x 2 MFMA tiles of 32 x 32.  Per k step of 32
// the 128 rows of both sides go to LDS (rows beyond n and columns beyond d as
// zeros); v_mfma_f32_32x32x2_f32 takes A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31] from one VGPR each and is an exact f32 fmaf chain
// in k order, so S[a,b] and S[b,a] (the same products in the same order) are
// the same bits wherever they are computed.
constexpr int kTile = 128;
constexpr int kStep = 32;
constexpr int kLd = kStep + 1;               // LDS row stride: conflict-free column reads
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ void __launch_bounds__(kBlock)
k_content_similarity(const float* __restrict__ X, int32_t n, int32_t d, float* __restrict__ S) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;                      // the mirror tile writes this one
    __shared__ float As[kTile * kLd];
    __shared__ float Bs[kTile * kLd];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int64_t r0 = (int64_t)bi * kTile, c0 = (int64_t)bj * kTile;
    const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
    const int li = lane & 31, lh = lane >> 5;

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    // a thread moves column tk of the rows tr, tr + 8, ... of both sides: the
    // next step's values are fetched into registers before this step's MFMAs
    // and go to LDS after them, so the loads run under the matrix work
    constexpr int kPer = kTile * kStep / kBlock;
    const int tk = tid & (kStep - 1), tr = tid / kStep;
    float ra[kPer], rb[kPer];
    auto fetch = [&](int k0) {
        const bool kin = k0 + tk < d;
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const int64_t ga = r0 + tr + 8 * e, gb = c0 + tr + 8 * e;
            ra[e] = (kin && ga < n) ? X[ga * d + k0 + tk] : 0.f;
            rb[e] = (kin && gb < n) ? X[gb * d + k0 + tk] : 0.f;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < d; k0 += kStep) {
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            As[(tr + 8 * e) * kLd + tk] = ra[e];
            Bs[(tr + 8 * e) * kLd + tk] = rb[e];
        }
        __syncthreads();
        if (k0 + kStep < d) fetch(k0 + kStep);
#pragma unroll 4
        for (int kk = 0; kk < kStep; kk += 2) {
            float av[2], bv[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                av[a] = As[(wr + 32 * a + li) * kLd + kk + lh];
                bv[a] = Bs[(wc + 32 * a + li) * kLd + kk + lh];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b],
                                                                     0, 0, 0);
        }
        __syncthreads();
    }

    // C layout: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
    // The tile goes out as it is (a row of 32 columns per store), and, off the
    // diagonal, transposed through a 32 x 33 LDS image per wave so that the
    // mirror's stores run along its rows too.
    float* ts = As + wave * (32 * kLd);       // 4 waves x 32 x 33 floats <= As
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int64_t gr0 = r0 + wr + 32 * a, gc0 = c0 + wc + 32 * b;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int64_t gr = gr0 + row, gc = gc0 + li;
                if (gr < n && gc < n) S[gr * n + gc] = acc[a][b][r];
                ts[row * kLd + li] = acc[a][b][r];
            }
            __syncthreads();
            if (bi != bj) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int col = 2 * r + lh;       // column of the tile = row of the mirror
                    const int64_t gr = gc0 + col, gc = gr0 + li;
                    if (gr < n && gc < n) S[gr * n + gc] = ts[li * kLd + col];
                }
            }
            __syncthreads();
        }
}

static int bad_count(const char* fn, const char* name, int64_t v) {
    if (v >= 0) return 0;
    set_error("%s: %s=%lld (must be >= 0)", fn, name, (long long)v);
    return 1;
}

static int bad_d(const char* fn, int32_t d, int lo) {
    if (d >= lo && d <= kMaxFactors) return 0;
    set_error("%s: d=%d (must be in [%d, %d])", fn, d, lo, kMaxFactors);
    return 1;
}

}  // namespace content
}  // namespace mf

using namespace mf;

extern "C" int mf_content_profiles(const int64_t* user_ptr, const int32_t* item_ids,
                                   const void* weights, const void* features,
                                   const uint8_t* has_features, int32_t n_users,
                                   int32_t n_items, int32_t d, int32_t dtype, void* profiles,
                                   void* stream) {
    const char* fn = "mf_content_profiles";
    if (dtype != MF_F64) {
        set_error("%s: dtype=%d (float64 only)", fn, dtype);
        return MF_ERR_INVALID;
    }
    if (content::bad_count(fn, "n_users", n_users) || content::bad_count(fn, "n_items", n_items)
        || content::bad_d(fn, d, 0))
        return MF_ERR_INVALID;
    if (n_users == 0 || d == 0) return MF_OK;
    const void* need[] = {user_ptr, profiles};
    const char* names[] = {"user_ptr", "profiles"};
    if (null_arg(fn, need, names, 2)) return MF_ERR_INVALID;
    if (n_items > 0) {                                // else every list is skipped
        const void* need2[] = {features, has_features};
        const char* names2[] = {"features", "has_features"};
        if (null_arg(fn, need2, names2, 2)) return MF_ERR_INVALID;
    }
    int G = 1;
    while (G < d && G < kWave) G <<= 1;
    const int64_t threads = (int64_t)n_users * G;
    hipLaunchKernelGGL(content::k_content_profiles, dim3((unsigned)((threads + kBlock - 1) / kBlock)),
                       dim3(kBlock), 0, (hipStream_t)stream, user_ptr, item_ids,
                       static_cast<const double*>(weights), static_cast<const double*>(features),
                       has_features, n_users, n_items, d, G, static_cast<double*>(profiles));
    MF_HIP_CHECK(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_content_normalize(const void* rows, int64_t n, int32_t d, int32_t out_stride,
                                    int32_t dtype, void* out, void* stream) {
    const char* fn = "mf_content_normalize";
    if (dtype != MF_F64) {
        set_error("%s: dtype=%d (float64 rows only)", fn, dtype);
        return MF_ERR_INVALID;
    }
    if (content::bad_count(fn, "n", n) || content::bad_d(fn, d, 0)) return MF_ERR_INVALID;
    if (n > ((int64_t)1 << 31) - 1) {
        set_error("%s: n=%lld (must be < 2^31)", fn, (long long)n);
        return MF_ERR_INVALID;
    }
    if (out_stride != 0 && (out_stride < d || out_stride > kMaxFactors)) {
        set_error("%s: out_stride=%d (must be 0 or in [d, %d])", fn, out_stride, kMaxFactors);
        return MF_ERR_INVALID;
    }
    const int32_t stride = out_stride ? out_stride : d;
    if (n == 0 || stride == 0) return MF_OK;
    const void* need[] = {d ? rows : out, out};
    const char* names[] = {"rows", "out"};
    if (null_arg(fn, need, names, 2)) return MF_ERR_INVALID;
    hipLaunchKernelGGL(content::k_content_normalize,
                       dim3((unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, static_cast<const double*>(rows), n, d, stride,
                       static_cast<float*>(out));
    MF_HIP_CHECK(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_content_similarity(const void* rows, int32_t n, int32_t d, int32_t dtype,
                                     void* similarity, void* stream) {
    const char* fn = "mf_content_similarity";
    if (dtype != MF_F32) {
        set_error("%s: dtype=%d (float32 rows only)", fn, dtype);
        return MF_ERR_INVALID;
    }
    if (content::bad_count(fn, "n", n) || content::bad_d(fn, d, 0)) return MF_ERR_INVALID;
    if (n == 0) return MF_OK;
    const void* need[] = {d ? rows : similarity, similarity};
    const char* names[] = {"rows", "similarity"};
    if (null_arg(fn, need, names, 2)) return MF_ERR_INVALID;
    const unsigned nb = (unsigned)((n + content::kTile - 1) / content::kTile);
    if (nb > 65535u) {
        set_error("%s: n=%d needs %u tile rows (at most 65535)", fn, n, nb);
        return MF_ERR_INVALID;
    }
    hipLaunchKernelGGL(content::k_content_similarity, dim3(nb, nb), dim3(kBlock), 0,
                       (hipStream_t)stream, static_cast<const float*>(rows), n, d,
                       static_cast<float*>(similarity));
    MF_HIP_CHECK(hipGetLastError());
    return MF_OK;
}
