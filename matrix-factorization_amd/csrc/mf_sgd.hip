// mf_sgd.hip -- C ABI of the KernelMF hot path (include/mf_hip.h):
//   mf_sgd_epoch  -> k_sgd_batch  (mf_rows.hpp; one launch per batch)
//   mf_sse        -> k_sse_lean  (mf_rows.hpp)
//   mf_predict    -> k_read       (this file)
//
// Compiled with -ffp-contract=off: every scalar expression rounds like the
// reference's FP64 evaluation of the same expression; only the k-long sums
// follow a fixed DPP order instead of BLAS ddot's.
#include <atomic>
#include <algorithm>
#include <new>
#include <type_traits>
#include <vector>

#include "mf_rows.hpp"
#include "mf_strata.hpp"
#include "mf_dispatch.hpp"

namespace mf {

template <typename T, int V> struct Tile {
    static constexpr int U = V >= 4 ? 1 : (V == 2 ? 2 : 4);
};

template <typename T>
struct PredictArgs {
    ModelView<T> m;
    const int32_t* u; const int32_t* i;
    int32_t bound; T* out;
};

// Batched prediction (_predict, kernel_matrix_factorization.py:448-541):
// -1 ids read as a zero bias and an all-zero factor row (:487-499).
template <typename T, int GS, int V, int KERN>
__global__ __launch_bounds__(kBlock) void k_read(PredictArgs<T> A, SliceTab S) {
    constexpr int R = kWave / GS;
    constexpr int U = Tile<T, V>::U;
    constexpr int RPW = U * R;
    const int lane = threadIdx.x & (kWave - 1);
    const int g = lane / GS;
    const int l = lane % GS;
    const Hyper<T> h = A.m.h;
    const int x_slice = blockIdx.x % S.n;
    const int64_t bps = gridDim.x / S.n;                 // blocks per slice
    const int64_t s_end = S.off[x_slice + 1];
    const int64_t nwaves = bps * kWavesPerBlock;
    const int64_t wave = (int64_t)(blockIdx.x / S.n) * kWavesPerBlock + threadIdx.x / kWave;

    for (int64_t w0 = S.off[x_slice] + wave * RPW; w0 < s_end; w0 += nwaves * RPW) {
        const int nw = (int)min((int64_t)RPW, s_end - w0);
        bool have[U];
        T p[U][V], q[U][V], bu[U], bi[U];
#pragma unroll
        for (int x = 0; x < U; ++x) {
            const int idx = x * R + g;
            have[x] = idx < nw;
            const int64_t j = w0 + (have[x] ? idx : 0);
            const int32_t ii = A.i[j];
            load_user<T, GS, V, KERN>(A.m, have[x] ? A.u[j] : -1, l, p[x], bu[x]);
            load_item<T, GS, V, KERN>(A.m, ii, have[x] && ii >= 0, l, q[x], bi[x]);
        }
#pragma unroll
        for (int x = 0; x < U; ++x) {
            T pred = score_pair<T, GS, V, KERN>(h, p[x], bu[x], q[x], bi[x]);
            if (have[x] && l == 0) {
                const int64_t j = w0 + x * R + g;
                if (A.bound) {                               // :532-536
                    if (pred > h.hi) pred = h.hi;
                    else if (pred < h.lo) pred = h.lo;
                }
                A.out[j] = pred;
            }
        }
    }
}

// Fixed-order sum of the per-block partials (one block).
__global__ __launch_bounds__(kBlock) void k_sum_partials(const double* part, int n,
                                                         double* out) {
    double t = 0.0;
    for (int j = threadIdx.x; j < n; j += kBlock) t += part[j];
    t = wave_sum(t);
    __shared__ double red[kWavesPerBlock];
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < kWavesPerBlock; ++w) s += red[w];
        *out = s;
    }
}

inline int read_bps(const SliceTab& S, int rpw) {
    int64_t mx = 0;
    for (int x = 0; x < S.n; ++x) mx = std::max(mx, S.off[x + 1] - S.off[x]);
    const int64_t waves = (mx + rpw - 1) / rpw;
    const int64_t blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
    return (int)std::max<int64_t>(1, std::min<int64_t>(blocks, kSseMaxBlocks / S.n));
}

struct ReadLaunch {
    const int32_t* u; const int32_t* i; Model m; int32_t bound; void* out;
    hipStream_t stream; SliceTab S;

    template <typename T, int GS, int V, int KERN>
    int run() {
        constexpr int RPW = Tile<T, V>::U * (kWave / GS);
        const PredictArgs<T> a{m.view<T>(), u, i, bound, static_cast<T*>(out)};
        const int blocks = read_bps(S, RPW) * S.n;
        hipLaunchKernelGGL((k_read<T, GS, V, KERN>), dim3(blocks), dim3(kBlock), 0,
                           stream, a, S);
        MF_HIP_CHECK(hipGetLastError());
        return MF_OK;
    }
};

}  // namespace mf

using namespace mf;

extern "C" int mf_max_factors(void) { return kMaxFactors; }

extern "C" size_t mf_sgd_workspace_bytes(int32_t n_launch) {
    return n_launch > 0 ? sizeof(int32_t) * 8 * (size_t)n_launch : 0;
}

extern "C" int mf_sgd_epoch(const int32_t* user_ids, const int32_t* item_ids,
                            const void* ratings, int64_t n_ratings,
                            const int32_t* order, const int64_t* batch_offsets,
                            int32_t n_batches, const int32_t* batch_seq,
                            int32_t n_seq, double global_mean, void* user_biases,
                            void* item_biases, void* user_features,
                            void* item_features, int32_t n_users,
                            int32_t n_items, int32_t n_factors, int32_t kernel,
                            int32_t dtype, double gamma, double lr, double reg,
                            double min_rating, double max_rating,
                            int32_t update_user_params,
                            int32_t update_item_params, int32_t flags,
                            void* workspace, size_t workspace_bytes,
                            void* stream, double* kernel_ms) {
    if (n_ratings < 0 || n_batches < 0 || n_users < 0 || n_items < 0 ||
        (batch_seq && n_seq < 0)) {
        set_error("negative size");
        return MF_ERR_INVALID;
    }
    if (n_batches > 0 && !batch_offsets) {
        set_error("batch_offsets is NULL");
        return MF_ERR_INVALID;
    }
    for (int32_t b = 0; b < n_batches; ++b) {
        if (batch_offsets[b] < 0 || batch_offsets[b + 1] < batch_offsets[b] ||
            batch_offsets[b + 1] > n_ratings) {
            set_error("batch_offsets[%d..%d] = %lld..%lld invalid for n_ratings=%lld", b, b + 1,
                      (long long)batch_offsets[b], (long long)batch_offsets[b + 1],
                      (long long)n_ratings);
            return MF_ERR_INVALID;
        }
    }
    const int32_t n_launch = batch_seq ? n_seq : n_batches;
    for (int32_t q = 0; batch_seq && q < n_seq; ++q) {
        if (batch_seq[q] < 0 || batch_seq[q] >= n_batches) {
            set_error("batch_seq[%d] = %d out of range [0, %d)", q, batch_seq[q], n_batches);
            return MF_ERR_INVALID;
        }
    }
    if (n_ratings > 0 && (!user_ids || !item_ids || !ratings)) {
        set_error("NULL triple array");
        return MF_ERR_INVALID;
    }
    if (kernel_ms) { kernel_ms[0] = 0.0; kernel_ms[1] = 0.0; }
    if (n_launch == 0 || n_ratings == 0) return MF_OK;
    int32_t* claim = nullptr;
    if (flags & MF_FLAG_XCD_CLAIM) {
        if (!workspace || workspace_bytes < mf_sgd_workspace_bytes(n_launch)) {
            set_error("MF_FLAG_XCD_CLAIM needs a workspace of mf_sgd_workspace_bytes(%d) bytes",
                      n_launch);
            return MF_ERR_INVALID;
        }
        claim = static_cast<int32_t*>(workspace);
    }
    SgdParams P{user_ids, item_ids, ratings, order, batch_offsets, batch_seq, n_launch,
                global_mean, user_biases, item_biases, user_features, item_features,
                n_factors, kernel, gamma, lr, reg, min_rating, max_rating,
                update_user_params ? 1 : 0, update_item_params ? 1 : 0, flags,
                (hipStream_t)stream, kernel_ms, claim};
    if (dtype == MF_F32) return sgd_launch_f32(P);
    if (dtype == MF_F64) return sgd_launch_f64(P);
    set_error("unknown dtype code %d", dtype);
    return MF_ERR_INVALID;
}

extern "C" size_t mf_strata_lds_bytes(int32_t max_block_items, int32_t max_block_users,
                                      int32_t n_factors, int32_t dtype) {
    if (max_block_items < 0 || max_block_users < 0 || n_factors < 0) return 0;
    return dtype == MF_F32 ? strata_lds_bytes<float>(max_block_items, max_block_users, n_factors)
                           : strata_lds_bytes<double>(max_block_items, max_block_users, n_factors);
}

extern "C" int32_t mf_strata_lds_limit(void) { return kLdsLimit; }

namespace mf {
static int64_t* g_strata_probe = nullptr;
int64_t* strata_probe_ptr() { return g_strata_probe; }
static std::atomic<int32_t> g_strata_inject{0};
bool strata_inject_fail() {
    int32_t v = g_strata_inject.load();
    while (v > 0)
        if (g_strata_inject.compare_exchange_weak(v, v - 1)) return true;
    return false;
}

// State of one engine's "RMSE pass beside the next sweep" (mf_beside_create):
// the flag word a side stream waits on, in signal memory, and the arrival
// counter of the persistent launches that carry a ticket.
struct Beside {
    int32_t* flag;
    int32_t* arrive;
};
}  // namespace mf

extern "C" int mf_strata_set_probe(int64_t* probe) {
    mf::g_strata_probe = probe;
    return MF_OK;
}

extern "C" int mf_strata_inject_fail(int32_t n_launches) {
    if (n_launches < 0) {
        set_error("mf_strata_inject_fail: n_launches < 0");
        return MF_ERR_INVALID;
    }
    mf::g_strata_inject.store(n_launches);
    return MF_OK;
}

extern "C" size_t mf_strata_workspace_bytes(int32_t n_blocks, int32_t n_seq) {
    return n_blocks > 0 && n_seq >= 0 ? strata_ws_bytes(n_blocks, n_seq) : 0;
}

// One empty launch: the runtime loads the library's code object for the
// device at the first launch of any of its kernels (tens of ms for this
// library), which otherwise lands in the first training epoch.
__global__ void k_warmup() {}

extern "C" int mf_warmup(int32_t flags, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    const LaunchTrace lt;
    hipLaunchKernelGGL(k_warmup, dim3(1), dim3(64), 0, s);
    lt.mark("warmup: sgd unit");
    touch_rows_f32(s);
    touch_rows_f64(s);
    lt.mark("warmup: rows units");
    touch_strata_f32(s);
    touch_strata_f64(s);
    lt.mark("warmup: strata units");
    touch_bias(s);
    touch_topk(s);
    touch_topk_mm(s);
    touch_als(s);
    touch_ials(s);
    touch_ials_cg(s);
    touch_rank(s);
    lt.mark("warmup: other units");
    if (!(flags & MF_FLAG_NO_COOP)) {   // the cooperative launch path (persistent sweeps)
        void* no_args[1] = {nullptr};
        (void)hipLaunchCooperativeKernel(reinterpret_cast<const void*>(k_warmup), dim3(1),
                                         dim3(64), no_args, 0u, s);
        (void)hipGetLastError();
    }
    lt.mark("warmup: cooperative");
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MF_OK : hip_fail(e, "mf_warmup");
}

extern "C" int mf_strata_status(const void* workspace, int32_t n_blocks, void* stream) {
    if (!workspace || n_blocks < 1) {
        set_error("mf_strata_status: NULL workspace");
        return MF_ERR_INVALID;
    }
    int32_t err = 0;
    MF_HIP_CHECK(hipMemcpyAsync(&err, static_cast<const int32_t*>(workspace) + n_blocks,
                                sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    MF_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    if (err != 0) {
        set_error("persistent strata sweep: a workgroup gave up waiting for its neighbour "
                  "(workgroups not co-resident?); the parameters are invalid");
        return MF_ERR_HIP;
    }
    return MF_OK;
}

extern "C" int32_t mf_strata_slots_waves(int32_t n_factors, int32_t dtype, int32_t waves) {
    if (n_factors < 0 || n_factors > kMaxFactors || (dtype != MF_F32 && dtype != MF_F64) ||
        (waves != 16 && waves != 8 && waves != 4)) {
        set_error("mf_strata_slots_waves: n_factors=%d / dtype=%d / waves=%d invalid", n_factors,
                  dtype, waves);
        return -1;
    }
    if (dtype == MF_F32) {
        StrataSlots<float> f{waves};
        return dispatch_rows<float>(n_factors, MF_LINEAR, f);
    }
    StrataSlots<double> f{waves};
    return dispatch_rows<double>(n_factors, MF_LINEAR, f);
}

extern "C" int32_t mf_strata_slots(int32_t n_factors, int32_t dtype) {
    return mf_strata_slots_waves(n_factors, dtype, 16);
}

static int strata_epoch(const int32_t* user_ids, const int32_t* item_ids,
                                   const void* ratings, int64_t n_positions, int32_t n_blocks,
                                   const int32_t* user_bounds, const int32_t* item_bounds,
                                   const int64_t* block_steps, int32_t n_slots,
                                   int32_t max_block_items, int32_t max_block_users,
                                   const int32_t* strata_seq, int32_t n_seq, uint32_t seed,
                                   double global_mean, void* user_biases, void* item_biases,
                                   void* user_features, void* item_features, int32_t n_users,
                                   int32_t n_items, int32_t n_factors, int32_t kernel,
                                   int32_t dtype, double gamma, double lr, double reg,
                                   double min_rating, double max_rating,
                                   int32_t update_user_params, int32_t update_item_params,
                                   int32_t flags, void* workspace, size_t workspace_bytes,
                                   void* stream, double* kernel_ms, void* dq, void* dbi,
                                   const mf::Beside* beside = nullptr, int32_t ticket = 0,
                                   int32_t* attrs_out = nullptr) {
    if (attrs_out) attrs_out[0] = attrs_out[1] = attrs_out[2] = 0;
    if (n_positions < 0 || n_blocks < 0 || n_seq < 0 || n_users < 0 || n_items < 0 ||
        max_block_items < 0 || max_block_users < 0 || n_slots < 1) {
        set_error("negative size");
        return MF_ERR_INVALID;
    }
    if (kernel_ms) { kernel_ms[0] = 0.0; kernel_ms[1] = 0.0; }
    if (n_seq == 0 || n_positions == 0) return MF_OK;
    if (n_blocks == 0 || !strata_seq || !user_bounds || !item_bounds || !block_steps ||
        !user_ids || !item_ids || !ratings) {
        set_error("NULL plan or triple array");
        return MF_ERR_INVALID;
    }
    const int n_cls = strata_classes(flags);       // user-range classes: C*B strata
    if (n_cls > MF_STRATA_MAX_CLASSES) {
        set_error("user-range classes %d > %d", n_cls, MF_STRATA_MAX_CLASSES);
        return MF_ERR_INVALID;
    }
    if ((int64_t)n_cls * n_blocks * n_blocks >= ((int64_t)1 << 31)) {
        set_error("n_blocks=%d too large", n_blocks);
        return MF_ERR_INVALID;
    }
    for (int32_t t = 0; t < n_seq; ++t) {
        if (strata_seq[t] < 0 || strata_seq[t] >= n_cls * n_blocks) {
            set_error("strata_seq[%d] = %d out of range [0, %d)", t, strata_seq[t],
                      n_cls * n_blocks);
            return MF_ERR_INVALID;
        }
    }
    if (!(flags & MF_FLAG_PREPARE) &&
        (!user_features || !item_features || (kernel != MF_RBF && (!user_biases || !item_biases)))) {
        set_error("NULL parameter array");
        return MF_ERR_INVALID;
    }
    StrataParams P{user_ids, item_ids, ratings, user_bounds, item_bounds, block_steps,
                   n_blocks, n_slots, max_block_items, max_block_users,
                   strata_seq, n_seq, seed, global_mean, user_biases, item_biases,
                   user_features, item_features, n_factors, kernel, gamma, lr, reg,
                   min_rating, max_rating, update_user_params ? 1 : 0,
                   update_item_params ? 1 : 0, flags, workspace, workspace_bytes, n_users,
                   (hipStream_t)stream, kernel_ms, n_items, dq, dbi, n_positions};
    if (beside) {
        P.tk_arrive = beside->arrive; P.tk_flag = beside->flag; P.tk_val = ticket;
    }
    P.attrs_out = attrs_out;
    if (dtype == MF_F32) return strata_launch_f32(P);
    if (dtype == MF_F64) return strata_launch_f64(P);
    set_error("unknown dtype code %d", dtype);
    return MF_ERR_INVALID;
}

extern "C" int mf_sgd_epoch_strata(const int32_t* user_ids, const int32_t* item_ids,
                                   const void* ratings, int64_t n_positions, int32_t n_blocks,
                                   const int32_t* user_bounds, const int32_t* item_bounds,
                                   const int64_t* block_steps, int32_t n_slots,
                                   int32_t max_block_items, int32_t max_block_users,
                                   const int32_t* strata_seq, int32_t n_seq, uint32_t seed,
                                   double global_mean, void* user_biases, void* item_biases,
                                   void* user_features, void* item_features, int32_t n_users,
                                   int32_t n_items, int32_t n_factors, int32_t kernel,
                                   int32_t dtype, double gamma, double lr, double reg,
                                   double min_rating, double max_rating,
                                   int32_t update_user_params, int32_t update_item_params,
                                   int32_t flags, void* workspace, size_t workspace_bytes,
                                   void* stream, double* kernel_ms) {
    return strata_epoch(user_ids, item_ids, ratings, n_positions, n_blocks, user_bounds,
                        item_bounds, block_steps, n_slots, max_block_items, max_block_users,
                        strata_seq, n_seq, seed, global_mean, user_biases, item_biases,
                        user_features, item_features, n_users, n_items, n_factors, kernel, dtype,
                        gamma, lr, reg, min_rating, max_rating, update_user_params,
                        update_item_params, flags, workspace, workspace_bytes, stream, kernel_ms,
                        nullptr, nullptr);
}

extern "C" int mf_sgd_epoch_strata_delta(
    const int32_t* user_ids, const int32_t* item_ids, const void* ratings, int64_t n_positions,
    int32_t n_blocks, const int32_t* user_bounds, const int32_t* item_bounds,
    const int64_t* block_steps, int32_t n_slots, int32_t max_block_items,
    int32_t max_block_users, const int32_t* strata_seq, int32_t n_seq, uint32_t seed,
    double global_mean, void* user_biases, void* item_biases, void* user_features,
    void* item_features, int32_t n_users, int32_t n_items, int32_t n_factors, int32_t kernel,
    int32_t dtype, double gamma, double lr, double reg, double min_rating, double max_rating,
    int32_t update_user_params, int32_t update_item_params, int32_t flags, void* workspace,
    size_t workspace_bytes, void* item_delta, void* item_bias_delta, void* stream,
    double* kernel_ms) {
    if (!item_delta || (kernel != MF_RBF && !item_bias_delta)) {
        set_error("mf_sgd_epoch_strata_delta: NULL delta buffer");
        return MF_ERR_INVALID;
    }
    return strata_epoch(user_ids, item_ids, ratings, n_positions, n_blocks, user_bounds,
                        item_bounds, block_steps, n_slots, max_block_items, max_block_users,
                        strata_seq, n_seq, seed, global_mean, user_biases, item_biases,
                        user_features, item_features, n_users, n_items, n_factors, kernel, dtype,
                        gamma, lr, reg, min_rating, max_rating, update_user_params,
                        update_item_params, flags, workspace, workspace_bytes, stream, kernel_ms,
                        item_delta, item_bias_delta);
}

extern "C" size_t mf_sse_workspace_bytes(int64_t n_ratings) {
    (void)n_ratings;
    return sizeof(double) * (size_t)kSseMaxBlocks;
}

// mf_sse_capped; attrs_out (nullable): no launch, the pass kernel's attributes
static int sse_capped(const int32_t* user_ids, const int32_t* item_ids, const void* ratings,
                      int64_t n_ratings, double global_mean, const void* user_biases,
                      const void* item_biases, const void* user_features,
                      const void* item_features, int32_t n_users, int32_t n_items,
                      int32_t n_factors, int32_t kernel, int32_t dtype, double gamma,
                      double min_rating, double max_rating, const int64_t* slice_offsets,
                      int32_t n_slices, void* workspace, int32_t max_blocks, double* sse_out,
                      void* stream, int32_t* attrs_out) {
    if (attrs_out) attrs_out[0] = attrs_out[1] = attrs_out[2] = 0;
    if (n_ratings < 0 || !sse_out || !workspace || n_users < 0 || n_items < 0 ||
        (slice_offsets && (n_slices < 1 || n_slices > kMaxSlices))) {
        set_error("mf_sse: bad arguments (n_slices must be in [1, %d])", kMaxSlices);
        return MF_ERR_INVALID;
    }
    SliceTab S;
    if (slice_offsets) {
        S.n = n_slices;
        for (int x = 0; x <= n_slices; ++x) S.off[x] = slice_offsets[x];
        for (int x = 0; x < n_slices; ++x) {
            if (S.off[x] < 0 || S.off[x + 1] < S.off[x] || S.off[n_slices] > n_ratings) {
                set_error("mf_sse: slice_offsets invalid");
                return MF_ERR_INVALID;
            }
        }
    } else {
        S.n = 1; S.off[0] = 0; S.off[1] = n_ratings;
    }
    if (n_ratings == 0) {
        if (!attrs_out)
            MF_HIP_CHECK(hipMemsetAsync(sse_out, 0, sizeof(double), (hipStream_t)stream));
        return MF_OK;
    }
    if (max_blocks < 0) {
        set_error("mf_sse_capped: max_blocks < 0");
        return MF_ERR_INVALID;
    }
    SseParams P{user_ids, item_ids, ratings, n_ratings, global_mean, user_biases,
                item_biases, user_features, item_features, n_users, n_items, n_factors,
                kernel, gamma, min_rating, max_rating, (double*)workspace, sse_out,
                (hipStream_t)stream, S, max_blocks};
    P.attrs_out = attrs_out;
    if (dtype == MF_F32) return sse_launch_f32(P);
    if (dtype == MF_F64) return sse_launch_f64(P);
    set_error("unknown dtype code %d", dtype);
    return MF_ERR_INVALID;
}

extern "C" int mf_sse_capped(const int32_t* user_ids, const int32_t* item_ids,
                             const void* ratings, int64_t n_ratings,
                             double global_mean, const void* user_biases,
                             const void* item_biases, const void* user_features,
                             const void* item_features, int32_t n_users, int32_t n_items,
                             int32_t n_factors, int32_t kernel, int32_t dtype, double gamma,
                             double min_rating, double max_rating,
                             const int64_t* slice_offsets, int32_t n_slices, void* workspace,
                             int32_t max_blocks, double* sse_out, void* stream) {
    return sse_capped(user_ids, item_ids, ratings, n_ratings, global_mean, user_biases,
                      item_biases, user_features, item_features, n_users, n_items, n_factors,
                      kernel, dtype, gamma, min_rating, max_rating, slice_offsets, n_slices,
                      workspace, max_blocks, sse_out, stream, nullptr);
}

// ---------------------------------------------------------------------------
// The item-stationary RMSE pass (k_sse_slab).
static_assert(kSlabLdsLimit == kLdsLimit, "one LDS size");

extern "C" size_t mf_sse_slab_workspace_bytes(int32_t n_groups) {
    (void)n_groups;                     // one partial per workgroup, at most kSseMaxBlocks
    return sizeof(double) * (size_t)kSseMaxBlocks;
}

extern "C" int mf_sse_slab_plan(int32_t n_items, int32_t n_factors, int32_t dtype,
                                int32_t n_workgroups, int32_t lds_budget, int32_t pad_values,
                                int32_t* plan_out) {
    if (plan_out) plan_out[0] = plan_out[1] = plan_out[2] = plan_out[3] = plan_out[4] = 0;
    const int64_t sz = dtype == MF_F32 ? 4 : dtype == MF_F64 ? 8 : 0;
    if (!plan_out || sz == 0 || n_items < 1 || n_factors < 1 || n_factors > kMaxFactors ||
        n_workgroups < 1)
        return 0;
    const int64_t limit = kSlabLdsLimit - kSlabScratch;
    const int64_t budget = lds_budget > 0 ? std::min<int64_t>(lds_budget, limit) : limit;
    // rows moved 16 B per lane keep a 16-B aligned stride
    const int64_t wv = 16 / sz;
    int64_t pad = pad_values > 0 ? pad_values : 0;
    if (n_factors % wv == 0) pad = (pad + wv - 1) / wv * wv;
    const int64_t ks = n_factors + pad;
    const int64_t per_item = (ks + 1) * sz;              // the row and its bias
    if (per_item > budget) return 0;
    const int64_t fit = budget / per_item;               // items the budget holds
    // the smallest multiple of the workgroup count with ceil(ni / G) <= fit
    const int64_t need = ((int64_t)n_items + fit - 1) / fit;
    const int64_t G = (need + n_workgroups - 1) / n_workgroups * n_workgroups;
    if (G > (int64_t)1 << 24) return 0;
    const int64_t nit = ((int64_t)n_items + G - 1) / G;
    plan_out[0] = (int32_t)nit;
    plan_out[1] = (int32_t)G;
    plan_out[2] = (int32_t)(G / n_workgroups);
    plan_out[3] = (int32_t)(nit * per_item);
    plan_out[4] = (int32_t)ks;
    return 1;
}

extern "C" int mf_sse_slab(const int32_t* user_ids, const int32_t* item_ids, const void* ratings,
                           int64_t n_ratings, double global_mean, const void* user_biases,
                           const void* item_biases, const void* user_features,
                           const void* item_features, int32_t n_users, int32_t n_items,
                           int32_t n_factors, int32_t kernel, int32_t dtype, double gamma,
                           double min_rating, double max_rating, const int64_t* group_tab,
                           int32_t n_groups, int32_t n_windows, int32_t items_per_group,
                           int32_t row_stride, void* workspace, int32_t max_blocks,
                           double* sse_out, void* stream, int32_t* attrs_out) {
    if (attrs_out) attrs_out[0] = attrs_out[1] = attrs_out[2] = 0;
    if (n_ratings < 0 || !sse_out || !workspace || n_users < 0 || n_items < 1 || !group_tab ||
        n_groups < 1 || n_windows < 1 || max_blocks < 0) {
        set_error("mf_sse_slab: bad arguments");
        return MF_ERR_INVALID;
    }
    const int64_t sz = dtype == MF_F32 ? 4 : 8;
    if (n_factors < 1 || row_stride < n_factors || items_per_group < 1 ||
        (int64_t)items_per_group * n_groups < n_items ||
        ((int64_t)row_stride + 1) * items_per_group * sz > kSlabLdsLimit - kSlabScratch) {
        set_error("mf_sse_slab: %d groups of %d rows (stride %d) do not hold %d items of rank %d "
                  "in LDS (mf_sse_slab_plan)", n_groups, items_per_group, row_stride, n_items,
                  n_factors);
        return MF_ERR_INVALID;
    }
    if ((uint64_t)n_users * (uint64_t)n_factors * (uint64_t)sz >= (1ull << 32) - 64) {
        set_error("mf_sse_slab: user_features must be below 4 GiB (buffer loads)");
        return MF_ERR_INVALID;
    }
    if (n_ratings == 0) {
        if (!attrs_out)
            MF_HIP_CHECK(hipMemsetAsync(sse_out, 0, sizeof(double), (hipStream_t)stream));
        return MF_OK;
    }
    SseSlabParams P{{user_ids, item_ids, ratings, n_ratings, global_mean, user_biases,
                     item_biases, user_features, item_features, n_users, n_items, n_factors,
                     kernel, gamma, min_rating, max_rating, (double*)workspace, sse_out,
                     (hipStream_t)stream, SliceTab{}, max_blocks},
                    SlabGeom{group_tab, n_groups, n_windows, n_items, items_per_group,
                             row_stride, 0, 0, 0}};
    P.s.attrs_out = attrs_out;
    if (dtype == MF_F32) return sse_slab_launch_f32(P);
    if (dtype == MF_F64) return sse_slab_launch_f64(P);
    set_error("unknown dtype code %d", dtype);
    return MF_ERR_INVALID;
}

// ---------------------------------------------------------------------------
// The RMSE pass beside the next epoch's persistent sweep.
extern "C" int mf_beside_supported(void) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeCanUseStreamWaitValue, dev) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return v ? 1 : 0;
}

extern "C" int mf_beside_create(void** handle) {
    if (!handle) {
        set_error("mf_beside_create: NULL handle");
        return MF_ERR_INVALID;
    }
    *handle = nullptr;
    Beside* b = new (std::nothrow) Beside{nullptr, nullptr};
    if (!b) {
        set_error("mf_beside_create: out of host memory");
        return MF_ERR_NOMEM;
    }
    // (signal memory: one 8-byte word; the flag is its low 32 bits)
    hipError_t e = hipExtMallocWithFlags(reinterpret_cast<void**>(&b->flag), 8,
                                         hipMallocSignalMemory);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&b->arrive), sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(b->flag, 0, 8);
    if (e == hipSuccess) e = hipMemset(b->arrive, 0, sizeof(int32_t));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        if (b->flag) (void)hipFree(b->flag);
        if (b->arrive) (void)hipFree(b->arrive);
        delete b;
        (void)hipGetLastError();
        return hip_fail(e, "mf_beside_create");
    }
    *handle = b;
    return MF_OK;
}

extern "C" void mf_beside_destroy(void* handle) {
    Beside* b = static_cast<Beside*>(handle);
    if (!b) return;
    (void)hipFree(b->flag);
    (void)hipFree(b->arrive);
    delete b;
}

extern "C" int mf_beside_fit(int32_t sweep_regs, int32_t sweep_waves, int32_t sweep_lds,
                             int32_t pass_regs, int32_t pass_waves, int32_t pass_lds,
                             int32_t simd_regs, int32_t cu_simds, int32_t cu_lds) {
    if (sweep_regs < 1 || sweep_waves < 1 || pass_regs < 1 || pass_waves < 1 || sweep_lds < 0 ||
        pass_lds < 0 || simd_regs < 1 || cu_simds < 1 || cu_lds < 1)
        return 0;
    // registers are allocated per wave in granules of 8; a workgroup's waves
    // are dealt evenly over the CU's SIMDs
    auto per_simd = [&](int32_t regs, int32_t waves) {
        return (int64_t)((regs + 7) / 8 * 8) * ((waves + cu_simds - 1) / cu_simds);
    };
    const int64_t sw = per_simd(sweep_regs, sweep_waves), ps = per_simd(pass_regs, pass_waves);
    const bool one = sw + ps <= simd_regs && (int64_t)sweep_lds + pass_lds <= cu_lds;
    const bool two = sw + 2 * ps <= simd_regs && (int64_t)sweep_lds + 2 * (int64_t)pass_lds <= cu_lds;
    return one && !two ? 1 : 0;
}

extern "C" int mf_sgd_epoch_strata_ticket(
    const int32_t* user_ids, const int32_t* item_ids, const void* ratings, int64_t n_positions,
    int32_t n_blocks, const int32_t* user_bounds, const int32_t* item_bounds,
    const int64_t* block_steps, int32_t n_slots, int32_t max_block_items,
    int32_t max_block_users, const int32_t* strata_seq, int32_t n_seq, uint32_t seed,
    double global_mean, void* user_biases, void* item_biases, void* user_features,
    void* item_features, int32_t n_users, int32_t n_items, int32_t n_factors, int32_t kernel,
    int32_t dtype, double gamma, double lr, double reg, double min_rating, double max_rating,
    int32_t update_user_params, int32_t update_item_params, int32_t flags, void* workspace,
    size_t workspace_bytes, void* beside, int32_t ticket, int32_t* kernel_attrs, void* stream,
    double* kernel_ms) {
    const Beside* b = static_cast<const Beside*>(beside);
    if (b && ticket < 1) {
        set_error("mf_sgd_epoch_strata_ticket: ticket < 1");
        return MF_ERR_INVALID;
    }
    int rc = strata_epoch(user_ids, item_ids, ratings, n_positions, n_blocks, user_bounds,
                          item_bounds, block_steps, n_slots, max_block_items, max_block_users,
                          strata_seq, n_seq, seed, global_mean, user_biases, item_biases,
                          user_features, item_features, n_users, n_items, n_factors, kernel,
                          dtype, gamma, lr, reg, min_rating, max_rating, update_user_params,
                          update_item_params, flags, workspace, workspace_bytes, stream,
                          kernel_ms, nullptr, nullptr, b, ticket, kernel_attrs);
    // the backstop: whatever strata_epoch did -- a persistent launch, one
    // launch per stratum, a refused cooperative launch, an error return --
    // the same ticket is written behind it on the launch stream, so a side
    // stream waiting for it (mf_sse_beside) is released at the latest when
    // the sweep has ended
    if (b && !(flags & MF_FLAG_PREPARE)) {
        const hipError_t e = hipStreamWriteValue32((hipStream_t)stream, b->flag,
                                                   (uint32_t)ticket, 0);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (rc == MF_OK) rc = hip_fail(e, "hipStreamWriteValue32 (ticket backstop)");
        }
    }
    return rc;
}

extern "C" int mf_sse_beside(void* beside, int32_t ticket, const int32_t* user_ids,
                             const int32_t* item_ids, const void* ratings, int64_t n_ratings,
                             double global_mean, const void* user_biases,
                             const void* item_biases, const void* user_features,
                             const void* item_features, int32_t n_users, int32_t n_items,
                             int32_t n_factors, int32_t kernel, int32_t dtype, double gamma,
                             double min_rating, double max_rating,
                             const int64_t* slice_offsets, int32_t n_slices, void* workspace,
                             double* sse_out, void* stream, int32_t* kernel_attrs) {
    int dev = 0, cus = 0;
    MF_HIP_CHECK(hipGetDevice(&dev));
    MF_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (cus < 1) {
        set_error("mf_sse_beside: no compute units reported");
        return MF_ERR_HIP;
    }
    if (!kernel_attrs) {
        const Beside* b = static_cast<const Beside*>(beside);
        if (!b || ticket < 1) {
            set_error("mf_sse_beside: NULL handle or ticket < 1");
            return MF_ERR_INVALID;
        }
        MF_HIP_CHECK(hipStreamWaitValue32((hipStream_t)stream, b->flag, (uint32_t)ticket,
                                          hipStreamWaitValueGte, 0xFFFFFFFFu));
    }
    return sse_capped(user_ids, item_ids, ratings, n_ratings, global_mean, user_biases,
                      item_biases, user_features, item_features, n_users, n_items, n_factors,
                      kernel, dtype, gamma, min_rating, max_rating, slice_offsets, n_slices,
                      workspace, cus, sse_out, stream, kernel_attrs);
}

namespace mf {
struct CopyJobs {
    const char* src[MF_PERMUTE_MAX_JOBS];
    char* dst[MF_PERMUTE_MAX_JOBS];
    int64_t end16[MF_PERMUTE_MAX_JOBS];   // running total of whole 16-B chunks
    int64_t bytes[MF_PERMUTE_MAX_JOBS];
    int32_t n;
};

// Up to 4 arrays copied in one launch (the parameter snapshot): the 16-B
// chunks of all jobs form one index space; the < 16 B tails go word by word.
__global__ __launch_bounds__(kBlock) void k_copy_jobs(CopyJobs J) {
    const int64_t total = J.end16[J.n - 1];
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total;
         t += (int64_t)gridDim.x * kBlock) {
        int j = 0;
        while (t >= J.end16[j]) ++j;                     // (j < n: t < total)
        const int64_t c = t - (j ? J.end16[j - 1] : 0);
        reinterpret_cast<uint4*>(J.dst[j])[c] = reinterpret_cast<const uint4*>(J.src[j])[c];
    }
    if (blockIdx.x == 0) {
        for (int j = 0; j < J.n; ++j) {
            const int64_t done = (J.bytes[j] / 16) * 16;
            const int64_t o = done + 4 * (int64_t)threadIdx.x;
            if (o < J.bytes[j])
                *reinterpret_cast<uint32_t*>(J.dst[j] + o) =
                    *reinterpret_cast<const uint32_t*>(J.src[j] + o);
        }
    }
}
}  // namespace mf

extern "C" int mf_copy_arrays(int32_t n_jobs, void* const* dst, const void* const* src,
                              const int64_t* n_bytes, void* stream) {
    if (n_jobs < 0 || n_jobs > MF_PERMUTE_MAX_JOBS || (n_jobs > 0 && (!dst || !src || !n_bytes))) {
        set_error("mf_copy_arrays: bad arguments");
        return MF_ERR_INVALID;
    }
    CopyJobs J{};
    int64_t run = 0;
    for (int32_t j = 0; j < n_jobs; ++j) {
        if (n_bytes[j] < 0 || n_bytes[j] % 4 != 0 ||
            (n_bytes[j] > 0 && (!dst[j] || !src[j] ||
                                (reinterpret_cast<uintptr_t>(dst[j]) |
                                 reinterpret_cast<uintptr_t>(src[j])) % 16 != 0))) {
            set_error("mf_copy_arrays: job %d invalid (sizes in multiples of 4 bytes, 16-byte "
                      "aligned arrays)", j);
            return MF_ERR_INVALID;
        }
        if (n_bytes[j] == 0) continue;
        J.src[J.n] = static_cast<const char*>(src[j]);
        J.dst[J.n] = static_cast<char*>(dst[j]);
        J.bytes[J.n] = n_bytes[j];
        run += n_bytes[j] / 16;
        J.end16[J.n] = run;
        ++J.n;
    }
    if (J.n == 0) return MF_OK;
    const int64_t need = (run / 4 + kBlock - 1) / kBlock;            // ~four chunks per thread
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>(need, 8192));
    hipLaunchKernelGGL(k_copy_jobs, dim3(g), dim3(kBlock), 0, (hipStream_t)stream, J);
    MF_HIP_CHECK(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_sse(const int32_t* user_ids, const int32_t* item_ids,
                      const void* ratings, int64_t n_ratings,
                      double global_mean, const void* user_biases,
                      const void* item_biases, const void* user_features,
                      const void* item_features, int32_t n_users, int32_t n_items,
                      int32_t n_factors, int32_t kernel, int32_t dtype, double gamma,
                      double min_rating, double max_rating,
                      const int64_t* slice_offsets, int32_t n_slices, void* workspace,
                      double* sse_out, void* stream) {
    return mf_sse_capped(user_ids, item_ids, ratings, n_ratings, global_mean, user_biases,
                         item_biases, user_features, item_features, n_users, n_items,
                         n_factors, kernel, dtype, gamma, min_rating, max_rating,
                         slice_offsets, n_slices, workspace, 0, sse_out, stream);
}

extern "C" int mf_predict(const int32_t* user_ids, const int32_t* item_ids,
                          int64_t n_pairs, double global_mean,
                          const void* user_biases, const void* item_biases,
                          const void* user_features, const void* item_features,
                          int32_t n_factors, int32_t kernel, int32_t dtype,
                          double gamma, double min_rating, double max_rating,
                          int32_t bound_ratings, void* out, void* stream) {
    if (n_pairs < 0 || (n_pairs > 0 && !out)) {
        set_error("mf_predict: bad arguments");
        return MF_ERR_INVALID;
    }
    if (n_pairs == 0) return MF_OK;
    SliceTab S;
    S.n = 1; S.off[0] = 0; S.off[1] = n_pairs;
    // (n_items = 0: mf_predict is not told the item count; k_read bounds an id by >= 0 alone
    // and must not read m.n_items)
    ReadLaunch L{user_ids, item_ids,
                 {global_mean, user_biases, item_biases, user_features, item_features, 0,
                  n_factors, gamma, min_rating, max_rating},
                 bound_ratings ? 1 : 0, out, (hipStream_t)stream, S};
    return dispatch("mf_predict", dtype, n_factors, kernel, L);
}
