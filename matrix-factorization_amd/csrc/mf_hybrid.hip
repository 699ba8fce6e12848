// mf_hybrid.hip -- second stage of HybridRecommender (hybrid.py): the
// candidates an embedding retrieval returned for a query are filtered, scored
// by the factor model, blended with their similarities and reordered, in one
// pass (project_template/pipeline/evaluate_hybrid.py:133-153 of the reference).
//
// k_hybrid_rerank, one workgroup per query:
//   1. kept candidates: positions whose index row is in range and not in the
//      query's sorted exclusion list, compacted in retrieval order (ballot
//      prefix per wave, wave totals through LDS);
//   2. model score of each kept row's item: mf_predict's value (score_pair
//      of mf_score.hpp), cast to float32; the user's row stays in registers
//      and a wave scores 64 / GS candidates per step;
//   3. min and max of the model scores and of the similarities (wave shuffles
//      plus LDS), min-max normalisation and the blend in float32, nothing
//      contracted;
//   4. bitonic sort by (score desc, position asc, NaN last): cand_sort of
//      mf_order.hpp with the kept position as the id -- the stable order;
//   5. the first `amount` are written, the rest padded with -1 / NaN.
// Rows, similarities, model scores, keys and ids live in LDS: 24 B per
// candidate slot, 48 KB at 2048.  Counting and ordering are integer and
// compare only, min / max are exact, and a blended -0 is written as +0 (the
// two compare equal in the reference's argsort), so the output does not
// depend on the launch.
#include <cmath>

#include "mf_score.hpp"
#include "mf_order.hpp"

namespace mf {

constexpr int kHybridMaxCand = 2048;                 // mf_topk's cap on amount

template <typename T>
struct HybridArgs {
    ModelView<T> m;                                   // m.P == nullptr: no model, scores 0
    const int32_t* users; int32_t nq;
    const int32_t* cand_rows; const float* cand_sims; int32_t n_cand;
    const int32_t* row_item; int32_t n_rows;
    const int64_t* ex_ptr; const int32_t* ex_rows;
    float alpha, beta;                                // fl32(alpha), fl32(1.0 - alpha)
    int32_t amount, cap;                              // cap: LDS slots, a power of two >= n_cand
    int32_t* out_rows; float* out_scores; float* out_model; float* out_sims;
    int32_t* out_n_cand;
};

struct MinMax { float lo, hi; bool nan; };

// min, max and "holds a NaN" of x[0, m), m >= 1, the same in every thread
__device__ __forceinline__ MinMax block_minmax(const float* x, int m, float* red, int t) {
    float lo = INFINITY, hi = -INFINITY;
    int nan = 0;
    for (int j = t; j < m; j += kBlock) {
        const float v = x[j];
        if (v != v) nan = 1;
        else {
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
    }
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const float a = __shfl_xor(lo, o, kWave), b = __shfl_xor(hi, o, kWave);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
        nan |= __shfl_xor(nan, o, kWave);
    }
    const int wv = t / kWave;
    if ((t & (kWave - 1)) == 0) {
        red[wv] = lo;
        red[kWavesPerBlock + wv] = hi;
        red[2 * kWavesPerBlock + wv] = nan ? 1.0f : 0.0f;
    }
    __syncthreads();
    MinMax r{red[0], red[kWavesPerBlock], red[2 * kWavesPerBlock] != 0.0f};
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) {
        const float a = red[w], b = red[kWavesPerBlock + w];
        r.lo = a < r.lo ? a : r.lo;
        r.hi = b > r.hi ? b : r.hi;
        r.nan = r.nan || red[2 * kWavesPerBlock + w] != 0.0f;
    }
    __syncthreads();                                  // red is reused
    return r;
}

// evaluate_hybrid.py:72-79 on one value
__device__ __forceinline__ float minmax_value(float x, const MinMax& r) {
    if (r.nan) return __int_as_float(0x7fc00000);     // np.min is NaN: the whole term is
    const double d = (double)r.hi - (double)r.lo;
    if (d < 1e-8) return 0.0f;
    const float num = x - r.lo;
    return num / (float)d;
}

template <typename T, int GS, int V, int KERN>
__global__ __launch_bounds__(kBlock) void k_hybrid_rerank(HybridArgs<T> A) {
    constexpr int R = kWave / GS;
    extern __shared__ __align__(16) unsigned char smem[];
    const int cap = A.cap;
    uint64_t* key = reinterpret_cast<uint64_t*>(smem);               // [cap]
    int32_t* id = reinterpret_cast<int32_t*>(key + cap);             // [cap]
    int32_t* rows = id + cap;                                        // [cap]
    float* sm = reinterpret_cast<float*>(rows + cap);                // [cap] model scores
    float* ss = sm + cap;                                            // [cap] similarities
    __shared__ int s_cnt[kWavesPerBlock];
    __shared__ float s_red[3 * kWavesPerBlock];

    const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    const int g = lane / GS, l = lane % GS;
    const int qy = blockIdx.x;
    const int64_t qb = (int64_t)qy * A.n_cand;
    const int64_t xlo = A.ex_ptr ? A.ex_ptr[qy] : 0, xhi = A.ex_ptr ? A.ex_ptr[qy + 1] : 0;

    // 1. kept candidates, in retrieval order
    int m = 0;                                                       // workgroup-uniform
    for (int c0 = 0; c0 < A.n_cand; c0 += kBlock) {
        const int c = c0 + t;
        int32_t row = -1;
        bool keep = false;
        if (c < A.n_cand) {
            row = A.cand_rows[qb + c];
            keep = row >= 0 && row < A.n_rows && !in_sorted(A.ex_rows, xlo, xhi, row);
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_cnt[wv] = __popcll(bal);
        __syncthreads();
        int before = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) {
            const int cw = s_cnt[w];
            before += w < wv ? cw : 0;
            total += cw;
        }
        if (keep) {
            rows[m + before] = row;
            ss[m + before] = A.cand_sims[qb + c];
        }
        m += total;
        __syncthreads();                                             // s_cnt is reused
    }
    if (t == 0) A.out_n_cand[qy] = m;

    // 2. model scores
    if (A.m.P) {
        T p[V], bu;
        load_user<T, GS, V, KERN>(A.m, A.users[qy], l, p, bu);
        for (int jb = wv * R; jb < m; jb += kWavesPerBlock * R) {    // wave-uniform bound
            const int j = jb + g;
            const bool have = j < m;
            const int32_t row = have ? rows[j] : 0;
            const int32_t it = have ? (A.row_item ? A.row_item[row] : row) : -1;
            T q[V], bi;
            load_item<T, GS, V, KERN>(A.m, it, it >= 0 && it < A.m.n_items, l, q, bi);
            const T pred = score_pair<T, GS, V, KERN>(A.m.h, p, bu, q, bi);
            if (have && l == 0) sm[j] = (float)pred;
        }
    } else {
        for (int j = t; j < m; j += kBlock) sm[j] = 0.0f;
    }
    __syncthreads();

    // 3. min-max and blend -> order keys; 4. sort
    int n_sort = 1;
    while (n_sort < m) n_sort <<= 1;
    if (m > 0) {
        const MinMax rm = block_minmax(sm, m, s_red, t);
        const MinMax rs = block_minmax(ss, m, s_red, t);
        for (int j = t; j < n_sort; j += kBlock) {
            if (j < m) {
                const float a = minmax_value(sm[j], rm), b = minmax_value(ss[j], rs);
                const float ta = A.alpha * a, tb = A.beta * b;
                const float score = (ta + tb) + 0.0f;                // -0 -> +0
                key[j] = order_key((double)score);
                id[j] = j;
            } else {
                key[j] = 0ull;                                       // below NaN's key
                id[j] = 0x7fffffff;
            }
        }
        __syncthreads();
        cand_sort(key, id, n_sort, t, kBlock);
    }

    // 5. output
    const int64_t ob = (int64_t)qy * A.amount;
    const float qnan = __int_as_float(0x7fc00000);
    for (int x = t; x < A.amount; x += kBlock) {
        int32_t row = -1;
        float sc = qnan, mo = qnan, si = qnan;
        if (x < m) {
            const int j = id[x];
            row = rows[j];
            sc = (float)key_score(key[x]);
            mo = sm[j];
            si = ss[j];
        }
        A.out_rows[ob + x] = row;
        A.out_scores[ob + x] = sc;
        if (A.out_model) A.out_model[ob + x] = mo;
        if (A.out_sims) A.out_sims[ob + x] = si;
    }
}

struct HybridLaunch {
    const int32_t* users; int32_t nq;
    const int32_t* cand_rows; const float* cand_sims; int32_t n_cand;
    const int32_t* row_item; int32_t n_rows;
    Model m;
    const int64_t* ex_ptr; const int32_t* ex_rows;
    double alpha; int32_t amount;
    int32_t* out_rows; float* out_scores; float* out_model; float* out_sims;
    int32_t* out_n_cand;
    hipStream_t stream;

    template <typename T, int GS, int V, int KERN>
    int run() {
        HybridArgs<T> a;
        a.m = m.view<T>();
        a.users = users; a.nq = nq; a.cand_rows = cand_rows; a.cand_sims = cand_sims;
        a.n_cand = n_cand; a.row_item = row_item; a.n_rows = n_rows;
        const bool ex = ex_ptr && ex_rows;
        a.ex_ptr = ex ? ex_ptr : nullptr; a.ex_rows = ex ? ex_rows : nullptr;
        a.alpha = (float)alpha; a.beta = (float)(1.0 - alpha);
        a.amount = amount;
        int cap = kWave;
        while (cap < n_cand) cap <<= 1;
        a.cap = cap;
        a.out_rows = out_rows; a.out_scores = out_scores; a.out_model = out_model;
        a.out_sims = out_sims; a.out_n_cand = out_n_cand;
        const size_t lds = (size_t)cap * 24;
        hipLaunchKernelGGL((k_hybrid_rerank<T, GS, V, KERN>), dim3((unsigned)nq), dim3(kBlock),
                           lds, stream, a);
        MF_HIP_CHECK(hipGetLastError());
        return MF_OK;
    }
};

}  // namespace mf

#include "mf_dispatch.hpp"

using namespace mf;

extern "C" size_t mf_hybrid_rerank_workspace_bytes(int32_t n_query, int32_t n_cand) {
    (void)n_query;
    (void)n_cand;
    return 0;                                         // everything lives in LDS
}

extern "C" int mf_hybrid_rerank(const int32_t* query_users, int32_t n_query,
                                const int32_t* cand_rows, const float* cand_sims, int32_t n_cand,
                                const int32_t* row_item, int32_t n_rows, double global_mean,
                                const void* user_biases, const void* item_biases,
                                const void* user_features, const void* item_features,
                                int32_t n_items, int32_t n_factors, int32_t kernel, int32_t dtype,
                                double gamma, double min_rating, double max_rating,
                                const int64_t* exclude_ptr, const int32_t* exclude_rows,
                                double alpha, int32_t amount, void* workspace, int32_t* out_rows,
                                float* out_scores, float* out_model, float* out_sims,
                                int32_t* out_n_cand, void* stream) {
    (void)workspace;
    const char* fn = "mf_hybrid_rerank";
    if (check_model(fn, dtype, n_factors, kernel) != MF_OK) return MF_ERR_INVALID;
    if (n_query < 0) {
        set_error("mf_hybrid_rerank: n_query=%d (must be >= 0)", n_query);
        return MF_ERR_INVALID;
    }
    if (n_rows < 0) {
        set_error("mf_hybrid_rerank: n_rows=%d (must be >= 0)", n_rows);
        return MF_ERR_INVALID;
    }
    if (n_items < 0) {
        set_error("mf_hybrid_rerank: n_items=%d (must be >= 0)", n_items);
        return MF_ERR_INVALID;
    }
    if (n_cand < 1 || n_cand > kHybridMaxCand) {
        set_error("mf_hybrid_rerank: n_cand=%d (must be in [1, %d])", n_cand, kHybridMaxCand);
        return MF_ERR_INVALID;
    }
    if (amount < 0 || amount > n_cand) {
        set_error("mf_hybrid_rerank: amount=%d (must be in [0, n_cand = %d])", amount, n_cand);
        return MF_ERR_INVALID;
    }
    if (!std::isfinite(alpha)) {
        set_error("mf_hybrid_rerank: alpha=%g (must be finite)", alpha);
        return MF_ERR_INVALID;
    }
    if (n_query == 0) return MF_OK;
    const void* need[] = {cand_rows, cand_sims, out_n_cand};
    const char* names[] = {"cand_rows", "cand_sims", "out_n_cand"};
    if (null_arg(fn, need, names, 3)) return MF_ERR_INVALID;
    if (amount > 0 && (!out_rows || !out_scores)) {
        set_error("mf_hybrid_rerank: %s is NULL", out_rows ? "out_scores" : "out_rows");
        return MF_ERR_INVALID;
    }
    if (user_features && (!query_users || !item_features || !user_biases || !item_biases)) {
        set_error("mf_hybrid_rerank: %s is NULL (a model needs it)",
                  !query_users ? "query_users" : !item_features ? "item_features"
                  : !user_biases ? "user_biases" : "item_biases");
        return MF_ERR_INVALID;
    }
    HybridLaunch L{query_users, n_query, cand_rows, cand_sims, n_cand, row_item, n_rows,
                   {global_mean, user_biases, item_biases, user_features, item_features, n_items,
                    n_factors, gamma, min_rating, max_rating},
                   exclude_ptr, exclude_rows, alpha, amount, out_rows, out_scores, out_model,
                   out_sims, out_n_cand, (hipStream_t)stream};
    // without a model the scores are 0 whatever the layout: one instantiation serves
    if (!user_features) return L.run<float, 16, 1, MF_LINEAR>();
    return dispatch(fn, dtype, n_factors, kernel, L);
}
