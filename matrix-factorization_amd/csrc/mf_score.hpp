// mf_score.hpp -- the score of one (user, item) pair: the one definition that
// mf_predict, mf_topk, mf_rank and mf_hybrid_rerank share, so their scores are
// bit-identical in every row layout (GS, V), every kernel and both dtypes.
//
// A pair is scored by a group of GS lanes; lane l holds the factors
// f = l + v * GS (v < V) of both rows, zero for f >= k.  The lane partials run
// in ascending v from (T)0, group_sum<GS> leaves their sum in every lane of
// the group, and predict_one adds the biases.  Nothing is contracted
// (-ffp-contract=off) and no sum is reordered.
#pragma once

#include "mf_common.hpp"

namespace mf {

// kernels.py:21-105.  `s` = group-reduced dot product (linear/sigmoid) or
// squared distance (rbf).
template <typename T, int KERN>
__device__ __forceinline__ T predict_one(T s, T bu, T bi, const Hyper<T> h) {
    if constexpr (KERN == MF_LINEAR) {
        return ((h.mu + bi) + bu) + s;                       // kernels.py:42-44
    } else if constexpr (KERN == MF_SIGMOID) {
        const T lin = ((h.mu + bu) + bi) + s;                // kernels.py:73-75
        const T sg = (T)1 / ((T)1 + dexp<T>(-lin));          // kernels.py:17
        return h.a + h.c * sg;                               // kernels.py:77
    } else {
        return h.a + h.c * dexp<T>((-h.gamma) * s);          // kernels.py:102-104
    }
}

// The model as a kernel sees it.
template <typename T>
struct ModelView {
    const T* P; const T* Q; const T* Bu; const T* Bi;
    int32_t n_items, k;
    Hyper<T> h;
};

// The model as the C ABI passes it; view<T>() is what a launcher hands its kernel.
struct Model {
    double mu; const void* bu; const void* bi; const void* P; const void* Q;
    int32_t n_items, k; double gamma, lo, hi;

    template <typename T>
    ModelView<T> view() const {
        return {static_cast<const T*>(P), static_cast<const T*>(Q), static_cast<const T*>(bu),
                static_cast<const T*>(bi), n_items, k,
                make_hyper<T>(mu, 0.0, 0.0, gamma, lo, hi)};
    }
};

// User uu's factor row in lane l's part of the (GS, V) layout, and its bias.
// uu < 0 (unknown, or no such slot): a zero row and a zero bias.  RBF reads no bias.
template <typename T, int GS, int V, int KERN>
__device__ __forceinline__ void load_user(const ModelView<T>& M, int32_t uu, int l, T (&p)[V],
                                          T& bu) {
    const bool uk = uu >= 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int f = l + v * GS;
        p[v] = (uk && f < M.k) ? M.P[(int64_t)uu * M.k + f] : (T)0;
    }
    bu = (uk && KERN != MF_RBF) ? M.Bu[uu] : (T)0;
}

// Item `it` likewise; the caller says whether there is one (`have`: in range, slot in use).
template <typename T, int GS, int V, int KERN>
__device__ __forceinline__ void load_item(const ModelView<T>& M, int64_t it, bool have, int l,
                                          T (&q)[V], T& bi) {
    const T* qr = M.Q + (have ? it : 0) * M.k;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int f = l + v * GS;
        q[v] = (have && f < M.k) ? qr[f] : (T)0;
    }
    bi = (have && KERN != MF_RBF) ? M.Bi[it] : (T)0;
}

// mf_predict's value (bound_ratings = 0) for two loaded rows, in every lane of the group.
template <typename T, int GS, int V, int KERN>
__device__ __forceinline__ T score_pair(const Hyper<T>& h, const T (&p)[V], T bu,
                                        const T (&q)[V], T bi) {
    T s = (T)0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        if constexpr (KERN == MF_RBF) {
            const T d = p[v] - q[v];
            s = s + d * d;
        } else {
            s = s + p[v] * q[v];
        }
    }
    return predict_one<T, KERN>(group_sum<GS>(s), bu, bi, h);
}

}  // namespace mf
