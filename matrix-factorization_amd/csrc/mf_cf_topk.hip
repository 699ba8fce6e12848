// mf_cf_topk.hip -- neighbourhood models, one query against EVERY target:
// the dense scores, the best `amount` per query, and the exact ranks of given
// targets (include/mf_hip.h, "neighbourhood models").
//
// Ranking one user means predicting every item for them, and all those pairs
// share one operand that mf_cf_predict's workgroup-per-pair re-reads:
//   MF_CF_QUERY_OTHER   (item-item: the query user is the OTHER o, the targets
//     are all entities e): o's candidate list.  Staged once per workgroup in
//     LDS (id, or -1 where r <= 0; (double)r - mean[b]) for lists of up to
//     kKeysLds entries; a wave then only gathers S[e, b] along row e.
//   MF_CF_QUERY_ENTITY  (user-user: the query user is the ENTITY e, the
//     targets are all others o): row S[e, :].  It stays in L1 / L2, or, with
//     MF_CF_ROW_LDS=1 and up to kRowLdsMax entities, is staged in LDS.
// k_cf_scores: workgroup (query, block of targets), four waves, each taking
// every fourth target of the block through pair_predict (mf_cf.hpp) -- the
// arithmetic of k_cf_predict, so a score is mf_cf_predict's bit for bit.  The
// waves share nothing but the staged operand: inside the target loop they
// order their own LDS accesses and meet at no workgroup barrier.
//   LDS = 4 x (8 KiB keys + 1 KiB bins) + 12 KiB list (or the row): 48 KiB,
//   3 workgroups = 12 waves per CU.
// With stored neighbours (Sim = ListSim, the *_nbr entry points) a target's
// similarities are its id-ascending row of at most 4096 (id, sim): a binary
// search per candidate.  MF_CF_QUERY_ENTITY stages the query's row in LDS
// (8 B an entry: up to 32 KiB + the 36 KiB above, 2 workgroups per CU at the
// longest); MF_CF_QUERY_OTHER reads each target's short row through L2.
// k_cf_rank_count: integer only; a workgroup per query, a thread per target,
// the row's keys passing through LDS in tiles of 256.
// No floating-point atomics; no result depends on the blocking of the targets
// or on the chunking of the queries.
#include <climits>
#include <cstdlib>

#include "mf_cf.hpp"
#include "mf_order.hpp"

namespace mf {
namespace cf {

constexpr int kAutoTargets = 64;             // targets per workgroup: 16 per wave
constexpr int kRowLdsMax = 4096;             // entities whose S row fits 16 KiB of LDS
constexpr size_t kListLds = kKeysLds * (sizeof(double) + sizeof(int32_t));

template <typename Sim>
struct ScoreArgs {
    const int32_t* query;
    const int64_t* optr; const int32_t* oent; const float* orr;
    Sim sim; const double* mean;
    uint64_t* out;                               // [n_query x n_targets]: keys, or the doubles' bits
    int32_t n_query, side, n_entities, n_others, n_targets, n_neighbors, tpb, nblk, as_keys,
        row_lds, query_major;
    double global_mean;
};

template <typename Sim>
__global__ void __launch_bounds__(kBlock)
k_cf_scores(const ScoreArgs<Sim> A) {
    __shared__ uint64_t keys[kWavesPerBlock][kKeysLds];
    __shared__ uint32_t bins[kWavesPerBlock][256];
    extern __shared__ double stage[];            // the query's list, or its S row
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    // QUERY_OTHER: target-block major, each XCD a contiguous range of it -- the workgroups in
    // flight on an XCD are the queries of one or two target blocks, whose S rows then come
    // from that XCD's L2 and leave HBM once.  QUERY_ENTITY: query major in launch order
    // (the query's S row is the hot operand).  Measured both ways, DESIGN.md section 7.2;
    // MF_CF_QUERY_MAJOR=0 / 1 forces one (probes).
    const int64_t wg = A.query_major ? (int64_t)blockIdx.x : xcd_swizzle(blockIdx.x, gridDim.x);
    const int64_t q = A.query_major ? wg / A.nblk : wg % A.n_query;
    const int32_t t0 = (int32_t)(A.query_major ? wg % A.nblk : wg / A.n_query) * A.tpb;
    const int32_t t1 = (int32_t)min((int64_t)A.n_targets, (int64_t)t0 + A.tpb);
    const int32_t qid = A.query[q];
    uint64_t* out = A.out + q * A.n_targets;
    auto emit = [&](double v) -> uint64_t {
        return A.as_keys ? order_key(v) : (uint64_t)__double_as_longlong(v);
    };
    const int32_t n_ids = A.side == MF_CF_QUERY_OTHER ? A.n_others : A.n_entities;
    if ((uint32_t)qid >= (uint32_t)n_ids) {                 // unknown id (-1): workgroup-uniform
        for (int32_t t = t0 + tid; t < t1; t += kBlock) out[t] = emit(A.global_mean);
        return;
    }
    // this wave's LDS accesses in program order (they complete in issue order)
    auto wsync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    if (A.side == MF_CF_QUERY_OTHER) {
        const int64_t beg = A.optr[qid], len = A.optr[qid + 1] - beg;
        const bool staged = len <= kKeysLds;
        double* sdev = stage;
        int32_t* sid = reinterpret_cast<int32_t*>(stage + kKeysLds);
        if (staged)
            for (int64_t j = tid; j < len; j += kBlock) {
                const int32_t b = A.oent[beg + j];
                const float r = A.orr[beg + j];
                const bool ok = (uint32_t)b < (uint32_t)A.n_entities && r > 0.f;
                sid[j] = ok ? b : -1;
                sdev[j] = ok ? (double)r - A.mean[b] : 0.0;
            }
        __syncthreads();
        for (int32_t e = t0 + wv; e < t1; e += kWavesPerBlock) {
            const auto srow = A.sim.row(e);
            const double me = A.mean[e];
            double pred;
            if (staged) {
                auto build = [&](int64_t j) -> uint64_t {
                    const int32_t b = sid[j];
                    return (b < 0 || b == e) ? 0 : srow.key(b);
                };
                auto dev = [&](int64_t j, uint64_t) -> double { return sdev[j]; };
                pred = pair_predict(keys[wv], bins[wv], len, A.n_neighbors, lane, me, build, dev,
                                    wsync);
            } else {
                auto build = [&](int64_t j) -> uint64_t {
                    const int32_t b = A.oent[beg + j];
                    if ((uint32_t)b >= (uint32_t)A.n_entities || b == e ||
                        !(A.orr[beg + j] > 0.f))
                        return 0;
                    return srow.key(b);
                };
                auto dev = [&](int64_t j, uint64_t k) -> double {
                    return (double)A.orr[beg + j] - A.mean[key_id(k)];
                };
                pred = pair_predict(keys[wv], bins[wv], len, A.n_neighbors, lane, me, build, dev,
                                    wsync);
            }
            if (lane == 0) out[e] = emit(pred);
        }
    } else {
        const int32_t e = qid;
        auto srow = A.sim.row(e);
        if constexpr (Sim::kLists) {                 // the query's stored row: sims, then ids
            float* sims = reinterpret_cast<float*>(stage);
            int32_t* ids = reinterpret_cast<int32_t*>(sims + srow.n);
            for (int32_t c = tid; c < srow.n; c += kBlock) {
                sims[c] = srow.sims[c];
                ids[c] = srow.ids[c];
            }
            srow.sims = sims;
            srow.ids = ids;
        } else if (A.row_lds) {
            float* row = reinterpret_cast<float*>(stage);
            for (int32_t c = tid; c < A.n_entities; c += kBlock) row[c] = srow.s[c];
            srow.s = row;
        }
        __syncthreads();
        const double me = A.mean[e];
        for (int32_t o = t0 + wv; o < t1; o += kWavesPerBlock) {
            const int64_t beg = A.optr[o], len = A.optr[o + 1] - beg;
            auto build = [&](int64_t j) -> uint64_t {
                const int32_t b = A.oent[beg + j];
                if ((uint32_t)b >= (uint32_t)A.n_entities || b == e || !(A.orr[beg + j] > 0.f))
                    return 0;
                return srow.key(b);
            };
            auto dev = [&](int64_t j, uint64_t k) -> double {
                return (double)A.orr[beg + j] - A.mean[key_id(k)];
            };
            const double pred = pair_predict(keys[wv], bins[wv], len, A.n_neighbors, lane, me,
                                             build, dev, wsync);
            if (lane == 0) out[o] = emit(pred);
        }
    }
}

// Query q = blockIdx.x: out_rank[t] = number of the row's non-zero keys that
// come before target t's (cand_before), -1 for a target out of range or with
// key 0; out_cand[q] = number of non-zero keys.  Thread j of a segment of 256
// targets holds one target; the row passes through LDS 256 keys at a time and
// every thread of a wave that holds a target compares all of them with its
// own.  One writer per output: no atomics.
__global__ void __launch_bounds__(kBlock)
k_cf_rank_count(const uint64_t* __restrict__ keys, int32_t n_targets,
                const int64_t* __restrict__ tg_ptr, const int32_t* __restrict__ tg_items,
                int32_t* __restrict__ out_rank, int32_t* __restrict__ out_cand) {
    __shared__ uint64_t tile[kBlock];
    __shared__ int wsum[kWavesPerBlock];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const uint64_t* K = keys + q * n_targets;
    const int64_t tb = tg_ptr[q], tn = tg_ptr[q + 1] - tb;
    const int64_t nseg = tn > 0 ? (tn + kBlock - 1) / kBlock : 1;   // segment 0 also counts
    int ncand = 0;
    for (int64_t seg = 0; seg < nseg; ++seg) {
        const int64_t j = seg * kBlock + tid;
        const bool have = j < tn;
        const int32_t it = have ? tg_items[tb + j] : -1;
        bool ok = have && (uint32_t)it < (uint32_t)n_targets;
        const uint64_t tk = ok ? K[it] : 0ull;
        ok = ok && tk != 0ull;
        const bool wave_has = __ballot(ok) != 0ull;
        int cnt = 0;
        for (int32_t c0 = 0; c0 < n_targets; c0 += kBlock) {
            const int32_t c = c0 + tid;
            const uint64_t kk = c < n_targets ? K[c] : 0ull;
            tile[tid] = kk;
            if (seg == 0) ncand += kk != 0ull;
            __syncthreads();
            if (wave_has) {                                      // wave-uniform
                const int m = min(kBlock, n_targets - c0);
                for (int x = 0; x < m; ++x) {
                    const uint64_t kx = tile[x];
                    cnt += (kx != 0ull && cand_before(kx, c0 + x, tk, it)) ? 1 : 0;
                }
            }
            __syncthreads();
        }
        if (have) out_rank[tb + j] = ok ? cnt : -1;
    }
    ncand = wave_sum(ncand);
    if ((tid & (kWave - 1)) == 0) wsum[tid / kWave] = ncand;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) t += wsum[w];
        out_cand[q] = t;
    }
}


// Dense: S.  Stored neighbours (n_stored >= 1): nbr_ids / nbr_sims.
struct Model {
    const int64_t* optr; const int32_t* oent; const void* orr;
    const void* S; const double* mean;
    int32_t n_entities, n_others, dtype, n_neighbors;
    double global_mean;
    int32_t targets_per_block;
    const int32_t* nbr_ids = nullptr; const void* nbr_sims = nullptr;
    int32_t n_stored = 0;
};

inline int32_t targets_of(int32_t side, int32_t n_entities, int32_t n_others) {
    return side == MF_CF_QUERY_OTHER ? n_entities : n_others;
}

inline bool row_in_lds(int32_t n_entities) {
    const char* e = std::getenv("MF_CF_ROW_LDS");
    return e && std::atoi(e) == 1 && n_entities <= kRowLdsMax;
}

// the checks every entry point shares, up to the NULL pointers; *done: nothing to do
static int check(const char* fn, const int32_t* query, int32_t n_query, int32_t side,
                 const Model& M, bool lists, bool* done) {
    *done = false;
    if (M.dtype != MF_F32) {
        set_error("%s: dtype=%d (float32 only)", fn, M.dtype);
        return MF_ERR_INVALID;
    }
    if (side != MF_CF_QUERY_OTHER && side != MF_CF_QUERY_ENTITY) {
        set_error("%s: query_side=%d (must be MF_CF_QUERY_OTHER or MF_CF_QUERY_ENTITY)", fn,
                  side);
        return MF_ERR_INVALID;
    }
    if (M.n_neighbors < 1) {
        set_error("%s: n_neighbors=%d (must be >= 1)", fn, M.n_neighbors);
        return MF_ERR_INVALID;
    }
    if (lists && bad_n_stored(fn, M.n_stored)) return MF_ERR_INVALID;
    if (M.targets_per_block < 0) {
        set_error("%s: targets_per_block=%d (must be >= 0; 0 = automatic)", fn,
                  M.targets_per_block);
        return MF_ERR_INVALID;
    }
    if (n_query < 0) {
        set_error("%s: n_query=%d (must be >= 0)", fn, n_query);
        return MF_ERR_INVALID;
    }
    if (M.n_entities < 0) {
        set_error("%s: n_entities=%d (must be >= 0)", fn, M.n_entities);
        return MF_ERR_INVALID;
    }
    if (M.n_others < 0) {
        set_error("%s: n_others=%d (must be >= 0)", fn, M.n_others);
        return MF_ERR_INVALID;
    }
    if (n_query == 0) {
        *done = true;
        return MF_OK;
    }
    if (!query) {
        set_error("%s: query_ids is NULL", fn);
        return MF_ERR_INVALID;
    }
    if (M.n_entities > 0 && M.n_others > 0) {         // else every query is unknown or has no target
        const void* dense[] = {M.optr, M.S, M.mean};
        const char* dense_names[] = {"other_ptr", "similarity", "mean"};
        const void* stored[] = {M.optr, M.nbr_ids, M.nbr_sims, M.mean};
        const char* stored_names[] = {"other_ptr", "nbr_ids", "nbr_sims", "mean"};
        if (lists ? null_arg(fn, stored, stored_names, 4) : null_arg(fn, dense, dense_names, 3))
            return MF_ERR_INVALID;
    }
    const int32_t nt = targets_of(side, M.n_entities, M.n_others);
    const int32_t tpb = mf_cf_targets_per_block(nt, M.targets_per_block);
    const int64_t nblk = nt > 0 ? ((int64_t)nt + tpb - 1) / tpb : 0;
    if ((int64_t)n_query * nblk > INT_MAX) {
        set_error("%s: n_query=%d needs %lld workgroups (at most %d a call)", fn, n_query,
                  (long long)n_query * nblk, INT_MAX);
        return MF_ERR_INVALID;
    }
    return MF_OK;
}

template <typename Sim>
static int launch_scores_as(const Sim& sim, const int32_t* query, int32_t n_query, int32_t side,
                            const Model& M, uint64_t* out, bool as_keys, hipStream_t stream) {
    ScoreArgs<Sim> a;
    a.query = query; a.n_query = n_query;
    a.optr = M.optr; a.oent = M.oent; a.orr = static_cast<const float*>(M.orr);
    a.sim = sim; a.mean = M.mean; a.out = out;
    a.side = side; a.n_entities = M.n_entities; a.n_others = M.n_others;
    a.n_targets = targets_of(side, M.n_entities, M.n_others);
    if (a.n_targets == 0) return MF_OK;
    a.n_neighbors = M.n_neighbors;
    a.tpb = mf_cf_targets_per_block(a.n_targets, M.targets_per_block);
    a.nblk = (a.n_targets + a.tpb - 1) / a.tpb;
    a.as_keys = as_keys ? 1 : 0;
    a.row_lds = !Sim::kLists && side == MF_CF_QUERY_ENTITY && row_in_lds(M.n_entities) ? 1 : 0;
    a.global_mean = M.global_mean;
    const char* qm = std::getenv("MF_CF_QUERY_MAJOR");
    a.query_major = qm && *qm ? (std::atoi(qm) == 1 ? 1 : 0) : (side == MF_CF_QUERY_ENTITY ? 1 : 0);
    size_t lds = kListLds;
    if (side == MF_CF_QUERY_ENTITY) lds = a.row_lds ? sizeof(float) * (size_t)M.n_entities : 0;
    auto kfn = k_cf_scores<Sim>;
    if constexpr (Sim::kLists)
        if (side == MF_CF_QUERY_ENTITY) {
            // the query's stored row (<= 32 KiB) beside the 36 KiB of keys and bins
            lds = (sizeof(float) + sizeof(int32_t)) * (size_t)sim.n_valid;
            MF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kfn),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(kMaxStored * (sizeof(float) + sizeof(int32_t)))));
        }
    hipLaunchKernelGGL(kfn, dim3((unsigned)((int64_t)n_query * a.nblk)), dim3(kBlock), lds,
                       stream, a);
    return MF_OK;
}

static int launch_scores(const int32_t* query, int32_t n_query, int32_t side, const Model& M,
                         uint64_t* out, bool as_keys, hipStream_t stream) {
    if (M.n_stored)
        return launch_scores_as(list_sim(M.nbr_ids, M.nbr_sims, M.n_stored, M.n_entities), query,
                                n_query, side, M, out, as_keys, stream);
    return launch_scores_as(DenseSim{static_cast<const float*>(M.S), M.n_entities}, query,
                            n_query, side, M, out, as_keys, stream);
}

// the three entry points, dense (mf_cf_*) and stored-neighbours (mf_cf_*_nbr) alike
static int scores(const char* fn, bool lists, const int32_t* query_ids, int32_t n_query,
                  int32_t query_side, const Model& M, double* out, void* stream) {
    bool done;
    if (int rc = check(fn, query_ids, n_query, query_side, M, lists, &done)) return rc;
    if (done || targets_of(query_side, M.n_entities, M.n_others) == 0) return MF_OK;
    if (!out) {
        set_error("%s: out is NULL", fn);
        return MF_ERR_INVALID;
    }
    if (int rc = launch_scores(query_ids, n_query, query_side, M, reinterpret_cast<uint64_t*>(out),
                               false, (hipStream_t)stream))
        return rc;
    MF_HIP_CHECK(hipGetLastError());
    return MF_OK;
}

static int topk(const char* fn, bool lists, const int32_t* query_ids, int32_t n_query,
                int32_t query_side, const Model& M, const int64_t* exclude_ptr,
                const int32_t* exclude_items, int32_t amount, void* workspace,
                int32_t* out_items, double* out_scores, void* stream) {
    if (amount < 1 || amount > 2048) {
        set_error("%s: amount=%d (must be in [1, 2048])", fn, amount);
        return MF_ERR_INVALID;
    }
    bool done;
    if (int rc = check(fn, query_ids, n_query, query_side, M, lists, &done)) return rc;
    if (done) return MF_OK;
    const int32_t nt = targets_of(query_side, M.n_entities, M.n_others);
    const void* need[] = {workspace, out_items, out_scores};
    const char* names[] = {"workspace", "out_items", "out_scores"};
    if (null_arg(fn, need, names, 3)) return MF_ERR_INVALID;
    uint64_t* keys = static_cast<uint64_t*>(workspace);
    if (int rc = launch_scores(query_ids, n_query, query_side, M, keys, true, (hipStream_t)stream))
        return rc;
    topk_select_f64(keys, n_query, nt, exclude_ptr, exclude_items, amount, out_items, out_scores,
                    (hipStream_t)stream);
    MF_HIP_CHECK(hipGetLastError());
    return MF_OK;
}

static int rank(const char* fn, bool lists, const int32_t* query_ids, int32_t n_query,
                int32_t query_side, const Model& M, const int64_t* exclude_ptr,
                const int32_t* exclude_items, const int64_t* target_ptr,
                const int32_t* target_items, void* workspace, int32_t* out_rank,
                int32_t* out_candidates, void* stream) {
    bool done;
    if (int rc = check(fn, query_ids, n_query, query_side, M, lists, &done)) return rc;
    if (done) return MF_OK;
    const int32_t nt = targets_of(query_side, M.n_entities, M.n_others);
    const void* need[] = {target_ptr, target_items, workspace, out_rank, out_candidates};
    const char* names[] = {"target_ptr", "target_items", "workspace", "out_rank",
                           "out_candidates"};
    if (null_arg(fn, need, names, 5)) return MF_ERR_INVALID;
    uint64_t* keys = static_cast<uint64_t*>(workspace);
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = launch_scores(query_ids, n_query, query_side, M, keys, true, s)) return rc;
    if (nt > 0 && exclude_ptr && exclude_items)
        topk_exclude_keys(keys, n_query, nt, exclude_ptr, exclude_items, s);
    hipLaunchKernelGGL(k_cf_rank_count, dim3((unsigned)n_query), dim3(kBlock), 0, s,
                       (const uint64_t*)keys, nt, target_ptr, target_items, out_rank,
                       out_candidates);
    MF_HIP_CHECK(hipGetLastError());
    return MF_OK;
}

}  // namespace cf
}  // namespace mf

using namespace mf;

extern "C" int32_t mf_cf_targets_per_block(int32_t n_targets, int32_t targets_per_block) {
    if (n_targets <= 0 || targets_per_block < 0) return 0;
    const int32_t want = targets_per_block == 0 ? cf::kAutoTargets : targets_per_block;
    return want < n_targets ? want : n_targets;
}

extern "C" size_t mf_cf_topk_workspace_bytes(int32_t n_query, int32_t n_targets) {
    if (n_query <= 0 || n_targets <= 0) return 0;
    return sizeof(uint64_t) * (size_t)n_query * (size_t)n_targets;
}

extern "C" size_t mf_cf_rank_workspace_bytes(int32_t n_query, int32_t n_targets) {
    return mf_cf_topk_workspace_bytes(n_query, n_targets);
}

extern "C" int mf_cf_scores(const int32_t* query_ids, int32_t n_query, int32_t query_side,
                            const int64_t* other_ptr, const int32_t* list_entity_ids,
                            const void* list_ratings, const void* similarity, const double* mean,
                            int32_t n_entities, int32_t n_others, int32_t dtype,
                            int32_t n_neighbors, double global_mean, int32_t targets_per_block,
                            double* out, void* stream) {
    const cf::Model M{other_ptr, list_entity_ids, list_ratings, similarity, mean, n_entities,
                      n_others, dtype, n_neighbors, global_mean, targets_per_block};
    return cf::scores("mf_cf_scores", false, query_ids, n_query, query_side, M, out, stream);
}

extern "C" int mf_cf_topk(const int32_t* query_ids, int32_t n_query, int32_t query_side,
                          const int64_t* other_ptr, const int32_t* list_entity_ids,
                          const void* list_ratings, const void* similarity, const double* mean,
                          int32_t n_entities, int32_t n_others, int32_t dtype,
                          int32_t n_neighbors, double global_mean, int32_t targets_per_block,
                          const int64_t* exclude_ptr, const int32_t* exclude_items,
                          int32_t amount, void* workspace, int32_t* out_items,
                          double* out_scores, void* stream) {
    const cf::Model M{other_ptr, list_entity_ids, list_ratings, similarity, mean, n_entities,
                      n_others, dtype, n_neighbors, global_mean, targets_per_block};
    return cf::topk("mf_cf_topk", false, query_ids, n_query, query_side, M, exclude_ptr,
                    exclude_items, amount, workspace, out_items, out_scores, stream);
}

extern "C" int mf_cf_rank(const int32_t* query_ids, int32_t n_query, int32_t query_side,
                          const int64_t* other_ptr, const int32_t* list_entity_ids,
                          const void* list_ratings, const void* similarity, const double* mean,
                          int32_t n_entities, int32_t n_others, int32_t dtype,
                          int32_t n_neighbors, double global_mean, int32_t targets_per_block,
                          const int64_t* exclude_ptr, const int32_t* exclude_items,
                          const int64_t* target_ptr, const int32_t* target_items,
                          void* workspace, int32_t* out_rank, int32_t* out_candidates,
                          void* stream) {
    const cf::Model M{other_ptr, list_entity_ids, list_ratings, similarity, mean, n_entities,
                      n_others, dtype, n_neighbors, global_mean, targets_per_block};
    return cf::rank("mf_cf_rank", false, query_ids, n_query, query_side, M, exclude_ptr,
                    exclude_items, target_ptr, target_items, workspace, out_rank, out_candidates,
                    stream);
}

// ---- the same three from stored neighbour lists (mf_cf_neighbours' output)
extern "C" int mf_cf_scores_nbr(const int32_t* query_ids, int32_t n_query, int32_t query_side,
                                const int64_t* other_ptr, const int32_t* list_entity_ids,
                                const void* list_ratings, const int32_t* nbr_ids,
                                const void* nbr_sims, int32_t n_stored, const double* mean,
                                int32_t n_entities, int32_t n_others, int32_t dtype,
                                int32_t n_neighbors, double global_mean,
                                int32_t targets_per_block, double* out, void* stream) {
    const cf::Model M{other_ptr, list_entity_ids, list_ratings, nullptr, mean, n_entities,
                      n_others, dtype, n_neighbors, global_mean, targets_per_block,
                      nbr_ids, nbr_sims, n_stored};
    return cf::scores("mf_cf_scores_nbr", true, query_ids, n_query, query_side, M, out, stream);
}

extern "C" int mf_cf_topk_nbr(const int32_t* query_ids, int32_t n_query, int32_t query_side,
                              const int64_t* other_ptr, const int32_t* list_entity_ids,
                              const void* list_ratings, const int32_t* nbr_ids,
                              const void* nbr_sims, int32_t n_stored, const double* mean,
                              int32_t n_entities, int32_t n_others, int32_t dtype,
                              int32_t n_neighbors, double global_mean, int32_t targets_per_block,
                              const int64_t* exclude_ptr, const int32_t* exclude_items,
                              int32_t amount, void* workspace, int32_t* out_items,
                              double* out_scores, void* stream) {
    const cf::Model M{other_ptr, list_entity_ids, list_ratings, nullptr, mean, n_entities,
                      n_others, dtype, n_neighbors, global_mean, targets_per_block,
                      nbr_ids, nbr_sims, n_stored};
    return cf::topk("mf_cf_topk_nbr", true, query_ids, n_query, query_side, M, exclude_ptr,
                    exclude_items, amount, workspace, out_items, out_scores, stream);
}

extern "C" int mf_cf_rank_nbr(const int32_t* query_ids, int32_t n_query, int32_t query_side,
                              const int64_t* other_ptr, const int32_t* list_entity_ids,
                              const void* list_ratings, const int32_t* nbr_ids,
                              const void* nbr_sims, int32_t n_stored, const double* mean,
                              int32_t n_entities, int32_t n_others, int32_t dtype,
                              int32_t n_neighbors, double global_mean, int32_t targets_per_block,
                              const int64_t* exclude_ptr, const int32_t* exclude_items,
                              const int64_t* target_ptr, const int32_t* target_items,
                              void* workspace, int32_t* out_rank, int32_t* out_candidates,
                              void* stream) {
    const cf::Model M{other_ptr, list_entity_ids, list_ratings, nullptr, mean, n_entities,
                      n_others, dtype, n_neighbors, global_mean, targets_per_block,
                      nbr_ids, nbr_sims, n_stored};
    return cf::rank("mf_cf_rank_nbr", true, query_ids, n_query, query_side, M, exclude_ptr,
                    exclude_items, target_ptr, target_items, workspace, out_rank, out_candidates,
                    stream);
}
