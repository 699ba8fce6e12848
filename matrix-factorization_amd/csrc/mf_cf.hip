// mf_cf.hip -- neighbourhood models (ItemItemCF / UserUserCF): per-entity
// statistics, the entity x entity similarity from the sparse ratings, and the
// top-n_neighbors weighted prediction (include/mf_hip.h, "neighbourhood
// models").
//
// One model, roles swapped: the ENTITIES are the items (ItemItemCF) or the
// users (UserUserCF), the OTHERS are the other side.  Ratings come in both
// orientations as device CSR (int64 offsets, int32 ids, float ratings).
//
// Every kernel here runs ONE WAVE per workgroup (64 threads): a wave's LDS
// traffic needs no cross-wave hand-off, its barrier is free, and neither
// kernel has work that four waves could share without atomics.
//   k_cf_similarity  LDS = 8 B x pass_cols (16 KiB at the automatic 2048
//                    columns: 10 workgroups = 10 waves per CU by LDS)
//   k_cf_neighbours  the stored-neighbours (top-M) build: k_cf_similarity's
//                    LDS + 1 KiB of bins (17 KiB: 9 per CU), persistent, one
//                    float32 scratch row per workgroup in the workspace
//   k_cf_predict     LDS = 8 KiB of keys + 1 KiB of bins (17 per CU by LDS,
//                    so the 16-workgroup-per-CU cap is what binds); a template
//                    over where the similarities come from (mf_cf.hpp)
// No floating-point atomics anywhere: equal inputs give equal bits.
#include "mf_cf.hpp"

namespace mf {
namespace cf {

constexpr int kAutoPassCols = 2048;          // 16 KiB of FP64 accumulators
constexpr int kMaxPassCols = 4096;           // 32 KiB: 5 workgroups per CU still
constexpr int kSearchMin = 128;              // lists longer than this are range-searched per pass

// ------------------------------------------------------------- statistics
// One thread per entity, its list read in list order: sum and sum of squares
// in FP64 (a float's square is exact in FP64).
__global__ void __launch_bounds__(kBlock)
k_cf_stats(const int64_t* __restrict__ ptr, const float* __restrict__ r, int32_t n_entities,
           double n_others, double* __restrict__ mean, double* __restrict__ norm) {
    const int64_t a = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (a >= n_entities) return;
    double s = 0.0, q = 0.0;
    for (int64_t j = ptr[a], e = ptr[a + 1]; j < e; ++j) {
        const double v = (double)r[j];
        s = s + v;
        q = q + v * v;
    }
    const double m = n_others > 0 ? s / n_others : 0.0;
    const double var = q - n_others * (m * m);
    mean[a] = m;
    norm[a] = var > 0.0 ? sqrt(var) : 0.0;
}

// ------------------------------------------------------------- similarity
__device__ __forceinline__ int64_t lower_bound(const int32_t* ids, int64_t lo, int64_t hi,
                                               int32_t key) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ids[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct SimArgs {
    const int64_t* eptr; const int32_t* eoth; const float* er;   // entity-major
    const int64_t* optr; const int32_t* oent; const float* orr;  // other-major, ids ascending
    const double* mean; const double* norm;
    float* S;
    int32_t n_entities, n_others, pass_cols;
};

// One wave (the workgroup): row a of S, columns [c0, c0 + nc), summed into
// acc[0 .. nc), this wave's LDS; wa = norm[a].
// acc[b] += r_ao * r_bo for every b of every other o of a, the o's in a's list
// order with a barrier between them; inside one o the b's are distinct, so no
// two lanes ever add into one address at a time and the order of the sum is
// that of a's list, whatever the column range.  With a's list ascending in o,
// S[a,b] and S[b,a] add the same (commuting) products in the same order: S is
// bitwise symmetric.  Shared by k_cf_similarity and k_cf_neighbours: one
// arithmetic, one order.
__device__ __forceinline__ void sim_accumulate(const SimArgs& A, int32_t a, int32_t c0, int32_t nc,
                                               double wa, double* acc, int lane) {
    const bool whole = A.pass_cols >= A.n_entities;
    for (int32_t c = lane; c < nc; c += kWave) acc[c] = 0.0;
    __syncthreads();
    if (wa > 0.0) {                                   // else the whole row is 0
        // 64 others of a at a time, one per lane: id, rating, list bounds (and
        // the range search) are loaded by all lanes at once, so the serial
        // walk below has one dependent load per other left, and that one --
        // the first 64 entries of the NEXT other's list -- is issued before
        // the current other's LDS updates
        for (int64_t j0 = A.eptr[a], je = A.eptr[a + 1]; j0 < je; j0 += kWave) {
            double ra_l = 0.0;
            int64_t lo_l = 0, hi_l = 0;               // lo == hi: nothing to apply
            if (j0 + lane < je) {
                const int32_t o = A.eoth[j0 + lane];
                if ((uint32_t)o < (uint32_t)A.n_others) {
                    ra_l = (double)A.er[j0 + lane];
                    lo_l = A.optr[o];
                    hi_l = A.optr[o + 1];
                    if (!whole && hi_l - lo_l > kSearchMin) {
                        lo_l = lower_bound(A.oent, lo_l, hi_l, c0);
                        hi_l = lower_bound(A.oent, lo_l, hi_l, c0 + nc);
                    }
                }
            }
            const int cnt = (int)min((int64_t)kWave, je - j0);
            auto first = [&](int64_t lo, int64_t hi, uint32_t& c, float& r) {
                const bool in = lo + lane < hi;
                c = in ? (uint32_t)A.oent[lo + lane] - (uint32_t)c0 : ~0u;
                r = in ? A.orr[lo + lane] : 0.f;
            };
            int64_t lo = __shfl(lo_l, 0, kWave), hi = __shfl(hi_l, 0, kWave);
            uint32_t c_cur, c_nxt = ~0u;
            float r_cur, r_nxt = 0.f;
            first(lo, hi, c_cur, r_cur);
            for (int s = 0; s < cnt; ++s) {
                const double ra = __shfl(ra_l, s, kWave);
                int64_t lo_n = 0, hi_n = 0;
                if (s + 1 < cnt) {                    // uniform
                    lo_n = __shfl(lo_l, s + 1, kWave);
                    hi_n = __shfl(hi_l, s + 1, kWave);
                    first(lo_n, hi_n, c_nxt, r_nxt);
                }
                if (c_cur < (uint32_t)nc) acc[c_cur] = acc[c_cur] + ra * (double)r_cur;
                for (int64_t t = lo + kWave + lane; t < hi; t += kWave) {
                    const uint32_t c = (uint32_t)A.oent[t] - (uint32_t)c0;
                    if (c < (uint32_t)nc) acc[c] = acc[c] + ra * (double)A.orr[t];
                }
                __syncthreads();
                lo = lo_n; hi = hi_n; c_cur = c_nxt; r_cur = r_nxt;
            }
        }
    }
}

// the FP64 epilogue: S[a, c0 .. c0 + nc) from the accumulators, rounded once, to row[0 .. nc)
__device__ __forceinline__ void sim_finish(const SimArgs& A, int32_t a, int32_t c0, int32_t nc,
                                           double wa, const double* acc, int lane, float* row) {
    const double n = (double)A.n_others, ma = A.mean[a];
    for (int32_t c = lane; c < nc; c += kWave) {
        const double wb = A.norm[c0 + c];
        float s = 0.f;
        if (wa > 0.0 && wb > 0.0)
            s = (float)((acc[c] - n * (ma * A.mean[c0 + c])) / (wa * wb));
        row[c] = s;
    }
}

// Workgroup (a, p): row a of S, columns [p * pass_cols, (p + 1) * pass_cols).
__global__ void __launch_bounds__(kWave)
k_cf_similarity(const SimArgs A) {
    extern __shared__ double acc[];
    const int32_t a = (int32_t)blockIdx.x;
    const int32_t c0 = (int32_t)blockIdx.y * A.pass_cols;
    const int32_t nc = min(A.pass_cols, A.n_entities - c0);
    const int lane = threadIdx.x;
    const double wa = A.norm[a];
    sim_accumulate(A, a, c0, nc, wa, acc, lane);
    sim_finish(A, a, c0, nc, wa, acc, lane, A.S + (size_t)a * (size_t)A.n_entities + c0);
}

// ------------------------------------------------------------- stored neighbours
struct NbrArgs {
    SimArgs sim;                                  // sim.S is not used
    float* scratch;                               // gridDim.x rows of n_entities floats
    int32_t* ids; float* sims;                    // n_entities x n_stored, every element written
    int32_t n_stored;
};

// Persistent one-wave workgroup: rows a = blockIdx.x, += gridDim.x.  Row a of S
// goes, one column range after the other (sim_accumulate / sim_finish: the
// dense kernel's values bit for bit), to this workgroup's scratch row; the
// n_stored-th key under make_key's order is found by select_cut, the keys
// rebuilt from the scratch row on every pass (pair_predict's long-list mode);
// the columns whose key is >= the cut are then emitted in ONE ordered pass, a
// ballot prefix count per 64 columns giving each its place: the row comes out
// id-ascending without a sort.  The dense row never leaves the scratch row
// (which the wave re-reads through L2).  Rows of a zero norm are all zeros and
// keep the lowest ids.  Integer LDS atomics only (the select's bins).
__global__ void __launch_bounds__(kWave)
k_cf_neighbours(const NbrArgs A) {
    extern __shared__ double acc[];
    __shared__ uint32_t bins[256];
    const SimArgs& P = A.sim;
    const int lane = threadIdx.x;
    const int32_t ne = P.n_entities, M = A.n_stored;
    float* srow = A.scratch + (size_t)blockIdx.x * (size_t)ne;
    for (int32_t a = (int32_t)blockIdx.x; a < ne; a += (int32_t)gridDim.x) {
        const double wa = P.norm[a];
        for (int32_t c0 = 0; c0 < ne; c0 += P.pass_cols) {
            const int32_t nc = min(P.pass_cols, ne - c0);
            sim_accumulate(P, a, c0, nc, wa, acc, lane);
            sim_finish(P, a, c0, nc, wa, acc, lane, srow + c0);
        }
        __syncthreads();                              // the scratch row, written by other lanes
        auto key_at = [&](int64_t j) -> uint64_t {
            return (int32_t)j == a ? 0 : make_key(srow[j], (int32_t)j);
        };
        const uint64_t cut = ne - 1 > M ? select_cut(bins, ne, (uint32_t)M, lane, key_at,
                                                     [] { __syncthreads(); })
                                        : 1;
        int32_t* oid = A.ids + (size_t)a * (size_t)M;
        float* osim = A.sims + (size_t)a * (size_t)M;
        int32_t base = 0;                             // kept so far: uniform
        for (int32_t j0 = 0; j0 < ne; j0 += kWave) {
            const int32_t j = j0 + lane;
            const float s = j < ne ? srow[j] : 0.f;
            const bool keep = j < ne && j != a && make_key(s, j) >= cut;
            const unsigned long long kept = __ballot(keep);
            const int32_t at = base + __popcll(kept & ((1ull << lane) - 1ull));
            if (keep && at < M) {                     // at < M: exactly min(M, ne - 1) are kept
                oid[at] = j;
                osim[at] = s;
            }
            base += __popcll(kept);
        }
        for (int32_t t = base + lane; t < M; t += kWave) {
            oid[t] = -1;
            osim[t] = 0.f;
        }
        __syncthreads();                              // the scratch row is read before the next row's writes
    }
}

// ------------------------------------------------------------- prediction
template <typename Sim>
struct PredArgs {
    const int32_t* ent; const int32_t* oth; int64_t n_pairs;
    const int64_t* optr; const int32_t* oent; const float* orr;
    Sim sim; const double* mean;
    double* out;
    int32_t n_entities, n_others, n_neighbors, bound;
    double global_mean, lo, hi;
};

// One wave per pair (e, o): pair_predict (mf_cf.hpp) over o's list.  The
// candidates are o's entries with r > 0 and id != e (Sim = ListSim: and id in
// e's stored row, which is searched through L2 -- at most 32 KiB, and one pair
// reads each candidate once: staging it would cost what it saves).
template <typename Sim>
__global__ void __launch_bounds__(kWave)
k_cf_predict(const PredArgs<Sim> A) {
    __shared__ uint64_t keys[kKeysLds];
    __shared__ uint32_t bins[256];
    const int64_t p = blockIdx.x;
    const int lane = threadIdx.x;
    const int32_t e = A.ent[p], o = A.oth[p];
    double pred;
    if ((uint32_t)e >= (uint32_t)A.n_entities || (uint32_t)o >= (uint32_t)A.n_others) {
        pred = A.global_mean;                         // unknown id (-1)
    } else {
        const int64_t beg = A.optr[o], end = A.optr[o + 1];
        const auto srow = A.sim.row(e);
        auto build = [&](int64_t j) -> uint64_t {     // 0: not a candidate
            const int32_t b = A.oent[beg + j];
            if ((uint32_t)b >= (uint32_t)A.n_entities || b == e || !(A.orr[beg + j] > 0.f))
                return 0;
            return srow.key(b);
        };
        auto dev = [&](int64_t j, uint64_t k) -> double {
            return (double)A.orr[beg + j] - A.mean[key_id(k)];
        };
        pred = pair_predict(keys, bins, end - beg, A.n_neighbors, lane, A.mean[e], build, dev,
                            [] { __syncthreads(); });
    }
    if (A.bound) pred = fmax(A.lo, fmin(A.hi, pred));
    if (lane == 0) A.out[p] = pred;
}

}  // namespace cf
}  // namespace mf

using namespace mf;

extern "C" int mf_cf_stats(const int64_t* entity_ptr, const void* ratings, int32_t n_entities,
                           int32_t n_others, int32_t dtype, double* mean, double* norm,
                           void* stream) {
    if (dtype != MF_F32) {
        set_error("mf_cf_stats: dtype=%d (float32 ratings only)", dtype);
        return MF_ERR_INVALID;
    }
    if (n_entities < 0) {
        set_error("mf_cf_stats: n_entities=%d (must be >= 0)", n_entities);
        return MF_ERR_INVALID;
    }
    if (n_others < 0) {
        set_error("mf_cf_stats: n_others=%d (must be >= 0)", n_others);
        return MF_ERR_INVALID;
    }
    if (n_entities == 0) return MF_OK;
    const void* need[] = {entity_ptr, mean, norm};
    const char* names[] = {"entity_ptr", "mean", "norm"};
    if (null_arg("mf_cf_stats", need, names, 3)) return MF_ERR_INVALID;
    hipLaunchKernelGGL(cf::k_cf_stats, dim3((unsigned)((n_entities + kBlock - 1) / kBlock)),
                       dim3(kBlock), 0, (hipStream_t)stream, entity_ptr,
                       static_cast<const float*>(ratings), n_entities, (double)n_others, mean,
                       norm);
    MF_HIP_CHECK(hipGetLastError());
    return MF_OK;
}

extern "C" int32_t mf_cf_pass_cols(int32_t n_entities, int32_t pass_cols) {
    if (n_entities <= 0 || pass_cols < 0 || pass_cols > cf::kMaxPassCols) return 0;
    const int32_t want = pass_cols == 0 ? cf::kAutoPassCols : pass_cols;
    return want < n_entities ? want : n_entities;
}

namespace mf {
namespace cf {

// what mf_cf_similarity and mf_cf_neighbours check alike, up to the NULL pointers
static int sim_check(const char* fn, int32_t n_entities, int32_t n_others, int32_t dtype,
                     int32_t pass_cols) {
    if (dtype != MF_F32) {
        set_error("%s: dtype=%d (float32 only)", fn, dtype);
        return MF_ERR_INVALID;
    }
    if (n_entities < 0) {
        set_error("%s: n_entities=%d (must be >= 0)", fn, n_entities);
        return MF_ERR_INVALID;
    }
    if (n_others < 0) {
        set_error("%s: n_others=%d (must be >= 0)", fn, n_others);
        return MF_ERR_INVALID;
    }
    if (pass_cols < 0 || pass_cols > kMaxPassCols) {
        set_error("%s: pass_cols=%d (must be in [0, %d]; 0 = automatic)", fn, pass_cols,
                  kMaxPassCols);
        return MF_ERR_INVALID;
    }
    return MF_OK;
}

// mf_cf_predict / mf_cf_predict_nbr; sim_need / sim_names: the similarity's arrays
template <typename Sim>
static int predict(const char* fn, const int32_t* entity_ids, const int32_t* other_ids,
                   int64_t n_pairs, const int64_t* other_ptr, const int32_t* list_entity_ids,
                   const void* list_ratings, const Sim& sim, const void* const* sim_need,
                   const char* const* sim_names, int n_sim, const double* mean,
                   int32_t n_entities, int32_t n_others, int32_t dtype, int32_t n_neighbors,
                   double global_mean, double min_rating, double max_rating,
                   int32_t bound_ratings, double* out, void* stream) {
    if (dtype != MF_F32) {
        set_error("%s: dtype=%d (float32 only)", fn, dtype);
        return MF_ERR_INVALID;
    }
    if (n_neighbors < 1) {
        set_error("%s: n_neighbors=%d (must be >= 1)", fn, n_neighbors);
        return MF_ERR_INVALID;
    }
    if (n_pairs < 0 || n_pairs > kMaxGrid) {
        set_error("%s: n_pairs=%lld (must be in [0, %lld]: one workgroup per pair)", fn,
                  (long long)n_pairs, (long long)kMaxGrid);
        return MF_ERR_INVALID;
    }
    if (n_entities < 0) {
        set_error("%s: n_entities=%d (must be >= 0)", fn, n_entities);
        return MF_ERR_INVALID;
    }
    if (n_others < 0) {
        set_error("%s: n_others=%d (must be >= 0)", fn, n_others);
        return MF_ERR_INVALID;
    }
    if (n_pairs == 0) return MF_OK;
    const void* need[] = {entity_ids, other_ids, out};
    const char* names[] = {"entity_ids", "other_ids", "out"};
    if (null_arg(fn, need, names, 3)) return MF_ERR_INVALID;
    if (n_entities > 0 && n_others > 0) {             // else every pair is unknown
        const void* need2[] = {other_ptr, mean};
        const char* names2[] = {"other_ptr", "mean"};
        if (null_arg(fn, need2, names2, 2) || null_arg(fn, sim_need, sim_names, n_sim))
            return MF_ERR_INVALID;
    }
    PredArgs<Sim> a;
    a.ent = entity_ids; a.oth = other_ids; a.n_pairs = n_pairs;
    a.optr = other_ptr; a.oent = list_entity_ids; a.orr = static_cast<const float*>(list_ratings);
    a.sim = sim; a.mean = mean; a.out = out;
    a.n_entities = n_entities; a.n_others = n_others; a.n_neighbors = n_neighbors;
    a.bound = bound_ratings ? 1 : 0;
    a.global_mean = global_mean; a.lo = min_rating; a.hi = max_rating;
    hipLaunchKernelGGL(k_cf_predict<Sim>, dim3((unsigned)n_pairs), dim3(kWave), 0,
                       (hipStream_t)stream, a);
    MF_HIP_CHECK(hipGetLastError());
    return MF_OK;
}

}  // namespace cf
}  // namespace mf

extern "C" int mf_cf_similarity(const int64_t* entity_ptr, const int32_t* other_ids,
                                const void* ratings, const int64_t* other_ptr,
                                const int32_t* entity_ids, const void* other_ratings,
                                int32_t n_entities, int32_t n_others, int32_t dtype,
                                const double* mean, const double* norm, int32_t pass_cols,
                                void* similarity, void* stream) {
    if (int rc = cf::sim_check("mf_cf_similarity", n_entities, n_others, dtype, pass_cols))
        return rc;
    if (n_entities == 0) return MF_OK;
    const void* need[] = {entity_ptr, other_ptr, mean, norm, similarity};
    const char* names[] = {"entity_ptr", "other_ptr", "mean", "norm", "similarity"};
    if (null_arg("mf_cf_similarity", need, names, 5)) return MF_ERR_INVALID;
    cf::SimArgs a;
    a.eptr = entity_ptr; a.eoth = other_ids; a.er = static_cast<const float*>(ratings);
    a.optr = other_ptr; a.oent = entity_ids; a.orr = static_cast<const float*>(other_ratings);
    a.mean = mean; a.norm = norm; a.S = static_cast<float*>(similarity);
    a.n_entities = n_entities; a.n_others = n_others;
    a.pass_cols = mf_cf_pass_cols(n_entities, pass_cols);
    const unsigned n_pass = (unsigned)((n_entities + a.pass_cols - 1) / a.pass_cols);
    if ((int64_t)n_entities * n_pass > cf::kMaxGrid) {
        set_error("mf_cf_similarity: n_entities=%d needs %lld workgroups (at most %lld)",
                  n_entities, (long long)n_entities * n_pass, (long long)cf::kMaxGrid);
        return MF_ERR_INVALID;
    }
    hipLaunchKernelGGL(cf::k_cf_similarity, dim3((unsigned)n_entities, n_pass), dim3(kWave),
                       (size_t)a.pass_cols * sizeof(double), (hipStream_t)stream, a);
    MF_HIP_CHECK(hipGetLastError());
    return MF_OK;
}

extern "C" size_t mf_cf_neighbours_workspace_bytes(int32_t n_entities, int32_t n_stored) {
    if (n_entities <= 0 || n_stored < 1 || n_stored > cf::kMaxStored) return 0;
    const size_t rows = n_entities < cf::kNbrSlots ? n_entities : cf::kNbrSlots;
    return rows * (size_t)n_entities * sizeof(float);
}

extern "C" int mf_cf_neighbours(const int64_t* entity_ptr, const int32_t* other_ids,
                                const void* ratings, const int64_t* other_ptr,
                                const int32_t* entity_ids, const void* other_ratings,
                                int32_t n_entities, int32_t n_others, int32_t dtype,
                                const double* mean, const double* norm, int32_t pass_cols,
                                int32_t n_stored, void* workspace, int32_t* nbr_ids,
                                void* nbr_sims, void* stream) {
    if (int rc = cf::sim_check("mf_cf_neighbours", n_entities, n_others, dtype, pass_cols))
        return rc;
    if (cf::bad_n_stored("mf_cf_neighbours", n_stored)) return MF_ERR_INVALID;
    if (n_entities == 0) return MF_OK;
    const void* need[] = {entity_ptr, other_ptr, mean, norm, workspace, nbr_ids, nbr_sims};
    const char* names[] = {"entity_ptr", "other_ptr", "mean", "norm", "workspace", "nbr_ids",
                           "nbr_sims"};
    if (null_arg("mf_cf_neighbours", need, names, 7)) return MF_ERR_INVALID;
    cf::NbrArgs a;
    a.sim.eptr = entity_ptr; a.sim.eoth = other_ids; a.sim.er = static_cast<const float*>(ratings);
    a.sim.optr = other_ptr; a.sim.oent = entity_ids;
    a.sim.orr = static_cast<const float*>(other_ratings);
    a.sim.mean = mean; a.sim.norm = norm; a.sim.S = nullptr;
    a.sim.n_entities = n_entities; a.sim.n_others = n_others;
    a.sim.pass_cols = mf_cf_pass_cols(n_entities, pass_cols);
    a.scratch = static_cast<float*>(workspace);
    a.ids = nbr_ids; a.sims = static_cast<float*>(nbr_sims); a.n_stored = n_stored;
    // one scratch row per workgroup: the grid is what the workspace was sized for
    const unsigned grid = (unsigned)(n_entities < cf::kNbrSlots ? n_entities : cf::kNbrSlots);
    hipLaunchKernelGGL(cf::k_cf_neighbours, dim3(grid), dim3(kWave),
                       (size_t)a.sim.pass_cols * sizeof(double), (hipStream_t)stream, a);
    MF_HIP_CHECK(hipGetLastError());
    return MF_OK;
}

extern "C" int mf_cf_predict(const int32_t* entity_ids, const int32_t* other_ids, int64_t n_pairs,
                             const int64_t* other_ptr, const int32_t* list_entity_ids,
                             const void* list_ratings, const void* similarity,
                             const double* mean, int32_t n_entities, int32_t n_others,
                             int32_t dtype, int32_t n_neighbors, double global_mean,
                             double min_rating, double max_rating, int32_t bound_ratings,
                             double* out, void* stream) {
    const cf::DenseSim sim{static_cast<const float*>(similarity), n_entities};
    const void* need[] = {similarity};
    const char* names[] = {"similarity"};
    return cf::predict("mf_cf_predict", entity_ids, other_ids, n_pairs, other_ptr,
                       list_entity_ids, list_ratings, sim, need, names, 1, mean, n_entities,
                       n_others, dtype, n_neighbors, global_mean, min_rating, max_rating,
                       bound_ratings, out, stream);
}

extern "C" int mf_cf_predict_nbr(const int32_t* entity_ids, const int32_t* other_ids,
                                 int64_t n_pairs, const int64_t* other_ptr,
                                 const int32_t* list_entity_ids, const void* list_ratings,
                                 const int32_t* nbr_ids, const void* nbr_sims, int32_t n_stored,
                                 const double* mean, int32_t n_entities, int32_t n_others,
                                 int32_t dtype, int32_t n_neighbors, double global_mean,
                                 double min_rating, double max_rating, int32_t bound_ratings,
                                 double* out, void* stream) {
    if (cf::bad_n_stored("mf_cf_predict_nbr", n_stored)) return MF_ERR_INVALID;
    const cf::ListSim sim = cf::list_sim(nbr_ids, nbr_sims, n_stored, n_entities);
    const void* need[] = {nbr_ids, nbr_sims};
    const char* names[] = {"nbr_ids", "nbr_sims"};
    return cf::predict("mf_cf_predict_nbr", entity_ids, other_ids, n_pairs, other_ptr,
                       list_entity_ids, list_ratings, sim, need, names, 2, mean, n_entities,
                       n_others, dtype, n_neighbors, global_mean, min_rating, max_rating,
                       bound_ratings, out, stream);
}

