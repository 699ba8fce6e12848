/*
 * mf_hip.h -- C ABI of libmf_hip.so, the MI355X (gfx950) implementation of
 * the SGD latent-factor update loop of SHEEPididoo/matrix-factorization.
 *
 * Drop-in boundary.  The reference crosses from Python into native (numba
 * JIT) code at exactly three functions of
 * matrix_factorization/kernel_matrix_factorization.py and four of
 * matrix_factorization/baseline_model.py; each entry point below replaces
 * one of them (file:line of the reference cited per function).  The
 * reference passes NumPy arrays that the callee mutates in place; here the
 * caller passes device pointers (HBM, e.g. torch-ROCm tensor storage) that
 * the callee mutates in place, plus an explicit hipStream_t.
 *
 * Conventions
 *   - every function returns 0 on success, a MF_ERR_* code otherwise;
 *     mf_last_error() returns a thread-local message for the last failure;
 *   - device pointers are caller-owned; no entry point allocates device
 *     memory except where a workspace size is documented;
 *   - `dtype` selects the parameter/rating storage type: MF_F32 or MF_F64;
 *     ids are int32 (internal ids 0..n-1, -1 = unknown where allowed);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     all kernels are enqueued asynchronously on it, no host sync unless the
 *     optional timing output is requested;
 *   - host-side schedulers (mf_sched_*) take host pointers and never touch
 *     the GPU.
 */
#ifndef MF_HIP_H
#define MF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MF_ABI_VERSION 1

enum {
    MF_OK = 0,
    MF_ERR_INVALID = 1,   /* bad argument (shape, enum, range)             */
    MF_ERR_HIP = 2,       /* HIP runtime error                             */
    MF_ERR_CAPACITY = 3,  /* caller-provided output buffer too small        */
    MF_ERR_NOMEM = 4      /* host allocation failed (schedulers)            */
};

enum { MF_F32 = 0, MF_F64 = 1 };

/* kernel codes: KernelMF(kernel=...) kernel_matrix_factorization.py:56,66 */
enum { MF_LINEAR = 0, MF_SIGMOID = 1, MF_RBF = 2 };

/* flags for mf_sgd_epoch */
enum {
    MF_FLAG_XCD_SWIZZLE = 1,  /* map consecutive tiles of a batch onto one XCD */
    MF_FLAG_NT_USER = 2,      /* stream user rows/biases/triples non-temporally */
    MF_FLAG_NT_ITEM = 4,      /* (unused by the current kernels)                */
    MF_FLAG_XCD_CLAIM = 8,    /* workgroups claim the tiles of the item slice of
                                 the XCD they run on (needs `workspace`)        */
    MF_FLAG_PERSISTENT = 16,  /* mf_sgd_epoch_strata: the whole epoch in one
                                 launch, item slabs resident in LDS (needs
                                 `workspace`; falls back to one launch per
                                 stratum when the grid cannot be co-resident) */
    MF_FLAG_DEEP_PIPE = 32,   /* with MF_FLAG_PERSISTENT: user rows gathered two
                                 steps ahead (blocks of few steps)               */
    MF_FLAG_NO_COOP = 64,     /* with MF_FLAG_PERSISTENT: plain launch instead of
                                 hipLaunchCooperativeKernel (diagnostic A/B; the
                                 occupancy check is then the only guard)         */
    MF_FLAG_NARROW = 128,     /* strata: a plan built for mf_strata_slots_waves(k,
                                 dtype, 4) runs on 4-wave workgroups whose lane
                                 groups are half as wide (two vectors per lane;
                                 FP32, n_factors a multiple of 4 up to 32) */
    MF_FLAG_L2_HANDOFF = 256, /* with MF_FLAG_PERSISTENT and an XCD-class stratum
                                 order: a block whose user range goes next to a
                                 workgroup on the SAME XCD (checked at run time
                                 from the XCC ids the workgroups publish) stores
                                 its user rows plainly, so they stay in that
                                 XCD's L2 for the successor's loads; before a
                                 hand-off to another XCD the producer writes its
                                 XCD's L2 back (agent release).  Needs rows of a
                                 whole number of 128-B lines and a 128-B aligned
                                 P; ignored otherwise (and with user-range
                                 classes C > 1). */
    MF_FLAG_NO_EARLY_POLL = 512, /* with MF_FLAG_PERSISTENT and classes C > 1: wait
                                 for each position's user range at its start
                                 instead of polling it once during the previous
                                 block (diagnostic A/B) */
    MF_FLAG_STREAM = 1024,    /* with MF_FLAG_PERSISTENT, MF_FLAG_DEEP_PIPE and
                                 classes C > 1: the stream form -- one software
                                 pipeline through all positions of the launch
                                 (the next block's triples and user rows loaded
                                 while the current block's last steps apply,
                                 the bias slices double-buffered in LDS); the
                                 same sequential order, bit for bit */
    MF_FLAG_PREPARE = 2048,   /* mf_sgd_epoch_strata: no launch -- only the
                                 launcher's one-time runtime work for this plan
                                 (kernel attributes, the co-residency query),
                                 so the first epoch does not pay it; the
                                 parameter pointers are not touched */
    /* mf_sgd_epoch_strata: bits 24..27 = C - 1, the plan's user-range classes
       (mf_strata_plan_build_classes; 0 = C = 1, the plain B x B plan) */
    MF_FLAG_CLASSES_SHIFT = 24
};
/* Jobs of one mf_permute_rows launch. */
#define MF_PERMUTE_MAX_JOBS 4
/* Largest number of user-range classes a strata plan may have. */
#define MF_STRATA_MAX_CLASSES 4

const char* mf_last_error(void);
int mf_abi_version(void);
/* One empty kernel launch per translation unit of this library on `stream`,
 * and one cooperative launch: makes the runtime load the code objects for
 * the current device now (the engine calls it while it is built) instead of
 * inside the first training epoch.  flags & MF_FLAG_NO_COOP: no cooperative
 * launch (rocprofv3's dispatch interception crashes on one). */
int mf_warmup(int32_t flags, void* stream);
/* Up to MF_PERMUTE_MAX_JOBS row arrays permuted in one launch (the relabelled
 * strata plans' parameter moves): job j has n_rows[j]
 * rows of row_bytes[j] bytes (a multiple of 4); mode 0 gathers dst[r] =
 * src[idx[r]], mode 1 scatters dst[idx[r]] = src[r].  DEVICE pointers in
 * HOST arrays of n_jobs; idx[j] has n_rows[j] entries in [0, n_rows[j]). */
int mf_permute_rows(int32_t n_jobs, void* const* dst, const void* const* src,
                    const int64_t* const* idx, const int64_t* n_rows,
                    const int32_t* row_bytes, int32_t mode, void* stream);
/* Largest n_factors the kernels accept (inclusive). */
int mf_max_factors(void);

/*
 * One SGD epoch over a conflict-free batch schedule.
 *
 * Replaces the body of one epoch of `_sgd`
 * (kernel_matrix_factorization.py:369-425: the sweep that calls
 * kernel_{linear,sigmoid,rbf}_sgd_update, kernels.py:108-327, once per
 * rating).  The reference visits ratings in one sequential order.  Here that
 * order is given as batches: batch b holds the ratings at schedule positions
 * [batch_offsets[b], batch_offsets[b+1]); no two ratings of a batch share a
 * user row (when update_user_params) or an item row (when
 * update_item_params), so every batch is applied in parallel and the result
 * equals the sequential sweep in the order
 *     batch_seq[0], batch_seq[1], ...   (each batch in any internal order).
 * The schedulers below produce such batches (exactly for a given
 * permutation, or by edge colouring for throughput).
 *
 *   user_ids, item_ids, ratings  device, n_ratings each (ratings: dtype)
 *   order          device, nullable: schedule position -> rating index; when
 *                  NULL, position p is rating p (ratings pre-sorted)
 *   batch_offsets  HOST, n_batches + 1 positions (non-decreasing, last <= n)
 *   batch_seq      HOST, nullable, n_seq batch indices: launch order (a full
 *                  epoch passes a permutation of 0..n_batches-1; a prefix
 *                  applies a partial epoch).  NULL = 0, 1, ..., n_batches-1
 *                  and n_seq is ignored
 *   user_biases / item_biases      device, dtype, n_users / n_items
 *   user_features / item_features  device, dtype, row-major
 *                  (n_users, n_factors) / (n_items, n_factors)
 *   kernel, gamma, lr, reg, min_rating, max_rating
 *                  as KernelMF (a = min_rating, c = max_rating - min_rating,
 *                  kernel_matrix_factorization.py:405-406)
 *   update_user_params / update_item_params   as _sgd (:336-337)
 *   flags          MF_FLAG_* bits; bits 16..23 = timing stride S (0 = 1)
 *   workspace      device, nullable: >= mf_sgd_workspace_bytes(launches)
 *                  bytes, required by MF_FLAG_XCD_CLAIM (tile counters,
 *                  zeroed by the call on `stream`)
 *   kernel_ms      host, nullable, 2 doubles: when given, every S-th launch
 *                  is bracketed by hipEvents on `stream`, the stream is
 *                  synchronised, kernel_ms[0] = summed time (ms) of the
 *                  bracketed launches and kernel_ms[1] = their count.
 */
int mf_sgd_epoch(const int32_t* user_ids, const int32_t* item_ids,
                 const void* ratings, int64_t n_ratings, const int32_t* order,
                 const int64_t* batch_offsets, int32_t n_batches,
                 const int32_t* batch_seq, int32_t n_seq,
                 double global_mean, void* user_biases,
                 void* item_biases, void* user_features, void* item_features,
                 int32_t n_users, int32_t n_items, int32_t n_factors,
                 int32_t kernel, int32_t dtype, double gamma, double lr,
                 double reg, double min_rating, double max_rating,
                 int32_t update_user_params, int32_t update_item_params,
                 int32_t flags, void* workspace, size_t workspace_bytes,
                 void* stream, double* kernel_ms);
size_t mf_sgd_workspace_bytes(int32_t n_launch);

/*
 * One epoch (or the strata listed in strata_seq) of the STRATIFIED sweep:
 * the throughput form of `_sgd`'s loop (kernel_matrix_factorization.py:
 * 371-425), same per-rating updates (kernels.py:108-327).  The plan comes
 * from mf_strata_plan_build: B user ranges and B item ranges
 * (user_bounds/item_bounds, DEVICE, B+1 each); block (s, w) = user range
 * (w+s) mod B x item range w is a grid of (block_steps[s*B+w+1] -
 * block_steps[s*B+w]) steps x n_slots rating slots (block_steps: DEVICE,
 * B*B+1); the triples (user_ids/item_ids/ratings, DEVICE, n_positions =
 * block_steps[B*B] * n_slots each) are stored in plan order, an idle slot
 * holding user id -1.  n_slots must equal mf_strata_slots(n_factors, dtype).
 * Stratum strata_seq[t] (HOST, n_seq entries) is one launch of B
 * workgroups; workgroup w stages item range w (rows + biases) and the bias
 * slice of its user range in LDS and applies the block's steps starting at
 * step (mix(seed, block) mod n_steps), one LDS barrier apart.
 * max_block_items / max_block_users size the LDS (mf_strata_lds_bytes must
 * not exceed mf_strata_lds_limit()).  flags: MF_FLAG_PERSISTENT runs the
 * strata of strata_seq in ONE launch: workgroup w keeps item slab w in LDS
 * throughout and, before each stratum, waits for the workgroup that last
 * applied the same user range (bounded wait; on timeout it sets an error
 * flag that mf_strata_status reports); it needs workspace (DEVICE, >=
 * mf_strata_workspace_bytes(n_blocks, n_seq) bytes, zero-initialised once by
 * the caller -- and zeroed WHOLE again after a reported failure, since the
 * position counters in it grow across launches) and is used only when
 * n_seq <= 256 and all n_blocks workgroups fit on the device at once, else
 * the call falls back to one launch per stratum.  The result
 * is the same sequential order either way.  kernel_ms (HOST, optional):
 * elapsed ms of the whole call and the launch count (synchronises).
 *
 * User-range classes (flags bits 24..27 = C - 1, a plan from
 * mf_strata_plan_build_classes): C*B user ranges, B item ranges, C*B strata;
 * block (s, w) = user range (s + C*w) mod C*B x item range w, so stratum s
 * touches the user ranges of class s mod C only.  The persistent kernel
 * then needs strata_seq to cycle through the classes (seq[t] mod C ==
 * seq[t mod C] mod C, the first C entries of distinct classes): a user range
 * used at position t was last used at t - C, so every hand-off has C - 1
 * whole blocks of slack (no waiting on the chain's jitter); any other order
 * runs as one launch per stratum.  n_seq may then be up to 1024.
 */
int mf_sgd_epoch_strata(const int32_t* user_ids, const int32_t* item_ids,
                        const void* ratings, int64_t n_positions, int32_t n_blocks,
                        const int32_t* user_bounds, const int32_t* item_bounds,
                        const int64_t* block_steps, int32_t n_slots,
                        int32_t max_block_items, int32_t max_block_users,
                        const int32_t* strata_seq, int32_t n_seq, uint32_t seed,
                        double global_mean, void* user_biases, void* item_biases,
                        void* user_features, void* item_features, int32_t n_users,
                        int32_t n_items, int32_t n_factors, int32_t kernel, int32_t dtype,
                        double gamma, double lr, double reg, double min_rating,
                        double max_rating, int32_t update_user_params,
                        int32_t update_item_params, int32_t flags, void* workspace,
                        size_t workspace_bytes, void* stream, double* kernel_ms);
/*
 * The same epoch in DELTA-OUT form, for user-sharded data parallelism (every
 * rank holds a replica of the item rows and biases; no
 * counterpart in the single-process reference): item_features / item_biases
 * are left at their values before the call, and item_delta (DEVICE, n_items
 * x n_factors) / item_bias_delta (DEVICE, n_items; unused by rbf) receive
 * the local update (value after the epoch - value before).  The caller
 * all-reduces the deltas and adds them damped with mf_replica_apply, scale =
 * min(1/2, 2/world) (distributed.default_delta_scale: the plain sum diverges
 * at N >= 4 on C3).  This is the "delta" exchange; the default "rotate"
 * exchange needs no delta form (ranks pass item ranges instead, each applied
 * in place by mf_sgd_epoch_strata on its rows of Q / b_i).
 * The persistent kernel writes the delta where it would write the slab back;
 * the per-stratum fallback keeps the start values in the delta buffers and
 * swaps at the end.  User rows and biases are updated in place as usual.
 */
int mf_sgd_epoch_strata_delta(const int32_t* user_ids, const int32_t* item_ids,
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
                              void* item_delta, void* item_bias_delta, void* stream,
                              double* kernel_ms);
size_t mf_strata_workspace_bytes(int32_t n_blocks, int32_t n_seq);
/* Synchronises `stream` and reports whether a persistent strata sweep using
 * `workspace` gave up waiting (MF_ERR_HIP) since the workspace was zeroed. */
int mf_strata_status(const void* workspace, int32_t n_blocks, void* stream);
size_t mf_strata_lds_bytes(int32_t max_block_items, int32_t max_block_users,
                           int32_t n_factors, int32_t dtype);
int32_t mf_strata_lds_limit(void);
/* Diagnostic (tools/strata_probe.py): when `probe` (DEVICE, 4 * n_seq * B
 * int64) is set, the persistent strata kernel records s_memrealtime stamps
 * (100 MHz) per (position t, workgroup w) at [(t*B + w)*4 + q]: q = 0 wait
 * start, 1 wait end, 2 block end, 3 signal.  NULL turns it off (default). */
int mf_strata_set_probe(int64_t* probe);
/* Test hook: the next n_launches persistent strata launches of this process
 * start with their error word set, as if a neighbour wait had timed out, so
 * callers can exercise their recovery (KernelMF.fit / distributed.fit_sharded
 * replay the epochs as per-stratum launches).  0 turns it off. */
int mf_strata_inject_fail(int32_t n_launches);
/* Rating slots per step of the strata kernel for (n_factors, dtype); -1 on
 * invalid arguments. */
int32_t mf_strata_slots(int32_t n_factors, int32_t dtype);
/* The same for a workgroup of `waves` waves: 16 (the default) or, FP32 with
 * n_factors <= 64 or FP64 with n_factors <= 64, 8 -- a plan built with that
 * many slots runs the
 * 8-wave kernels (blocks whose step count is set by the item degree, not by
 * the slot count); 4 = the narrow form of the 8-wave plan (same slot count,
 * run with MF_FLAG_NARROW; FP32, n_factors a multiple of 4 up to 32); -1
 * where the layout has no such kernels. */
int32_t mf_strata_slots_waves(int32_t n_factors, int32_t dtype, int32_t waves);

/*
 * Sum of squared training errors, sum_j (r_j - pred_j)^2, accumulated in
 * FP64 -- replaces `_calculate_rmse` (kernel_matrix_factorization.py:240-317;
 * rmse = sqrt(sse / n_ratings), :315).  The sum is written to the DEVICE
 * double *sse_out (no host sync).  `workspace` is a device buffer of at
 * least mf_sse_workspace_bytes(n_ratings) bytes.  Deterministic: the same
 * inputs give the same bits.
 * slice_offsets (HOST, nullable, n_slices + 1 <= 129 entries): the ratings
 * are ordered by mf_sched_slices; slice x is walked by the workgroups
 * b % n_slices == x (XCD-local Q slices).  NULL = one slice.  n_slices > 8
 * and a multiple of 8 (mf_sched_tiles): the grid is cut into n_slices / 8
 * consecutive parts in dispatch order and part p walks slices 8 p .. 8 p + 7,
 * one per XCD.  (Placement only changes speed; 8 slices measured fastest.)
 * n_users / n_items: rows of user_features / item_features (every id must
 * be below them).
 */
size_t mf_sse_workspace_bytes(int64_t n_ratings);
int mf_sse(const int32_t* user_ids, const int32_t* item_ids,
           const void* ratings, int64_t n_ratings, double global_mean,
           const void* user_biases, const void* item_biases,
           const void* user_features, const void* item_features,
           int32_t n_users, int32_t n_items,
           int32_t n_factors, int32_t kernel, int32_t dtype, double gamma,
           double min_rating, double max_rating,
           const int64_t* slice_offsets, int32_t n_slices, void* workspace,
           double* sse_out, void* stream);
/* mf_sse with its grid capped at max_blocks workgroups of 256 threads (0 = no
 * cap; at least n_slices): the pass then leaves CUs free for a kernel running
 * beside it on another stream (the rotation schedule runs epoch e's RMSE
 * beside epoch e+1's sub-epochs).  The same sum up to
 * FP64 rounding (another grouping of the per-workgroup partial sums). */
int mf_sse_capped(const int32_t* user_ids, const int32_t* item_ids,
                  const void* ratings, int64_t n_ratings, double global_mean,
                  const void* user_biases, const void* item_biases,
                  const void* user_features, const void* item_features,
                  int32_t n_users, int32_t n_items,
                  int32_t n_factors, int32_t kernel, int32_t dtype, double gamma,
                  double min_rating, double max_rating,
                  const int64_t* slice_offsets, int32_t n_slices, void* workspace,
                  int32_t max_blocks, double* sse_out, void* stream);

/*
 * The same sum with the ITEM rows stationary in LDS (k_sse_slab; DESIGN.md
 * section 5, "Item-stationary RMSE pass").  The ratings are ordered by (item
 * group, user), users ascending: item group g of n_groups holds the items i
 * with i * n_groups / n_items == g (mf_sched_tiles(1, n_groups)'s slices).
 * group_tab (DEVICE, n_groups x (n_windows + 1) int64): the first rating of
 * group g whose user is >= user boundary w of n_windows user super-windows
 * (any ascending boundaries; entry n_windows is the group's end).  One
 * workgroup per group keeps the group's item rows (items_per_group rows of
 * row_stride >= n_factors values) and biases in LDS; one launch per phase of
 * min(CUs, max_blocks or all, n_groups) groups and per window, on `stream`.
 * Every rating's error has mf_sse's bits; the FP64 sum is taken in another,
 * fixed order (deterministic).  user_features must be below 4 GiB.
 * attrs_out (nullable, int32[3]): no launch, the kernel as {registers per
 * thread, waves per workgroup, LDS bytes}.
 *
 * mf_sse_slab_plan (host arithmetic only): the smallest n_groups that is a
 * multiple of n_workgroups and whose largest group fits lds_budget bytes
 * (<= 0: all of a CU's LDS the kernel may use), rows padded by pad_values
 * (<= 0: none).  Returns 1 and plan_out = {items_per_group, n_groups, phases,
 * LDS bytes, row_stride}, or 0 where not even one row fits.
 */
size_t mf_sse_slab_workspace_bytes(int32_t n_groups);
int mf_sse_slab_plan(int32_t n_items, int32_t n_factors, int32_t dtype, int32_t n_workgroups,
                     int32_t lds_budget, int32_t pad_values, int32_t* plan_out);
int mf_sse_slab(const int32_t* user_ids, const int32_t* item_ids, const void* ratings,
                int64_t n_ratings, double global_mean, const void* user_biases,
                const void* item_biases, const void* user_features,
                const void* item_features, int32_t n_users, int32_t n_items,
                int32_t n_factors, int32_t kernel, int32_t dtype, double gamma,
                double min_rating, double max_rating, const int64_t* group_tab,
                int32_t n_groups, int32_t n_windows, int32_t items_per_group,
                int32_t row_stride, void* workspace, int32_t max_blocks, double* sse_out,
                void* stream, int32_t* attrs_out);

/*
 * The RMSE pass of epoch e beside the persistent sweep of epoch e + 1
 * (off unless the engine is asked, MF_SSE_BESIDE=1).
 *
 * A handle (mf_beside_create / mf_beside_destroy) owns a flag word in signal
 * memory and an arrival counter.  mf_sgd_epoch_strata_ticket is
 * mf_sgd_epoch_strata whose persistent launch carries `ticket` (>= 1, growing
 * from call to call on one handle): every workgroup counts itself in when it
 * starts, and the last of the launch's B stores the ticket to the flag --
 * from then on the whole grid is resident.  Nothing in the sweep waits on
 * either word; its order and every result bit are those of
 * mf_sgd_epoch_strata.  Behind whatever the call launched (persistent, one
 * launch per stratum, nothing after an error) it enqueues a
 * hipStreamWriteValue32 of the same ticket on `stream`: the backstop.
 * `beside` NULL: plain mf_sgd_epoch_strata.  kernel_attrs (nullable, int32[3],
 * with MF_FLAG_PREPARE): the persistent kernel the plan runs as {registers per
 * thread, waves per workgroup, LDS bytes}, zeros if it runs per stratum.
 *
 * mf_sse_beside, called after that launch, makes `stream` (a side stream)
 * wait until the flag is >= ticket (hipStreamWaitValue32) and then runs
 * mf_sse_capped there with one workgroup per compute unit.  The wait can only
 * be for something already enqueued; at worst the pass starts when the sweep
 * ends.  kernel_attrs non-NULL: no wait and no launch, the pass kernel's
 * attributes as above (`beside` may be NULL).
 *
 * mf_beside_fit (host arithmetic only): 1 if exactly one workgroup of the
 * pass fits on a compute unit beside one resident sweep workgroup and a second
 * does not -- registers per SIMD (allocated per wave in granules of 8, a
 * workgroup's waves dealt evenly over cu_simds SIMDs of simd_regs registers)
 * and LDS (cu_lds bytes); else 0.  mf_beside_supported: 1 if the current
 * device can hipStreamWaitValue32.
 */
int mf_beside_supported(void);
int mf_beside_create(void** handle);
void mf_beside_destroy(void* handle);
int mf_beside_fit(int32_t sweep_regs, int32_t sweep_waves, int32_t sweep_lds,
                  int32_t pass_regs, int32_t pass_waves, int32_t pass_lds,
                  int32_t simd_regs, int32_t cu_simds, int32_t cu_lds);
int mf_sgd_epoch_strata_ticket(
    const int32_t* user_ids, const int32_t* item_ids, const void* ratings, int64_t n_positions,
    int32_t n_blocks, const int32_t* user_bounds, const int32_t* item_bounds,
    const int64_t* block_steps, int32_t n_slots, int32_t max_block_items,
    int32_t max_block_users, const int32_t* strata_seq, int32_t n_seq, uint32_t seed,
    double global_mean, void* user_biases, void* item_biases, void* user_features,
    void* item_features, int32_t n_users, int32_t n_items, int32_t n_factors, int32_t kernel,
    int32_t dtype, double gamma, double lr, double reg, double min_rating, double max_rating,
    int32_t update_user_params, int32_t update_item_params, int32_t flags, void* workspace,
    size_t workspace_bytes, void* beside, int32_t ticket, int32_t* kernel_attrs, void* stream,
    double* kernel_ms);
int mf_sse_beside(void* beside, int32_t ticket, const int32_t* user_ids,
                  const int32_t* item_ids, const void* ratings, int64_t n_ratings,
                  double global_mean, const void* user_biases, const void* item_biases,
                  const void* user_features, const void* item_features, int32_t n_users,
                  int32_t n_items, int32_t n_factors, int32_t kernel, int32_t dtype,
                  double gamma, double min_rating, double max_rating,
                  const int64_t* slice_offsets, int32_t n_slices, void* workspace,
                  double* sse_out, void* stream, int32_t* kernel_attrs);
/* Up to MF_PERMUTE_MAX_JOBS device arrays copied in one launch (the parameter
 * snapshot of the overlapped RMSE pass): n_bytes[j] a multiple of 4, arrays
 * 16-byte aligned; dst / src / n_bytes are HOST arrays of n_jobs. */
int mf_copy_arrays(int32_t n_jobs, void* const* dst, const void* const* src,
                   const int64_t* n_bytes, void* stream);

/*
 * Predictions for (user, item) pairs -- replaces `_predict`
 * (kernel_matrix_factorization.py:448-541).  An id of -1 is unknown: zero
 * bias and an all-zero factor vector (:487-499).  Clipped to
 * [min_rating, max_rating] when bound_ratings (:532-536).  `out` is a device
 * array of n_pairs values of `dtype`.
 */
int mf_predict(const int32_t* user_ids, const int32_t* item_ids,
               int64_t n_pairs, double global_mean, const void* user_biases,
               const void* item_biases, const void* user_features,
               const void* item_features, int32_t n_factors, int32_t kernel,
               int32_t dtype, double gamma, double min_rating,
               double max_rating, int32_t bound_ratings, void* out,
               void* stream);

/*
 * Top-`amount` items for each of n_query users (scores = unbounded
 * prediction of every item, as recommend() scores them,
 * recommender_base.py:245-260).  Exclusions (recommend's items_known,
 * :245-250) as a DEVICE CSR list, both nullable: the items
 * exclude_items[exclude_ptr[q] .. exclude_ptr[q+1]) (int32, each user's list
 * SORTED ASCENDING -- the kernels binary-search it; ids outside [0, n_items)
 * ignored) are skipped for query q.  An unsorted list makes the result
 * undefined (items may come back although listed).  Ties are broken by
 * the lower item id (the order a stable sort_values gives; the reference's
 * default quicksort leaves tie order unspecified, :259).  out_items (int32) /
 * out_scores (dtype): device, n_query * amount.  Rows with fewer than
 * `amount` candidates are padded with id -1.  The workspace grows with
 * n_query * n_items: callers chunk the users.
 * workspace: device, >= mf_topk_workspace_bytes(n_query, n_items, amount).
 */
size_t mf_topk_workspace_bytes(int32_t n_query, int32_t n_items,
                               int32_t amount);
int mf_topk(const int32_t* query_users, int32_t n_query, double global_mean,
            const void* user_biases, const void* item_biases,
            const void* user_features, const void* item_features,
            int32_t n_items, int32_t n_factors, int32_t kernel, int32_t dtype,
            double gamma, double min_rating, double max_rating,
            const int64_t* exclude_ptr, const int32_t* exclude_items,
            int32_t amount, void* workspace,
            int32_t* out_items, void* out_scores, void* stream);

/*
 * The same top-k through an MFMA filter (linear kernel, float32, n_factors a
 * multiple of 4 in [4, 64], 1 <= amount <= 64: mf_topk_mm_supported): scores
 * of 64-user x 32-item tiles on v_mfma_f32_32x32x2_f32 (another summation
 * order than predict) only select candidates -- every item whose exact score
 * can reach the top `amount` within a per-user error bound -- which are then
 * rescored with predict's arithmetic and ranked exactly as mf_topk ranks
 * them.  *overflow (device int32, the caller zeroes it) is OR-ed with 1 when
 * a candidate band outgrew its list (masses of near-equal scores): the
 * results are then not guaranteed and the caller re-runs mf_topk.  Items
 * whose score is NaN are never candidates here (mf_topk ranks them last).
 * Exclusion lists as for mf_topk: each user's list sorted ascending.
 * workspace: device, >= mf_topk_mm_workspace_bytes(n_query, n_items).
 */
int32_t mf_topk_mm_supported(int32_t n_factors, int32_t kernel, int32_t dtype,
                             int32_t amount);
size_t mf_topk_mm_workspace_bytes(int32_t n_query, int32_t n_items);
int mf_topk_mm(const int32_t* query_users, int32_t n_query, double global_mean,
               const void* user_biases, const void* item_biases,
               const void* user_features, const void* item_features,
               int32_t n_items, int32_t n_factors, int32_t kernel, int32_t dtype,
               const int64_t* exclude_ptr, const int32_t* exclude_items,
               int32_t amount, void* workspace, int32_t* out_items,
               void* out_scores, int32_t* overflow, void* stream);

/*
 * Exact rank of held-out items: for each of n_query users, the 0-based
 * position of each of its target items among the user's candidate items in
 * mf_topk's order -- out_rank[t] = number of candidates that come before
 * target t.  Every top-k metric (precision, recall, NDCG, MAP, MRR at any k)
 * and AUC is a function of these ranks and of out_candidates, so one pass
 * serves them all and `amount` has no cap.
 * Candidates of query q: the items 0..n_items-1 not in q's exclusion list
 * (same contract as mf_topk: device CSR, both nullable, each list SORTED
 * ASCENDING, ids outside [0, n_items) ignored; duplicates count once).
 * out_candidates[q] (device int32, n_query) = their number.
 * Scores: the unbounded prediction, bit for bit mf_predict(bound_ratings=0)
 * (a query user of -1: zero row, zero bias).  Order: score descending, then
 * item id ascending; NaN below every number, all NaNs tie.
 * Targets: DEVICE CSR target_items[target_ptr[q] .. target_ptr[q+1]) (int32;
 * any order, repeats allowed, any number per user); out_rank (device int32)
 * and the workspace are indexed like target_items.  A target outside
 * [0, n_items), or excluded for its query, gets rank -1.
 * Counting is integer only (compares, integer adds and atomics), so equal
 * inputs give equal outputs whatever the launch geometry; nothing of size
 * n_query * n_items is written.  n_query == 0 returns MF_OK; dtype, kernel
 * and n_factors (mf_predict's range) are validated before any device work.
 * workspace: device, >= mf_rank_workspace_bytes(n_query, n_targets, n_items)
 * with n_targets = target_ptr[n_query].
 */
size_t mf_rank_workspace_bytes(int32_t n_query, int64_t n_targets,
                               int32_t n_items);
int mf_rank(const int32_t* query_users, int32_t n_query, double global_mean,
            const void* user_biases, const void* item_biases,
            const void* user_features, const void* item_features,
            int32_t n_items, int32_t n_factors, int32_t kernel, int32_t dtype,
            double gamma, double min_rating, double max_rating,
            const int64_t* exclude_ptr, const int32_t* exclude_items,
            const int64_t* target_ptr, const int32_t* target_items,
            void* workspace, int32_t* out_rank, int32_t* out_candidates,
            void* stream);

/* ---------------- BaselineModel (bias-only), baseline_model.py ---------- */

/* One bias-SGD epoch over a conflict-free batch schedule: replaces one epoch
 * of baseline_model.py `_sgd` (:250-266).  Same schedule contract as
 * mf_sgd_epoch. */
int mf_bias_sgd_epoch(const int32_t* user_ids, const int32_t* item_ids,
                      const void* ratings, int64_t n_ratings,
                      const int32_t* order, const int64_t* batch_offsets,
                      int32_t n_batches, const int32_t* batch_seq,
                      int32_t n_seq,
                      double global_mean, void* user_biases,
                      void* item_biases, int32_t dtype, double lr, double reg,
                      int32_t update_user_params, int32_t update_item_params,
                      void* stream);

/* Bias-model SSE, replaces baseline_model.py `_calculate_rmse` (:183-212). */
int mf_bias_sse(const int32_t* user_ids, const int32_t* item_ids,
                const void* ratings, int64_t n_ratings, double global_mean,
                const void* user_biases, const void* item_biases,
                int32_t dtype, void* workspace, double* sse_out, void* stream);

/*
 * One alternating-least-squares epoch of the bias model: replaces one epoch
 * of baseline_model.py `_als` (:326-348).  Sums are taken per id in the
 * reference's order through CSR lists:
 *   user_ptr (n_users+1) / user_list: rating indices of each user, ascending
 *   item_ptr (n_items+1) / item_list: rating indices of each item, ascending
 * (all device, int64 ptr / int32 list), so results are bit-identical to the
 * sequential reference loop.  Counts are the list lengths (:317-323).
 */
int mf_bias_als_epoch(const int32_t* user_ids, const int32_t* item_ids,
                      const void* ratings, double global_mean,
                      void* user_biases, void* item_biases, int32_t n_users,
                      int32_t n_items, const int64_t* user_ptr,
                      const int32_t* user_list, const int64_t* item_ptr,
                      const int32_t* item_list, int32_t dtype, double reg,
                      void* stream);

/* Bias-model prediction, replaces baseline_model.py `_predict` (:365-417). */
int mf_bias_predict(const int32_t* user_ids, const int32_t* item_ids,
                    int64_t n_pairs, double global_mean,
                    const void* user_biases, const void* item_biases,
                    int32_t dtype, double min_rating, double max_rating,
                    int32_t bound_ratings, void* out, void* stream);

/* ---------------- factor-model ALS (BASELINE config 5) ------------------ */

/*
 * One half-sweep of alternating least squares for the factor model: solves,
 * for every entity e (users with the item side fixed, or items with the user
 * side fixed), the regularised normal equations of its factor row and bias
 *     (sum_n y_n y_n^T + reg I) [w_e; b_e] = sum_n t_n y_n,
 *     y_n = [other_features[o_n]; 1],  t_n = r_n - global_mean - other_biases[o_n]
 * No reference counterpart: it extends the bias-only ALS of
 * baseline_model.py:283-362 (`_als`, whose per-entity update
 * (reg + n_e) b_e = sum t_n, :328-337, is the k = 0 case) to the latent
 * factors of KernelMF's linear kernel.
 *   entity_ptr      DEVICE, n_entities + 1 (int64): CSR offsets
 *   other_ids       DEVICE, the other side's id per rating, CSR order
 *   ratings         DEVICE, float, CSR order
 *   other_biases / other_features   DEVICE, float, (n_other) / (n_other, k)
 *   biases / features               DEVICE, float, written: (n_entities) /
 *                                   (n_entities, k)
 * Entities without ratings keep their parameters (update_users re-solves
 * only the users present in its data).  The Gramian runs on f32-input MFMA
 * (v_mfma_f32_32x32x2_f32), the solve is an LDS elimination in f32.  dtype must be MF_F32; 1 <= n_factors <=
 * mf_als_max_factors().
 */
int mf_als_sweep(const int64_t* entity_ptr, const int32_t* other_ids,
                 const void* ratings, int32_t n_entities, double global_mean,
                 const void* other_biases, const void* other_features,
                 void* biases, void* features, int32_t n_factors, int32_t dtype,
                 double reg, void* stream);
int32_t mf_als_max_factors(void);
/* Profiling probe: mf_als_sweep that also writes 4 wall-clock stamps
 * (s_memrealtime, 100 MHz) per entity to probe[4 * n_entities] (DEVICE):
 * start, Gramian done, elimination done, end (entities without ratings:
 * untouched). */
int mf_als_sweep_probe(const int64_t* entity_ptr, const int32_t* other_ids,
                       const void* ratings, int32_t n_entities, double global_mean,
                       const void* other_biases, const void* other_features,
                       void* biases, void* features, int32_t n_factors, int32_t dtype,
                       double reg, void* stream, int64_t* probe);

/* ---------------- implicit-feedback ALS ---------------------------------- */

/*
 * Confidence-weighted ALS over ALL entity x other pairs (Hu, Koren & Volinsky
 * 2008; no reference counterpart).  An observation n of entity e has strength
 * r_n >= 0, confidence 1 + alpha r_n and preference [r_n > 0]; every pair
 * that is not observed has confidence 1 and preference 0.  No biases, no
 * global mean.  One half-sweep solves, for every entity e,
 *     (G + sum_n alpha r_n z_n z_n^T + reg I) x_e = sum_{n: r_n > 0} (1 + alpha r_n) z_n,
 *     z_n = other_features[o_n],  G = other_features^T other_features (all rows)
 * with the sums over e's observed list.
 *
 * mf_gramian: gram = features^T features, (k, k) row-major float, both
 * triangles, of a row-major (n_rows, k) matrix.  f32-input MFMA
 * (v_mfma_f32_32x32x2_f32) per slab of rows, the slabs summed in a fixed order
 * in FP64: no atomics, the same input gives the same bits.  n_rows == 0 writes
 * zeros.
 *   features        DEVICE, float, (n_rows, k)
 *   workspace       DEVICE, mf_gramian_workspace_bytes(n_rows, k) bytes
 *                   (0 for n_rows == 0 or an invalid n_factors)
 *   gram            DEVICE, float, k * k, written
 *
 * mf_ials_sweep: one half-sweep.
 *   entity_ptr      DEVICE, n_entities + 1 (int64): CSR offsets
 *   other_ids       DEVICE, the other side's id per observation, CSR order
 *   strengths       DEVICE, float, CSR order, >= 0
 *   other_features  DEVICE, float, (n_other, k)
 *   gram            DEVICE, float, k * k: mf_gramian(other_features)
 *   features        DEVICE, float, written: (n_entities, k)
 * Entities with an empty list keep their row (update_users re-solves only the
 * users present in its data); an entity whose strengths are all 0 gets the
 * zero vector.  The weighted Gramian runs on f32-input MFMA, the solve is an
 * LDS elimination in f32 (the matrix is SPD: alpha >= 0, reg > 0).
 *
 * dtype must be MF_F32; 1 <= n_factors <= mf_als_max_factors(); alpha finite
 * and >= 0; reg finite and > 0; counts >= 0 -- else MF_ERR_INVALID, before any
 * device work, with the argument's name in mf_last_error().  n_entities == 0
 * returns MF_OK.
 *
 * mf_ials_sweep_cg: the same half-sweep with the per-entity system solved
 * inexactly by conjugate gradients (Takacs, Pilaszy & Tikk 2011), warm-started
 * from the entity's current row: arguments as mf_ials_sweep, except that
 * `features` is read (the start) and written, plus
 *   cg_steps        number of CG steps per entity, 1..1024
 * With A and b the matrix and right-hand side above and x the current row:
 *     res = b - A x;  p = res;  rs = res . res
 *     repeat cg_steps times:
 *         if not (rs > 1e-30): stop
 *         Ap = A p;  a = rs / (p . Ap)
 *         x += a p;  res -= a Ap;  rs' = res . res
 *         p = res + (rs' / rs) p;  rs = rs'
 * A is assembled once per entity (f32-input MFMA, into LDS), so the list rows
 * are read once whatever cg_steps; a step is O(k^2).  Entities with an empty
 * list keep their row bit for bit.  An entity whose strengths are all 0 has
 * b = 0 and gets the CG iterate towards 0 from its current row, NOT exactly
 * the zero vector (the one visible difference from mf_ials_sweep).  No atomics:
 * the same input gives the same bits.  Validation as mf_ials_sweep, plus
 * cg_steps in [1, 1024].
 */
size_t mf_gramian_workspace_bytes(int64_t n_rows, int32_t n_factors);
int mf_gramian(const void* features, int64_t n_rows, int32_t n_factors, int32_t dtype,
               void* workspace, void* gram /* k*k, row-major */, void* stream);
int mf_ials_sweep(const int64_t* entity_ptr, const int32_t* other_ids, const void* strengths,
                  int32_t n_entities, const void* other_features, const void* gram,
                  void* features, int32_t n_factors, int32_t dtype,
                  double alpha, double reg, void* stream);
int mf_ials_sweep_cg(const int64_t* entity_ptr, const int32_t* other_ids, const void* strengths,
                     int32_t n_entities, const void* other_features, const void* gram,
                     void* features /* read (warm start) and written */, int32_t n_factors,
                     int32_t dtype, double alpha, double reg, int32_t cg_steps, void* stream);

/* ---------------- neighbourhood models ----------------------------------- */

/*
 * ItemItemCF / UserUserCF (collaborative_filtering.py).  One model with the
 * roles swapped: the ENTITIES are the items (ItemItemCF) or the users
 * (UserUserCF), the OTHERS are the other side; n = n_others.  With r_ao the
 * rating of entity a by other o (0 where there is none) and all sums over the
 * stored entries:
 *     m_a    = (sum_o r_ao) / n                      (zeros included)
 *     w_a    = sqrt(max(sum_o r_ao^2 - n m_a^2, 0))
 *     S[a,b] = (sum_o r_ao r_bo - n m_a m_b) / (w_a w_b),  0 where w_a w_b = 0
 * Ratings are DEVICE CSR in both orientations: int64 offsets, int32 ids, float
 * ratings (dtype must be MF_F32).
 *
 * mf_cf_stats: replaces the pivot's row / column mean
 * (collaborative_filtering.py:62-73, :241-252) and the row norms that
 * sklearn's cosine_similarity takes of the centred matrix (:87-89, :266-268).
 *   entity_ptr      DEVICE, n_entities + 1 (int64): CSR offsets by entity
 *   ratings         DEVICE, float, in that CSR's order
 *   mean, norm      DEVICE, double, n_entities each, written
 * Each entity's list is summed in list order, in FP64.
 *
 * mf_cf_similarity: replaces `_compute_user_similarity` /
 * `_compute_item_similarity` (collaborative_filtering.py:80-96, :259-274),
 * where 'cosine' and 'pearson' are the same computation.
 *   entity_ptr, other_ids, ratings          DEVICE: the entity-major lists
 *   other_ptr, entity_ids, other_ratings    DEVICE: the other-major lists, every
 *                   list sorted by entity id ascending
 *   mean, norm      DEVICE, double: mf_cf_stats' output
 *   pass_cols       columns of a row held in LDS at once, 0 = automatic
 *                   (2048), at most 4096; mf_cf_pass_cols() gives the value
 *                   used (min(that, n_entities)).  A row is done in
 *                   ceil(n_entities / pass_cols) column ranges, each of which
 *                   binary-searches the longer other-lists for its range; the
 *                   result does not depend on pass_cols, bit for bit
 *   similarity      DEVICE, float, n_entities x n_entities row-major; EVERY
 *                   element is written (no zeroing by the caller)
 * One wave owns (entity a, column range): FP64 accumulators in LDS, a's others
 * applied in a's list order, sum_o deg(o)^2 multiply-adds in all, FP64
 * epilogue.  No atomics.  With the entity-major lists sorted by other id
 * ascending, S[a,b] and S[b,a] add the same products in the same order: the
 * matrix is bitwise symmetric.
 *
 * mf_cf_predict: replaces `_predict_rating` and predict's loop
 * (collaborative_filtering.py:98-190, :276-368).  For pair p with target
 * entity e = entity_ids[p] and other o = other_ids[p]:
 *   either id outside its range (-1 = unknown): global_mean;
 *   candidates: the entities b != e of o's list with r_bo > 0; with more than
 *     n_neighbors of them the n_neighbors first under (S[e,b] descending,
 *     b ascending) are kept -- an exact radix select, any list length; the
 *     keys of lists of up to 1024 entries stay in LDS, longer lists re-read
 *     S[e,.] on each of the select's passes;
 *   out[p] = m_e + sum S[e,b] (r_bo - m_b) / sum |S[e,b]| over the kept, in
 *     FP64 in a fixed order; m_e with no candidate or a zero denominator;
 *   clipped to [min_rating, max_rating] when bound_ratings.
 * Differences from the reference: e is never its own neighbour (the
 * reference's exclusion indexes the compressed list with the uncompressed id),
 * and ties at the cut go to the lower id (argsort leaves them unspecified).
 *   other_ptr, list_entity_ids, list_ratings   DEVICE: the other-major lists
 *   similarity, mean                            DEVICE: as above
 *   out             DEVICE, double, n_pairs, written
 * n_pairs is at most 2^25 a call (one workgroup per pair).
 *
 * All three: dtype must be MF_F32, counts >= 0, n_neighbors >= 1, pass_cols in
 * [0, 4096], no NULL for an array that is read or written -- else
 * MF_ERR_INVALID, before any device work, with the argument's name in
 * mf_last_error().  n_entities == 0 (n_pairs == 0) returns MF_OK.
 */
int mf_cf_stats(const int64_t* entity_ptr, const void* ratings, int32_t n_entities,
                int32_t n_others, int32_t dtype, double* mean, double* norm, void* stream);
int32_t mf_cf_pass_cols(int32_t n_entities, int32_t pass_cols);
int mf_cf_similarity(const int64_t* entity_ptr, const int32_t* other_ids, const void* ratings,
                     const int64_t* other_ptr, const int32_t* entity_ids,
                     const void* other_ratings, int32_t n_entities, int32_t n_others,
                     int32_t dtype, const double* mean, const double* norm, int32_t pass_cols,
                     void* similarity, void* stream);
int mf_cf_predict(const int32_t* entity_ids, const int32_t* other_ids, int64_t n_pairs,
                  const int64_t* other_ptr, const int32_t* list_entity_ids,
                  const void* list_ratings, const void* similarity, const double* mean,
                  int32_t n_entities, int32_t n_others, int32_t dtype, int32_t n_neighbors,
                  double global_mean, double min_rating, double max_rating,
                  int32_t bound_ratings, double* out, void* stream);

/*
 * One query against EVERY target: scores, top-k and exact ranks (the
 * neighbourhood models' recommend_batch / rank_items / evaluate_topk).
 *   query_side      MF_CF_QUERY_OTHER   the queries are OTHER ids, the targets
 *                     all n_entities entities (ItemItemCF: a user against
 *                     every item)
 *                   MF_CF_QUERY_ENTITY  the queries are ENTITY ids, the targets
 *                     all n_others others (UserUserCF: a user against every
 *                     item)
 *   query_ids       DEVICE, int32, n_query; an id outside its range (-1 =
 *                   unknown) scores every target at global_mean
 *   other_ptr .. global_mean               as for mf_cf_predict
 *   targets_per_block  targets a workgroup walks, 0 = automatic (64);
 *                   mf_cf_targets_per_block() gives the value used
 *                   (min(that, n_targets)).  No result depends on it.
 * The score of query q and target t is, bit for bit, mf_cf_predict's
 * (bound_ratings = 0) for the corresponding (entity, other) pair: the same
 * candidates, order at the cut, exact select and FP64 summation order.  A
 * workgroup takes one query and a block of targets and keeps what its pairs
 * share on the chip: with MF_CF_QUERY_OTHER the query's list (ids, r > 0,
 * (double)r - mean[b]) in LDS when it has at most 1024 entries, with
 * MF_CF_QUERY_ENTITY row S[e, :] in the caches (MF_CF_ROW_LDS=1 in the
 * environment: in LDS, for up to 4096 entities).  n_query * ceil(n_targets /
 * targets per block) is at most 2^31 - 1 a call.  No floating-point atomics.
 *
 * mf_cf_scores:  out DEVICE, double, n_query x n_targets row-major, written.
 *
 * mf_cf_topk:  the scores go as order keys (mf_topk's order: score descending,
 * NaN last, then target id ascending) into `workspace`, the keys of the pairs
 * in the exclusion CSR (query q skips targets exclude_items[exclude_ptr[q] ..
 * exclude_ptr[q+1]); NULL: none; ids out of range are ignored, any order,
 * duplicates count once) are zeroed, and mf_topk's exact select writes
 *   out_items       DEVICE, int32, n_query x amount: target ids, -1 padding
 *   out_scores      DEVICE, double, n_query x amount: scores, NaN padding
 *   workspace       DEVICE, mf_cf_topk_workspace_bytes(n_query, n_targets) =
 *                   8 n_query n_targets bytes
 *   amount          in [1, 2048]
 *
 * mf_cf_rank:  the same key matrix and exclusions, then an integer count:
 *   target_ptr, target_items   DEVICE CSR: query q's targets (any order,
 *                   repeats allowed)
 *   out_rank        DEVICE, int32, one per CSR entry: the number of
 *                   non-excluded candidates that come before the target in
 *                   mf_cf_topk's order; -1 for a target out of range or
 *                   excluded
 *   out_candidates  DEVICE, int32, n_query: the non-excluded candidates
 *   workspace       DEVICE, mf_cf_rank_workspace_bytes(n_query, n_targets) =
 *                   8 n_query n_targets bytes
 * mf_rank's semantics, so utils.ranking_metrics_from_ranks applies unchanged.
 *
 * All three: dtype must be MF_F32, query_side one of the two, n_neighbors >= 1,
 * targets_per_block >= 0, amount in [1, 2048], counts >= 0, no NULL for
 * query_ids, an output, the workspace or the target CSR (nor, with
 * n_entities > 0 and n_others > 0, for other_ptr, similarity and mean) -- else
 * MF_ERR_INVALID, before any device work, with the argument's name in
 * mf_last_error().  n_query == 0 returns MF_OK.
 */
#define MF_CF_QUERY_OTHER 0
#define MF_CF_QUERY_ENTITY 1
int32_t mf_cf_targets_per_block(int32_t n_targets, int32_t targets_per_block);
int mf_cf_scores(const int32_t* query_ids, int32_t n_query, int32_t query_side,
                 const int64_t* other_ptr, const int32_t* list_entity_ids,
                 const void* list_ratings, const void* similarity, const double* mean,
                 int32_t n_entities, int32_t n_others, int32_t dtype, int32_t n_neighbors,
                 double global_mean, int32_t targets_per_block, double* out, void* stream);
size_t mf_cf_topk_workspace_bytes(int32_t n_query, int32_t n_targets);
int mf_cf_topk(const int32_t* query_ids, int32_t n_query, int32_t query_side,
               const int64_t* other_ptr, const int32_t* list_entity_ids,
               const void* list_ratings, const void* similarity, const double* mean,
               int32_t n_entities, int32_t n_others, int32_t dtype, int32_t n_neighbors,
               double global_mean, int32_t targets_per_block, const int64_t* exclude_ptr,
               const int32_t* exclude_items, int32_t amount, void* workspace,
               int32_t* out_items, double* out_scores, void* stream);
size_t mf_cf_rank_workspace_bytes(int32_t n_query, int32_t n_targets);
int mf_cf_rank(const int32_t* query_ids, int32_t n_query, int32_t query_side,
               const int64_t* other_ptr, const int32_t* list_entity_ids,
               const void* list_ratings, const void* similarity, const double* mean,
               int32_t n_entities, int32_t n_others, int32_t dtype, int32_t n_neighbors,
               double global_mean, int32_t targets_per_block, const int64_t* exclude_ptr,
               const int32_t* exclude_items, const int64_t* target_ptr,
               const int32_t* target_items, void* workspace, int32_t* out_rank,
               int32_t* out_candidates, void* stream);

/*
 * Stored neighbours: a top-M similarity in place of the dense matrix, for
 * entity counts whose n_entities^2 floats do not fit.
 *
 * The model.  With n_stored = M, the neighbour set N_M(a) of entity a is the
 * first min(M, n_entities - 1) entities b != a under the order of the
 * n_neighbors cut: S[a,b] descending with -0 tied to +0, then b ascending; S
 * is mf_cf_similarity's float32 value.  A prediction for target e and other o
 * is mf_cf_predict's with one change: the candidates are the b != e of o's
 * list with r_bo > 0 AND b in N_M(e).  An entity outside N_M(e) is no
 * candidate (not "similarity 0").  Everything else -- the cut at n_neighbors,
 * the FP64 sum and its order, m_e with no candidate or a zero denominator,
 * global_mean for an unknown id, the clipping -- is unchanged.  N_M is per row
 * and not symmetric: row e serves target e.  Hence: the stored similarities
 * are the dense S[a,b] bit for bit, and with M >= n_entities - 1 every
 * prediction, score, top-k and rank is the dense entry point's bit for bit.
 *
 * mf_cf_neighbours: builds the lists from the inputs of mf_cf_similarity.
 *   entity_ptr .. pass_cols                as for mf_cf_similarity
 *   n_stored        M, in [1, 4096]
 *   workspace       DEVICE, mf_cf_neighbours_workspace_bytes(n_entities,
 *                   n_stored) = 4 n_entities min(n_entities, 2048) bytes: one
 *                   float32 scratch row for each of the (at most 2048)
 *                   workgroups in flight -- it scales with the rows in
 *                   flight, not with n_entities^2; free after the call's work
 *   nbr_ids         DEVICE, int32, n_entities x n_stored row-major: row a
 *                   holds N_M(a) sorted by id ascending, then -1 where
 *                   n_entities - 1 < n_stored; EVERY element is written
 *   nbr_sims        DEVICE, float, same shape: S[a, nbr_ids[a, j]], 0 in the
 *                   padding; every element is written
 * A persistent one-wave workgroup takes rows a = w, w + 2048, ...: the row's
 * column ranges in sequence through mf_cf_similarity's accumulation and FP64
 * epilogue (one code path: the same values bit for bit) into its scratch row,
 * the M-th key by mf_cf_predict's exact radix select with the keys rebuilt
 * from the scratch row, then one ordered pass that emits the columns at or
 * above the cut, placed by a ballot prefix count.  A row of zero norm is all
 * zeros: its set is the M lowest ids != a.  The dense row never exists in HBM
 * outside the scratch row.  No floating-point atomics; the result depends
 * neither on pass_cols nor on the grid.
 *
 * mf_cf_predict_nbr, mf_cf_scores_nbr, mf_cf_topk_nbr, mf_cf_rank_nbr: the
 * four entry points above with (nbr_ids, nbr_sims, n_stored) -- mf_cf_neighbours'
 * output -- in place of `similarity`; every other argument, output and limit
 * as documented there.  The kernels are the same (a template parameter picks
 * the accessor): candidate b of target e is looked up by binary search in e's
 * id-ascending row, absent = not a candidate.  With MF_CF_QUERY_ENTITY the
 * query's row (8 n_stored bytes, at most 32 KiB) is staged in LDS; with
 * MF_CF_QUERY_OTHER the query's list is staged as before and each target's
 * row is read through L2.
 *
 * All six: the checks of their dense counterparts, and n_stored in [1, 4096],
 * no NULL for nbr_ids, nbr_sims (where `similarity` may not be NULL) or the
 * workspace -- else MF_ERR_INVALID, before any device work, with the
 * argument's name in mf_last_error().  Zero sizes return MF_OK.
 */
size_t mf_cf_neighbours_workspace_bytes(int32_t n_entities, int32_t n_stored);
int mf_cf_neighbours(const int64_t* entity_ptr, const int32_t* other_ids, const void* ratings,
                     const int64_t* other_ptr, const int32_t* entity_ids,
                     const void* other_ratings, int32_t n_entities, int32_t n_others,
                     int32_t dtype, const double* mean, const double* norm, int32_t pass_cols,
                     int32_t n_stored, void* workspace, int32_t* nbr_ids, void* nbr_sims,
                     void* stream);
int mf_cf_predict_nbr(const int32_t* entity_ids, const int32_t* other_ids, int64_t n_pairs,
                      const int64_t* other_ptr, const int32_t* list_entity_ids,
                      const void* list_ratings, const int32_t* nbr_ids, const void* nbr_sims,
                      int32_t n_stored, const double* mean, int32_t n_entities, int32_t n_others,
                      int32_t dtype, int32_t n_neighbors, double global_mean, double min_rating,
                      double max_rating, int32_t bound_ratings, double* out, void* stream);
int mf_cf_scores_nbr(const int32_t* query_ids, int32_t n_query, int32_t query_side,
                     const int64_t* other_ptr, const int32_t* list_entity_ids,
                     const void* list_ratings, const int32_t* nbr_ids, const void* nbr_sims,
                     int32_t n_stored, const double* mean, int32_t n_entities, int32_t n_others,
                     int32_t dtype, int32_t n_neighbors, double global_mean,
                     int32_t targets_per_block, double* out, void* stream);
int mf_cf_topk_nbr(const int32_t* query_ids, int32_t n_query, int32_t query_side,
                   const int64_t* other_ptr, const int32_t* list_entity_ids,
                   const void* list_ratings, const int32_t* nbr_ids, const void* nbr_sims,
                   int32_t n_stored, const double* mean, int32_t n_entities, int32_t n_others,
                   int32_t dtype, int32_t n_neighbors, double global_mean,
                   int32_t targets_per_block, const int64_t* exclude_ptr,
                   const int32_t* exclude_items, int32_t amount, void* workspace,
                   int32_t* out_items, double* out_scores, void* stream);
int mf_cf_rank_nbr(const int32_t* query_ids, int32_t n_query, int32_t query_side,
                   const int64_t* other_ptr, const int32_t* list_entity_ids,
                   const void* list_ratings, const int32_t* nbr_ids, const void* nbr_sims,
                   int32_t n_stored, const double* mean, int32_t n_entities, int32_t n_others,
                   int32_t dtype, int32_t n_neighbors, double global_mean,
                   int32_t targets_per_block, const int64_t* exclude_ptr,
                   const int32_t* exclude_items, const int64_t* target_ptr,
                   const int32_t* target_items, void* workspace, int32_t* out_rank,
                   int32_t* out_candidates, void* stream);

/* ---------------- Content-based ------------------------------------------- */

/*
 * ContentBasedRecommender (content_based.py).  F is the n_items x d FP64
 * matrix of item feature rows (row-major, a zero row for an item without
 * features), has_features[i] != 0 where item i has a row.  d is in
 * [0, mf_max_factors()] everywhere.  All three entry points validate dtype,
 * counts and d before any device work (MF_ERR_INVALID, the argument's name in
 * mf_last_error()); a zero count returns MF_OK without touching the device.
 *
 * mf_content_profiles: one profile row per user,
 *     P_u = sum_p w_p F_{i_p} / sum_p w_p     when sum_p w_p > 0,
 *           sum_p w_p F_{i_p}                 otherwise (content_based.py:131),
 * over the pairs p of the user's list whose item has features, in list order;
 * a user without such a pair gets zeros.  FP64 throughout, no atomics: the
 * same inputs give the same bits.
 *   user_ptr        DEVICE, int64[n_users + 1]: CSR offsets of the lists
 *   item_ids        DEVICE, int32: item of each pair (outside [0, n_items): skipped)
 *   weights         DEVICE, double: w of each pair (rating - min_rating)
 *   features        DEVICE, double[n_items * d]
 *   has_features    DEVICE, uint8[n_items]
 *   dtype           MF_F64
 *   profiles        DEVICE, double[n_users * d]: output
 *
 * mf_content_normalize: out[r] = fl32(rows[r] / ||rows[r]||), the norm taken
 * in FP64, a zero row where the norm is 0.  out_stride (0: d) is the row
 * stride of `out` in floats, >= d; columns d .. out_stride - 1 are zeroed.
 *   rows            DEVICE, double[n * d];  dtype MF_F64
 *   out             DEVICE, float[n * out_stride]
 *
 * mf_content_similarity: S = X X^T for the n x d float32 rows X (the cosine
 * when the rows are mf_content_normalize's), on v_mfma_f32_32x32x2_f32: each
 * entry is one f32 fmaf chain in k order.  Only the 128 x 128 tiles on or
 * above the diagonal are computed and each is written to both places:
 * S[a,b] and S[b,a] are the same bits, and a zero row gives exact zeros.
 * Nothing but S is allocated.
 *   rows            DEVICE, float[n * d];  dtype MF_F32
 *   similarity      DEVICE, float[n * n]: output
 */
int mf_content_profiles(const int64_t* user_ptr, const int32_t* item_ids, const void* weights,
                        const void* features, const uint8_t* has_features, int32_t n_users,
                        int32_t n_items, int32_t d, int32_t dtype, void* profiles, void* stream);
int mf_content_normalize(const void* rows, int64_t n, int32_t d, int32_t out_stride,
                         int32_t dtype, void* out, void* stream);
int mf_content_similarity(const void* rows, int32_t n, int32_t d, int32_t dtype,
                          void* similarity, void* stream);

/* ---------------- Hybrid: embedding retrieval, model rerank --------------- */

/*
 * HybridRecommender's second stage (hybrid.py; the reference's
 * project_template/pipeline/evaluate_hybrid.py:133-153): per query, the
 * n_cand candidates an embedding retrieval returned (index rows and their
 * float32 similarities, in retrieval order; mf_topk's output) are filtered,
 * scored by the factor model, blended and reordered.  One workgroup per query;
 * nothing of size n_query x n_rows is touched.
 *
 *  1. kept: position c is kept when 0 <= cand_rows[c] < n_rows and the row is
 *     not in the query's exclusion list (binary search; each list sorted
 *     ascending).  Kept positions stay in retrieval order; out_n_cand[q] = m,
 *     their count.  Dropping happens after the retrieval, as in the reference,
 *     so m can be below n_cand.
 *  2. model score: s_c = (float) mf_predict(query_users[q], item of the row,
 *     bound_ratings = 0), bit for bit; the item is row_item[row] (row_item
 *     null: the row itself), and a user or item that is negative (an item also
 *     when >= n_items) reads as a zero row and zero bias.  user_features
 *     null: no model, s_c = 0 (dtype, kernel and n_factors are still checked).
 *  3. min-max (evaluate_hybrid.py:72-79) of the model scores and of the
 *     similarities, each over the kept candidates: with lo / hi their min /
 *     max, every value is 0 when (double)hi - (double)lo < 1e-8, else
 *     fl32(fl32(x - lo) / fl32((double)hi - (double)lo)); a NaN among the kept
 *     values makes the whole term NaN (np.min).
 *  4. score = fl32(fl32(fl32(alpha) * a) + fl32(fl32(1.0 - alpha) * b)), a the
 *     model term and b the similarity term, 1.0 - alpha taken in double: NumPy's
 *     float32 result of alpha * a + (1.0 - alpha) * b.  A score of -0 is
 *     written as +0.
 *  5. order: score descending, then position in the retrieval order
 *     ascending, NaN last -- the STABLE order; the reference's
 *     np.argsort(-score) leaves the order of equal scores unspecified.  The
 *     first `amount` are written, the rest of each output row is padded with
 *     row -1 and NaN.
 * No float32 operation is contracted, counting and ordering are integer and
 * compare only: the same inputs give the same bytes whatever the grid.
 *
 *   query_users     DEVICE, int32[n_query]: the MODEL's internal user ids
 *   cand_rows       DEVICE, int32[n_query * n_cand]; -1 entries are skipped
 *   cand_sims       DEVICE, float[n_query * n_cand]
 *   n_cand          1 .. 2048 (mf_topk's largest amount)
 *   row_item        DEVICE, int32[n_rows], nullable
 *   user_biases .. max_rating   the model, as for mf_predict
 *   exclude_ptr / exclude_rows  DEVICE CSR of index rows per query, nullable
 *   alpha           finite
 *   amount          0 .. n_cand
 *   workspace       mf_hybrid_rerank_workspace_bytes() bytes (0: may be null)
 *   out_rows / out_scores       DEVICE, [n_query * amount]
 *   out_model / out_sims        DEVICE, nullable, same shape: s_c and the raw
 *                               similarity of each output
 *   out_n_cand      DEVICE, int32[n_query]
 * Invalid arguments (dtype, kernel, n_factors as for mf_predict; n_cand,
 * amount, a non-finite alpha, negative counts) return MF_ERR_INVALID before
 * any device work, the argument's name in mf_last_error(); n_query == 0
 * returns MF_OK.
 */
size_t mf_hybrid_rerank_workspace_bytes(int32_t n_query, int32_t n_cand);
int mf_hybrid_rerank(const int32_t* query_users, int32_t n_query, const int32_t* cand_rows,
                     const float* cand_sims, int32_t n_cand, const int32_t* row_item,
                     int32_t n_rows, double global_mean, const void* user_biases,
                     const void* item_biases, const void* user_features,
                     const void* item_features, int32_t n_items, int32_t n_factors,
                     int32_t kernel, int32_t dtype, double gamma, double min_rating,
                     double max_rating, const int64_t* exclude_ptr, const int32_t* exclude_rows,
                     double alpha, int32_t amount, void* workspace, int32_t* out_rows,
                     float* out_scores, float* out_model, float* out_sims, int32_t* out_n_cand,
                     void* stream);

/* ---------------- BPR: Bayesian personalised ranking ---------------------- */

/*
 * BPRMF (bpr_matrix_factorization.py; Rendle et al. 2009; no counterpart in the
 * reference).  The data are interaction strengths: the pairs with r > 0 are
 * the POSITIVES, an observed pair with r = 0 counts as unobserved.  The score
 * is s(u,i) = x_u . y_i + b_i -- mf_predict's linear kernel with global mean 0
 * and zero user biases.  One update takes a triple (u, i, j), i a positive of
 * u and j not; every right-hand side takes the values from before the triple:
 *     d   = y_i - y_j                       (elementwise)
 *     z   = x_u . d + (b_i - b_j)
 *     g   = 1 / (1 + exp(z))
 *     x_u = x_u + lr (g d - reg x_u)
 *     y_i = y_i + lr ( g x_u - reg y_i)     b_i = b_i + lr ( g - reg b_i)
 *     y_j = y_j + lr (-g x_u - reg y_j)     b_j = b_j + lr (-g - reg b_j)
 * (gradient ascent on ln sigmoid(z) - reg/2 (|x_u|^2 + |y_i|^2 + |y_j|^2 +
 * b_i^2 + b_j^2)).  FP64 evaluates exactly these expressions, unfused, IEEE
 * exp and division; only the k-long sum follows the lane group's fixed order.
 * FP32 uses fused multiply-adds, v_exp_f32 of z log2(e) and v_rcp_f32.
 *
 * One EPOCH has one triple per positive.  The visit order is a permutation of
 * the positives; the triple at visit position t (0-based) takes its negative
 * from a counter-based generator.  With 64-bit wrap-around arithmetic and
 *     mix(x):  x ^= x >> 30;  x *= 0xbf58476d1ce4e5b9;  x ^= x >> 27;
 *              x *= 0x94d049bb133111eb;  x ^= x >> 31        (splitmix64's finaliser)
 *     base     = mix(seed + (t + 1) * 0x9e3779b97f4a7c15)
 *     h(a)     = mix(base + (a + 1) * 0xd1b54a32d192ed03)
 *     j(a)     = ((h(a) >> 32) * n_items) >> 32               (multiply-shift)
 * the negative is the first j(a), a = 0..15, that is neither i nor in u's
 * sorted positive list (binary search); if all 16 attempts fail the triple is
 * SKIPPED: neg = -1, no update, no part in the loss.  The multiply-shift maps
 * 2^32 values onto n_items: every item has floor or ceil(2^32 / n_items)
 * preimages, a relative bias of at most n_items / 2^32 (2.4e-4 at 10^6 items).
 * The generator has no state and uses no atomics: the integers do not depend
 * on the launch geometry.  The epoch's result is the sequential sweep over the
 * kept triples in visit order.
 *
 * mf_bpr_sample: one thread per visit position.
 *   order           DEVICE, nullable, n_pos (int32): visit position -> positive
 *   pos_users/items DEVICE, n_pos: the positives
 *   user_ptr        DEVICE, n_users + 1 (int64): CSR offsets by user
 *   user_items      DEVICE, int32: each user's positive items, ascending
 *   neg_items       DEVICE, n_pos (int32), written: per visit position, -1 = skipped
 *
 * mf_bpr_epoch: mf_sgd_epoch's batch contract for triples.  The three id
 * arrays are DEVICE arrays of n_triples entries (a triple index is whatever
 * `order` holds, e.g. the visit position); batch_offsets (n_batches + 1) and
 * batch_seq (nullable) are HOST arrays; order (DEVICE, nullable) lists triple
 * indices batch by batch -- mf_sched_levels3's output.  One launch per batch;
 * no two triples of a batch may share a user, or an item in either role.
 *   item_biases, user_features, item_features   DEVICE, dtype, updated in place
 *   update_user_params / update_item_params     0: that side is read only
 *   z_out           DEVICE, dtype, one per schedule position: the triple's
 *                   pre-update z (the loss is the mean of softplus(-z), the
 *                   pairwise accuracy the mean of [z > 0])
 * A listed triple with neg = -1 makes no update and leaves its z_out entry.
 *
 * mf_bpr_max_factors(): the largest n_factors mf_bpr_epoch takes (three rows
 * per triple are held in registers; no instantiation spills, so it equals
 * mf_max_factors()).
 *
 * Both: counts >= 0, dtype MF_F32 or MF_F64, n_factors in [0,
 * mf_bpr_max_factors()], no NULL for an array that is read or written -- else
 * MF_ERR_INVALID, before any device work, with the argument's name in
 * mf_last_error().  n_pos == 0 (n_triples == 0, no batch) returns MF_OK.
 */
int32_t mf_bpr_max_factors(void);
int mf_bpr_sample(const int32_t* order, const int32_t* pos_users, const int32_t* pos_items,
                  int64_t n_pos, const int64_t* user_ptr, const int32_t* user_items,
                  int32_t n_users, int32_t n_items, uint64_t seed, int32_t* neg_items,
                  void* stream);
int mf_bpr_epoch(const int32_t* user_ids, const int32_t* item_ids, const int32_t* neg_items,
                 int64_t n_triples, const int32_t* order, const int64_t* batch_offsets,
                 int32_t n_batches, const int32_t* batch_seq, int32_t n_seq, void* item_biases,
                 void* user_features, void* item_features, int32_t n_users, int32_t n_items,
                 int32_t n_factors, int32_t dtype, double lr, double reg,
                 int32_t update_user_params, int32_t update_item_params, void* z_out,
                 void* stream);

/* ---------------- multi-GPU replica exchange ----------------------------- */

/*
 * Element-wise helper around the per-epoch all-reduce of the replicated item
 * parameters (user-sharded data parallelism, "delta" exchange, DESIGN.md
 * section 6; no
 * counterpart in the single-process reference):
 *   mode 0 (MF_DELTA_TAKE):  cur[j] = cur[j] - base[j]   (local update delta)
 *   mode 1 (MF_DELTA_APPLY): cur[j] = cur[j] + base[j]   (base + summed delta)
 * cur, base: device, n values of dtype.
 */
enum { MF_DELTA_TAKE = 0, MF_DELTA_APPLY = 1 };
int mf_replica_delta(void* cur, const void* base, int64_t n, int32_t dtype,
                     int32_t mode, void* stream);
/* cur[j] = cur[j] + scale * delta[j] (device, n values of dtype): applies
 * the all-reduced item deltas; scale = min(1/2, 2/world) is the default of
 * the delta exchange (distributed.default_delta_scale) -- the plain sum
 * (scale 1) overshoots once each rank's local epoch moves an item most of the
 * way to its local optimum (measured at C3: N = 4 and 8 diverge), plain
 * averaging (1/world) under-steps. */
int mf_replica_apply(void* cur, const void* delta, int64_t n, int32_t dtype, double scale,
                     void* stream);

/* ---------------- host-side schedulers (no GPU) -------------------------- */

/*
 * Exact-order schedule.  Given the visit order of one epoch (the row order
 * of X after `np.random.shuffle(X)`, kernel_matrix_factorization.py:371),
 * assign every rating the level 1 + max(level of the previous rating of the
 * same user, ... of the same item) and group positions by level.  Applying
 * the levels in increasing order (mf_sgd_epoch) is bit-for-bit the
 * reference's sequential sweep.  use_user / use_item drop a row family
 * from the conflict test when it is not written (update_users passes
 * use_item = 0, kernel_matrix_factorization.py:234).
 *
 *   order            host, nullable, n: visit order (rating indices)
 *   sched_out        host, n: rating indices grouped by level, each level
 *                    in visit order
 *   level_offsets    host, capacity `offsets_cap` (>= n_levels + 1)
 *   n_levels_out     host
 */
int mf_sched_levels(const int32_t* user_ids, const int32_t* item_ids,
                    int64_t n, const int64_t* order, int32_t n_users,
                    int32_t n_items, int32_t use_user, int32_t use_item,
                    int32_t* sched_out, int64_t* level_offsets,
                    int64_t offsets_cap, int32_t* n_levels_out);

/*
 * The exact-order schedule at scale (replaces the per-epoch host cost of
 * `np.random.shuffle(X)` + the sequential sweep's order,
 * kernel_matrix_factorization.py:369-425).  The visit order is cut into
 * n_chunks contiguous chunks (<= 0: min(16, cores) from 2^20 ratings, else
 * 1) levelled on as many threads, each chunk's levels placed after all of
 * the earlier chunks'.  Every level is conflict-free and every rating's
 * level is above each earlier rating of its user and item, so the levels
 * applied in order (mf_sgd_epoch) give the same bits as mf_sched_levels'
 * greedy levels -- more levels (the sum of the chunk depths), built in a
 * fraction of the time.  order: 32-bit rating indices, n < 2^31.
 * sched_out[lo_c, hi_c) holds chunk c's ratings (the chunk's own range of
 * visit positions), by level, each level in visit order.
 */
int mf_sched_levels_chunked(const int32_t* user_ids, const int32_t* item_ids,
                            int64_t n, const int32_t* order, int32_t n_users,
                            int32_t n_items, int32_t use_user, int32_t use_item,
                            int32_t n_chunks, int32_t* sched_out, int64_t* level_offsets,
                            int64_t offsets_cap, int32_t* n_levels_out);

/*
 * The exact-order schedule for BPR's (user, positive item, negative item)
 * triples (mf_bpr_epoch).  The three arrays are in VISIT order (triple t is
 * visit position t).  level(t) = 1 + max(last level of the user, of item i, of
 * item j); both item roles share one last-level table, so an item that is i in
 * one triple and j in another conflicts.  use_user / use_item as in
 * mf_sched_levels (use_item = 0: items frozen, levels by user only).  Triples
 * with neg = -1 (skipped by the sampler) get no level and are left out;
 * n_kept_out receives the number listed.  n_chunks as in
 * mf_sched_levels_chunked: 1 gives the greedy levels, more (<= 0: by size)
 * level each chunk of visit positions alone and place its levels after the
 * previous chunk's -- the same sequential sweep, more levels.  Ids outside
 * [0, n_users) x [0, n_items) x [-1, n_items), and triples with i == j, are
 * rejected (MF_ERR_INVALID).  n < 2^31.
 *   sched_out        host, n: the kept visit positions by level, each level
 *                    in visit order (n_kept entries written)
 *   level_offsets    host, capacity `offsets_cap` (>= n_levels + 1)
 */
int mf_sched_levels3(const int32_t* user_ids, const int32_t* item_ids, const int32_t* neg_ids,
                     int64_t n, int32_t n_users, int32_t n_items, int32_t use_user,
                     int32_t use_item, int32_t n_chunks, int32_t* sched_out,
                     int64_t* level_offsets, int64_t offsets_cap, int32_t* n_levels_out,
                     int64_t* n_kept_out);

/*
 * Throughput schedule.  Greedy edge colouring of the bipartite rating graph
 * (no two ratings of one colour share a user or an item), ratings visited
 * item by item.  Output: rating indices grouped by colour, each colour sorted
 * by item id (so a batch walks Q in address order), plus colour offsets.
 * Any order of colours is a valid sequential order of the ratings.
 *   colour count <= max user degree + max item degree - 1 (offsets_cap must
 *   be at least that + 1).
 */
int mf_sched_color(const int32_t* user_ids, const int32_t* item_ids,
                   int64_t n, int32_t n_users, int32_t n_items,
                   int32_t* sched_out, int64_t* color_offsets,
                   int64_t offsets_cap, int32_t* n_colors_out);

/*
 * Evaluation order for the read-only passes (mf_sse, mf_sse_sliced).  Items
 * are cut into n_slices contiguous id ranges (n_slices = 8: one per XCD, so
 * one slice of Q fits an XCD's 4 MiB L2); ratings are grouped by slice and,
 * inside a slice, by user (consecutive ratings share the user's P row).
 *   sched_out      host, n: rating indices in that order
 *   slice_offsets  host, n_slices + 1
 */
int mf_sched_slices(const int32_t* user_ids, const int32_t* item_ids,
                    int64_t n, int32_t n_users, int32_t n_items,
                    int32_t n_slices, int32_t* sched_out,
                    int64_t* slice_offsets);

/*
 * Tiled evaluation order (replaces the per-rating loop order of
 * _calculate_rmse, kernel_matrix_factorization.py:240-317, which any order
 * serves: the pass is read-only).  Users are cut into n_chunks contiguous id
 * ranges of about equal rating counts, items into n_slices id ranges; tile
 * c * n_slices + s holds the ratings of user chunk c and item slice s, users
 * ascending inside a tile; (1, n_slices) is mf_sched_slices' order.  With
 * the offsets passed to mf_sse and more than 8 tiles (a multiple of 8), the
 * pass deals the tiles 8 at a time (one per XCD) in dispatch order.  The
 * library's own pass uses mf_sched_slices' 8 slices: every finer tiling
 * measured slower.
 *   n_chunks * n_slices <= 128
 *   sched_out      host, n: rating indices in that order
 *   tile_offsets   host, n_chunks * n_slices + 1
 */
int mf_sched_tiles(const int32_t* user_ids, const int32_t* item_ids,
                   int64_t n, int32_t n_users, int32_t n_items,
                   int32_t n_chunks, int32_t n_slices, int32_t* sched_out,
                   int64_t* tile_offsets);

/*
 * Plan of the stratified sweep (mf_sgd_epoch_strata), host only.
 * user_bounds / item_bounds (HOST, n_blocks+1 each, non-decreasing from 0 to
 * n_users / n_items) cut the ids into B contiguous ranges; block (s, w) =
 * user range (w+s) mod B x item range w.  Inside a block every user is owned
 * by one of n_slots rating slots (largest degree first onto the least loaded
 * slot) and the ratings are edge-coloured as a bipartite (slot, item)
 * multigraph with exactly D = max(slot load, item degree) colours, one step
 * per colour: no step holds a slot or an item twice.
 *   mf_strata_plan_build      plans all blocks into an opaque handle
 *   mf_strata_plan_positions  n_positions = (total steps) * n_slots
 *   mf_strata_plan_fetch      sched_out[n_positions] = rating index per
 *                             position, -1 = idle slot (block-major, step-
 *                             major, slot-minor); block_steps[B*B+1] = step
 *                             offsets of the blocks
 *   mf_strata_plan_free
 */
typedef struct mf_strata_plan mf_strata_plan;
/* The same with n_classes user-range classes: user_bounds has
 * n_classes * n_blocks + 1 entries, block_steps (fetch) n_classes * n_blocks^2
 * + 1; block (s, w), s < n_classes * n_blocks, = user range (s + n_classes*w)
 * mod (n_classes * n_blocks) x item range w.  n_classes = 1 is
 * mf_strata_plan_build. */
int mf_strata_plan_build_classes(const int32_t* user_ids, const int32_t* item_ids, int64_t n,
                                 int32_t n_users, int32_t n_items, int32_t n_blocks,
                                 int32_t n_classes, const int32_t* user_bounds,
                                 const int32_t* item_bounds, int32_t n_slots,
                                 mf_strata_plan** plan_out);
/* mf_strata_plan_build_classes over n_cands (slots, waves) kernel shapes
 * (1..8): the step counts of each (no colouring) pick the shape of least
 * steps * waves (ties: the earlier one), the first one outright when its plan
 * fills at least fill_stop of its positions (n / (steps * slots); 0 = never);
 * only the pick is planned in full.  *picked = its index.  The plan is the
 * one mf_strata_plan_build_classes builds with that shape's slot count. */
int mf_strata_plan_build_pick(const int32_t* user_ids, const int32_t* item_ids, int64_t n,
                              int32_t n_users, int32_t n_items, int32_t n_blocks,
                              int32_t n_classes, const int32_t* user_bounds,
                              const int32_t* item_bounds, const int32_t* slot_cands,
                              const int32_t* wave_cands, int32_t n_cands, double fill_stop,
                              int32_t* picked, mf_strata_plan** plan_out);
int mf_strata_plan_build(const int32_t* user_ids, const int32_t* item_ids, int64_t n,
                         int32_t n_users, int32_t n_items, int32_t n_blocks,
                         const int32_t* user_bounds, const int32_t* item_bounds,
                         int32_t n_slots, mf_strata_plan** plan_out);
int64_t mf_strata_plan_positions(const mf_strata_plan* plan);
int mf_strata_plan_fetch(const mf_strata_plan* plan, int32_t* sched_out,
                         int64_t* block_steps);
void mf_strata_plan_free(mf_strata_plan* plan);

/* ---------------------------------------------------------------------------
 * fit() preprocessing, host only (mf_prep.cpp).  Replaces the three costly
 * steps of RecommenderBase._preprocess_data (recommender_base.py:97-173 of
 * the reference) for integer ids, with identical results:
 *
 * mf_legacy_shuffle      numpy.random.RandomState.shuffle(data) of a 1-D
 *     8-byte array, drawn from the MT19937 state (key[624], *pos) given and
 *     advancing it exactly as NumPy does (numpy 2.2 mtrand _shuffle_raw +
 *     random_interval).  On arange(n) this is permutation(n), which is the
 *     draw of X.sample(frac=1, replace=False) (recommender_base.py:131 =
 *     RandomState.choice(n, n, replace=False)); on the row order it is the
 *     per-epoch np.random.shuffle (kernel_matrix_factorization.py:371).
 *     n <= 2^32 + 1 (NumPy's 32-bit draw branch); MF_ERR_INVALID otherwise.
 * mf_legacy_permutation  out = np.random.permutation(n) (int64), the same
 *     draws as mf_legacy_shuffle of arange(n), swapped on 4-byte elements
 *     while n < 2^31.
 * mf_pairs_duplicated    *has_dup = 1 iff two rows hold the same (a, b)
 *     pair of integer ids (X.duplicated(subset=[user_id, item_id]).sum()
 *     != 0, :127-128).
 * mf_factorize           pd.factorize(vals, sort=False) of integer ids, as
 *     X[col].unique() + the id map of the shuffled frame (:135-140):
 *     uniques[0..*n_uniques) in first-appearance order (capacity n) and
 *     codes[p] = position of vals[p] in uniques.
 * mf_id_range            *lo / *hi = min / max of vals (n > 0).
 * mf_first_appearance    pd.factorize(vals[perm], sort=False) given dense ids
 *     of the unshuffled column: dense[p] - base in [0, n_dense) (the ids
 *     themselves when they span a small range, else mf_factorize's codes of
 *     the unshuffled column), n_dense <= 2^32 - 1.  codes[t] = code of row
 *     perm[t]; order[0..*n_uniques) = the dense ids in code order (capacity
 *     n_dense), so uniques = base + order or the unshuffled uniques[order].
 * mf_gather              dst[p] = src[idx[p]], idx[p] in [0, n_src), for
 *     elem_bytes 4 or 8.
 * Threads: min(16, cores) unless MF_HOST_THREADS is set. */
int mf_legacy_shuffle(uint32_t* mt_key, int32_t* mt_pos, int64_t* data, int64_t n);
/* mf_legacy_shuffle on a 1-D array of 4-byte elements: the same draws and
 * swaps (they depend on n only), half the bytes moved; the exact schedule's
 * per-epoch np.random.shuffle of the row order (kernel_matrix_factorization.py:371)
 * runs on 32-bit rating indices. */
int mf_legacy_shuffle_i32(uint32_t* mt_key, int32_t* mt_pos, int32_t* data, int64_t n);
int mf_legacy_permutation(uint32_t* mt_key, int32_t* mt_pos, int64_t* out, int64_t n);
/* np.random.shuffle of n elements in two parts (the exact schedule's
 * per-epoch shuffle, kernel_matrix_factorization.py:371, with its swaps on the
 * GPU): mf_legacy_shuffle_draws makes the draws only -- targets[d] = the
 * position swapped with n-1-d, d = 0 .. n-2 -- advancing the MT19937 state
 * exactly as the whole shuffle does; mf_legacy_apply_swaps_i32 applies swaps
 * d_begin .. n-2 of them, in order, on the host; mf_shuffle_swaps_device
 * (device pointers; stream a hipStream_t) applies swaps 0 .. d_end-1 on the
 * GPU by rounds of deterministic reservations (the same result as in
 * order): reservations = n zeroed 64-bit words kept between calls, tag_io =
 * the next round tag (start at 1; advanced), workspace >=
 * mf_shuffle_swaps_workspace_bytes(n). */
int mf_legacy_shuffle_draws(uint32_t* mt_key, int32_t* mt_pos, int64_t n, uint32_t* targets);
int mf_legacy_apply_swaps_i32(const uint32_t* targets, int64_t n, int64_t d_begin, int32_t* data);
size_t mf_shuffle_swaps_workspace_bytes(int64_t n);
int mf_shuffle_swaps_device(const uint32_t* targets, int64_t n, int64_t d_end, int32_t* data,
                            unsigned long long* reservations, void* workspace, uint64_t* tag_io,
                            void* stream);
int mf_pairs_duplicated(const int64_t* a, const int64_t* b, int64_t n, int32_t* has_dup);
int mf_factorize(const int64_t* vals, int64_t n, int64_t* codes, int64_t* uniques,
                 int64_t* n_uniques);
int mf_id_range(const int64_t* vals, int64_t n, int64_t* lo, int64_t* hi);
int mf_first_appearance(const int64_t* dense, int64_t base, int64_t n_dense, const int64_t* perm,
                        int64_t n, int64_t* codes, int64_t* order, int64_t* n_uniques);
int mf_gather(const void* src, int64_t n_src, int32_t elem_bytes, const int64_t* idx, int64_t n,
              void* dst);
/* mf_gather with 32-bit indices: the relabelled strata plans' host ids
 * (user x -> pu[x] over 10^8 int32 ids, engine.py _build_regroup). */
int mf_gather_i32(const void* src, int64_t n_src, int32_t elem_bytes, const int32_t* idx,
                  int64_t n, void* dst);
/* dst[p] = (int32)src[p] for ids in [0, bound) (else MF_ERR_INVALID; bound
 * <= 2^31), and dst[p] = (float)src[p]: the engine's host ids and FP32
 * ratings from fit()'s int64 codes and float64 ratings, threaded
 * (kernel_matrix_factorization.py _make_engine). */
int mf_ids_to_i32(const int64_t* src, int64_t n, int64_t bound, int32_t* dst);
int mf_f64_to_f32(const double* src, int64_t n, float* dst);
/* 64-bit fingerprint of a HOST buffer (threaded, not cryptographic): lets the
 * estimator tell whether the device copy of a parameter array is still the
 * NumPy attribute's content (the reference predicts from the live arrays,
 * kernel_matrix_factorization.py:148-160). */
uint64_t mf_fingerprint(const void* data, int64_t n_bytes);

#ifdef __cplusplus
}
#endif

#endif /* MF_HIP_H */
