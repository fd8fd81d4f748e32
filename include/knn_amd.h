/*
 * knn_amd.h -- C ABI of the MI355X-native KNN classifier (libknn_amd.so).
 *
 * Plain pointers and sizes only; no exceptions cross this boundary.  Every
 * entry point below names the reference interface it replaces
 * (srna99/KNN-using-p_threads-and-MPI, file:line).  The C++ surface that keeps
 * the reference's own names (ArffParser / ArffData / KNN / computeConfusionMatrix
 * / computeAccuracy) lives in knn_arff.hpp and is implemented on top of this ABI.
 *
 * Semantics (all paths, bit-exact with the reference serial KNN, main.cpp:25-85):
 *   distance  = sum_{i<d} (q_i - t_i)^2, fp32, i ascending, no FMA (main.cpp:14-23)
 *   neighbours= the k smallest (distance, train index) pairs -- the reference's
 *               strict-'<' insertion queue keeps the lower index on ties
 *               (main.cpp:45-61); distances >= FLT_MAX or NaN never qualify
 *   vote      = bincount of the k labels, argmax with ties to the smallest label
 *               (main.cpp:64-78)
 * Data layout: row-major features [n][ld] (ld >= d elements, rows 16-B aligned
 * for the device entry points), int32 labels in [0, num_classes).  Features are fp32
 * or bf16 (KNN_BF16: raw bf16 bits; distances are the fp32 direct form on the exactly
 * widened values, i.e. what the reference computes on those values as floats).
 */
#ifndef KNN_AMD_H
#define KNN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: KNN_OPT_CACHE_TRAIN no longer reuses operands derived from a caller's DEVICE train buffer;
 *    that is the separate opt-in KNN_OPT_CACHE_TRAIN_DEVICE (ABI 2 did it under the one flag) */
#define KNN_AMD_ABI_VERSION 3

typedef enum {
    KNN_OK = 0,
    KNN_EINVAL = 1,   /* bad argument: k > n_train, d mismatch, label outside [0,C), ... */
    KNN_ENOMEM = 2,   /* host or device allocation failed */
    KNN_EHIP = 3,     /* a HIP runtime call failed */
    KNN_ERANGE = 4,   /* fewer than k neighbours with a finite distance (< FLT_MAX) */
    KNN_ENODEV = 5,   /* no usable gfx950 device */
    KNN_EIO = 6,      /* file could not be opened / parsed (ARFF loader) */
    KNN_ERCCL = 7     /* an RCCL call failed (train-sharded exchange) */
} knn_status;

typedef enum { KNN_F32 = 0, KNN_BF16 = 1 } knn_dtype;

typedef enum {
    KNN_ALGO_AUTO = 0,    /* direct form for low d / small problems, MFMA GEMM form otherwise */
    KNN_ALGO_DIRECT = 1,  /* direct form, tiled (k_direct_tile: LDS-staged train tiles shared by
                             the queries of a block, scalar query operands, wave top-k + vote) */
    KNN_ALGO_GEMM = 2,    /* ||q||^2+||t||^2-2q.t on MFMA (fp32 data: fp32 MFMA, bf16 data: bf16
                             MFMA) + certified exact rescore */
    KNN_ALGO_GEMM_SPLIT = 3, /* GEMM form with fp32 data split into bf16 hi + lo (q.t = hi.hi +
                               hi.lo + lo.hi on the bf16 MFMA, fp32-grade certificate) + the
                               same exact fp32 rescore; bf16 data: as KNN_ALGO_GEMM */
    KNN_ALGO_GEMM_BF16 = 4, /* GEMM form with fp32 data rounded to bf16 for the filter only (one
                               bf16 MFMA per 16 features, certificate widened by the rounding
                               error, 2^-7 (|q|^2+|t|^2)) + the same exact fp32 rescore; AUTO
                               runs it first and re-runs a call as KNN_ALGO_GEMM_SPLIT when
                               more than 1/16 of its queries overflow their candidate lists.
                               bf16 data: as KNN_ALGO_GEMM */
    KNN_ALGO_DIRECT_SCAN = 5, /* direct form, one block per query (k_exact_scan, the GEMM path's
                                per-query fallback) */
    KNN_ALGO_GEMM_I8 = 6   /* as KNN_ALGO_GEMM_BF16, with the fp32 rows quantised to int8 for the
                              filter only (one symmetric scale per train set, max|t| / 127, used for
                              the queries too; v_mfma_i32_32x32x32_i8, half the MFMA work per
                              feature; the certificate carries the measured rounding) + the same
                              exact fp32 rescore.  Runs at d = 128, k <= 32 on a train set with a
                              finite non-zero range; anywhere else the call runs the bf16 operands
                              of KNN_ALGO_GEMM_BF16.  knn_last_stats()[11] says which ran. */
} knn_algo;

/* knn_opts.flags */
#define KNN_OPT_CACHE_TRAIN 1  /* knn_predict keeps the device copy of train across calls, keyed
                                  by (feat, labels, n, d, ld, dtype) and the generation set by
                                  knn_set_generation, together with the train-side operands of
                                  the bf16 MFMA filter derived from that copy (train norms, tile
                                  statistics, bf16 tile blocks) */
#define KNN_OPT_CACHE_TRAIN_DEVICE 2  /* (with KNN_OPT_CACHE_TRAIN) the device entry points
                                  (knn_predict_device, knn_shard_topk_device,
                                  knn_predict_train_sharded) also keep the filter operands derived
                                  from the CALLER's device train buffer, keyed by (feat, n, d, ld,
                                  dtype, filter tile height) and the generation.  The library
                                  cannot see writes to that buffer: a caller that rewrites it in
                                  place (hipMemcpy, its own kernels) or frees it and reuses the
                                  address must bump the generation (knn_set_generation) before
                                  the next call, or it gets results for the old rows.  Without
                                  this flag every device call rebuilds them (A: ~0.3 ms) */

/* Context options.  One context drives one device (a compute stream and a copy stream). */
typedef struct {
    int32_t device;        /* HIP device ordinal */
    int32_t algo;          /* knn_algo */
    int32_t train_splits;  /* GEMM path: train segments per query tile (0 = auto) */
    int32_t profile;       /* 1 = record per-stage HIP events (knn_stage_times); 2 = also count the
                              filter's candidates (an extra read of the counts per call); 3 = events
                              around the dominant stages only (filter, rescore, direct form, exact
                              scan, exchange, merge): a few microseconds less per stage skipped */
    int32_t flags;         /* KNN_OPT_* */
} knn_opts;

/* A dataset view.  feat: row-major [n][ld] of dtype; labels: int32 [n] (train only). */
typedef struct {
    const void* feat;
    const int32_t* labels;
    int64_t n;
    int32_t d;
    int32_t ld;
    int32_t dtype;         /* knn_dtype */
} knn_dataset;

typedef struct knn_ctx knn_ctx;

/* Library / ABI version (KNN_AMD_ABI_VERSION). */
int32_t knn_version(void);

/* Source hash of the tree this library was built from (16 hex digits; computed by
 * knn-using-p_threads-and-mpi_amd/build_id.py over the package's Makefile, csrc/ and
 * include/).  Tests compare it with the sources beside the library they load. */
const char* knn_build_id(void);

/* Create / destroy a context (replaces the per-run setup in main.cpp:114-131,
 * multi-thread.cpp:133-160 and mpi.cpp:119-149).  A context serves one call at a time:
 * threads that share one serialise their calls (the C++ KNN() does, per device), or each
 * creates its own. */
knn_status knn_create(knn_ctx** out, const knn_opts* opts);
void knn_destroy(knn_ctx* ctx);

/* Text of the last error on this context ("" if none). */
const char* knn_last_error(const knn_ctx* ctx);

/*
 * Metrics.  A context computes one distance, KNN_METRIC_SQEUCLIDEAN (the reference's, and the
 * default: everything in "Semantics" above, bit for bit as before) or one of
 *   KNN_METRIC_MANHATTAN  D = sum_{i<d} |q_i - t_i|: sum = +0, then for i ascending
 *                         df = fl(q_i - t_i), sum = fl(sum + |df|) in IEEE binary32 -- no FMA, no
 *                         reordering, no tree, subnormals kept;
 *   KNN_METRIC_CHEBYSHEV  D = max_i |q_i - t_i|: m = +0, then m = fmaxf(m, |fl(q_i - t_i)|).
 *                         fmaxf ignores a NaN operand, as numpy.fmax does: a NaN difference (a NaN
 *                         feature, inf - inf) leaves the maximum as it was, so such a row is
 *                         ranked by its other features.  Under Manhattan it makes the sum NaN and
 *                         the row never qualifies.
 * bf16 rows widen exactly to fp32 first.  Everything else is "Semantics": neighbours are the k
 * smallest (D, train index) pairs, lower index first on ties, with the strict '<' against the
 * FLT_MAX sentinel (a D that is NaN, inf or >= FLT_MAX never qualifies); the reported distance is
 * D itself; vote, k-sweep, self-removal, KNN_ERANGE and KNN_EINVAL are unchanged.
 * Weighted vote under a non-Euclidean metric: the reported distance is no square, so
 * KNN_W_INV_DIST (sklearn's weights="distance") is w = 1.0f / D, and KNN_W_INV_SQDIST is
 * KNN_EINVAL (there is no 1 / D^2 kind); knn_vote_weighted_device on lists the caller holds
 * follows the context's metric in the same way.  The zero rule (D == 0) and the sums are unchanged.
 *
 * knn_set_metric may be called between any two calls on the context; every entry point that
 * runs a top-k pass then uses it (knn_predict, knn_predict_device, knn_shard_topk_device,
 * knn_predict_train_sharded, knn_sweep, knn_sweep_device and the weighted entry points), through
 * the direct form's metric kernel (k_metric_tile) for every shape.  KNN_EINVAL for an unknown
 * metric, and for a non-zero metric on a context created with KNN_ALGO_GEMM, KNN_ALGO_GEMM_SPLIT,
 * KNN_ALGO_GEMM_BF16 or KNN_ALGO_DIRECT_SCAN (the GEMM form and its certificate are Euclidean,
 * and the scan kernel has no metric version); KNN_ALGO_AUTO and KNN_ALGO_DIRECT accept it.  Cached
 * train uploads and filter operands do not depend on the metric and stay valid across a switch.
 * With profile = 1 the pass's stage is named "metric_tile" (then "merge_vote" when segmented).
 * Cosine ranking needs no metric: it is Euclidean ranking on rows the caller normalised.
 */
typedef enum { KNN_METRIC_SQEUCLIDEAN = 0, KNN_METRIC_MANHATTAN = 1, KNN_METRIC_CHEBYSHEV = 2 } knn_metric;
knn_status knn_set_metric(knn_ctx* ctx, int32_t metric);
int32_t knn_get_metric(const knn_ctx* ctx);

/* Invalidates cached train uploads and cached train-side filter operands
 * (KNN_OPT_CACHE_TRAIN): both cache keys include this generation.  The reference has no counterpart (every KNN() call re-reads ArffData,
 * main.cpp:40-43). */
knn_status knn_set_generation(knn_ctx* ctx, uint64_t generation);

/* Page-locked host memory for datasets and outputs of knn_predict: copies from/to it run
 * as asynchronous DMA, overlapping the device's compute (pageable buffers work too, at
 * the runtime's staged rate). */
knn_status knn_alloc_pinned(size_t bytes, void** out);
void knn_free_pinned(void* p);

/*
 * Host-buffer entry point.  Replaces `int* KNN(ArffData* train, ArffData* test, int k)`
 * (main.cpp:25) for queries [0, test->n) and the MPI variant
 * `int* KNN(train, test, k, start, end)` (mpi.cpp:26) / pthreads thread body
 * `void* KNN(void*)` (multi-thread.cpp:37) for a [q_begin, q_end) slice.
 * out_pred: caller-allocated int32[q_end - q_begin].
 * out_topk_dist / out_topk_idx: optional (NULL) [q_end-q_begin][k], ascending.
 * k must satisfy 1 <= k <= train->n (the reference crashes for k > n_train and
 * returns all-zero predictions for k <= 0; the C++ KNN() wrapper reproduces the
 * latter, the ABI reports KNN_EINVAL).
 * Data movement: train is uploaded once per call, or once per context with
 * KNN_OPT_CACHE_TRAIN; queries stream through two device slots in batches -- batch b+1
 * uploads on the context's copy stream while batch b computes, and batch b's results
 * download while b+1 computes.  knn_last_stats()[6] / [7] report the train / query bytes
 * this call moved host -> device.
 */
knn_status knn_predict(knn_ctx* ctx, const knn_dataset* train, const knn_dataset* test,
                       int32_t k, int32_t num_classes, int64_t q_begin, int64_t q_end,
                       int32_t* out_pred, float* out_topk_dist, int32_t* out_topk_idx);

/*
 * Device-buffer entry point (inputs already resident in HBM): all pointers in the
 * datasets and outputs are device pointers on ctx's device; work is enqueued on
 * `hip_stream` (a hipStream_t; NULL = the context's own stream, a blocking stream: ordered
 * after work issued earlier on the legacy null stream).  Returns after
 * the stream has drained and the device-side status word was checked.
 *
 * The stream contract, of this and of every other entry point that takes a `hip_stream`: every
 * fill, copy, kernel and mid-call read-back of the call is enqueued on that one stream, so the call
 * is ordered after whatever the caller enqueued there before it (the work that produces its
 * inputs need not have finished, or started) and after nothing else; its result does not depend
 * on any other stream or on what is pending there.  Where a call adds into an output the caller
 * zeroes (a d_correct, d_outliers or d_summary that says so), that zero fill is the caller's work
 * and must be enqueued on the same stream, or have finished.  The Python wrappers hold their own
 * tensor work (zero fills, read-backs, conversions) to this rule: with `stream=` given it runs on
 * that stream, whatever torch's current stream is.
 */
knn_status knn_predict_device(knn_ctx* ctx, const knn_dataset* train, const knn_dataset* test,
                              int32_t k, int32_t num_classes, int32_t* d_pred,
                              float* d_topk_dist, int32_t* d_topk_idx, void* hip_stream);

/*
 * Train-sharded runs (the reference has only test-sharded drivers,
 * multi-thread.cpp:154-192 / mpi.cpp:141-186, so these two calls replace the inner
 * loop of `KNN` main.cpp:40-62 split over train shards, and its vote main.cpp:64-78).
 *
 * knn_shard_topk_device: the exact k nearest rows of ONE train shard for every query,
 * written as packed int32 records d_rec[nq][3][k]: k distance bits (fp32, the
 * reference's direct form), k global indices (idx_base + local row; -1 = none) and
 * k labels, ascending by (distance, index).  k may exceed the shard's rows (missing
 * entries are -1).  Device pointers; work on `hip_stream` (NULL = context stream).
 *
 * knn_merge_vote_device: merges nsrc such record blocks, d_rec[nsrc][nq][3][k] (e.g.
 * after an all-to-all over the ranks that own the shards), into each query's k nearest
 * by (distance, global index) -- the reference's tie rule over the whole train set --
 * and votes (smallest label on ties).  d_dist / d_idx (optional) receive [nq][k].
 * Each source list must ascend by (distance, index) with -1 padding last, as
 * knn_shard_topk_device writes it: the merge reads a list in sorted runs and stops at the
 * first run that cannot enter the top k.  A descent inside what it reads gives KNN_EINVAL.
 * KNN_ERANGE if some query has fewer than k neighbours over all shards.
 */
knn_status knn_shard_topk_device(knn_ctx* ctx, const knn_dataset* train_shard, const knn_dataset* test,
                                 int32_t k, int32_t num_classes, int64_t idx_base, int32_t* d_rec,
                                 void* hip_stream);
knn_status knn_merge_vote_device(knn_ctx* ctx, int32_t nsrc, int64_t nq, int32_t k, int32_t num_classes,
                                 const int32_t* d_rec, int32_t* d_pred, float* d_dist, int32_t* d_idx,
                                 void* hip_stream);

/*
 * Train-sharded KNN over ranks, one process per GPU (replaces the MPI
 * collective pattern of mpi.cpp:130-201 -- MPI_Init / Scatter / Gatherv -- for a train set
 * sharded instead of replicated).  The communicator is RCCL (over xGMI on one node),
 * loaded at knn_comm_create.
 *   knn_comm_unique_id: 128 opaque bytes made on one rank and handed to every rank by the
 *     caller's own bootstrap (MPI_Bcast, torch.distributed, a file).
 *   knn_comm_create: ncclCommInitRank on ctx's device; collective over the nranks ranks.
 *   knn_predict_train_sharded: rank r holds train rows [idx_base, idx_base + shard->n) and
 *     every query (test, device buffers); it computes its shard's exact top-k of every query
 *     (knn_shard_topk_device), one grouped send/recv all-to-all hands each rank the lists of
 *     the queries it owns, shard_range(test->n, nranks, rank), and k_merge_vote merges them
 *     by (distance, global index) -- the reference's lower-index tie rule over the whole
 *     train set -- and votes.  d_pred (and optional d_dist / d_idx [owned][k]) receive the
 *     owned queries' results.  Collective: every rank calls it with the same test set and k.
 *     A failure local to one rank (memory, its shard's arguments, a HIP error that leaves the
 *     device usable) is voted on by every rank (one max-allreduce of a preset device word)
 *     before the exchange: the failing rank returns its own status, its peers KNN_ERCCL, and
 *     no rank is left waiting inside the exchange.  A failure of a collective itself (e.g. after
 *     a device fault) aborts the communicator (ncclCommAbort): that rank returns KNN_ERCCL,
 *     every later call on the communicator fails, and peers inside the collective are released
 *     by their own RCCL / watchdog timeout.  With profile = 1 the
 *     context's stage times hold the shard's stages, "exchange" and "merge_vote".
 *   knn_shard_range: the reference's contiguous split with the remainder on the last worker
 *     (multi-thread.cpp:154-158, mpi.cpp:141-170).
 *   knn_exchange_layout: element offsets / counts of the all-to-all for `rank` (int32
 *     records [nq][3][k] sent, [world][owned][3][k] received); arrays of `world` entries.
 */
#define KNN_COMM_ID_BYTES 128
typedef struct knn_comm knn_comm;
knn_status knn_comm_unique_id(void* id_out);
knn_status knn_comm_create(knn_ctx* ctx, const void* id, int32_t nranks, int32_t rank, knn_comm** out);
void knn_comm_destroy(knn_comm* comm);
/* the number of ranks the RCCL communicator spans (ncclCommCount) */
knn_status knn_comm_count(const knn_comm* comm, int32_t* nranks);
/* *broken = 1 once a collective on this communicator failed and it was aborted: every later
 * knn_predict_train_sharded on it returns KNN_ERCCL at once (no shard pass, no collective), so
 * a caller that sees KNN_ERCCL can tell "a peer's shard failed, the communicator is fine" (0)
 * from "tear down every rank and build a new communicator" (1). */
knn_status knn_comm_broken(const knn_comm* comm, int32_t* broken);
/* The exchange's message plan (round 6).  Every RCCL send / recv of knn_predict_train_sharded
 * carries at most chunk_elems int32 (<= 0: the default, 64 Mi elements = 256 MiB); with
 * self_via_rccl = 0 (the default) the rank's own block is a device copy, with 1 it goes through
 * the same grouped ncclSend / ncclRecv loop as the peers' blocks -- so a one-rank communicator
 * executes the multi-rank loop's chunk offsets and counts (the GPU test of that loop; a one-GPU
 * box cannot hold two RCCL ranks).  Not collective; call it alike on every rank. */
knn_status knn_comm_set_exchange(knn_comm* comm, int64_t chunk_elems, int32_t self_via_rccl);
knn_status knn_predict_train_sharded(knn_ctx* ctx, knn_comm* comm, const knn_dataset* train_shard, int64_t idx_base,
                                     const knn_dataset* test, int32_t k, int32_t num_classes, int32_t* d_pred,
                                     float* d_dist, int32_t* d_idx, void* hip_stream);
knn_status knn_shard_range(int64_t n, int32_t world, int32_t rank, int64_t* begin, int64_t* end);
/* The partition of a `world`-GPU run (north_star "Partitioning"; the reference only splits the
 * test set, multi-thread.cpp:154-158 / mpi.cpp:141-170): *policy = KNN_SHARD_TEST (queries split
 * by knn_shard_range, train replicated, no collective on the data path) while one copy of train
 * and its bf16 filter operands fits half of `hbm_bytes` (<= 0: 288 GiB), else KNN_SHARD_TRAIN
 * (knn_predict_train_sharded).  The C++ KNN() (KNN_AMD_SHARD=auto), knn_cli --shard=auto and
 * bench.py --shard auto ask it; every caller may force either partition. */
typedef enum { KNN_SHARD_TEST = 0, KNN_SHARD_TRAIN = 1 } knn_shard_kind;
knn_status knn_shard_policy(int64_t n_train, int64_t n_query, int32_t d, int32_t dtype, int32_t world,
                            int64_t hbm_bytes, int32_t* policy);
knn_status knn_exchange_layout(int64_t nq, int32_t k, int32_t world, int32_t rank, int64_t* send_off,
                               int64_t* send_cnt, int64_t* recv_off, int64_t* recv_cnt);

/*
 * k-sweep: the predictions (and accuracy) for EVERY k in 1..kmax from one top-kmax pass.
 * The neighbour lists ascend by (distance, train index), so the k nearest of a query are the
 * first k entries of its kmax nearest; only the vote (main.cpp:64-78) is redone per prefix
 * (k_vote_sweep).  Row k - 1 of pred_all, laid out [kmax][nq], is exactly what the predict
 * entry points return for that k, and can go straight into knn_confusion_matrix_device.
 *
 * Leave-one-out (self_base >= 0): query q is train row self_base + q, and that row is taken
 * out of its own neighbour list.  The prediction for row i at k then equals the reference's
 * KNN (main.cpp:25) on the train set with row i removed: removing a row keeps the order of the
 * others, so the lower-index tie rule is unchanged.  The pass asks for kin = kmax + 1
 * neighbours; the entry equal to self_base + q is removed, and when it is absent -- at least
 * kin rows with a lower index tie or beat the self row -- the last entry is dropped, the first
 * kmax being right already.  The caller passes as `test` the slice of train rows
 * [self_base, self_base + nq).  self_base < 0: no exclusion, kin = kmax.
 *
 * knn_vote_sweep_device: the vote alone, on lists the caller already holds: d_idx[nq][idx_stride]
 *   (the first kin entries of a row: train rows ascending by (distance, index), -1 = none), as
 *   written by knn_predict_device (d_topk_idx), knn_merge_vote_device or
 *   knn_predict_train_sharded -- a train-sharded run gets its sweep without a new collective.
 *   d_train_labels is indexed by the list's (global) train rows.  With self_base >= 0 the
 *   effective list has kmax = kin - 1 entries, else kmax = kin.
 * knn_sweep_device: one top-kin pass over device datasets (the pipeline of knn_predict_device,
 *   without its vote) into context workspace, then k_vote_sweep on the same stream; one
 *   synchronisation.  d_topk_dist / d_topk_idx (optional) receive the [nq][kmax] lists after
 *   self-removal.  Needs 1 <= kmax, kin <= n_train, kin <= 1024, and with self_base:
 *   self_base + nq <= n_train.  With profile = 1 the stage times hold the pass's stages and
 *   "vote_sweep".
 * knn_sweep: host buffers in and out (the reference-style callers).  Train is uploaded and
 *   cached as in knn_predict; the queries go through one device slot, one batch after another:
 *   this path is NOT pipelined (no upload / compute / download overlap).  out_correct is summed
 *   over the batches on the host.
 * Outputs: d_query_labels (int32[nq]), d_pred_all (int32[kmax][nq]) and d_correct
 *   (int64[kmax], overwritten: correct[k - 1] = queries whose prediction for k equals their
 *   label; needs the query labels) are each optional, but not all three may be NULL.
 * KNN_ERANGE if a prefix reaches a missing entry (that k predicts 0), KNN_EINVAL for a train
 * label outside [0, num_classes).  There is no multi-rank driver: test-sharded callers run the
 * sweep on their own queries and sum `correct` over the ranks themselves.
 */
knn_status knn_vote_sweep_device(knn_ctx* ctx, int64_t nq, int32_t kin, int32_t num_classes,
                                 const int32_t* d_idx, int64_t idx_stride, const int32_t* d_train_labels,
                                 int64_t self_base, const int32_t* d_query_labels, int32_t* d_pred_all,
                                 int64_t* d_correct, void* hip_stream);
knn_status knn_sweep_device(knn_ctx* ctx, const knn_dataset* train, const knn_dataset* test, int32_t kmax,
                            int32_t num_classes, int64_t self_base, const int32_t* d_query_labels,
                            int32_t* d_pred_all, int64_t* d_correct, float* d_topk_dist, int32_t* d_topk_idx,
                            void* hip_stream);
knn_status knn_sweep(knn_ctx* ctx, const knn_dataset* train, const knn_dataset* test, int32_t kmax,
                     int32_t num_classes, int64_t self_base, const int32_t* query_labels,
                     int32_t* out_pred_all, int64_t* out_correct);

/*
 * Weighted vote: "should nearer neighbours count more?" and "how sure is the prediction?",
 * answered from the same ordered neighbour lists as the k-sweep (no reference counterpart; the
 * uniform kind is the reference's vote, main.cpp:64-78).  The neighbour list is unchanged: the k
 * smallest (distance, train index) pairs, distances the fp32 squared Euclidean values reported
 * everywhere else (the default metric; "Metrics" above gives the mapping under the others).
 *   weight    w_j = 1 (KNN_W_UNIFORM), 1.0f / sqrtf(d_j) (KNN_W_INV_DIST: sklearn's
 *             weights="distance" on the Euclidean distance) or 1.0f / d_j (KNN_W_INV_SQDIST), in
 *             IEEE binary32: round to nearest, subnormals kept, inf an ordinary value.
 *   zero rule (sklearn's; the two weighted kinds, after self-removal): when the list's first
 *             entry has d == 0, every entry with d == 0 gets weight 1 and every other entry 0.
 *   score     S_c(k) = the sum of w_j over j < k with label_j == c, accumulated in fp32 in
 *             ascending list position, S = fl(S + w_j): no FMA, no tree, no reordering.
 *   vote      the prediction for k is the argmax over c of S_c(k), ties (equal inf included) to
 *             the smallest label.  With KNN_W_UNIFORM this is exactly the k-sweep's vote.
 *   scores    d_scores (optional) fp32 [nq][num_classes] receives S_c(kmax), +0.0 for absent
 *             classes; with KNN_W_UNIFORM the bincount as floats.  Probabilities are
 *             scores / scores.sum(1), left to the caller.
 * Leave-one-out (self_base >= 0) removes the self row by the k-sweep's rule first; the zero rule
 * and the sums run on what is left.  A prefix that reaches a missing entry (-1) predicts 0 and
 * gives KNN_ERANGE, and that query's score row is all zero; a train label outside
 * [0, num_classes) gives KNN_EINVAL; an unknown `weights` gives KNN_EINVAL.  Limits as the
 * k-sweep: kin <= 1024, num_classes <= 16384; d_query_labels, d_pred_all, d_correct and d_scores
 * are each optional (d_correct needs the query labels), but not all may be NULL.
 *
 * knn_vote_weighted_device: the vote alone on lists the caller holds, d_idx / d_dist
 *   [nq][stride] of which the first kin entries of a row are read (as knn_vote_sweep_device's
 *   d_idx; d_dist may be NULL with KNN_W_UNIFORM) -- from knn_predict_device,
 *   knn_merge_vote_device or knn_predict_train_sharded, so a train-sharded run gets weighted
 *   votes with no new collective.  A non-missing entry whose distance is NaN or negative gives
 *   KNN_EINVAL.  kmax = kin, or kin - 1 with self_base; d_pred_all is [kmax][nq].
 * knn_sweep_weighted_device: knn_sweep_device's top-kin pass (its distances always kept, in
 *   context workspace), then k_vote_weighted on the same stream; one synchronisation per pass.
 *   With profile = 1 the vote's stage is named "vote_weighted".
 * knn_predict_weighted_device: the single-k form.  Only row k - 1 of the prefix votes is
 *   staged and stored: d_pred is int32[nq], no [k][nq] buffer exists.  d_pred and d_scores are
 *   each optional, not both NULL.
 * knn_sweep_weighted: host buffers, batched like knn_sweep and NOT pipelined; out_scores
 *   (optional) [nq][num_classes].
 */
typedef enum { KNN_W_UNIFORM = 0, KNN_W_INV_DIST = 1, KNN_W_INV_SQDIST = 2 } knn_weight;
knn_status knn_vote_weighted_device(knn_ctx* ctx, int64_t nq, int32_t kin, int32_t num_classes,
                                    const int32_t* d_idx, const float* d_dist, int64_t stride,
                                    const int32_t* d_train_labels, int32_t weights, int64_t self_base,
                                    const int32_t* d_query_labels, int32_t* d_pred_all, int64_t* d_correct,
                                    float* d_scores, void* hip_stream);
knn_status knn_sweep_weighted_device(knn_ctx* ctx, const knn_dataset* train, const knn_dataset* test,
                                     int32_t kmax, int32_t num_classes, int32_t weights, int64_t self_base,
                                     const int32_t* d_query_labels, int32_t* d_pred_all, int64_t* d_correct,
                                     float* d_scores, float* d_topk_dist, int32_t* d_topk_idx, void* hip_stream);
knn_status knn_predict_weighted_device(knn_ctx* ctx, const knn_dataset* train, const knn_dataset* test,
                                       int32_t k, int32_t num_classes, int32_t weights, int32_t* d_pred,
                                       float* d_scores, float* d_topk_dist, int32_t* d_topk_idx,
                                       void* hip_stream);
knn_status knn_sweep_weighted(knn_ctx* ctx, const knn_dataset* train, const knn_dataset* test, int32_t kmax,
                              int32_t num_classes, int32_t weights, int64_t self_base,
                              const int32_t* query_labels, int32_t* out_pred_all, int64_t* out_correct,
                              float* out_scores);

/*
 * Regression: a numeric target per train row instead of a class (sklearn's KNeighborsRegressor;
 * no reference counterpart), predicted for EVERY k in 1..kmax from the same ordered neighbour
 * lists as the k-sweep and the weighted vote.  The neighbour list is unchanged: the k smallest
 * (distance, train index) pairs under the context's metric, after the k-sweep's self-removal
 * when self_base >= 0.
 *   targets    float (binary32) per train row, indexed by the list's train rows (global rows for
 *              merged shards).
 *   weight     w_j is exactly the weighted vote's binary32 weight: the same three kinds
 *              (knn_weight), the same zero rule, and the same mapping under the non-Euclidean
 *              metrics (KNN_W_INV_DIST is 1.0f / D, KNN_W_INV_SQDIST is KNN_EINVAL).
 *   sums       binary64, in ascending list position, no tree and no reordering:
 *                N_k = N_{k-1} + (double)w_j * (double)y_j,   D_k = D_{k-1} + (double)w_j.
 *              The product of two binary32 values is exact in binary64, so whether the step is
 *              contracted to an FMA or not cannot change a bit.
 *   prediction for k: (float)(N_k / D_k) -- the binary64 division correctly rounded, then rounded
 *              to binary32.  KNN_W_UNIFORM gives the mean of the k nearest targets; under the zero
 *              rule it is the mean over the zero-distance entries of the prefix.
 *   IEEE       a +inf weight (a subnormal squared distance under KNN_W_INV_SQDIST) or a non-finite
 *              target gives whatever IEEE gives, NaN included (NaN payloads are unspecified).
 *   missing    a prefix that reaches a missing entry (-1) predicts NaN for that k and every larger
 *              k, and the call returns KNN_ERANGE (the outputs are written).
 *   errors     (optional; need the query targets) e_k(q) = (double)pred_k(q) - (double)yq_q,
 *              sse[k - 1] = sum_q e_k(q)^2 and sae[k - 1] = sum_q |e_k(q)| in binary64 (e * e is
 *              rounded, then added).  The order over queries is fixed and depends on the query
 *              numbers alone -- no floating-point atomics: queries are added in ascending order
 *              within chunks of 16, the chunks in ascending order within spans of 256, and the
 *              spans in ascending order into the output (block partials in context workspace and
 *              a second kernel).  The same call on the same inputs returns the same bits, and so
 *              does every entry point below on the same lists.  A NaN prediction makes that k's
 *              sums NaN.  RMSE = sqrt(sse / nq) and MAE = sae / nq are left to the caller.
 * Outputs: d_pred_all fp32 [kmax][nq] (row k - 1 is what knn_regress_device returns for k), d_sse /
 *   d_sae double[kmax] (overwritten) are each optional, but not all may be NULL; sse / sae need
 *   d_query_targets (fp32 [nq]).  Limits are the sweep's: kin <= 1024, kin <= n_train,
 *   self_base + nq <= n_train.  train->labels is not read and may be NULL on these entry points
 *   (the pass runs with a context-owned all-zero label array and one class).  An unknown `weights`
 *   gives KNN_EINVAL.
 *
 * knn_regress_vote_device: the regression alone on lists the caller holds (as
 *   knn_vote_weighted_device: d_idx / d_dist [nq][stride], the first kin entries of a row; d_dist
 *   may be NULL with KNN_W_UNIFORM) -- from knn_predict_device, knn_merge_vote_device or
 *   knn_predict_train_sharded, so a train-sharded run gets regression with no new collective.
 *   A non-missing entry whose distance is NaN or negative gives KNN_EINVAL.  kmax = kin, or
 *   kin - 1 with self_base.
 * knn_regress_sweep_device: knn_sweep_device's top-kin pass, then k_regress_sweep on the same
 *   stream; one synchronisation per pass.  The GEMM path's passes are cut at multiples of 4096
 *   queries, so the sums do not depend on them.  d_topk_dist / d_topk_idx (optional) receive the
 *   [nq][kmax] lists after self-removal.  With profile = 1 the stage is named "regress".
 * knn_regress_device: the single-k form; only row k - 1 is staged and stored (d_pred fp32 [nq]).
 * knn_regress_sweep: host buffers, batched like knn_sweep_weighted and NOT pipelined.  Batches
 *   are cut at multiples of 4096 queries and sse / sae stay on the device, added into batch after
 *   batch in batch order: they are the bits knn_regress_sweep_device returns for all queries.
 * There is no multi-rank driver: test-sharded callers sum sse / sae over the ranks themselves.
 */
knn_status knn_regress_vote_device(knn_ctx* ctx, int64_t nq, int32_t kin, const int32_t* d_idx,
                                   const float* d_dist, int64_t stride, const float* d_train_targets,
                                   int32_t weights, int64_t self_base, const float* d_query_targets,
                                   float* d_pred_all, double* d_sse, double* d_sae, void* hip_stream);
knn_status knn_regress_sweep_device(knn_ctx* ctx, const knn_dataset* train, const knn_dataset* test,
                                    const float* d_train_targets, int32_t kmax, int32_t weights,
                                    int64_t self_base, const float* d_query_targets, float* d_pred_all,
                                    double* d_sse, double* d_sae, float* d_topk_dist, int32_t* d_topk_idx,
                                    void* hip_stream);
knn_status knn_regress_device(knn_ctx* ctx, const knn_dataset* train, const knn_dataset* test,
                              const float* d_train_targets, int32_t k, int32_t weights, float* d_pred,
                              float* d_topk_dist, int32_t* d_topk_idx, void* hip_stream);
knn_status knn_regress_sweep(knn_ctx* ctx, const knn_dataset* train, const knn_dataset* test,
                             const float* train_targets, int32_t kmax, int32_t weights, int64_t self_base,
                             const float* query_targets, float* out_pred_all, double* out_sse,
                             double* out_sae);

/*
 * Local outlier factor: LOF (Breunig et al. 2000; sklearn's LocalOutlierFactor; no reference
 * counterpart) of every train row for EVERY k in [k_lo, k_hi] from one top-(k_hi + 1) pass, and
 * novelty scores of queries against the fitted tables.  A row's score reads its NEIGHBOURS' lists,
 * so the scores are computed after the last pass, over all rows, in two gather rounds.
 * Let T be the train set of n rows under the context's metric and Kr = k_hi - k_lo + 1.  Limits:
 * 1 <= k_lo <= k_hi <= 255, anything else is KNN_EINVAL.
 *   lists      row i's list is the k-sweep's leave-one-out list: the top-(k_hi + 1) list of row i
 *              against T with row i removed -- the first entry equal to i, or the last entry when
 *              none is (more than k_hi duplicates sit ahead of i at distance 0).  o_1 .. o_k are its
 *              first k entries: exactly k neighbours, no tie extension at the k-distance (sklearn's
 *              selection).
 *   distance   delta(i, o_j) is binary32: sqrtf(D) of the reported squared distance under the
 *              Euclidean metric (the correctly rounded sqrtf, as the weighted vote's), D itself
 *              under Manhattan / Chebyshev.
 *   k-distance kd_k(i) = delta(i, o_k).
 *   reach sum  reach = fmaxf(kd_k(o_j), delta(i, o_j)) in binary32;
 *              S_k(i) = sum over j = 1..k of (double)reach, binary64, ascending j, no tree and no
 *              reordering.  (A neighbour whose own list has no k-th entry makes S_k(i) NaN.)
 *   lrd        lrd_k(i) = 1.0 / (S_k(i) / (double)k + 1e-10), binary64, every operation correctly
 *              rounded and none contracted.  The 1e-10 is sklearn's: rows inside a clump of more
 *              than k duplicates stay finite.
 *   LOF        L_k(i) = sum over j = 1..k of lrd_k(o_j), binary64, ascending j;
 *              LOF_k(i) = (float)(L_k(i) / ((double)k * lrd_k(i))): one rounding to binary32.
 *   novelty    a query's list is its plain top-k_hi list against T, nothing removed (a query equal
 *              to a train row keeps that row at delta = 0); kd_k(o_j) and lrd_k(o_j) come from T's
 *              fitted tables, the query's own lrd_k and LOF_k from the formulas above.
 *   missing    a prefix that reaches a missing entry (-1; n - 1 < k) gives NaN for that k and
 *              every larger k, and the call returns KNN_ERANGE (the outputs are written).
 *   errors     on lists the caller holds, an index outside [0, n) that is not -1, or a non-missing
 *              distance that is NaN or negative, gives KNN_EINVAL.  k_lof_compact checks every
 *              entry before any gather: no kernel reads a table with an unchecked index.
 *   determinism the same inputs give the same bits on every run and through every algorithm
 *              (direct, MFMA filter, wide rows), however the pass loop cuts the rows.
 * Outputs: d_kd fp32 [n][Kr] (kd[i][k - k_lo]), d_lrd fp64 [n][Kr], d_lof fp32 [Kr][n] (row
 *   k - k_lo is LOF_k) are each optional, but not all may be NULL.
 *
 * knn_lof_fit_device: the vote-less top-(k_hi + 1) pass of train against itself (context-owned zero
 *   labels, one class: train->labels is not read), the lists of ALL rows in context workspace or in
 *   d_dist / d_idx ([n][k_hi + 1], before self-removal: what knn_lof_lists_device takes with
 *   self_base = 0) when given, then k_lof_compact, k_lof_lrd, k_lof_score on the same stream and
 *   one synchronisation for the last pass and the kernels.  k_hi + 1 may exceed n (KNN_ERANGE).
 *   With profile = 1 the three stages are named "lof".
 * knn_lof_score_device: novelty -- the plain top-k_hi pass of test against train, then d_lof_out
 *   [Kr][nq] from the fitted d_kd / d_lrd of train (all three needed).
 * knn_lof_lists_device: the kernels alone on lists [n][stride] the caller holds, the first kin
 *   entries of a row: kin = k_hi + 1 with self_base = 0 (row i is removed from list i), kin = k_hi
 *   with self_base < 0 (already removed).  List i belongs to row i of the same n rows the indices
 *   name; merged train-shard lists qualify.
 */
knn_status knn_lof_fit_device(knn_ctx* ctx, const knn_dataset* train, int32_t k_lo, int32_t k_hi, float* d_kd,
                              double* d_lrd, float* d_lof, float* d_dist, int32_t* d_idx, void* hip_stream);
knn_status knn_lof_score_device(knn_ctx* ctx, const knn_dataset* train, const knn_dataset* test, int32_t k_lo,
                                int32_t k_hi, const float* d_kd, const double* d_lrd, float* d_lof_out,
                                void* hip_stream);
knn_status knn_lof_lists_device(knn_ctx* ctx, int64_t n, int32_t kin, const int32_t* d_idx, const float* d_dist,
                                int64_t stride, int64_t self_base, int32_t k_lo, int32_t k_hi, float* d_kd,
                                double* d_lrd, float* d_lof, void* hip_stream);

/*
 * Radius neighbours: "which train rows lie within thr of this query, how many, and what do they
 * vote?" (sklearn's radius_neighbors, RadiusNeighborsClassifier and RadiusNeighborsRegressor; no
 * reference counterpart).  A neighbourhood may hold any number of rows, or none, so the answer is a
 * count and a CSR list per query, not a fixed-length top-k list.
 *   threshold  thr is a binary32 value in the units of the distance the context reports: the
 *              SQUARED Euclidean distance under the default metric, D itself under Manhattan /
 *              Chebyshev.  KNN_EINVAL unless 0 <= thr < FLT_MAX (NaN refused).
 *   membership train row t is a neighbour of query q iff D(q, t) <= thr, where D is the value, bit
 *              for bit, that knn_predict_device exports for that pair under the context's metric:
 *              Euclidean df = fl(q_i - t_i), sum = fl(sum + fl(df * df)), i ascending, no FMA
 *              ("Semantics"); Manhattan / Chebyshev by the rules of "Metrics", the fmaxf NaN rule
 *              included.  A NaN or inf D is never <= thr.  bf16 rows widen exactly.
 *   self       with self_base >= 0, train row self_base + q is not a neighbour of q.  The test is by
 *              index: equal copies of the row stay.  Requires self_base + nq <= n_train.
 *   counts     d_count[q], int32: the number of neighbours.  d_class_counts[q][c], int32
 *              [nq][num_classes]: the number of neighbours with label c.  These are integers, so
 *              any accumulation order is exact (integer atomics are used; no floating-point atomic
 *              is used anywhere in this feature).  A train label outside [0, num_classes) gives
 *              KNN_EINVAL, whether or not that row is anyone's neighbour; num_classes <= 16384.
 *   vote       d_pred[q] = the argmax over c of class_counts[q][c], ties to the smallest label.  A
 *              query with no neighbour gets outlier_label, an int32 that may take any value; this is
 *              not an error.  d_correct (int64[1], needs d_query_labels) = the number of q with
 *              pred[q] == label[q].
 *   lists      CSR: d_offsets int64 [nq + 1] is the exclusive scan of count, total = offsets[nq];
 *              d_idx int32 [total], d_dist fp32 [total].  Query q's segment is
 *              [offsets[q], offsets[q + 1]), in ASCENDING TRAIN INDEX: a fixed order, whatever the
 *              train segments of the pass, which makes every later sum reproducible.  The lists are
 *              NOT distance-sorted; a caller who wants that sorts each segment itself.
 *   weighted vote on lists: w_j is the weighted vote's binary32 weight (knn_weight: the same three
 *              kinds and the same metric mapping -- under a non-Euclidean metric KNN_W_INV_DIST is
 *              1.0f / D and KNN_W_INV_SQDIST is KNN_EINVAL).  Zero rule: if ANY entry of the segment
 *              has d == 0, those entries weigh 1 and all others 0 (the lists are not distance-ordered,
 *              so the top-k lists' "first entry" becomes "any entry").  S_c = fl(S_c + w_j) in
 *              binary32 in ascending list position; the vote is the argmax of S_c, ties to the
 *              smallest label.  An empty segment gives outlier_label and an all +0 score row.
 *              d_scores is fp32 [nq][num_classes].  With KNN_W_UNIFORM this equals the count pass's
 *              pred, and its class counts as floats.
 *   regression on lists: N = N + (double)w_j * (double)y_j and Dn = Dn + (double)w_j in list order,
 *              pred = (float)(N / Dn), the weights and the zero rule as above.  An empty segment
 *              predicts NaN (as sklearn does) and is not an error.  There are no error sums.
 *
 * knn_radius_count_device: one distance pass under the context's metric, one synchronisation.  The
 *   pass has two forms with the same results, bit for bit: the direct form (k_radius_tile, every
 *   metric and shape) and an MFMA-filtered form (k_radius_gemm: squared Euclidean, d = 64, 128 or
 *   256), which brackets each distance on the bf16 MFMA and computes the direct form's D only for
 *   the rows whose bracket holds thr.  knn_radius_policy says which a call takes.  d_count,
 *   d_class_counts, d_pred, d_correct and d_offsets are each optional, but not all may be NULL;
 *   train->labels may be NULL when none of d_class_counts / d_pred / d_correct is asked.
 * knn_radius_fill_device: the pass again, storing the lists.  The caller read offsets[nq] from a
 *   count call with the SAME train, test, thr, self_base and metric, and allocated d_idx (and
 *   d_dist, optional) with that many elements.  A query whose neighbours do not number
 *   offsets[q + 1] - offsets[q] gives KNN_EINVAL ("offsets do not belong to this call"); no element
 *   outside [offsets[q], offsets[q + 1]) is written for query q in any case.
 * knn_radius_vote_device / knn_radius_regress_device: the vote / regression alone on lists the
 *   caller holds (d_dist may be NULL with KNN_W_UNIFORM).  A distance that is NaN or negative, an
 *   index outside [0, n_train) (it is not followed), offsets that decrease, or a label outside
 *   [0, num_classes) give KNN_EINVAL.  d_pred, d_correct and d_scores are each optional, not all
 *   NULL; regression's d_pred is fp32 [nq].
 * nq == 0 returns KNN_OK.  With profile = 1 the stages are named "radius_count", "radius_fill",
 * "radius_vote" and "radius_regress" (and "radius_scan" for the scan of the counts, "radius_argmax"
 * for the vote of a pass that did not vote itself: several train segments, or more than 64 classes);
 * knn_last_stats()[2] is the number of train segments of the pass.  The MFMA form adds the stages
 * "radius_norms" and "radius_operands" in front (its train-side operands are kept across calls under
 * KNN_OPT_CACHE_TRAIN[_DEVICE], knn_last_stats()[8]); knn_last_stats()[13] is the form that ran: 0
 * direct, 1 MFMA, 2 direct because a row norm is NaN, inf or >= 2^125 (the bracket does not hold
 * there; not an error), and [14], under profile = 2, the pairs the MFMA form evaluated exactly.
 * knn_radius_vote_device / knn_radius_regress_device run no distance pass and leave [13] and [14] as
 * the last count or fill call set them.
 * knn_radius_policy: the form (0 direct, 1 MFMA) of a radius pass of n_query queries against n_train
 *   rows on a context of that metric and algo; no GPU call.  Direct for Manhattan / Chebyshev, for
 *   d outside {64, 128, 256}, an empty set, and under KNN_ALGO_DIRECT / KNN_ALGO_DIRECT_SCAN; MFMA
 *   at any size under KNN_ALGO_GEMM_BF16; under KNN_ALGO_AUTO and the other GEMM algos MFMA from a floor of train
 *   rows (>= 16384) and a floor of queries.  KNN_EINVAL for an unknown metric, dtype or algo.
 * Not here: host-buffer entry points, a multi-rank driver (counts and class counts add over train
 * shards, CSR lists concatenate by shard), distance-sorted segments (several thresholds in one
 * pass: "Radius sweep" below), regression error sums, and an int8 operand class for the MFMA form.
 */
knn_status knn_radius_count_device(knn_ctx* ctx, const knn_dataset* train, const knn_dataset* test, float thr,
                                   int32_t num_classes, int64_t self_base, int32_t outlier_label,
                                   const int32_t* d_query_labels, int32_t* d_count, int32_t* d_class_counts,
                                   int32_t* d_pred, int64_t* d_correct, int64_t* d_offsets, void* hip_stream);
knn_status knn_radius_fill_device(knn_ctx* ctx, const knn_dataset* train, const knn_dataset* test, float thr,
                                  int64_t self_base, const int64_t* d_offsets, int32_t* d_idx, float* d_dist,
                                  void* hip_stream);
int32_t knn_radius_policy(int32_t metric, int32_t dtype, int32_t d, int64_t n_train, int64_t n_query, int32_t algo,
                          int32_t* form);
knn_status knn_radius_vote_device(knn_ctx* ctx, int64_t nq, int64_t n_train, const int64_t* d_offsets,
                                  const int32_t* d_idx, const float* d_dist, const int32_t* d_train_labels,
                                  int32_t num_classes, int32_t weights, int32_t outlier_label,
                                  const int32_t* d_query_labels, int32_t* d_pred, int64_t* d_correct,
                                  float* d_scores, void* hip_stream);
knn_status knn_radius_regress_device(knn_ctx* ctx, int64_t nq, int64_t n_train, const int64_t* d_offsets,
                                     const int32_t* d_idx, const float* d_dist, const float* d_train_targets,
                                     int32_t weights, float* d_pred, void* hip_stream);

/*
 * Radius sweep: "which r?" in one distance pass, as knn_sweep_device answers "which k?".  The
 * distances do not depend on the threshold, so R thresholds cost one pass, not R.
 *   thresholds  a HOST array thr[0 .. R - 1], 1 <= R <= 32, each a binary32 value in [0, FLT_MAX) in
 *               the units of "Radius neighbours", NON-DECREASING (equal neighbours are allowed and
 *               give equal rows).  KNN_EINVAL otherwise, before anything is launched.
 *   membership  train row t is in query q's neighbourhood at index r iff D(q, t) <= thr[r], D being
 *               the very bits knn_radius_count_device tests; the self row is excluded under
 *               self_base; a NaN D is never a member.  Neighbourhoods are nested, so a pair has one
 *               bucket -- the smallest r with D <= thr[r] -- and every output is a prefix sum over
 *               buckets.  Row r of every output equals, bit for bit, what the single-threshold entry
 *               point returns for thr[r] on the same context.
 *   outputs     row r of an [R][...] output starts at r * ld_out (elements; times num_classes for
 *               class_counts / scores), with ld_out >= nq the caller's row pitch: a caller may walk
 *               its queries in blocks and fill column blocks of larger arrays.  Elements outside the
 *               call's nq columns are not written.
 * knn_radius_sweep_count_device: one distance pass under the context's metric, then
 *   k_radius_sweep_finish.  The pass has the two forms of the single-threshold pass, with the same
 *   results bit for bit, and takes the one knn_radius_policy states for the call's shape: the
 *   direct form (k_radius_sweep_tile) or the MFMA-filtered form (k_radius_sweep_gemm: the bracket
 *   [L, U] of a pair decides its bucket where no threshold lies inside it, and only the other
 *   pairs get the direct form's D).  knn_last_stats()[13], [14] and [8] read as after
 *   knn_radius_count_device.  d_count int32 [R][ld_out]; d_class_counts int32 [R][ld_out][num_classes];
 *   d_pred int32 [R][ld_out], the uniform vote, ties to the smallest label, outlier_label where
 *   count is 0; d_correct int64 [R] (needs d_query_labels), the queries with pred == label;
 *   d_outliers int64 [R], the queries with no neighbour.  Each is optional, not all NULL.
 *   d_correct and d_outliers are ADDED TO, NOT ZEROED, so that the blocks of a query set accumulate:
 *   THE CALLER ZEROES THEM before the first block.  The pass keeps integer histograms of
 *   nq * (R + 1) * (1 + num_classes) int32 (num_classes counts as 0 when no class output is asked);
 *   a call whose histograms exceed the context's workspace budget (the bytes of its GEMM-path
 *   candidate workspace) is refused with KNN_ERANGE before anything is launched, and the message
 *   names the largest nq that fits -- split the queries into blocks of at most that many.
 *   knn_radius_sweep_max_queries says that number for (R, num_classes) without a GPU call
 *   (num_classes = 0: no class output; 0 for a bad argument).
 * knn_radius_vote_sweep_device: the weighted vote of every threshold on CSR lists the caller holds,
 *   from a fill at any threshold >= thr[R - 1].  Row r is knn_radius_vote_device on the sub-list of
 *   the entries with dist <= thr[r], in list order: the same binary32 weights, the zero rule over
 *   the SUB-list ("any entry of it has d == 0"), one thread's chain of adds per class in ascending
 *   list position, ties to the smallest label; an empty sub-list gives outlier_label and a +0 score
 *   row.  d_dist is needed under every kind of weights (the filter reads it).  d_pred int32
 *   [R][ld_out], d_correct int64 [R] (ADDED TO: the caller zeroes it), d_scores fp32
 *   [R][ld_out][num_classes] (this call's nq rows of every r are zeroed here); each optional, not
 *   all NULL.  The checks of knn_radius_vote_device run on every entry of the lists, whether or not
 *   it is in a sub-list.
 * Stages under profile = 1: "radius_sweep", "radius_sweep_finish", "radius_vote_sweep".
 * Not here: a regression sweep (error sums per r), host-buffer entry points, a swept fill that
 * returns per-r offsets, the MFMA form at other widths, int8 operands.
 */
knn_status knn_radius_sweep_count_device(knn_ctx* ctx, const knn_dataset* train, const knn_dataset* test,
                                         const float* thresholds, int32_t R, int32_t num_classes,
                                         int64_t self_base, int32_t outlier_label, const int32_t* d_query_labels,
                                         int64_t ld_out, int32_t* d_count, int32_t* d_class_counts, int32_t* d_pred,
                                         int64_t* d_correct, int64_t* d_outliers, void* hip_stream);
int64_t knn_radius_sweep_max_queries(const knn_ctx* ctx, int32_t R, int32_t num_classes);
knn_status knn_radius_vote_sweep_device(knn_ctx* ctx, int64_t nq, int64_t n_train, const int64_t* d_offsets,
                                        const int32_t* d_idx, const float* d_dist, const int32_t* d_train_labels,
                                        int32_t num_classes, int32_t weights, const float* thresholds, int32_t R,
                                        int32_t outlier_label, const int32_t* d_query_labels, int64_t ld_out,
                                        int32_t* d_pred, int64_t* d_correct, float* d_scores, void* hip_stream);

/*
 * DBSCAN: the clustering most fixed-radius self-joins are run for, from three distance passes over
 * the train set against itself and no neighbour list.  Per pair it needs one bit, D <= thr.
 *   T, thr, min_samples
 *               T is the train set of n rows under the context's metric.  thr follows "Radius
 *               neighbours": binary32, 0 <= thr < FLT_MAX, in the units of the reported distance (a
 *               radius r is float32(r) * float32(r) under the Euclidean metric).  min_samples >= 1.
 *   neighbourhood
 *               N(i) = { t : D(i, t) <= thr }, D bit for bit what knn_radius_count_device tests.  The
 *               row itself is a member and so are its exact copies: a self-join with self_base = -1.
 *               D is symmetric to the bit under all three metrics ((q - t)^2 and |q - t| commute and
 *               the features are taken in the same order).  A row with a NaN feature has an empty
 *               neighbourhood and is noise (Euclidean, Manhattan: its D is NaN against every row,
 *               itself included; the Chebyshev maximum skips a NaN difference, see "Metrics").
 *   core        row i is a core row iff |N(i)| >= min_samples (sklearn's rule: the row counts itself).
 *   clusters    the connected components of the graph on the core rows with an edge wherever
 *               D <= thr.  A component's representative is its smallest row index, and clusters are
 *               numbered 0, 1, ... in ascending order of representative.
 *   border      a non-core row with at least one core neighbour takes the SMALLEST CLUSTER NUMBER
 *               AMONG ITS CORE NEIGHBOURS.  (sklearn expands cluster c completely before it starts
 *               cluster c + 1 and labels every unlabelled row a core row reaches: the first cluster
 *               to claim a border row is the smallest-numbered one next to it.)
 *   noise       every other row: -1.
 *   Together: labels == sklearn.cluster.DBSCAN(metric="precomputed").fit(D).labels_ exactly, given
 *   the same membership matrix.
 *   outputs     d_labels int32 [n]; d_count int32 [n], optional, |N(i)| -- the very bits
 *               knn_radius_count_device returns for (T, T, thr, self_base = -1); d_summary int64 [4],
 *               optional, {clusters, core rows, border rows, noise rows}.
 *   determinism the same bits on every run, through both forms of the pass and any number of train
 *               segments: every step is integer, and the union-find's roots do not depend on the
 *               order of the unions (parents only ever decrease, so a component's root is its
 *               smallest row).
 * knn_dbscan_device: the count pass (as knn_radius_count_device; the form knn_radius_policy states
 *   for (n, n)), the link pass (a passing pair of core rows q > t is joined in a lock-free
 *   union-find; only rows below a block's last query are scanned), the numbering (flatten, an
 *   exclusive scan of the roots, labels), and the border pass over the compacted rows with
 *   !core && count >= 2, in the link pass's form, whose per-query minimum of the core neighbours'
 *   cluster numbers meets across train segments in an integer atomicMin.  One synchronisation.
 *   KNN_EINVAL for min_samples < 1, a thr outside [0, FLT_MAX), n > INT32_MAX or a NULL d_labels, the
 *   outputs untouched; n == 0 returns KNN_OK (and a zero summary).
 * knn_dbscan_lists_device: the same union-find and labelling on CSR lists the caller holds --
 *   d_offsets int64 [n + 1], d_idx int32 [offsets[n]]: a knn_radius_fill_device self-join with
 *   self_base = -1 (the row itself is in its list), or lists concatenated from train shards.
 *   count[i] = offsets[i + 1] - offsets[i].  An index outside [0, n) gives KNN_EINVAL (it is checked
 *   before any table is read with it), and so do offsets that decrease.
 * Stages under profile = 1: "radius_count" (and the MFMA form's "radius_norms", "radius_operands",
 * "radius_scan" with several segments), "dbscan_link", "dbscan_border" (compaction and pass),
 * "dbscan_labels" (init, flatten, scan, labels, summary).  knn_last_stats()[13] reads as after a radius
 * call; [18] is the number of rows sent through the border pass, [19], under profile = 2, the
 * successful hooks of the union-find.  A union-find loop that reaches its iteration cap (3 n + 8
 * steps, a bound no correct run can reach) gives KNN_EHIP, "internal error", never a hang.
 * Not here: sample_weight, OPTICS, a host-buffer entry point, a multi-rank driver (lists
 * concatenate by shard: knn_dbscan_lists_device).  The eps sweep is "DBSCAN sweep" below, HDBSCAN's
 * spanning tree (every eps at once, core rows only) "Spanning tree".
 */
knn_status knn_dbscan_device(knn_ctx* ctx, const knn_dataset* train, float thr, int32_t min_samples,
                             int32_t* d_labels, int32_t* d_count, int64_t* d_summary, void* hip_stream);
knn_status knn_dbscan_lists_device(knn_ctx* ctx, int64_t n, const int64_t* d_offsets, const int32_t* d_idx,
                                   int32_t min_samples, int32_t* d_labels, int32_t* d_count, int64_t* d_summary,
                                   void* hip_stream);

/*
 * DBSCAN sweep: DBSCAN's labels at every one of R <= 32 thresholds -- the eps ladder a user walks to
 * find the radius -- from three distance passes over the train set against itself, whatever R is,
 * and no neighbour list.
 *   thresholds  thr[0 .. R - 1], a HOST array, 1 <= R <= 32, each in [0, FLT_MAX), non-decreasing
 *               (equal neighbours are allowed and give equal rows): "Radius sweep"'s checks.
 *               min_samples >= 1.
 *   definitions D, neighbourhood, core, clusters, border, noise and the numbering are "DBSCAN"'s,
 *               applied per r.  Row r of every output equals, bit for bit, what knn_dbscan_device
 *               returns at thr[r] on the same context.
 *   outputs     d_labels int32 [R][ld_out] (ld_out >= n; the columns past n are not touched);
 *               d_count int32 [R][ld_out], optional -- the very bits knn_radius_sweep_count_device
 *               gives for (T, T, self_base = -1), which are by that entry's contract
 *               knn_radius_count_device's at thr[r]; d_summary int64 [R][4], optional, per r
 *               {clusters, core rows, border rows, noise rows}.
 *   level       c(i) = the smallest r with count[r][i] >= min_samples, R if there is none.  The
 *               counts are nested, so row i is a core row at r iff c(i) <= r.
 *   determinism every step is integer: the same bits on every run, through both forms of the pass
 *               and with any number of train segments.
 * The passes:
 *   1. count    the sweep's count pass as a self-join (classes = 0), in the form knn_radius_policy
 *               states for (n, n).  The histograms are bounded by the workspace budget: the entry
 *               walks the rows in query blocks of knn_radius_sweep_max_queries(ctx, R, 0) itself (no
 *               KNN_ERANGE).  A small kernel derives level[i] = c(i) and compacts the border
 *               candidates: c(i) >= 1 and count[c(i) - 1][i] >= 2.
 *   2. link     R union-find forests parent[R][n], each starting as the identity.  A pair of rows
 *               t < q with c(q) < R, c(t) < R and D <= thr[R - 1] first becomes a core-core edge at
 *               level a = max(bucket(q, t), c(q), c(t)), bucket = the smallest r with D <= thr[r].
 *               If a < R the pair makes ONE union, into forest a.  Only rows below a block's last
 *               query are scanned; the MFMA form applies the level table's ballot and the t < q
 *               mask before the band is resolved, and gives a pair its exact distance only when a
 *               threshold of index >= max(c(q), c(t)) lies inside its bracket.
 *   3. chain    one small kernel per level, ascending.  For a row with c(i) <= r: root_r[i] =
 *               find(forest r, i), and if r + 1 < R the row is joined to that root in forest r + 1.
 *               The graph at level r is the core rows of level r with the edges of level <= r; its
 *               components are the closure of the edges of level exactly r (put into forest r by
 *               the pass) together with the components of level r - 1 (carried in by this step).
 *               Forest r - 1 is final when kernel r - 1 starts, and the union-find's invariant (the
 *               larger root is hooked under the smaller) makes each root the component's smallest
 *               row whatever the order.  Cluster numbers per level: the exclusive scan of isroot.
 *   4. border   one pass over the candidates, read through cand[] (not gathered).  A pair (q, t)
 *               with c(t) < R offers root_r[t] to best[r][q] for r in [max(bucket, c(t)), c(q)), an
 *               unsigned integer atomicMin.  Clusters are numbered in ascending order of root, so
 *               the smallest root is the smallest cluster number.  The self pair's range is empty.
 *   5. labels   per (r, i): a core row its root's number, a row with an offer that root's number,
 *               every other row -1; summary[r] by integer adds.  One synchronisation.
 *   Unsafe norms: "Radius neighbours"' protocol in all three passes (the MFMA kernel returns, the
 *   direct kernel runs behind the gate, knn_last_stats()[13] == 2).
 * KNN_EINVAL before anything is launched, the outputs untouched, for everything
 * knn_radius_sweep_count_device and knn_dbscan_device refuse, and for ld_out < n.  n == 0 returns
 * KNN_OK and zero summaries.  A failed workspace allocation (about R * n * 4 bytes each for parent,
 * root, best, the roots' flags and own counts, R * n * 8 for the scans) returns KNN_ENOMEM.
 * Stages under profile = 1: "radius_sweep" and "radius_sweep_finish" (once per query block; and the
 * MFMA form's "radius_norms", "radius_operands"), "dbscan_sweep_link", "dbscan_sweep_border",
 * "dbscan_labels" (levels and candidates, init, the chain and its scans, labels, summary).
 * knn_last_stats(): [13] and [14] read as after a radius call ([14]: all three passes together);
 * [18] the rows sent through the border pass; [19], under profile = 2, the successful hooks of the
 * link pass and the level chain together.  The union-find's step cap gives KNN_EHIP, never a hang.
 * Not here: sample_weight, a lists-held sweep, a min_samples sweep, OPTICS, host-buffer entry points,
 * the MFMA form at widths other than 64 / 128 / 256.  Every eps without a ladder: "Spanning tree".
 */
knn_status knn_dbscan_sweep_device(knn_ctx* ctx, const knn_dataset* train, const float* thresholds, int32_t R,
                                   int32_t min_samples, int64_t ld_out, int32_t* d_labels /* [R][ld_out] */,
                                   int32_t* d_count /* optional */, int64_t* d_summary /* [R][4], optional */,
                                   void* hip_stream);

/*
 * Spanning tree: the minimum spanning tree of the mutual-reachability graph of the train set -- the
 * part of HDBSCAN that needs a GPU.  It has n - 1 edges and answers every radius at once: cutting it at
 * thr gives DBSCAN's clusters of core rows (DBSCAN*) at thr, for any number of thresholds, with no
 * further distance pass; it is also the single-linkage dendrogram the condensed tree is computed from.
 *   T           the train set of n rows under the context's metric.
 *   D           the value knn_radius_count_device tests: squared under the Euclidean metric, symmetric
 *               to the bit.  Everything below is in D's units, like thr in "Radius neighbours".  sqrtf
 *               is monotone, so the tree is a minimum spanning tree in unsquared units too.
 *   core        c(i) is the min_samples-th smallest D(i, .) over all of T, the row itself and its copies
 *               included (sklearn's rule, and DBSCAN's "the row counts itself"): entry min_samples - 1
 *               of row i's plain top-K list against T, self_base = -1, nothing removed.  So c(i) <= thr
 *               iff knn_dbscan_device's count[i] >= min_samples at thr.  c(i) = +inf when that entry is
 *               missing (fewer than min_samples rows qualify under top-k's rule D < FLT_MAX: a row
 *               with a NaN feature under the Euclidean and Manhattan metrics, whose D is NaN against
 *               every row, itself included; the Chebyshev maximum skips a NaN difference, "Metrics").
 *               1 <= min_samples <= 256; min_samples > n is KNN_EINVAL, the outputs untouched.
 *   edges       a pair a != b is an edge iff D(a, b) < FLT_MAX (top-k's rule: NaN, inf and the sentinel
 *               never qualify), with weight w = fmaxf(fmaxf(c(a), c(b)), D) in binary32.  w >= +0, so
 *               its bit pattern orders as an unsigned integer; w may be +inf.
 *   order       edges are STRICTLY ordered by (w, min(a, b), max(a, b)), and the tree is the unique
 *               minimum spanning forest under that order (one tree per component of the graph of
 *               edges).  For a fixed row q, ordering its candidates t by (w, t) is the same order.
 *   outputs     d_w fp32 [n - 1], d_a / d_b int32 [n - 1] with a < b, ascending by that order; d_core
 *               fp32 [n], optional; d_summary int64 [4] = {edges E, components n - E, rounds run, rows
 *               sent through distance passes summed over the rounds}.  Entries past E are left as
 *               the caller had them.
 *   determinism the same bits on every run, with any train_splits and with the list shortcut on or
 *               off: every reduction is an integer minimum, the forest does not depend on the order
 *               of the unions, the final sort fixes the edge order.  No floating-point atomics.
 * knn_mst_device: Boruvka rounds.
 *   1. lists    the vote-less top-K pass of all rows against T (knn_lof_fit_device's, nothing
 *               removed), K = max(min_samples, 32) capped at n; c(i) and dlast(i), the list's last
 *               distance.
 *   2. resolve  per round and row, the smallest key bits(w) << 32 | t over the listed rows t of another
 *               component.  The row is resolved when its list holds every candidate it has (K == n, or
 *               a missing entry) or a listed candidate has w < dlast(i) STRICTLY (an unlisted row has
 *               D >= dlast, and only the strict test excludes a tie the (w, t) order could give to an
 *               unlisted row of smaller index).  The other rows are compacted into a candidate list.
 *   3. pass     the candidates against T, k_radius_tile's direct form and segments: per pair
 *               ok = D < FLT_MAX && comp[t] != comp[q], the lane keeps its minimum key per query, the
 *               wave's minimum meets the other segments' in a 64-bit integer atomicMin.
 *   4. pick     the component's smallest edge under (w, lo, hi) by two integer atomicMin steps; one
 *               union per component root in DBSCAN's lock-free union-find; the call that hooked
 *               appends the edge (the strict order makes the chosen edges cycle-free, so an edge
 *               chosen from both sides hooks once); flatten.  One counter read-back, the round's one
 *               synchronisation.
 *   5. sort     by (w, a, b) (rocPRIM's radix sort, stable: on (a, b), then on bits(w)).
 *   Rounds run until the tree is complete or no component has a candidate, at most
 *   ceil(log2 n) + 1; more, a round that hooks nothing while candidates exist, or the union-find's
 *   step cap give KNN_EHIP "internal error", never a spin.  The test hook KNN_MST_LISTS=0 (read at
 *   knn_create) turns the list shortcut off: every row goes through every pass.
 *   KNN_EINVAL, the outputs untouched, for min_samples outside [1, 256] or above n, n > INT32_MAX, a
 *   NULL d_summary, and NULL d_w / d_a / d_b when n >= 2.  n == 0 and n == 1 return KNN_OK with zero
 *   edges.
 * knn_mst_cut_device: DBSCAN* at R thresholds from a tree the caller holds.
 *   thresholds  a HOST array thr[0 .. R - 1], 1 <= R <= 32, each in [0, FLT_MAX), non-decreasing: the
 *               DBSCAN sweep's checks and error codes.
 *   cut         row i is a core row at r iff c(i) <= thr[r]; the clusters at r are the components of
 *               the forest's edges with w <= thr[r], numbered 0, 1, ... by ascending smallest row
 *               ("DBSCAN"'s numbering); every other row is -1.  BORDER ROWS ARE NOT ASSIGNED: this is
 *               DBSCAN*, HDBSCAN's own definition.  labels[r][i] equals knn_dbscan_sweep_device's
 *               label where its count[r][i] >= min_samples, and is -1 elsewhere.
 *   outputs     d_labels int32 [R][ld_out] (ld_out >= n; the columns past n are not touched);
 *               d_summary int64 [R][3], optional, {clusters, core rows, other rows}.
 *   The levels are nested: one union-find forest is carried over, level r joins the edges with
 *   thr[r - 1] < w <= thr[r] in parallel, then the components of the core rows are numbered.  The
 *   edges need not be sorted.  Every edge index is checked against [0, n) before any table is read
 *   with it: KNN_EINVAL.  KNN_EINVAL too, before anything is launched, for n > INT32_MAX, n_edges
 *   outside [0, n - 1], ld_out < n, bad thresholds, and NULL d_core / d_labels (n > 0) or d_w / d_a /
 *   d_b (n_edges > 0).  n == 0 returns KNN_OK and zero summaries.
 * Stages under profile = 1: the list pass under its own names ("direct_tile", "gemm_filter", ...),
 * "mst_lists" (c and dlast), per round "mst_resolve", "mst_pass", "mst_pick", then "mst_sort"; the cut
 * is "mst_cut".  knn_last_stats()[20] is the rounds run and [21] the rows sent through passes.
 * Not here: the condensed tree and EOM / leaf extraction (ties among mutual-reachability weights are
 * the rule -- every edge at a row's core distance -- and sklearn's flat labels then depend on its
 * Prim order: that needs a tie rule of its own), an MFMA-bracketed form of the pass, skipping rows by
 * a per-component upper bound, halving the pass by symmetry, a multi-rank driver, a host-buffer entry.
 */
knn_status knn_mst_device(knn_ctx* ctx, const knn_dataset* train, int32_t min_samples, float* d_w, int32_t* d_a,
                          int32_t* d_b, float* d_core /* optional */, int64_t* d_summary /* [4] */, void* hip_stream);
knn_status knn_mst_cut_device(knn_ctx* ctx, int64_t n, int64_t n_edges, const float* d_w, const int32_t* d_a,
                              const int32_t* d_b, const float* d_core, const float* thresholds, int32_t R,
                              int64_t ld_out, int32_t* d_labels /* [R][ld_out] */,
                              int64_t* d_summary /* [R][3], optional */, void* hip_stream);

/* Per-stage device times (ms) of the last predict call when opts.profile >= 1.
 * names: optional array of n const char* to receive stage names. Returns the
 * number of stages recorded (<= n). */
int32_t knn_stage_times(const knn_ctx* ctx, const char** names, float* ms, int32_t n);

/* Counters of the last predict call: [0] GEMM candidates kept, [1] queries sent to
 * the exact fallback, [2] train segments used, [3] filter operand type (-1 = no GEMM
 * filter ran, 0 = fp32, 1 = bf16, 2 = bf16 hi/lo split of fp32, 3 = bf16 rounding of
 * fp32), [4] 1 when AUTO re-ran the call with the split filter, [5] 1 when the filter
 * ran with the train norm folded into the MFMA (the fused-norm bf16 filter), [6] train
 * bytes and [7] query bytes a knn_predict call copied host -> device, [8] 1 when the
 * filter's train-side operands came from the KNN_OPT_CACHE_TRAIN cache (no train norm or
 * tile-block pass ran), [9] 32 when the fused filter ran (the rows of its MFMA tile; it has
 * one shape), 0 when no fused filter ran, [10] the fused filter's queries per
 * wave (32 or 64, knn_fused_plan's rule; 0: no fused filter ran), [11] the element the filter
 * multiplied: 1 int8 (KNN_ALGO_GEMM_I8's form; [3] stays 3, fp32 rows rounded once to a narrow
 * MFMA operand), 0 the data's own type or bf16, [12] the records the int8 filter parked in LDS
 * for its batched slow path in the last pass (counted under profile = 2 only, like [0]; 0
 * otherwise), [13] the form of a radius pass (0 direct, 1 MFMA, 2 direct because of unsafe norms),
 * [14] the pairs a radius pass's MFMA form evaluated exactly (profile = 2 only), [15] the operand
 * width of the last filter pass in features (the rows the MFMA multiplied: d padded with zero
 * columns, knn_filter_policy's operand_width; 0 when no filter ran), [16] the chunks the filter
 * cut an operand row into (1 for k_gemm_fused and k_gemm_filter, operand width / 128 for
 * k_gemm_wide; 0 when no filter ran), [17] the queries of the last pass whose start threshold the
 * int8 filter's seed pass lowered to a finite bound (k_seed_thr; counted under profile = 2 only,
 * like [0] and [12]; 0 otherwise), [18] the rows a DBSCAN call sent through its border pass (the
 * non-core rows with a neighbour besides themselves), [19] the successful hooks of its union-find
 * (profile = 2 only; 0 otherwise), [20] the rounds a spanning-tree call ran and [21] the rows its rounds
 * sent through distance passes (knn_mst_device).
 * Returns the number written (<= 22); a caller that asks for 11, 12, 13, 15, 17, 18 or 20 gets the first
 * 11, 12, 13, 15, 17, 18 or 20 as before. */
int32_t knn_last_stats(const knn_ctx* ctx, int64_t* out, int32_t n);

/*
 * knn_filter_policy: which form a top-k pass of n_query queries of d features against n_train
 * rows of that dtype takes at this k on a context created with `algo` -- the default squared
 * Euclidean metric, no train_splits, no test hooks; no GPU call.
 *   *form: 0 direct (k_direct_tile / k_exact_scan: no filter), 1 fused (k_gemm_fused), 2 filter
 *   (the non-fused k_gemm_filter), 3 wide (k_gemm_wide: the K-chunked filter of rows wider than
 *   256 features).
 *   *operand_width: the filter's operand row width in features (0 for the direct form).  The
 *   bf16 operand classes -- fp32 rows rounded to bf16 (KNN_ALGO_GEMM_BF16, AUTO, and
 *   KNN_ALGO_GEMM_I8 outside its own shapes) and bf16 data -- pad a row with zero columns: any
 *   d <= 256 to the smallest of 64, 128, 256 that holds it, 256 < d <= 4096 to the next multiple
 *   of 128 (the wide kernel's chunk).  The fp32 and split classes (KNN_ALGO_GEMM on fp32 data,
 *   KNN_ALGO_GEMM_SPLIT) multiply the caller's rows and exist at d = 32, 64, 128 only; the int8
 *   operands at d = 128 only.
 * Rules: KNN_ALGO_DIRECT / KNN_ALGO_DIRECT_SCAN are direct; k > 128, k > n_train and d > 4096 are
 * direct; a forced KNN_ALGO_GEMM_BF16 context (and KNN_ALGO_GEMM on bf16 data) takes the filter at
 * any d <= 4096 and any size; KNN_ALGO_AUTO takes it from d >= 32 and n_train >= 8192 when the
 * call has >= 10^9 pairs, and at d = 64, 128, 256 from n_train >= 16384 at any query count.
 * KNN_EINVAL for an unknown dtype or algo, d < 1, k < 1, a negative count or a NULL pointer.
 */
int32_t knn_filter_policy(int32_t dtype, int32_t d, int32_t k, int64_t n_train, int64_t n_query, int32_t algo,
                          int32_t* form, int32_t* operand_width);

/*
 * Synthetic generator, device side: fills rows [row0, row0+n) of a
 * row-major [n][ld] device buffer (pad columns zeroed) and optional labels,
 * from the counter-based hash keyed by (seed, stream, row, col).
 * kind: 0 = fp32 on the 2^-23 grid in [-1,1), 1 = bf16-exact k/128; 2 / 3 = the same two
 *       clustered: the row's class centroid + noise, so labels carry signal
 *       (needs num_classes >= 1; bf16 output: kinds 1 and 3).
 * out dtype follows `dtype` (KNN_BF16 stores bf16 bits).
 */
knn_status knn_generate(knn_ctx* ctx, void* d_feat, int32_t* d_labels, int64_t row0, int64_t n,
                        int32_t d, int32_t ld, int32_t dtype, int32_t kind, uint64_t seed,
                        uint32_t stream, int32_t num_classes, void* hip_stream);

/* Evaluation, host side.  computeConfusionMatrix (main.cpp:87-100): cm is
 * caller-allocated int32[C*C], row = true class, col = predicted. */
knn_status knn_confusion_matrix(const int32_t* pred, const int32_t* labels, int64_t n,
                                int32_t num_classes, int32_t* cm);
/* computeAccuracy (main.cpp:102-112): trace(cm) / n as float. */
float knn_accuracy(const int32_t* cm, int32_t num_classes, int64_t n);

/* On-device computeConfusionMatrix (main.cpp:87-100) for predictions that stay in HBM:
 * d_cm (device int32[C*C], overwritten) += 1 at [label][pred] for every query; d_correct
 * (optional device int64[1]) receives trace(cm), so accuracy = *d_correct / (float)n as in
 * computeAccuracy (main.cpp:102-112).  KNN_EINVAL if a label or prediction is outside
 * [0, C) (the reference writes out of bounds there). */
knn_status knn_confusion_matrix_device(knn_ctx* ctx, const int32_t* d_pred, const int32_t* d_labels,
                                       int64_t n, int32_t num_classes, int32_t* d_cm,
                                       int64_t* d_correct, void* hip_stream);

/* Self-test of the hardware assumption behind the bf16 GEMM-form certificate (no
 * reference counterpart; DESIGN.md "Certificate"): runs the bf16 filter's MFMA chain
 * (v_mfma_f32_32x32x16_bf16 over K/16 k-steps, the filter's lane map) on device
 * operands a, b = [32][K] bf16 bits (K % 16 == 0) and writes d_out[i][j] =
 * sum_k a[i][k] b[j][k] as the MFMA accumulates it (device float [32][32]). */
knn_status knn_mfma_probe_bf16(knn_ctx* ctx, const uint16_t* d_a, const uint16_t* d_b, int32_t K,
                               float* d_out, void* hip_stream);
/* The same for the int8 operand class: v_mfma_i32_32x32x32_i8 over K/32 k-steps on a, b =
 * [32][K] int8 (K % 32 == 0), d_out int32 [32][32]; every sum must be the integer dot product. */
knn_status knn_mfma_probe_i8(knn_ctx* ctx, const int8_t* d_a, const int8_t* d_b, int32_t K,
                             int32_t* d_out, void* hip_stream);

/* ARFF loader (replaces ArffParser::parse, libarff/arff_parser.cpp:23, for the
 * read path): NUMERIC attributes parsed with libarff's istringstream>>float rules.
 * The class is the last attribute. */
typedef struct knn_arff knn_arff;
knn_status knn_arff_open(const char* path, knn_arff** out, char* err, int32_t err_len);
void knn_arff_shape(const knn_arff* h, int64_t* n_instances, int32_t* n_attributes,
                    int32_t* num_classes);
/* Copies features [n][ld] (pad zeroed) and (int)(float) labels of the last attribute. */
knn_status knn_arff_copy(const knn_arff* h, float* feat, int32_t ld, int32_t* labels);
/* The same with the last attribute as a float, not truncated (regression targets): any finite
 * value, negative or fractional; num_classes is not meaningful for such a file. */
knn_status knn_arff_copy_targets(const knn_arff* h, float* feat, int32_t ld, float* targets);
void knn_arff_close(knn_arff* h);

#ifdef __cplusplus
}
#endif
#endif /* KNN_AMD_H */
