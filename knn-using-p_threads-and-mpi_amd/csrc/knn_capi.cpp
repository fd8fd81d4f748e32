// knn_capi.cpp -- the C ABI (include/knn_amd.h): contexts, workspace, stage launches.
//
// Replaces the reference's drivers: the serial loop of main.cpp:25-85, the pthreads
// fan-out of multi-thread.cpp:154-192 and the MPI scatter/gather of mpi.cpp:141-186
// become one device pipeline per context:
//   DIRECT:  k_exact_scan                                  (fused distance/top-k/vote)
//   GEMM:    k_row_norms x2 -> k_gemm_filter -> k_rescore -> k_exact_scan(fallback list)
//   a non-Euclidean metric (knn_set_metric): k_metric_tile (-> k_merge_vote), every shape
//   radius neighbours (knn_radius_*): k_radius_tile (-> k_radius_scan / k_radius_argmax), every shape;
//     squared Euclidean at d = 64 / 128 / 256 above knn_radius_policy's floors: k_row_norms x2 ->
//     k_tn_rows x2 -> k_radius_gemm (k_radius_tile behind it, gated on unsafe norms)
//   local outlier factor (knn_lof_*): the vote-less top-k pass of ALL rows, then k_lof_compact ->
//     k_lof_lrd -> k_lof_score (two gather rounds over the rows' own tables)
//   DBSCAN (knn_dbscan_*): the radius count pass of the train set against itself -> k_dbscan_init ->
//     the pass in RADIUS_LINK mode (a lock-free union-find) -> k_dbscan_flatten -> k_radius_scan ->
//     k_dbscan_labels -> k_dbscan_candidates -> the pass in RADIUS_BORDER mode -> k_dbscan_summary
//   the spanning tree (knn_mst_*): the vote-less top-k pass of ALL rows -> k_mst_core -> per Boruvka
//     round k_mst_resolve -> k_mst_tile -> k_mst_pick_lo / _hi -> k_mst_hook -> k_mst_flatten and one
//     counter read-back -> rocPRIM's radix sort -> k_mst_unpack; the cut: k_mst_cut_link / _roots / _labels
// Train-sharded runs use the same pipeline per shard with the vote
// replaced by a packed (dist, global idx, label) neighbour list, then k_merge_vote.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/knn_amd.h"
#include "knn_kernels.h"

static_assert(KNN_METRIC_SQEUCLIDEAN == METRIC_SQEUCLIDEAN && KNN_METRIC_MANHATTAN == METRIC_MANHATTAN &&
                  KNN_METRIC_CHEBYSHEV == METRIC_CHEBYSHEV,
              "knn_metric is passed to the launchers as is");

namespace {

struct DBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        hipError_t e = hipMalloc(&p, n ? n : 16);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct Stage {
    const char* name;
    hipEvent_t a, b;
};

}  // namespace

struct knn_ctx {
    int device = 0;
    int algo = KNN_ALGO_AUTO;
    int metric = KNN_METRIC_SQEUCLIDEAN;  // knn_set_metric; no cached operand depends on it
    int train_splits = 0;
    int profile = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // device workspace
    DBuf tnorm, tnp, qnorm, gthr, cnt, cand, fb_list, ctrl, scratch;
    DBuf split_t, split_q;  // KNN_ALGO_GEMM_SPLIT / _BF16: bf16 [hi | lo] / rn copies of fp32 rows
    DBuf pad_t;             // KNN_ALGO_GEMM, n_train not a multiple of 64: the rows padded to the tile grid
    DBuf seg_rec;           // k_direct_tile segment records [nseg][nq][3][k]
    DBuf tmax;              // fused filter: per-64-row train stats {max tn, max |t - rt|, max |rt|, 0}
    DBuf tsmax;             // fused filter: their maxima over all tiles (k_tile_stat_max; cached with tmax)
    DBuf cursor;            // fused filter: per-XCD scan cursors (64-row units; performance hint only) on the
                            // segment schedule, or the per-XCD pacing words (int32 pairs) on the balanced one
    DBuf lshare;            // fused filter: per (query, piece) threshold lists shared between pieces
    DBuf parkcnt;           // fused filter, profile = 2: the records its parked passes held (one 64-bit word)
    bool park_counted = false;  // the last pass's filter counted into parkcnt
    DBuf seedbuf;               // profile = 2: the last pass's seeds (k_seed_thr), ordered bits per query
    int64_t seed_nq = 0;        // ... and how many queries it holds (0: the pass ran no seed)
    DBuf qstat;             // fused filter: per-query {|q|, |q - rq|} upper bounds
    DBuf tblk;              // fused filter: train tile blocks [bn rows rn(t) | bn norms | tile stats]
    DBuf tctrl;             // the train norms' share of the status word: [unsafe bits, 0, max norm, 0]
    // train-side operands of the fused filter (tnorm, tnp, tmax, tblk, tctrl) kept across calls
    // under KNN_OPT_CACHE_TRAIN, keyed by the train view, the tile height and the generation;
    // epoch = the upload count of knn_predict's own train buffer (its pointer does not change)
    // (i8: the blocks hold the int8 operand class)
    struct { const void* feat; int64_t n; int d, ld, dtype, bn; uint64_t gen, epoch; bool valid; int i8; }
        tprep{nullptr, 0, 0, 0, 0, 0, 0, 0, false, 0};
    // the int8 operand class's view of a train set (KNN_ALGO_GEMM_I8), kept with tprep's key: the
    // scale s = max|t| / 127 (read back once per train set: the one host round trip of the
    // class, on the call that builds the operands), whether the class may run on it (finite,
    // non-zero range), and whether a call ended with more than 1/64 of its queries on the exact
    // fallback (demoted: AUTO then keeps to the bf16 operands for this train set)
    struct { const void* feat; int64_t n; int d, ld; uint64_t gen, epoch; bool valid; float s; bool ok, demoted; }
        i8c{nullptr, 0, 0, 0, 0, 0, false, 0.0f, false, false};
    DBuf i8max;              // the max-abs word of k_absmax
    float i8_coarsen = 1.0f; // test hook (knn_debug_set_i8_coarsen): the int8 step times a factor in [1, 8]
    int64_t i8_pass_nq = 0;  // queries of the last int8 pass (the demotion rule)
    uint64_t train_epoch = 0;
    // the same for the non-fused GEMM paths' train copy padded to the 64-row grid (pad_t)
    struct { const void* feat; int64_t n; int d, ld, dtype; uint64_t gen, epoch; bool valid; }
        tpad{nullptr, 0, 0, 0, 0, 0, 0, false};
    int rescore_su = 0;  // test hook KNN_RESCORE_SU: the rescore's LDS staging size (0 = sized)
    // test hooks of the fused filter's plan (KNN_FUSED_QG / _HEAPS / _PARK), read once at knn_create: a
    // call never reads the environment, and one pass uses one plan throughout
    FusedForce fforce;
    // the device entry points reuse derived train operands across calls only under
    // KNN_OPT_CACHE_TRAIN_DEVICE (the caller's device buffer may change behind the library)
    int cache_train_device = 0;
    // host-API staging (device copies of host inputs / outputs)
    DBuf h_train, h_labels, h_test, h_pred, h_dist, h_idx;
    int32_t* ctrl_host = nullptr;  // pinned, mapped, fine-grained: [0] status, [1] fallback count,
                                   // [4] the sequence number of the last k_finish
    uint32_t finish_seq = 0;
    int32_t* ctrl_host_dev = nullptr;  // its device address (k_finish writes it)
    bool ctrl_clean = false;  // the status words are zero (the last call ended in k_finish)
    // list consumers (lists_core / lists_host): the top-kin lists of the pass, and the host entry
    // points' device copies of pred_all, the queries' side input (labels or targets), the per-k
    // accumulators (correct | sse, sae) and the scores; sized once and grown like the others
    DBuf sw_dist, sw_idx, sw_pred, sw_qside, sw_acc, sw_scores;
    // regression (knn_regress_*): the error partials [2][kmax][chunks], the all-zero label array
    // the vote-less pass runs with (the caller has no classes), and the host entry point's device
    // copy of the train targets
    DBuf rg_part, rg_zero, rg_targets;
    // local outlier factor (knn_lof_*): the top-kin lists of ALL rows (the gathers need every row's
    // list, so they are not the per-pass sw_idx / sw_dist), the self-removed lists cidx / delta
    // [n][k_hi], and the tables kd [n][Kr] fp32 / lrd [n][Kr] fp64 the caller did not ask for;
    // lof_qlrd: the queries' own lrd of a novelty call
    DBuf lof_idx, lof_dist, lof_cidx, lof_delta, lof_kd, lof_lrd, lof_qlrd;
    // radius neighbours: per-(segment, query) counts [nseg][nq] and list bases [nseg][nq] int64 of
    // a segmented pass; class counts [nq][C] / scores [nq][C] the caller did not ask for but the
    // vote needs
    DBuf rd_segcnt, rd_base, rd_cc, rd_scores;
    // the radius sweep's bucket histograms: hist [nq][R + 1] | chist [nq][R + 1][C], int32
    DBuf rd_sweep;
    // DBSCAN: the int32 tables parent | root | isroot | cluster | cand [5][n], the int64 scan of the
    // roots [n + 1], the summary words {clusters, core, border, noise, unions} and the neighbour
    // counts a caller did not ask for
    DBuf db_tab, db_offs, db_info, db_count;
    // the DBSCAN sweep: the int32 tables level | cand [2][n] and parent | root | isroot | best [4][R][n],
    // the int64 scans of the roots [R][n + 1], the summary words [R][4] + unions, and the counts
    // [R][n] a caller did not ask for
    DBuf dbs_tab, dbs_offs, dbs_info, dbs_count;
    // the spanning tree (knn_mst_*): the top-K lists of all rows; core | dlast fp32 [2][n]; parent | comp |
    // cand | comphi int32 [4][n]; rowbest | compbest | the edge keys, 64-bit [3][n]; the edge weights'
    // bits [n]; the counters; the sort's storage.  The cut: parent | root | isroot int32 [3][n], the
    // int64 scan of the roots [n + 1], the summary words [3]
    DBuf mst_idx, mst_dist, mst_f, mst_i, mst_u, mst_w, mst_cnt, mst_sort, mst_cut, mst_offs, mst_info;
    int mst_lists = 1;       // test hook KNN_MST_LISTS=0: no list shortcut, every row through every pass
    int mst_list_l = -1;     // test hook KNN_MST_LIST_L=n: the list length beyond min_samples (-1: the library's)
    int64_t mst_summary[4];  // the fit's summary on its way to the device
    // the pass rd_segcnt's counts came from: a fill whose pass has the same key takes them as they
    // are instead of counting again.  (Rows rewritten in place in between are caught where stale
    // counts would matter: the fill checks every (segment, query) count against its own.)
    struct RadiusKey {
        const void *train, *test; int64_t nt, nq, self_base; int d, ld_t, ld_q, dtype, metric, nseg; uint32_t thr_bits;
        bool valid;
        int64_t seg_len;  // (the two forms cut the same number of segments at different rows)
        bool same(const RadiusKey& o) const {
            return valid && o.valid && train == o.train && test == o.test && nt == o.nt && nq == o.nq &&
                   self_base == o.self_base && d == o.d && ld_t == o.ld_t && ld_q == o.ld_q && dtype == o.dtype &&
                   metric == o.metric && nseg == o.nseg && thr_bits == o.thr_bits && seg_len == o.seg_len;
        }
    } rd_key{};
    // the MFMA form of the radius pass (k_radius_gemm): train norms, tile statistics and their
    // maxima, train tile blocks of 64 rows, the train norms' share of the status word; query norms,
    // statistics and operand rows; the exact-evaluation counter (profile = 2).  Buffers and a cache
    // key of their own (tprep's rule: the train view, the generation, the upload epoch) -- run_gemm
    // trusts tnorm / tmax / tblk / tctrl across calls, so the radius pass never writes them.
    DBuf rm_tnorm, rm_tmax, rm_tsmax, rm_tblk, rm_tctrl, rm_qnorm, rm_qstat, rm_qop, rm_exact;
    struct { const void* feat; int64_t n; int d, ld, dtype; uint64_t gen, epoch; bool valid; }
        rmprep{nullptr, 0, 0, 0, 0, 0, 0, false};
    bool rm_counted = false;  // the last radius pass counted into rm_exact
    DBuf arrive;              // k_direct_rows' fused merge: per query group, segments finished
    bool arrive_clean = false;  // arrive is all zero (the last launch ran to completion)
    // host-buffer calls (knn_predict): cached train upload, two query slots streamed on a copy stream
    int cache_train = 0;
    uint64_t generation = 0;
    struct { const void* feat; const int32_t* labels; int64_t n; int d, ld, dtype, ldd; uint64_t gen; bool valid; }
        tcache{nullptr, nullptr, 0, 0, 0, 0, 0, 0, false};
    hipStream_t cstream = nullptr;
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr}, ev_down[2] = {nullptr, nullptr};
    DBuf q_slot[2], pred_slot[2], dist_slot[2], idx_slot[2];
    std::vector<int32_t*> ctrl_slots;  // pinned copies of the status word, one per batch
    int64_t batch_rows = 131072;       // queries per streamed batch of a host-buffer call
    int64_t ws_queries = 1 << 22;      // GEMM-path queries per pass (candidate workspace budget)
    int64_t h2d_train = 0, h2d_query = 0;
    // profiling
    std::vector<hipEvent_t> events;
    std::vector<Stage> stages;
    bool stage_open = false;  // the last stage_begin recorded an event (profile = 3 skips some)
    std::vector<float> stage_ms;
    std::vector<const char*> stage_names;
    int64_t stats[22] = {0, 0, 0, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // candidates, fallback queries, segments, filter
                                                      // operand type, rerun, fused, train / query H2D
                                                      // bytes, train-side filter operands from the cache,
                                                      // MFMA form, queries per wave, [11] the filter's
                                                      // operand element (0: the data's / bf16, 1: int8),
                                                      // [12] records parked by the last pass's filter
                                                      // (profile = 2 only, like the candidates),
                                                      // [13] the radius pass's form (0 direct, 1 MFMA,
                                                      // 2 direct because of unsafe norms), [14] the
                                                      // pairs its MFMA form evaluated exactly
                                                      // (profile = 2 only), [18] DBSCAN's border
                                                      // candidates, [19] its successful unions
                                                      // (profile = 2 only), [20] the spanning
                                                      // tree's rounds, [21] the rows its rounds
                                                      // sent through distance passes
    int64_t rerun_stats[4] = {0, -1, 0, 0};  // segments, operand type, fused, operand width of AUTO's gated split re-run
    int num_cus = 256;
};

namespace {

knn_status fail(knn_ctx* c, knn_status s, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
knn_status fail(knn_ctx* c, knn_status s, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return s;
}

#define HIP_OR_FAIL(ctx, expr)                                                                  \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return fail(ctx, e__ == hipErrorOutOfMemory ? KNN_ENOMEM : KNN_EHIP, "%s: %s (%s:%d)", \
                        #expr, hipGetErrorString(e__), __FILE__, __LINE__);                    \
    } while (0)

// HIP_OR_FAIL inside a host-buffer call's enqueue phase (knn_predict, lists_host): drain and
// invalidate first (abort_call)
#define HIP_OR_ABORT(expr)                                                                     \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return abort_call(fail(c, e__ == hipErrorOutOfMemory ? KNN_ENOMEM : KNN_EHIP,       \
                                   "%s: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__)); \
    } while (0)

// profiling helpers: events are created lazily and reused across calls
// profile = 3: events only around the dominant kernels' stages.  Each event costs the
// stream a few microseconds: with every stage timed, A's 8-GPU share (12,500 queries) ran
// 3.44 -> 3.56 ms per step, A 22.58 -> 22.73 (scripts/event_overhead.py, profiles/r04n).
static bool hot_stage(const char* n) {
    static const char* const hot[] = {"gemm_filter", "rescore", "direct_tile", "metric_tile", "exact_scan", "merge_vote",
                                      "exchange", "radius_count", "radius_fill", "radius_sweep", "dbscan_link",
                                      "dbscan_border", "dbscan_sweep_link", "dbscan_sweep_border", "mst_pass"};
    for (const char* h : hot)
        if (!strcmp(n, h)) return true;
    return false;
}
void stage_begin(knn_ctx* c, hipStream_t st, const char* name) {
    c->stage_open = false;
    if (!c->profile || (c->profile == 3 && !hot_stage(name))) return;
    size_t i = c->stages.size();
    while (c->events.size() < 2 * (i + 1)) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        c->events.push_back(e);
    }
    Stage s{name, c->events[2 * i], c->events[2 * i + 1]};
    c->stages.push_back(s);
    (void)hipEventRecord(s.a, st);
    c->stage_open = true;
}
void stage_end(knn_ctx* c, hipStream_t st) {
    if (!c->profile || c->stages.empty() || !c->stage_open) return;
    c->stage_open = false;
    (void)hipEventRecord(c->stages.back().b, st);
}

int elem_size(int dtype) { return dtype == KNN_BF16 ? 2 : 4; }

knn_status check_dataset(knn_ctx* c, const knn_dataset* x, const char* what, bool need_labels) {
    if (!x) return fail(c, KNN_EINVAL, "%s dataset is NULL", what);
    if (x->n < 0) return fail(c, KNN_EINVAL, "%s: n < 0", what);
    if (x->d <= 0) return fail(c, KNN_EINVAL, "%s: d must be > 0", what);
    if (x->ld < x->d) return fail(c, KNN_EINVAL, "%s: ld < d", what);
    if (x->dtype != KNN_F32 && x->dtype != KNN_BF16)
        return fail(c, KNN_EINVAL, "%s: dtype must be KNN_F32 or KNN_BF16", what);
    if (x->n > 0 && !x->feat) return fail(c, KNN_EINVAL, "%s: feat is NULL", what);
    if (need_labels && x->n > 0 && !x->labels) return fail(c, KNN_EINVAL, "%s: labels are NULL", what);
    return KNN_OK;
}

// AUTO and the int8 operand class (DESIGN.md "int8 filter operands"): whether AUTO takes it where
// it can run, and the largest ratio E8 / Ebf of the train set's row residuals under the int8 and
// the bf16 rounding at which it still does (the guard against a scale set by outliers).  Measured
// on A's rows by coarsening the int8 step (profiles/r08_studies): against gemm_bf16's 19.0 ms per
// step, ratio 2.5 (the rule's own step) runs 14.2, 3.1 (x1.25) 14.8, 3.7 (x1.5) 15.6, 4.3 (x1.75)
// 16.2 -- still 15 % under -- and 5.0 (x2) 17.6 at best, 19.4 in the median: under 10 %.  R is the
// largest measured ratio that keeps the 10 %.
static constexpr bool KNN_AUTO_I8 = true;
static constexpr float KNN_I8_AUTO_R = 4.3f;

// filter operand type of a GEMM-path call: fp32 data runs split (ELEM_SPLIT, bf16 hi/lo
// rows of 4d bytes) under KNN_ALGO_GEMM_SPLIT, rounded (ELEM_ROUND, bf16 rows of 2d bytes)
// under KNN_ALGO_GEMM_BF16, else the data's own type.  KNN_ALGO_GEMM_I8 is the rounded class too
// (fp32 rows rounded once to a narrow MFMA operand): run_gemm rounds to int8 where the int8 form
// can run and to bf16 where it cannot, and reports which in stats[11]
int filter_elem(int algo, int dtype) {
    if (dtype != KNN_F32) return dtype;
    return algo == KNN_ALGO_GEMM_SPLIT ? ELEM_SPLIT
         : (algo == KNN_ALGO_GEMM_BF16 || algo == KNN_ALGO_GEMM_I8) ? ELEM_ROUND : dtype;
}
int filter_row_bytes(int felem, int d) {
    return felem == ELEM_SPLIT ? 4 * d : felem == ELEM_ROUND ? 2 * d : d * elem_size(felem);
}
// Operand width of the filter, separate from the caller's row width d.  The bf16 operand classes
// (rounded fp32 rows, bf16 data) build their own operand rows (k_tn_rows, k_round_rows), so a row of
// any d <= 256 is padded with zero columns to the next of the filter's tile widths 64 / 128 / 256,
// and a row of 256 < d <= 4096 to the next multiple of 128, the chunk of the K-chunked kernel
// (k_gemm_wide, knn_wide_width): zero products add nothing to the MFMA chain, and norms,
// statistics, the rescore and the fallback keep the true rows.  The fp32 and split classes read
// the caller's rows (or their [hi | lo] image) at their own width: they keep d.  0: no filter at
// this width.
int filter_width(int felem, int d) {
    if (felem == ELEM_ROUND || felem == ELEM_BF16)
        return d <= 64 ? 64 : d <= 128 ? 128 : d <= 256 ? 256 : knn_wide_width(d);
    return d;
}
// whether operands of that class and width run k_gemm_wide (chunks of 128 features)
bool is_wide(int felem, int dp) { return (felem == ELEM_ROUND || felem == ELEM_BF16) && dp > 256; }
// AUTO's split re-run (predict_enqueue) builds [hi | lo] operands of its own, so it pads like the
// rounded pass it follows; the split kernel has rows of 4 dp <= 512 bytes.  0: no split form.
int split_rerun_width(int d, int k) {
    const int dp = d <= 32 ? 32 : d <= 64 ? 64 : d <= 128 ? 128 : 0;
    return dp > 0 && knn_gemm_filter_lds(ELEM_SPLIT, 4 * dp, k) <= 160 * 1024 ? dp : 0;
}
bool is_gemm(int algo) {
    return algo == KNN_ALGO_GEMM || algo == KNN_ALGO_GEMM_SPLIT || algo == KNN_ALGO_GEMM_BF16 ||
           algo == KNN_ALGO_GEMM_I8;
}

// ctx_algo / metric: the context's (knn_filter_policy asks without one)
int choose_algo(int ctx_algo, int metric, int64_t nt, int64_t nq, int d, int k, int dtype) {
    // a non-Euclidean metric has the direct form only (k_metric_tile), whatever the shape
    if (metric != KNN_METRIC_SQEUCLIDEAN) return KNN_ALGO_DIRECT;
    if (ctx_algo == KNN_ALGO_DIRECT || ctx_algo == KNN_ALGO_DIRECT_SCAN) return ctx_algo;
    // the LDS-DMA filter stages whole operand rows: a row must be one of its tile widths
    // (128, 256 or 512 bytes: fp32 d = 32/64/128 (fp32 or split); the bf16 operands, which the
    // library builds itself, any d <= 256 padded to 64/128/256 and any d <= 4096 in chunks of
    // 128 -- filter_width)
    auto gemm_ok = [&](int algo) {
        const int fe = filter_elem(algo, dtype), dp = filter_width(fe, d);
        if (dp <= 0) return false;
        if (is_wide(fe, dp)) return k <= 128 && k <= nt && knn_wide_plan(k).lds <= 160 * 1024;  // k_gemm_wide
        const int rb = filter_row_bytes(fe, dp);
        return knn_gemm_filter_supported(fe, rb) && k <= 128 && k <= nt &&
               knn_gemm_filter_lds(fe, rb, k) <= 160 * 1024;
    };
    if (is_gemm(ctx_algo))
        return gemm_ok(ctx_algo) ? ctx_algo : KNN_ALGO_DIRECT;
    // AUTO: the direct form wins at low d (3 VALU ops per dim, no rescore) and on small jobs;
    // above that the rounded bf16 filter (one MFMA per 16 features), re-run as split when
    // its wider certificate overflows the candidate lists (predict_core).  For the fused
    // filter's widths (d = 64, 128, 256) "small" now means under 16k rows (round 6, with the
    // small-set pieces): same box, ms per call direct -> filter, d = 128 (rows x queries): 1M x 1
    // 11.7 -> 0.78, 1M x 64 13.0 -> 0.87, 100k x 100 1.07 -> 0.27, 30k x 300 0.41 -> 0.26, 100k x
    // 1000 1.38 -> 0.35, 1M x 500 8.72 -> 1.07; d = 64, k = 32: 50k x 200 0.61 -> 0.37, 100k x
    // 2000 2.51 -> 0.49; 20k x 150 0.29 either way; at 10k rows the two are equal (0.21-0.26)
    // and the direct form wins at d = 64, k = 32 (0.25 vs 0.31; profiles/r06_studies/r06au).
    // Other widths keep the 10^9-pair rule: a padded row pays its operand width's MFMA work and
    // the direct form the true d's, so the rule that holds at 64/128/256 on 10^9 pairs is kept for
    // the widths between them and beyond (DESIGN.md "Any row width").  At the rule's edge, 32,768 x
    // 32,768, k = 10, same box, direct -> filter: d = 96 (padded to 128) 10.09 -> 0.93 ms, d = 768
    // (k_gemm_wide) 125.2 -> 4.63 ms (profiles/wide_rows.json): no floor raised for either class.
    const double pairs = (double)nt * (double)nq;
    if (d >= 32 && nt >= 8192 && (pairs >= 1e9 || (knn_fused_supported(d) && nt >= 16384))) {
        // fp32 rows at d = 128, k <= 32: the int8 operand class (half
        // the MFMA work per feature), which run_gemm takes when the train set's range allows it
        // (finite, E8 <= R Ebf, not demoted) and otherwise runs as the bf16 operands
        if (gemm_ok(KNN_ALGO_GEMM_BF16))
            return KNN_AUTO_I8 && dtype == KNN_F32 && d == 128 && k <= 32
                       ? KNN_ALGO_GEMM_I8 : KNN_ALGO_GEMM_BF16;
        if (gemm_ok(KNN_ALGO_GEMM_SPLIT)) return KNN_ALGO_GEMM_SPLIT;
        if (gemm_ok(KNN_ALGO_GEMM)) return KNN_ALGO_GEMM;
    }
    return KNN_ALGO_DIRECT;
}
int choose_algo(const knn_ctx* c, int64_t nt, int64_t nq, int d, int k, int dtype) {
    return choose_algo(c->algo, c->metric, nt, nq, d, k, dtype);
}

// per-stage times of the drained stream (profile mode)
void collect_stages(knn_ctx* c) {
    if (!c->profile) return;
    c->stage_ms.clear();
    c->stage_names.clear();
    for (auto& s : c->stages) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, s.a, s.b);
        c->stage_ms.push_back(ms);
        c->stage_names.push_back(s.name);
    }
}

knn_status check_status(knn_ctx* c, const int32_t* ctrl) {
    const int32_t status = ctrl[0];
    if (status & KNN_STATUS_UF_LIMIT)
        return fail(c, KNN_EHIP, "dbscan: internal error: a union-find loop reached its iteration cap");
    if (status & KNN_STATUS_BAD_LABEL) return fail(c, KNN_EINVAL, "a train label is outside [0, num_classes)");
    if (status & KNN_STATUS_UNSORTED)
        return fail(c, KNN_EINVAL, "merge: a source neighbour list is not ascending by (distance, index)");
    if (status & KNN_STATUS_BAD_DIST) return fail(c, KNN_EINVAL, "weighted vote: a neighbour distance is NaN or negative");
    if (status & KNN_STATUS_BAD_OFFSETS) return fail(c, KNN_EINVAL, "radius: the offsets do not belong to this call");
    if (status & KNN_STATUS_BAD_INDEX) return fail(c, KNN_EINVAL, "radius: a list index is outside [0, n_train)");
    if (status & KNN_STATUS_TOO_FEW) return fail(c, KNN_ERANGE, "fewer than k train rows have a finite distance (< FLT_MAX)");
    return KNN_OK;
}

// the one host synchronisation of a call: k_finish writes the status words to the host's
// mapped copy and zeroes them for the next call, then the stream drains.  The host first spins
// (up to 200 us) on the sequence word k_finish writes last: a short call returns ~6 us sooner
// than through hipStreamSynchronize, whose completion signal costs ~12 us per wait even for a
// finished stream (scripts/diag/sync_latency.hip, profiles/r06_studies/r06sync.log).  Longer
// calls, and profile mode (its events are read through the runtime), end in the stream sync.
knn_status finish_call(knn_ctx* c, hipStream_t st) {
    const uint32_t seq = ++c->finish_seq;
    HIP_OR_FAIL(c, knn_launch_finish(c->ctrl.as<int32_t>(), c->ctrl_host_dev, 4, seq, st));
    bool done = false;
    if (!c->profile) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int spin = 0;; spin++) {
            if ((uint32_t)__atomic_load_n(c->ctrl_host + 4, __ATOMIC_ACQUIRE) == seq) {
                done = true;
                break;
            }
            if ((spin & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200)) break;
            __builtin_ia32_pause();  // (x86-64 host: yield the core's pipeline to its sibling thread)
        }
    }
    if (!done) HIP_OR_FAIL(c, hipStreamSynchronize(st));
    c->ctrl_clean = true;
    c->arrive_clean = true;  // every query group's merging wave reset its counter
    collect_stages(c);
    return check_status(c, c->ctrl_host);
}
// a call's first enqueue: the status words start at zero (k_finish left them so, unless the last
// call failed before it ran)
hipError_t reset_ctrl(knn_ctx* c, hipStream_t st) {
    const bool clean = c->ctrl_clean;
    c->ctrl_clean = false;
    return clean ? hipSuccess : hipMemsetAsync(c->ctrl.p, 0, 4 * sizeof(int32_t), st);
}

// k_direct_tile segments: enough (query block, segment) units to fill whole waves of
// resident blocks (more segments only when they raise the filled fraction by > 2 %, each
// one costs a merge pass), at least 4 tiles per segment, records within 2 GB
// (rec_bytes: workspace bytes per query and segment; nqb query blocks over `slots` resident blocks)
int fill_segments(int64_t nt, int64_t nq, int64_t nqb, int64_t slots, double rec_bytes) {
    int best = 1;
    double best_eff = 0.0;
    for (int s = 1; s <= 32; s++) {
        if (s > 1 && nt / s < 256) break;
        if (s > 1 && (double)s * (double)nq * rec_bytes > 2e9) break;
        const int64_t w = nqb * s;
        const double eff = (double)w / (double)(((w + slots - 1) / slots) * slots);
        if (eff > best_eff + 0.02) { best = s; best_eff = eff; }
    }
    return best;
}

int choose_direct_segments(const knn_ctx* c, int64_t nt, int64_t nq, int d, int k, int C, int elem) {
    int qb = 1, occ = 1;
    // (a metric has no rows form: its units are k_metric_tile's blocks for every shape)
    const bool metric = c->metric != KNN_METRIC_SQEUCLIDEAN;
    if ((metric ? knn_metric_units(c->metric, k, elem, d, C, &qb, &occ) : knn_direct_units(k, elem, d, C, &qb, &occ)) !=
            hipSuccess ||
        occ < 1)
        occ = 1;
    const int64_t nqb = (nq + qb - 1) / qb;
    const int64_t slots = (int64_t)occ * c->num_cus;
    if (!metric && qb < knn_direct_tile_qb(k)) {
        // k_direct_rows (a wave per unit): about one round of resident waves -- its waves need
        // no co-residents to hide a barrier, and every segment adds a sorted first tile and a
        // merge source (config L, 859 query pairs, same box: 4 segments 0.092 ms, 5 0.094, 8
        // 0.089, 12 0.097, 16 0.103, 32 0.131; r05y)
        const int64_t want = (slots + nqb / 2) / nqb;
        int64_t s = std::max<int64_t>(1, std::min<int64_t>(want, 32));
        while (s > 1 && nt / s < 256) s--;
        while (s > 1 && (double)s * (double)nq * 12.0 * k > 2e9) s--;
        return (int)s;
    }
    return fill_segments(nt, nq, nqb, slots, 12.0 * k);
}

// k_radius_tile segments: the same rule from that kernel's own blocks per CU (64 queries a block;
// 12 bytes of counts and bases per query and segment)
int choose_radius_segments(const knn_ctx* c, int64_t nt, int64_t nq, int d, int C, int elem) {
    int qb = 64, occ = 1;
    if (knn_radius_units(c->metric, elem, d, C, &qb, &occ) != hipSuccess || occ < 1) occ = 1;
    return fill_segments(nt, nq, (nq + qb - 1) / qb, (int64_t)occ * c->num_cus, 12.0);
}

// the direct form over the whole query set: k_direct_tile (+ k_merge_vote of its segments)
knn_status run_direct_tile(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int k, int C,
                           const QueryOut& out, hipStream_t st) {
    DirectTileArgs a{};
    a.train = tr->feat; a.labels = tr->labels; a.nt = tr->n; a.ld_t = tr->ld;
    a.test = te->feat; a.ld_q = te->ld; a.nq = te->n;
    a.d = tr->d; a.k = k; a.C = C; a.elem = tr->dtype;
    a.status = c->ctrl.as<int32_t>();
    const int nseg = c->train_splits > 0 ? std::min(32, c->train_splits)
                                         : choose_direct_segments(c, tr->n, te->n, tr->d, k, C, tr->dtype);
    a.nseg = nseg;
    a.seg_len = (tr->n + nseg - 1) / nseg;
    c->stats[2] = nseg;
    if (nseg == 1) {
        a.out = out;
        HIP_OR_FAIL(c, knn_launch_direct_tile(a, st));
        return KNN_OK;
    }
    HIP_OR_FAIL(c, c->seg_rec.ensure(sizeof(int32_t) * 3 * (size_t)k * (size_t)te->n * nseg));
    a.rec = c->seg_rec.as<int32_t>();
    if (knn_direct_rows_shape(k, tr->d)) {
        // k_direct_rows merges its segments itself (the last wave of a query group to finish):
        // one launch, no k_merge_vote pass (config L: 0.012 ms of merge + a launch, round 6)
        const int64_t groups = knn_direct_rows_groups(te->n);
        const void* before = c->arrive.p;
        const size_t had = c->arrive.bytes;
        HIP_OR_FAIL(c, c->arrive.ensure(sizeof(int32_t) * (size_t)groups));
        // (a grown buffer may come back at the old address: its new tail is not zero yet)
        if (c->arrive.p != before || c->arrive.bytes != had) c->arrive_clean = false;
        if (!c->arrive_clean) HIP_OR_FAIL(c, hipMemsetAsync(c->arrive.p, 0, c->arrive.bytes, st));
        c->arrive_clean = false;  // (set again when the call's stream synchronises)
        a.arrive = c->arrive.as<int32_t>();
        a.out = out;
        HIP_OR_FAIL(c, knn_launch_direct_tile(a, st));
        return KNN_OK;
    }
    HIP_OR_FAIL(c, knn_launch_direct_tile(a, st));
    // (the merge is its own stage: "direct_tile" times the distance kernel alone)
    stage_end(c, st);
    stage_begin(c, st, "merge_vote");
    MergeArgs m{};
    m.rec = a.rec; m.nsrc = nseg; m.nq = te->n; m.k = k; m.C = C;
    m.out = out; m.status = a.status; m.labels = tr->labels;
    HIP_OR_FAIL(c, knn_launch_merge(m, st));
    return KNN_OK;
}

// the direct form under a non-Euclidean metric: k_metric_tile (+ k_merge_vote of its segments,
// sized from this kernel's units); never the rows form or its arrival counters
knn_status run_metric_tile(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int k, int C,
                           const QueryOut& out, hipStream_t st) {
    DirectTileArgs a{};
    a.train = tr->feat; a.labels = tr->labels; a.nt = tr->n; a.ld_t = tr->ld;
    a.test = te->feat; a.ld_q = te->ld; a.nq = te->n;
    a.d = tr->d; a.k = k; a.C = C; a.elem = tr->dtype;
    a.status = c->ctrl.as<int32_t>();
    const int nseg = c->train_splits > 0 ? std::min(32, c->train_splits)
                                         : choose_direct_segments(c, tr->n, te->n, tr->d, k, C, tr->dtype);
    a.nseg = nseg;
    a.seg_len = (tr->n + nseg - 1) / nseg;
    c->stats[2] = nseg;
    if (nseg == 1) {
        a.out = out;
        HIP_OR_FAIL(c, knn_launch_metric_tile(a, c->metric, st));
        return KNN_OK;
    }
    HIP_OR_FAIL(c, c->seg_rec.ensure(sizeof(int32_t) * 3 * (size_t)k * (size_t)te->n * nseg));
    a.rec = c->seg_rec.as<int32_t>();
    HIP_OR_FAIL(c, knn_launch_metric_tile(a, c->metric, st));
    stage_end(c, st);
    stage_begin(c, st, "merge_vote");
    MergeArgs m{};
    m.rec = a.rec; m.nsrc = nseg; m.nq = te->n; m.k = k; m.C = C;
    m.out = out; m.status = a.status; m.labels = tr->labels;
    HIP_OR_FAIL(c, knn_launch_merge(m, st));
    return KNN_OK;
}

// one k_exact_scan block per query: KNN_ALGO_DIRECT_SCAN over every query, or the GEMM
// path's fallback over a device-side query list (qlist / qcount)
knn_status run_exact_scan(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int k, int C,
                          const QueryOut& out, hipStream_t st, const int32_t* qlist, const int32_t* qcount) {
    ExactScanArgs a{};
    a.train = tr->feat; a.labels = tr->labels; a.nt = tr->n; a.ld_t = tr->ld;
    a.test = te->feat; a.ld_q = te->ld; a.nq = te->n;
    a.d = tr->d; a.k = k; a.C = C; a.elem = tr->dtype;
    a.qlist = qlist; a.qcount = qcount;
    a.out = out; a.status = c->ctrl.as<int32_t>();
    const int grid = qlist ? std::max(1, 2 * c->num_cus) : (int)std::min<int64_t>(te->n, 16384);
    if (grid <= 0) return KNN_OK;
    HIP_OR_FAIL(c, knn_launch_exact_scan(a, grid, st));
    return KNN_OK;
}

// GEMM-form certificate constants: Delta = coef*(qn+tn) + eta, u = 2^-24.
//   fp32 MFMA (an exact fmaf chain):  coef = (4d+32) u, eta = (6d+8) 2^-149
//   bf16 MFMA (products exact; internal sums assumed no worse than 2u per add, and
//   denormal results possibly flushed):  coef = (6d+32) u, eta = (6d+8) 2^-125
//   split (fp32 x = hi + lo + r, |r| <= 2^-16 |x| (+2^-134); q.t ~ hi.hi + hi.lo + lo.hi
//   on the bf16 MFMA): the dropped terms lo.lo, (hi+lo) r_t, r_q (hi+lo) give
//   <= 3.04 2^-16 sum|q_i t_i| <= 1.52 2^-16 N (N = qn + tn), i.e. <= 779 u N in G; the
//   accumulation of 3d exact products at 2u per add gives <= 6.1 d u N in G; the norm
//   and final-rounding terms are the fp32 ones, (3d+32) u N.  Flushed subnormal operands
//   (<= 2^-126 |t_i| each, <= (1+N)/2 2^-126 by |t_i| <= (1+t_i^2)/2) add <= 3.1 d 2^-126
//   (1+N).  coef = (10d + 840) u, eta = (8d+8) 2^-125.
//   rounded (fp32 x -> bf16 rn(x), |rn(x) - x| <= 2^-8 |x| (+2^-134)): each product moves by
//   <= (2^-7 + 2^-16) |q_i t_i|, in sum <= (2^-7 + 2^-16) N/2, i.e. <= 131328 u N in G; the
//   accumulation of d exact products at 2u per add gives <= 2.02 d u N in G; norm and final
//   roundings (3d+32) u N; L/U/Delta roundings and slack within 512 u N.  Flushed or
//   subnormal operands as for split.  coef = (6d + 131840) u, eta = (8d+8) 2^-125.
void certificate(int d, int felem, float* coef, float* eta) {
    if (felem == ELEM_ROUND) {
        *coef = (float)(6 * d + 131840) * 0x1p-24f;
        *eta = (float)(8 * d + 8) * 0x1p-125f;
    } else if (felem == ELEM_SPLIT) {
        *coef = (float)(10 * d + 840) * 0x1p-24f;
        *eta = (float)(8 * d + 8) * 0x1p-125f;
    } else if (felem == KNN_BF16) {
        *coef = (float)(6 * d + 32) * 0x1p-24f;
        *eta = (float)(6 * d + 8) * 0x1p-125f;
    } else {
        *coef = (float)(4 * d + 32) * 0x1p-24f;
        *eta = (float)(6 * d + 8) * 0x1p-149f;
    }
}

// Fused-norm filter (knn_fused.hip): y = fl_mfma(tn + sum -2 rq_i rt_i) -- the fp32 norm from
// the tile block's header is the first MFMA's C operand, every d (the coefficient still covers
// the round-2 layout's three-term split of the norm over an augmented k-step, + tn_hi + tn_mid +
// tn_lo), G = fl(qn + y), Delta = coef (qn +
// tn) + eta; rq, rt = the bf16 operands (q, t themselves for bf16 data, rn(q), rn(t) for fp32
// data).  With N = qn + tn (exact norms):
//   MFMA accumulation of d + 3 terms (d + 1 with the C-operand norm) at <= 2u per add, terms
//   summing to <= 2.01 N: 4.02 (d+3) u N
//   tn split hi + mid + lo (each subtraction exact): <= 2^-24 tn <= u N (0 with the C operand)
//   fp32 norms (fmaf chains): <= 1.01 d u each, 2.02 d u N;  G's rounding: <= 3.01 u N
//   the reference's D vs the exact distance: <= 2 (d+2) u N
// -> (8.04 d + 20.1) u N; the roundings of s, coef s, L and U and slack in 512 u N:
//   coef = (9d + 512) u.
// Rounded fp32 data adds the operand rounding, exactly 2 (q.t - rq.rt) = 2 (q.(t - rt) +
// (q - rq).rt), bounded by Cauchy-Schwarz with the row statistics of k_row_norms:
//   |.| <= 2 (|q| |t - rt| + |q - rq| |rt|)   (rq = rn(-2q) / -2, rt = rn(t))
// -- per (query, 64-row tile) with the tile's maxima, added to Delta by the kernel (tq.y).
// For random rounding errors it is ~2.6x tighter than the worst case (2^-7 + 2^-16) N
// (the round-1 coefficient 131328 u); for bf16 data it is 0.  (The terms of the MFMA
// sum stay <= 2.01 N: |rq_i rt_i| <= (1 + 2^-8)^2 |q_i t_i|.)
// eta (products or partial sums flushed to zero, subnormal operand rounding): (8d + 16) 2^-125.
void certificate_fused(int d, bool /*rounded*/, float* coef, float* eta) {
    *coef = (float)(9 * d + 512) * 0x1p-24f;
    *eta = (float)(8 * d + 16) * 0x1p-125f;
}

// the most train segments (or schedule pieces) per query tile, at most smax, whose expected
// kept rows fit their slice of the candidate list (choose_splits' rule)
int max_splits(int64_t nt, int k, int cap, int smax = 8) {
    int best = 1;
    for (int s = 2; s <= smax; s++) {
        const double rows = (double)nt / s;
        const double expect = k * (1.0 + std::log(std::max(rows / k, 1.0))) + 64.0;
        if (1.5 * (0.5 * expect + 32.0) > (double)(cap / s / 2)) break;
        best = s;
    }
    return best;
}

int choose_splits(const knn_ctx* c, int64_t n_qtiles, int64_t nt, int dtype, int rb, int k, int cap,
                  bool fused = false, int d = 0, const FilterPlan* fplan = nullptr, int smax = 8, bool wide = false) {
    if (c->train_splits > 0) return std::min(8, c->train_splits);
    // More segments shrink the partial last wave of blocks (measured on config A:
    // S=3 224 ms, S=5 217 ms, S=8 216 ms), but each segment must fit its rows in its
    // slice of the candidate list: a running k-smallest threshold keeps about
    // k (1 + ln(rows / k)) rows (the expected number of records) plus a 64-row warm-up
    // tile; the slice gets a 1.5x margin.  Overflowing queries still finish exactly,
    // on the slow full-scan fallback.
    int occ = 1;
    const hipError_t oe = fused ? knn_fused_occupancy(d, *fplan, &occ)
                        : wide ? knn_wide_occupancy(k, &occ) : knn_gemm_filter_occupancy(dtype, rb, k, &occ);
    if (oe != hipSuccess || occ < 1) occ = 1;
    const int64_t slots = (int64_t)occ * c->num_cus;
    int best = 1;
    double best_eff = 0.0;
    for (int s = 1; s <= smax; s++) {
        const double rows = (double)nt / s;
        if (s > 1 && rows < 64 * 64) break;
        const double expect = k * (1.0 + std::log(std::max(rows / k, 1.0))) + 64.0;
        // each lane half of a query fills its own half of the slice with about half the rows
        if (s > 1 && 1.5 * (0.5 * expect + 32.0) > (double)(cap / s / 2)) break;
        const int64_t w = n_qtiles * s;
        const double eff = (double)w / (double)(((w + slots - 1) / slots) * slots);
        if (eff >= best_eff) { best = s; best_eff = eff; }
    }
    return best;
}

// The GEMM pipeline of one filter operand type, enqueued on st with no host round trip (one
// exception: a call that builds the int8 operand class's train operands reads the train set's
// scale back first -- a stream synchronisation, once per cached train set or per forced call):
// norms -> operand rows -> filter -> rescore (queries whose candidate list overflowed, or
// every query when a norm is too large for the certificate, go to the fallback list).
// gate (optional): every stage runs only when *gate != 0 (AUTO's re-run, decided on the
// device by k_rerun_decide).  The fallback scan is enqueued by the caller.
knn_status run_gemm(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int k, int C,
                    const QueryOut& out, hipStream_t st, int algo, const int32_t* gate) {
    const int64_t nt = tr->n, nq = te->n;
    const int d = tr->d;
    const int dtype = tr->dtype;
    const int felem = filter_elem(algo, dtype);  // the filter's operand type
    // the operand rows' width (filter_width: d padded with zero columns for the bf16 operands).
    // Norms, statistics, the rescore and the fallback below keep the caller's rows and d.
    const int dp = felem == ELEM_SPLIT && gate ? split_rerun_width(d, k) : filter_width(felem, d);
    const bool wide = is_wide(felem, dp);  // k_gemm_wide: rows in chunks of 128 features
    if (dp < d) return fail(c, KNN_EINVAL, "no filter operands at d=%d", d);  // (choose_algo never sends one)
    const int rb = filter_row_bytes(felem, dp);
    const int kelem = felem == ELEM_ROUND ? ELEM_BF16 : felem;  // ELEM_ROUND runs the bf16 kernel
    // Small query sets (round 6): when the base list's pieces would leave CUs idle (256-query
    // tiles x max_splits pieces under 80 % of the CUs -- a 3,125-query call on A's rows ran 13
    // tiles x 5 pieces on 256 CUs), a candidate list 2-4x as long per query, so the filter may
    // cut each query tile into up to 16 pieces (32 candidate sub-slices; 32 pieces for the tiny
    // sets below, 64 sub-slices, k_rescore's limit).  The
    // workspace stays within 1.5 GiB.  The queries-per-wave choice (knn_fused_plan) still
    // counts the base list's pieces: 64-query waves cut into more than ~5 pieces lost to the
    // 32-query shape (A's rows, 6,250 queries: 2.06 against 1.84 ms, r06bh).
    const size_t per_q = 12 * 64 * (size_t)KNN_RESCORE_CAPW, ws_lim = (size_t)1536 << 20;
    const bool idle = (nq + 255) / 256 * (int64_t)max_splits(nt, k, 64 * KNN_RESCORE_CAPW) * 5 < (int64_t)4 * c->num_cus;
    // (a handful of query tiles, idle even at 16 pieces each -- 1,000 queries: 4 tiles -- gets
    // an 8x list and up to 32 pieces, 64 sub-slices)
    const bool tiny = idle && (nq + 255) / 256 * 16 * 5 < (int64_t)4 * c->num_cus;
    const int capmul = !idle ? 1
                     : tiny && (size_t)nq * per_q * 8 <= ws_lim ? 8
                     : (size_t)nq * per_q * 4 <= ws_lim ? 4
                     : (size_t)nq * per_q * 2 <= ws_lim ? 2 : 1;
    const int cap = 64 * KNN_RESCORE_CAPW * capmul;
    const int smax = capmul == 8 ? 32 : capmul > 1 ? 16 : 8;
    // (k_row_norms writes +inf into rows [nt, nt + 64); the wide filter's 256-row groups read up to
    // 255 rows past nt: the rest of that range is filled below)
    const int wgr = knn_wide_group_rows();
    HIP_OR_FAIL(c, c->tnorm.ensure(sizeof(float) * (nt + 64 + wgr)));
    HIP_OR_FAIL(c, c->tnp.ensure(sizeof(float) * (nt + 64 + wgr)));
    HIP_OR_FAIL(c, c->qnorm.ensure(sizeof(float) * nq));
    HIP_OR_FAIL(c, c->gthr.ensure(sizeof(uint32_t) * nq));
    HIP_OR_FAIL(c, c->cnt.ensure(sizeof(int32_t) * nq * 64));  // [subs * nseg][nq], subs * nseg <= 64
    HIP_OR_FAIL(c, c->cand.ensure(sizeof(CandRec) * nq * cap));
    HIP_OR_FAIL(c, c->fb_list.ensure(sizeof(int32_t) * nq));

    // bf16 MFMA operands (rounded fp32 rows or bf16 data) run the fused-norm filter
    // the fused filter's plan, computed once: it sizes the tile blocks (bn_f), the occupancy,
    // the schedule and the launch of this pass
    // The int8 operand class (KNN_ALGO_GEMM_I8, fp32 data): taken when its plan exists (d = 128,
    // k <= 32) and the train set's range allows it; else this call runs
    // the bf16 operands below unchanged.  own_train / may_cache: as for tprep below.
    // AUTO takes the class only for a train set whose operands this context keeps (may_cache):
    // the scale, the guard's statistics and the demotion mark live with that cache.  Without it
    // every call would pay the scale's host round trip and the statistics passes again, and a
    // train set the guard misjudges could never be demoted -- so such calls run the bf16
    // operands exactly as before.  A forced context (KNN_ALGO_GEMM_I8) is not restricted.
    float i8s = 0.0f;
    FilterPlan iplan{};
    if (algo == KNN_ALGO_GEMM_I8 && dtype == KNN_F32 && !gate && knn_fused_supported(d) &&
        (c->algo != KNN_ALGO_AUTO || (c->cache_train && (tr->feat == c->h_train.p || c->cache_train_device)))) {
        const bool own = tr->feat == c->h_train.p;
        const bool mayc = c->cache_train && (own || c->cache_train_device);
        const uint64_t ep = own ? c->train_epoch : 0;
        auto& ic = c->i8c;
        const bool hit = mayc && ic.valid && ic.feat == tr->feat && ic.n == nt && ic.d == d && ic.ld == tr->ld &&
                         ic.gen == c->generation && ic.epoch == ep;
        // (a cached train set the class does not take costs a call nothing more than this test)
        if (!(hit && (!ic.ok || (ic.demoted && c->algo == KNN_ALGO_AUTO)))) {
            iplan = knn_fused_plan(d, k, nq, c->num_cus, c->fforce, max_splits(nt, k, 64 * KNN_RESCORE_CAPW), true);
            if (iplan.nw > 0 && !knn_fused_has_kernel(d, iplan)) iplan = FilterPlan{};
        }
    }
    if (iplan.nw > 0) {
        const bool own = tr->feat == c->h_train.p;
        const bool mayc = c->cache_train && (own || c->cache_train_device);
        const uint64_t ep = own ? c->train_epoch : 0;
        auto& ic = c->i8c;
        const bool hit = mayc && ic.valid && ic.feat == tr->feat && ic.n == nt && ic.d == d && ic.ld == tr->ld &&
                         ic.gen == c->generation && ic.epoch == ep;
        if (!hit) {
            uint32_t bits = 0;
            HIP_OR_FAIL(c, c->i8max.ensure(sizeof(uint32_t)));
            HIP_OR_FAIL(c, hipMemsetAsync(c->i8max.p, 0, sizeof(uint32_t), st));
            stage_begin(c, st, "i8_scale");
            HIP_OR_FAIL(c, knn_launch_absmax((const float*)tr->feat, nt, tr->ld, d, c->i8max.as<uint32_t>(), st));
            stage_end(c, st);
            HIP_OR_FAIL(c, hipMemcpyAsync(&bits, c->i8max.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_OR_FAIL(c, hipStreamSynchronize(st));
            float mx;
            std::memcpy(&mx, &bits, sizeof(float));
            // finite and > 0, and s2 = 2 s^2 far from the ends of the exponent range (norms at
            // or above 2^125 leave the GEMM form anyway).  max tn / s2 <= d 127^2 / 2 < 2^30 then
            // holds for every train set: one scale bounds every element by 127 s.
            const float s = mx / 127.0f * c->i8_coarsen;
            bool ok = bits < 0x7f800000u && s >= 0x1p-40f && s <= 0x1p40f;
            // AUTO's guard against a scale set by outliers: E8 <= R Ebf, the train set's largest row
            // residual |t - rt| under the int8 and under the bf16 rounding (two statistics passes
            // of k_row_norms, on the call that builds the operands only; they leave the cached
            // bf16 operands' statistics stale, so those are rebuilt below).  A forced context and
            // the test hook's coarser steps skip it.
            if (ok && c->algo == KNN_ALGO_AUTO && c->i8_coarsen == 1.0f) {
                HIP_OR_FAIL(c, c->tmax.ensure(sizeof(float4) * ((nt + 63) / 64 + 1)));
                HIP_OR_FAIL(c, c->tsmax.ensure(sizeof(float4)));
                HIP_OR_FAIL(c, c->tctrl.ensure(4 * sizeof(int32_t)));
                c->tprep.valid = false;
                float4 e[2];
                for (int pass = 0; pass < 2; pass++) {
                    HIP_OR_FAIL(c, knn_launch_row_norms(tr->feat, dtype, nt, tr->ld, d, c->tnorm.as<float>(),
                                                        c->tctrl.as<int32_t>(), nullptr, nullptr, 0.0f, st,
                                                        c->tmax.as<float4>(), nullptr, nullptr, 1.0f, pass ? s : 0.0f));
                    HIP_OR_FAIL(c, knn_launch_tile_stat_max(c->tmax.as<float4>(), (nt + 63) / 64, c->tsmax.as<float4>(), st));
                    HIP_OR_FAIL(c, hipMemcpyAsync(&e[pass], c->tsmax.p, sizeof(float4), hipMemcpyDeviceToHost, st));
                }
                HIP_OR_FAIL(c, hipStreamSynchronize(st));
                ok = e[1].y <= KNN_I8_AUTO_R * e[0].y;  // (false for NaN)
            }
            ic = {tr->feat, nt, d, tr->ld, c->generation, ep, mayc, s, ok, false};
        }
        // (AUTO leaves a demoted train set to the bf16 operands; a forced context keeps int8)
        if (ic.ok && !(ic.demoted && c->algo == KNN_ALGO_AUTO)) i8s = ic.s;
    }
    const bool i8 = i8s > 0.0f;
    const FilterPlan fplan = i8 ? iplan
                           : knn_fused_supported(dp) ? knn_fused_plan(dp, k, nq, c->num_cus, c->fforce, max_splits(nt, k, 64 * KNN_RESCORE_CAPW)) : FilterPlan{};
    const bool fused = (felem == ELEM_ROUND || felem == ELEM_BF16) && knn_fused_supported(dp) && fplan.nw > 0;
    // (the certificates take dp: their coefficient grows with the width, so the one for dp >= d
    // holds for a chain whose columns past d add exact zeros)
    float coef, eta;
    if (fused) {
        certificate_fused(dp, felem == ELEM_ROUND, &coef, &eta);
        HIP_OR_FAIL(c, c->tmax.ensure(sizeof(float4) * ((nt + 63) / 64 + 1)));
        HIP_OR_FAIL(c, c->tsmax.ensure(sizeof(float4)));
        HIP_OR_FAIL(c, c->qstat.ensure(sizeof(float2) * (nq + 1)));
    } else {
        certificate(dp, felem, &coef, &eta);
    }
    // train-side operands of the fused filter: norms + tile statistics (k_row_norms) and the
    // tile blocks (k_tn_rows), reused from an earlier call on the same train view when the
    // context caches train (no train pass at all then; main.cpp:40-43 re-reads every train row
    // per query, this is the part of that work that depends on train alone)
    const int bn_f = fused ? 32 * fplan.rg : 0;
    const bool own_train = tr->feat == c->h_train.p;  // knn_predict's uploaded copy
    // derived train operands are reused for knn_predict's own upload (KNN_OPT_CACHE_TRAIN), and
    // for a caller's device buffer only under KNN_OPT_CACHE_TRAIN_DEVICE
    const bool may_cache = c->cache_train && (own_train || c->cache_train_device);
    auto& tp = c->tprep;
    const bool prep_hit = fused && !gate && may_cache && tp.valid && tp.feat == tr->feat && tp.n == nt &&
                          tp.d == d && tp.ld == tr->ld && tp.dtype == dtype && tp.bn == bn_f && tp.i8 == (i8 ? 1 : 0) &&
                          tp.gen == c->generation && tp.epoch == (own_train ? c->train_epoch : 0);
    // (A non-fused or wide pass leaves tprep alone although it overwrites tnorm / tnp: a later hit
    // reads the tile blocks (tblk, the norms in their headers), tctrl and tsmax only -- the fused
    // kernel takes no norm from tnorm / tnp, and k_tn_rows reads tnorm / tmax only on a miss -- and
    // none of those three is written outside the fused branch and the int8 guard, which clears
    // tprep itself.)
    if (fused && !gate) {
        HIP_OR_FAIL(c, c->tctrl.ensure(4 * sizeof(int32_t)));
        tp.valid = false;  // (set again below once this call's train pass is enqueued)
    }
    stage_begin(c, st, gate ? "norms_rerun" : "norms");
    if (fused && !gate) {
        // train norms into their own status words, then into this call's status word
        if (!prep_hit) {
            HIP_OR_FAIL(c, hipMemsetAsync(c->tctrl.p, 0, 4 * sizeof(int32_t), st));
            HIP_OR_FAIL(c, knn_launch_row_norms(tr->feat, dtype, nt, tr->ld, d, c->tnorm.as<float>(),
                                                c->tctrl.as<int32_t>(), c->tctrl.as<uint32_t>() + 2,
                                                c->tnp.as<float>(), 1.0f - coef, st, c->tmax.as<float4>(), nullptr,
                                                nullptr, 1.0f, i8s));
            HIP_OR_FAIL(c, knn_launch_tile_stat_max(c->tmax.as<float4>(), (nt + 63) / 64, c->tsmax.as<float4>(), st));
        }
        HIP_OR_FAIL(c, hipMemcpyAsync(c->ctrl.p, c->tctrl.p, 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    } else {
        HIP_OR_FAIL(c, knn_launch_row_norms(tr->feat, dtype, nt, tr->ld, d, c->tnorm.as<float>(),
                                            c->ctrl.as<int32_t>(), c->ctrl.as<uint32_t>() + 2,
                                            c->tnp.as<float>(), 1.0f - coef, st, fused ? c->tmax.as<float4>() : nullptr,
                                            gate));
        if (fused && !gate)
            HIP_OR_FAIL(c, knn_launch_tile_stat_max(c->tmax.as<float4>(), (nt + 63) / 64, c->tsmax.as<float4>(), st));
    }
    // (the fused filter's query operand is rn(-2 q): its rounding is bounded for rn(-2 q) / -2;
    // the int8 class quantises q itself with the train set's scale -- the -2 is in s2)
    HIP_OR_FAIL(c, knn_launch_row_norms(te->feat, dtype, nq, te->ld, d, c->qnorm.as<float>(),
                                        c->ctrl.as<int32_t>(), nullptr, nullptr, 0.0f, st, nullptr, gate,
                                        fused ? c->qstat.as<float2>() : nullptr, -2.0f, i8s));
    if (wide) {
        HIP_OR_FAIL(c, knn_launch_fill_u32(c->tnorm.as<uint32_t>() + nt + 64, wgr, 0x7f800000u, gate, st));  // +inf
        HIP_OR_FAIL(c, knn_launch_fill_u32(c->tnp.as<uint32_t>() + nt + 64, wgr, 0x7f800000u, gate, st));
    }
    stage_end(c, st);
    // (a norm >= 2^125 sets GEMM_UNSAFE in the status word: the filter then skips and the
    // rescore sends every query to the exact fallback scan -- decided on the device)
    stage_begin(c, st, gate ? "filter_init_rerun" : "filter_init");
    HIP_OR_FAIL(c, knn_launch_fill_u32(c->gthr.as<uint32_t>(), nq, 0xFF800000u, gate, st));  // ordered(+inf)
    stage_end(c, st);

    // filter operands: the rows themselves, or their bf16 [hi | lo] split (2d elements per row);
    // train operand rows always cover the 64-row tile grid (ntp rows; the wide filter's grid of
    // 256-row groups)
    const int64_t ntp = wide ? (nt + wgr - 1) / wgr * wgr : (nt + 63) / 64 * 64;
    const void* ftrain = tr->feat;
    const void* ftest = te->feat;
    int fld_t = tr->ld, fld_q = te->ld;
    if (fused) {
        // train as tile blocks [bn rows of rn(t) | bn norms | tile statistics] (the
        // filter starts each accumulator from the norms), queries as rn(-2 q) rows; one more
        // tile of pad blocks past the grid (the filter scans tiles in twos, k_gemm_fused).
        // The gated split re-run never takes this branch (the fused filter is the first pass).
        const int64_t ntf = ntp + 256;  // (256 pad rows: a piece's scan may run up to 224 rows past
                                        //  its own -- seven 32-row tiles of an octet, k_gemm_fused)
        // (int8 class: rows of d bytes, the header's bn words the integer norm terms, k_i8_rows)
        const size_t tb = (size_t)bn_f * (i8 ? 1 : 2) * dp + 4 * bn_f + 16;
        HIP_OR_FAIL(c, c->split_q.ensure(sizeof(uint16_t) * (size_t)dp * nq));
        stage_begin(c, st, "aug");
        if (!prep_hit) {
            HIP_OR_FAIL(c, c->tblk.ensure(tb * (size_t)(ntf / bn_f)));
            if (i8)
                HIP_OR_FAIL(c, knn_launch_i8_rows((const float*)tr->feat, ntf, nt, tr->ld, d, c->tnorm.as<float>(), i8s,
                                                  c->tblk.p, c->tmax.as<float4>(), bn_f, st));
            else
                HIP_OR_FAIL(c, knn_launch_tn_rows(tr->feat, dtype, ntf, nt, tr->ld, d, dp, c->tnorm.as<float>(), 1.0f,
                                                  c->tblk.p, c->tmax.as<float4>(), bn_f, st, nullptr));
        }
        if (i8)
            HIP_OR_FAIL(c, knn_launch_i8_rows((const float*)te->feat, nq, nq, te->ld, d, nullptr, i8s, c->split_q.p,
                                              nullptr, 0, st));
        else
            HIP_OR_FAIL(c, knn_launch_tn_rows(te->feat, dtype, nq, nq, te->ld, d, dp, nullptr, -2.0f, c->split_q.p,
                                              nullptr, 0, st, nullptr));
        stage_end(c, st);
        ftrain = c->tblk.p; ftest = c->split_q.p;
        fld_t = fld_q = dp;
        c->stats[8] = prep_hit ? 1 : 0;
        if (may_cache)
            tp = {tr->feat, nt, d, tr->ld, dtype, bn_f, c->generation, own_train ? c->train_epoch : 0, true, i8 ? 1 : 0};
    } else if (felem == ELEM_SPLIT) {
        HIP_OR_FAIL(c, c->split_t.ensure(sizeof(uint16_t) * 2 * (size_t)dp * ntp));
        HIP_OR_FAIL(c, c->split_q.ensure(sizeof(uint16_t) * 2 * (size_t)dp * nq));
        stage_begin(c, st, gate ? "split_rerun" : "split");
        HIP_OR_FAIL(c, hipMemsetAsync(c->split_t.as<uint16_t>() + 2 * (size_t)dp * nt, 0, sizeof(uint16_t) * 2 * (size_t)dp * (ntp - nt), st));
        HIP_OR_FAIL(c, knn_launch_split_rows((const float*)tr->feat, nt, tr->ld, d, dp, c->split_t.as<uint16_t>(), st, gate));
        HIP_OR_FAIL(c, knn_launch_split_rows((const float*)te->feat, nq, te->ld, d, dp, c->split_q.as<uint16_t>(), st, gate));
        stage_end(c, st);
        ftrain = c->split_t.p; ftest = c->split_q.p;
        fld_t = fld_q = 2 * dp;
    } else if (felem == ELEM_ROUND) {
        HIP_OR_FAIL(c, c->split_t.ensure(sizeof(uint16_t) * (size_t)dp * ntp));
        HIP_OR_FAIL(c, c->split_q.ensure(sizeof(uint16_t) * (size_t)dp * nq));
        stage_begin(c, st, gate ? "round_rerun" : "round");
        HIP_OR_FAIL(c, hipMemsetAsync(c->split_t.as<uint16_t>() + (size_t)dp * nt, 0, sizeof(uint16_t) * (size_t)dp * (ntp - nt), st));
        HIP_OR_FAIL(c, knn_launch_round_rows((const float*)tr->feat, nt, tr->ld, d, dp, c->split_t.as<uint16_t>(), st, gate));
        HIP_OR_FAIL(c, knn_launch_round_rows((const float*)te->feat, nq, te->ld, d, dp, c->split_q.as<uint16_t>(), st, gate));
        stage_end(c, st);
        ftrain = c->split_t.p; ftest = c->split_q.p;
        fld_t = fld_q = dp;
    } else if (felem == ELEM_BF16 && (dp != d || wide)) {
        // bf16 data narrower than its operand width with no fused kernel at this k, or wide rows
        // (packed operands on the grid of row groups): [dp] rows with zero columns past d
        // (k_tn_rows' query form; scale 1 keeps the bits), the train rows on the tile grid with
        // zero pad rows
        HIP_OR_FAIL(c, c->split_t.ensure(sizeof(uint16_t) * (size_t)dp * ntp));
        HIP_OR_FAIL(c, c->split_q.ensure(sizeof(uint16_t) * (size_t)dp * nq));
        stage_begin(c, st, gate ? "round_rerun" : "round");
        HIP_OR_FAIL(c, knn_launch_tn_rows(tr->feat, dtype, ntp, nt, tr->ld, d, dp, nullptr, 1.0f, c->split_t.p, nullptr, 0, st, gate));
        HIP_OR_FAIL(c, knn_launch_tn_rows(te->feat, dtype, nq, nq, te->ld, d, dp, nullptr, 1.0f, c->split_q.p, nullptr, 0, st, gate));
        stage_end(c, st);
        ftrain = c->split_t.p; ftest = c->split_q.p;
        fld_t = fld_q = dp;
    } else if (nt % 64) {
        // the caller's rows, copied onto the 64-row tile grid: every tile the filter copies
        // into LDS is whole (one DMA form, knn_kernels.hip), the pad rows never pass (+inf norms).
        // Kept across calls like the fused operands (KNN_OPT_CACHE_TRAIN, same key).
        const size_t es = (size_t)elem_size(dtype), pitch = es * (size_t)tr->ld;
        auto& pk = c->tpad;
        const uint64_t ep = tr->feat == c->h_train.p ? c->train_epoch : 0;
        const bool hit = may_cache && pk.valid && pk.feat == tr->feat && pk.n == nt && pk.d == d &&
                         pk.ld == tr->ld && pk.dtype == dtype && pk.gen == c->generation && pk.epoch == ep;
        pk.valid = false;
        if (!hit) {
            HIP_OR_FAIL(c, c->pad_t.ensure(pitch * (size_t)ntp));
            // (the last row ends after its d elements: the caller's buffer may end there too -- a
            // column view of a wider table, or exactly (nt - 1) * ld + d elements)
            HIP_OR_FAIL(c, hipMemcpyAsync(c->pad_t.p, tr->feat, pitch * (size_t)(nt - 1) + es * (size_t)d,
                                          hipMemcpyDeviceToDevice, st));
            HIP_OR_FAIL(c, hipMemsetAsync((unsigned char*)c->pad_t.p + pitch * (size_t)nt, 0, pitch * (size_t)(ntp - nt), st));
        }
        if (may_cache) pk = {tr->feat, nt, d, tr->ld, dtype, c->generation, ep, true};
        ftrain = c->pad_t.p;
    }

    const FilterPlan plan = fused ? fplan : wide ? knn_wide_plan(k) : knn_gemm_filter_plan(kelem, rb, k);
    const bool shared = fused && knn_fused_list_share_width(plan) > 0;
    const int64_t n_qtiles = (nq + plan.bm - 1) / plan.bm;
    GemmFilterArgs g{};
    g.nt = nt; g.n_qtiles = (int)n_qtiles;
    // fused filter: the balanced schedule (knn_fused_schedule) when its pieces per query tile
    // fit the candidate list like segments do; else (or with explicit train_splits) segments
    int nseg = 0;
    // (the balanced schedule's ranges span two query tiles, a piece of each, so a block may pay
    // two threshold warm-ups; with the longer lists of small query sets (capmul > 1), whose
    // pieces are many and short, the even segments measured faster: A's rows, 6,250 queries,
    // 2.02 against 1.84 ms, r06bi)
    if (fused && c->train_splits <= 0 && capmul == 1) {
        int occ = 1;
        if (knn_fused_occupancy(dp, plan, &occ) != hipSuccess || occ < 1) occ = 1;
        int nb = 1;
        knn_fused_schedule(g, occ * c->num_cus, &nb);
        if (nb <= max_splits(nt, k, cap, smax)) nseg = nb;
    }
    if (nseg == 0) {
        nseg = choose_splits(c, n_qtiles, nt, kelem, rb, k, cap, fused, dp, &plan, smax, wide);
        g.g2 = -1;  // segment schedule
    }
    int64_t seg_len = (nt + nseg - 1) / nseg;
    seg_len = wide ? (seg_len + wgr - 1) / wgr * wgr : (seg_len + 63) / 64 * 64;
    g.train = ftrain; g.nt = nt; g.ld_t = fld_t;
    g.test = ftest; g.nq = nq; g.ld_q = fld_q; g.d = dp;  // (the operand rows' width)
    g.tnorm = c->tnorm.as<float>(); g.tnp = c->tnp.as<float>(); g.qnorm = c->qnorm.as<float>();
    g.tnmax = c->ctrl.as<uint32_t>() + 2;
    g.k = k; g.seg_len = seg_len; g.nseg = nseg;
    g.coef = coef; g.eta = eta;
    g.gthr = c->gthr.as<uint32_t>();
    g.cnt = c->cnt.as<int32_t>(); g.cand = c->cand.as<CandRec>(); g.cap = cap; g.cap_seg = cap / nseg;
    g.qstat = fused ? c->qstat.as<float2>() : nullptr;
    g.tsmax = fused ? c->tsmax.as<float4>() : nullptr;
    g.i8_s2 = i8 ? knn_i8_s2_of(i8s) : 0.0f;
    // per-XCD scan cursors for the multi-segment schedule (B: filter traffic beyond L2 664 ->
    // 494 GB per launch, time unchanged; with one segment or the balanced schedule they saved
    // nothing: r03s).
    if (fused && g.g2 < 0 && nseg > 1) {
        HIP_OR_FAIL(c, c->cursor.ensure(sizeof(uint32_t) * 8));
        HIP_OR_FAIL(c, hipMemsetAsync(c->cursor.p, 0, sizeof(uint32_t) * 8, st));
        g.cursor = c->cursor.as<uint32_t>();
    }
    // pacing of each XCD's blocks (fused_pace, knn_fused.hip: A 19.23 -> 18.70 ms, fetch beyond L2
    // 22.0 -> 4.7 GB) when the balanced schedule is one round of blocks that start and
    // end together: there a leader's wait costs nothing.  With whole rounds of query tiles before
    // it a held block keeps its CU from the next round's (A's rows, 200,000 queries: 37.9 -> 41.4
    // ms), so those grids are not paced.  The 64-query register-list shapes at d = 128 only (what was measured: A and
    // its 2- and 4-GPU shares; B's and C's grids take segments or several rounds; the 32-query
    // instantiations compile no pacing code).  The two uses of c->cursor exclude each other
    // (segments: g2 < 0).
    if (fused && g.g2 > 0 && g.p1_blocks == 0 && plan.qg == 2 && plan.kr > 0 && dp == 128) {
        HIP_OR_FAIL(c, c->cursor.ensure(sizeof(int32_t) * 16));
        HIP_OR_FAIL(c, hipMemsetAsync(c->cursor.p, 0, sizeof(int32_t) * 16, st));
        g.pace = c->cursor.as<int32_t>();
    }
    // the pieces of a query share their threshold lists, not just their k-th values: the
    // union's k-th smallest U is the bound a single scan would have.  The 32-queries-per-wave
    // shape only -- the small query counts, whose query tiles are cut into many pieces (A's
    // 8-GPU share: 5 pieces, 599 -> 447 kept rows per query, filter 3.38 -> 3.19 ms, r04g; on
    // A and B, 3 and 2 pieces, it measured equal or slower).
    if (shared && nseg > 1) {
        g.lshare_w = knn_fused_list_share_width(plan);
        const int64_t nls = nq * (int64_t)nseg * g.lshare_w;
        HIP_OR_FAIL(c, c->lshare.ensure(sizeof(float) * nls));
        HIP_OR_FAIL(c, knn_launch_fill_u32(c->lshare.as<uint32_t>(), nls, 0x7f800000u, gate, st));  // +inf
        g.lshare = c->lshare.as<float>();
    }
    g.status = c->ctrl.as<int32_t>();
    g.gate = gate;
    // the parked passes' count, like the candidates a diagnostic of profile = 2 only: the timed
    // path hands the kernel no counter
    if (fused && plan.park && c->profile == 2 && !gate) {
        HIP_OR_FAIL(c, c->parkcnt.ensure(sizeof(unsigned long long)));
        HIP_OR_FAIL(c, hipMemsetAsync(c->parkcnt.p, 0, sizeof(unsigned long long), st));
        g.park_cnt = c->parkcnt.as<unsigned long long>();
    }
    if (!gate) c->park_counted = g.park_cnt != nullptr;
    // seeded thresholds (k_seed_thr, knn_seed.hip): the int8 class's first pass lowers gthr from +inf
    // to a bound from a strided sample of the tile blocks the filter is about to read -- the same
    // cached operand, nothing of its own to keep.  Not on the gated re-run (never int8).  Like the
    // parked passes' count the seeds themselves are a diagnostic of profile = 2: the timed path
    // hands the kernel no side buffer.
    if (!gate) c->seed_nq = 0;
    if (i8 && fused && !gate && c->fforce.seed) {
        SeedArgs sa{};
        sa.sample = knn_seed_sample(nt, bn_f, nq, c->num_cus);
        if (sa.sample.ns > 0) {
            sa.tblk = c->tblk.p; sa.bn = bn_f; sa.qop = c->split_q.p; sa.nq = nq;
            sa.pad_blk = (ntp + 256) / bn_f - 1;  // (the operand ends in 256 pad rows, above)
            sa.qnorm = g.qnorm; sa.qstat = g.qstat; sa.tsmax = g.tsmax;
            sa.coef = coef; sa.eta = eta; sa.i8_s2 = g.i8_s2; sa.k = k;
            sa.gthr = g.gthr; sa.status = g.status; sa.gate = gate;
            if (c->profile == 2) {
                HIP_OR_FAIL(c, c->seedbuf.ensure(sizeof(uint32_t) * nq));
                HIP_OR_FAIL(c, knn_launch_fill_u32(c->seedbuf.as<uint32_t>(), nq, 0xFF800000u, nullptr, st));  // ordered(+inf)
                sa.seed_out = c->seedbuf.as<uint32_t>();
                c->seed_nq = nq;
            }
            stage_begin(c, st, "seed");
            HIP_OR_FAIL(c, knn_launch_seed_thr(sa, st));
            stage_end(c, st);
        }
    }
    const int subs = KNN_FILTER_SUBSLICES;  // candidate sub-slices per segment: one per lane half
    if (fused && g.g2 >= 0 && nseg > 1)  // whole query tiles write only their piece's sub-slices
        HIP_OR_FAIL(c, hipMemsetAsync(c->cnt.p, 0, sizeof(int32_t) * subs * nseg * nq, st));
    stage_begin(c, st, gate ? "gemm_filter_rerun" : "gemm_filter");
    if (fused) HIP_OR_FAIL(c, knn_launch_fused(g, plan, st));
    else if (wide) HIP_OR_FAIL(c, knn_launch_wide(g, st));
    else HIP_OR_FAIL(c, knn_launch_gemm_filter(g, kelem, rb, st));
    stage_end(c, st);

    RescoreArgs r{};
    r.train = tr->feat; r.labels = tr->labels; r.ld_t = tr->ld;
    r.test = te->feat; r.ld_q = te->ld; r.nq = nq; r.d = d; r.k = k; r.C = C; r.elem = dtype;
    r.cnt = g.cnt; r.cand = g.cand; r.cap = cap;
    r.nseg = subs * nseg; r.cap_seg = g.cap_seg / subs;  // sub-slices: (segment, lane half)
    r.out = out; r.status = c->ctrl.as<int32_t>();
    r.fb_list = c->fb_list.as<int32_t>(); r.fb_count = c->ctrl.as<int32_t>() + 1;
    r.gate = gate;
    // the fused filter's final thresholds: the selection stages only the candidates that can
    // survive
    r.gthr = fused ? g.gthr : nullptr;
    // LDS staging for about twice the expected kept rows -- k (1 + ln(nt / k)) for one scan,
    // +25 % per extra segment (they share thresholds through gthr), measured 238 per query on
    // A and 605 on B -- rounded to 64 by the launcher and capped at the list capacity: a
    // smaller footprint per wave lets more query waves share a CU
    {
        const double expect = k * (1.0 + std::log(std::max((double)nt / k, 1.0))) * (1.0 + 0.25 * (nseg - 1)) + 64.0;
        r.su_cap = c->rescore_su > 0 ? c->rescore_su : (int)std::min<double>(cap, 2.0 * expect);
    }
    stage_begin(c, st, gate ? "rescore_rerun" : "rescore");
    HIP_OR_FAIL(c, knn_launch_rescore(r, st));
    stage_end(c, st);

    if (!gate) {
        c->stats[2] = nseg;
        c->stats[3] = felem;
        c->stats[5] = fused;
        c->stats[9] = fused ? 32 : 0;
        c->stats[10] = fused ? 32 * plan.qg : 0;
        c->stats[11] = i8 ? 1 : 0;
        c->stats[15] = dp;
        c->stats[16] = wide ? dp / 128 : 1;
        if (i8) c->i8_pass_nq = nq;
    } else {
        c->rerun_stats[0] = nseg;
        c->rerun_stats[1] = felem;
        c->rerun_stats[2] = fused;
        c->rerun_stats[3] = dp;
    }
    return KNN_OK;
}

}  // namespace

extern "C" {

int32_t knn_version(void) { return KNN_AMD_ABI_VERSION; }

knn_status knn_create(knn_ctx** out, const knn_opts* opts) {
    if (!out) return KNN_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return KNN_ENODEV;
    knn_ctx* c = new (std::nothrow) knn_ctx();
    if (!c) return KNN_ENOMEM;
    if (opts) {
        c->device = opts->device;
        c->algo = opts->algo;
        c->train_splits = opts->train_splits;
        c->profile = opts->profile;
        c->cache_train = (opts->flags & KNN_OPT_CACHE_TRAIN) != 0;
        c->cache_train_device = c->cache_train && (opts->flags & KNN_OPT_CACHE_TRAIN_DEVICE) != 0;
    }
    // Test hooks: the only environment the library's plan depends on, read here once, never per
    // call.  They let the tests run shapes and paths the product rules pick only at large sizes:
    //   KNN_RESCORE_SU=n   the rescore's LDS staging size (entries; default: sized per call)
    //   KNN_FUSED_QG=1|2   the fused filter's queries per wave, 32 or 64 (knn_fused_plan's fill rule)
    //   KNN_FUSED_HEAPS    (set) the LDS-heap shape for 32 < k <= 104 at d = 256
    //   KNN_FUSED_PARK=0|1 the int8 filter's parked passes off (the immediate slow path) / on
    //   KNN_FUSED_SEED=0|1 the int8 filter's seeded thresholds (k_seed_thr) off / on
    //   KNN_MST_LISTS=0|1  the spanning tree's list shortcut off (every row through every pass) / on
    //   KNN_MST_LIST_L=n   its lists hold max(min_samples, n) entries (0 .. 256; scripts/time_mst.py's study)
    //   KNN_WS_QUERIES=n   queries per pass of the GEMM path's candidate workspace
    //   KNN_BATCH_ROWS=n   query rows per batch of the host pipeline
    if (const char* e = getenv("KNN_RESCORE_SU")) c->rescore_su = atoi(e);
    if (const char* e = getenv("KNN_FUSED_QG")) c->fforce.qg = atoi(e);
    c->fforce.heaps = getenv("KNN_FUSED_HEAPS") != nullptr;
    if (const char* e = getenv("KNN_FUSED_PARK")) c->fforce.park = atoi(e) != 0 ? 1 : 0;
    if (const char* e = getenv("KNN_FUSED_SEED")) c->fforce.seed = atoi(e) != 0 ? 1 : 0;
    if (const char* e = getenv("KNN_MST_LISTS")) c->mst_lists = atoi(e) != 0 ? 1 : 0;
    if (const char* e = getenv("KNN_MST_LIST_L")) c->mst_list_l = std::min(std::max(atoi(e), 0), 256);
    if (c->device < 0 || c->device >= ndev) { delete c; return KNN_ENODEV; }
    hipDeviceProp_t prop;
    if (hipSetDevice(c->device) != hipSuccess || hipGetDeviceProperties(&prop, c->device) != hipSuccess) {
        delete c;
        return KNN_ENODEV;
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        // kernels are built for gfx950 only
        delete c;
        return KNN_ENODEV;
    }
    c->num_cus = prop.multiProcessorCount;
    // the context's own stream (device calls given no stream) is a BLOCKING stream: ordered after
    // the work the caller issued on the legacy null stream (torch's default stream), as the
    // device entry points promise; the copy stream of the host pipeline stays non-blocking
    if (hipStreamCreateWithFlags(&c->stream, hipStreamDefault) != hipSuccess ||
        hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void**)&c->ctrl_host, 8 * sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent) !=
            hipSuccess ||
        hipHostGetDevicePointer((void**)&c->ctrl_host_dev, c->ctrl_host, 0) != hipSuccess ||
        c->ctrl.ensure(4 * sizeof(int32_t)) != hipSuccess) {
        knn_destroy(c);
        return KNN_EHIP;
    }
    for (int i = 0; i < 2; i++)
        if (hipEventCreateWithFlags(&c->ev_up[i], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_done[i], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_down[i], hipEventDisableTiming) != hipSuccess) {
            knn_destroy(c);
            return KNN_EHIP;
        }
    // GEMM-path candidate workspace: 12 B x 64 CAPW per query; passes of at most a quarter of
    // the free HBM (the test hooks above override)
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0)
        c->ws_queries = std::max<int64_t>(4096, (int64_t)(free_b / 4) / (12 * 64 * KNN_RESCORE_CAPW + 64));
    if (const char* e = getenv("KNN_WS_QUERIES")) c->ws_queries = std::max<int64_t>(1, atoll(e));
    if (const char* e = getenv("KNN_BATCH_ROWS")) c->batch_rows = std::max<int64_t>(1, atoll(e));
    *out = c;
    return KNN_OK;
}

void knn_destroy(knn_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (DBuf* b : {&c->tnorm, &c->tnp, &c->qnorm, &c->gthr, &c->cnt, &c->cand,
                    &c->fb_list, &c->ctrl, &c->scratch, &c->split_t, &c->split_q, &c->pad_t, &c->seg_rec, &c->arrive, &c->tmax, &c->tsmax, &c->qstat, &c->tblk, &c->tctrl, &c->cursor, &c->lshare, &c->parkcnt, &c->seedbuf, &c->h_train, &c->h_labels, &c->h_test, &c->h_pred,
                    &c->h_dist, &c->h_idx, &c->sw_dist, &c->sw_idx, &c->sw_pred, &c->sw_qside, &c->sw_acc, &c->sw_scores,
                    &c->rg_part, &c->rg_zero, &c->rg_targets, &c->rd_segcnt, &c->rd_base, &c->rd_cc, &c->rd_scores,
                    &c->rm_tnorm, &c->rm_tmax, &c->rm_tsmax, &c->rm_tblk, &c->rm_tctrl, &c->rm_qnorm, &c->rm_qstat,
                    &c->rm_qop, &c->rm_exact, &c->lof_idx, &c->lof_dist, &c->lof_cidx, &c->lof_delta, &c->lof_kd,
                    &c->lof_lrd, &c->lof_qlrd, &c->rd_sweep, &c->db_tab, &c->db_offs, &c->db_info, &c->db_count,
                    &c->dbs_tab, &c->dbs_offs, &c->dbs_info, &c->dbs_count, &c->mst_idx, &c->mst_dist, &c->mst_f,
                    &c->mst_i, &c->mst_u, &c->mst_w, &c->mst_cnt, &c->mst_sort, &c->mst_cut, &c->mst_offs, &c->mst_info})
        b->release();
    for (hipEvent_t e : c->events) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; i++) {
        for (hipEvent_t e : {c->ev_up[i], c->ev_done[i], c->ev_down[i]})
            if (e) (void)hipEventDestroy(e);
        for (DBuf* b : {&c->q_slot[i], &c->pred_slot[i], &c->dist_slot[i], &c->idx_slot[i]}) b->release();
    }
    for (int32_t* p : c->ctrl_slots) (void)hipHostFree(p);
    if (c->ctrl_host) (void)hipHostFree(c->ctrl_host);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->cstream) (void)hipStreamDestroy(c->cstream);
    delete c;
}

const char* knn_last_error(const knn_ctx* c) { return c ? c->err.c_str() : "null context"; }

}  // extern "C"

int knn_ctx_device(const knn_ctx* c) { return c->device; }
void* knn_ctx_stream(const knn_ctx* c) { return (void*)c->stream; }
void knn_ctx_stage_begin(knn_ctx* c, void* stream, const char* name);
void knn_ctx_stage_end(knn_ctx* c, void* stream);
knn_status knn_merge_vote_append(knn_ctx* c, int32_t nsrc, int64_t nq, int32_t k, int32_t C, const int32_t* d_rec,
                                 int32_t* d_pred, float* d_dist, int32_t* d_idx, void* hip_stream);

namespace {

// Validation shared by the device entry points.
// need_pred = false: the k-sweep's internal top-k pass, which votes in k_vote_sweep instead
// (the public predict entry points always pass true).
knn_status validate_call(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int32_t k, int32_t C,
                         const QueryOut& out, bool shard, bool need_pred = true) {
    knn_status s;
    if ((s = check_dataset(c, tr, "train", true)) != KNN_OK) return s;
    if ((s = check_dataset(c, te, "test", false)) != KNN_OK) return s;
    if (tr->d != te->d) return fail(c, KNN_EINVAL, "feature count mismatch: train d=%d test d=%d", tr->d, te->d);
    if (tr->dtype != te->dtype) return fail(c, KNN_EINVAL, "train and test dtypes differ");
    if (k < 1 || (!shard && k > tr->n))
        return fail(c, KNN_EINVAL, "k=%d outside [1, n_train=%lld]", k, (long long)tr->n);
    if (k > 1024) return fail(c, KNN_EINVAL, "k=%d exceeds the supported maximum 1024", k);
    if (C < 1 || C > 16384) return fail(c, KNN_EINVAL, "num_classes=%d outside [1, 16384]", C);
    if (tr->n + out.idx_base > 0x7fffffffLL || out.idx_base < 0)
        return fail(c, KNN_EINVAL, "train row indices exceed 2^31-1");
    const int es = elem_size(tr->dtype);
    if (((int64_t)tr->ld * es) % 16 || ((int64_t)te->ld * es) % 16 || (((uintptr_t)tr->feat) & 15) ||
        (((uintptr_t)te->feat) & 15))
        return fail(c, KNN_EINVAL, "device rows must be 16-byte aligned (ld * element size %% 16 == 0)");
    if (te->n > 0 && !shard && need_pred && !out.pred) return fail(c, KNN_EINVAL, "pred is NULL");
    // the exact scan (KNN_ALGO_DIRECT_SCAN, and every GEMM path's fallback) stages the query
    // row in LDS: bound d by it up front instead of failing at a launch
    if (knn_exact_scan_lds(tr->d, k, C) > 160 * 1024)
        return fail(c, KNN_EINVAL, "d=%d too wide for the exact scan's LDS query row at k=%d, C=%d (d <= ~%d)",
                    tr->d, k, C, (int)((160 * 1024 - knn_exact_scan_lds(0, k, C)) / 4));
    return KNN_OK;
}

// One pass of the pipeline over a query set, enqueued on st with no host synchronisation (but for
// the int8 operand class's scale read-back on the call that builds its train operands, run_gemm);
// the status word is copied to ctrl_copy (pinned host, optional) at the end.
knn_status predict_enqueue(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int32_t k, int32_t C,
                           const QueryOut& out, hipStream_t st, int algo, int32_t* ctrl_copy) {
    knn_status s;
    HIP_OR_FAIL(c, reset_ctrl(c, st));
    if (c->metric != KNN_METRIC_SQEUCLIDEAN) {
        // (choose_algo gave KNN_ALGO_DIRECT; knn_set_metric refused the contexts that cannot)
        stage_begin(c, st, "metric_tile");
        if ((s = run_metric_tile(c, tr, te, k, C, out, st)) != KNN_OK) return s;
        stage_end(c, st);
    } else if (is_gemm(algo)) {
        // AUTO on fp32 data runs the rounded filter first; when more than 1/16 of the queries
        // (at least 256) overflow its candidate lists, the call is re-run with the split
        // filter (every output is rewritten).  The decision is made on the device
        // (k_rerun_decide): the split stages are enqueued behind a gate, so a call ends in a
        // single stream synchronisation either way.
        // (where the split form exists at the padded width: rows of at most 128 features; elsewhere
        // the overflowing queries go to the exact fallback list)
        const bool adaptive = c->algo == KNN_ALGO_AUTO && filter_elem(algo, tr->dtype) == ELEM_ROUND &&
                              split_rerun_width(tr->d, k) > 0;
        if ((s = run_gemm(c, tr, te, k, C, out, st, algo, nullptr)) != KNN_OK) return s;
        if (adaptive) {
            const int64_t limit = std::max<int64_t>(256, te->n / 16);
            HIP_OR_FAIL(c, knn_launch_rerun_decide(c->ctrl.as<int32_t>(), limit, st));
            if ((s = run_gemm(c, tr, te, k, C, out, st, KNN_ALGO_GEMM_SPLIT, c->ctrl.as<int32_t>() + 3)) != KNN_OK)
                return s;
        }
        stage_begin(c, st, "fallback_scan");
        if ((s = run_exact_scan(c, tr, te, k, C, out, st, c->fb_list.as<int32_t>(), c->ctrl.as<int32_t>() + 1)) != KNN_OK)
            return s;
        stage_end(c, st);
    } else if (algo == KNN_ALGO_DIRECT_SCAN) {
        stage_begin(c, st, "exact_scan");
        if ((s = run_exact_scan(c, tr, te, k, C, out, st, nullptr, nullptr)) != KNN_OK) return s;
        stage_end(c, st);
    } else {
        stage_begin(c, st, "direct_tile");
        if ((s = run_direct_tile(c, tr, te, k, C, out, st)) != KNN_OK) return s;
        stage_end(c, st);
    }
    if (ctrl_copy) HIP_OR_FAIL(c, hipMemcpyAsync(ctrl_copy, c->ctrl.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    return KNN_OK;
}

// stats of a finished pass (status word in ctrl)
void pass_stats(knn_ctx* c, const int32_t* ctrl, bool gemm) {
    c->stats[1] += ctrl[1];
    // an int8 pass that sent more than 1/64 of its queries to the exact fallback: the scale
    // misjudged these rows (results are exact either way)
    // (or so many that AUTO re-ran the call with the split operands, which zeroes the count)
    if (gemm && c->stats[11] == 1 && c->i8c.valid && (ctrl[3] || (int64_t)ctrl[1] > c->i8_pass_nq / 64))
        c->i8c.demoted = true;
    if (gemm && ctrl[3]) {
        // the split re-run ran: its segments / operand type describe the results
        c->stats[4] = 1;
        c->stats[2] = c->rerun_stats[0];
        c->stats[3] = c->rerun_stats[1];
        c->stats[5] = c->rerun_stats[2];
        c->stats[11] = 0;
        c->stats[15] = c->rerun_stats[3];
    }
}

QueryOut offset_out(const QueryOut& o, int64_t q0) {
    QueryOut r = o;
    if (r.pred) r.pred += q0;
    if (r.dist) r.dist += q0 * r.stride;
    if (r.idx) r.idx += q0 * r.stride;
    if (r.label) r.label += q0 * r.stride;
    return r;
}

knn_dataset offset_rows(const knn_dataset& x, int64_t r0, int64_t n) {
    knn_dataset r = x;
    r.feat = (const unsigned char*)x.feat + (size_t)r0 * (size_t)x.ld * (size_t)elem_size(x.dtype);
    r.n = n;
    return r;
}

void reset_stats(knn_ctx* c) {
    c->stages.clear();
    for (int i = 0; i < 22; i++) c->stats[i] = 0;
    c->seed_nq = 0;
    c->stats[3] = -1;
}
// the vote / regression on CSR lists run no distance pass: the form and the exact evaluations of the
// radius pass that made the lists (stats[13], [14]) stay readable behind them, so a caller of
// radius_predict_device or radius_regress_device still sees which form its passes took
void reset_stats_keep_radius(knn_ctx* c) {
    const int64_t form = c->stats[13], exact = c->stats[14];
    reset_stats(c);
    c->stats[13] = form;
    c->stats[14] = exact;
}

// the last pass's seeds as floats (+inf: none); false when that pass recorded none
bool last_seeds(knn_ctx* c, std::vector<float>& out) {
    if (c->seed_nq <= 0 || !c->seedbuf.p) return false;
    std::vector<uint32_t> o((size_t)c->seed_nq);
    if (hipMemcpy(o.data(), c->seedbuf.p, sizeof(uint32_t) * o.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
    out.resize(o.size());
    for (size_t i = 0; i < o.size(); i++) {
        const uint32_t b = (o[i] & 0x80000000u) ? (o[i] & 0x7fffffffu) : ~o[i];  // (o2f, knn_device.h)
        std::memcpy(&out[i], &b, sizeof(float));
    }
    return true;
}

// Shared pipeline of knn_predict_device / knn_shard_topk_device: the GEMM path runs the
// queries in passes of at most c->ws_queries (the candidate workspace, 24 KB per query, is
// bounded by a quarter of the free HBM), each ending in one synchronisation.
// shard = true: the train set is one shard of a larger one; k may exceed its rows and
// queries with fewer than k neighbours are not an error (the merge decides).
knn_status predict_core(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int32_t k, int32_t C,
                        const QueryOut& out, void* hip_stream, bool shard) {
    knn_status s;
    if ((s = validate_call(c, tr, te, k, C, out, shard)) != KNN_OK) return s;
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    reset_stats(c);
    if (te->n == 0) return KNN_OK;
    const int algo = choose_algo(c, tr->n, te->n, tr->d, k, tr->dtype);
    const bool gemm = is_gemm(algo);
    const int64_t pass = gemm ? std::max<int64_t>(1, c->ws_queries) : te->n;
    for (int64_t q0 = 0; q0 < te->n; q0 += pass) {
        const knn_dataset tq = offset_rows(*te, q0, std::min(pass, te->n - q0));
        if ((s = predict_enqueue(c, tr, &tq, k, C, offset_out(out, q0), st, algo, nullptr)) != KNN_OK ||
            (s = finish_call(c, st)) != KNN_OK) {
            if (s != KNN_EINVAL && s != KNN_ERANGE) c->tprep.valid = c->tpad.valid = false;  // a HIP failure: the operands may be partial
            return s;
        }
        pass_stats(c, c->ctrl_host, gemm);
    }
    if (c->profile == 2 && gemm) {
        // diagnostic only: total candidates kept by the filter (last pass)
        std::vector<int32_t> h(std::min(pass, te->n) * KNN_FILTER_SUBSLICES * c->stats[2]);
        if (hipMemcpy(h.data(), c->cnt.p, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost) == hipSuccess) {
            int64_t tot = 0;
            for (int32_t v : h) tot += v;
            c->stats[0] = tot;
        }
        // ... and the records the int8 filter parked (last pass; the int8 pass was not re-run on bf16)
        unsigned long long parked = 0;
        if (c->stats[11] == 1 && c->park_counted &&
            hipMemcpy(&parked, c->parkcnt.p, sizeof(parked), hipMemcpyDeviceToHost) == hipSuccess)
            c->stats[12] = (int64_t)parked;
        // ... and the queries whose threshold the seed pass lowered (last pass)
        std::vector<float> seeds;
        if (c->stats[11] == 1 && last_seeds(c, seeds)) {
            int64_t n = 0;
            for (float v : seeds) n += std::isfinite(v) ? 1 : 0;
            c->stats[17] = n;
        }
    }
    return KNN_OK;
}

// the row stride of a host-buffer call's device copies: rows padded to 16 B
int device_ld(int d, int dtype) {
    const int per16 = 16 / elem_size(dtype);
    return (d + per16 - 1) / per16 * per16;
}

// The device call's checks on the shapes a host-buffer call will see (batches of B queries, rows
// ldd apart), before anything is enqueued: no early return may leave a copy to or from the
// caller's buffers in flight.  (The entry has checked the caller's label pointer already.)
knn_status validate_host_shapes(knn_ctx* c, const knn_dataset* tr, int64_t B, int ldd, int32_t k, int32_t C,
                                const QueryOut& out, bool need_pred) {
    const knn_dataset vtr{(const void*)(uintptr_t)256, (const int32_t*)(uintptr_t)256, tr->n, tr->d, ldd, tr->dtype};
    const knn_dataset vq{(const void*)(uintptr_t)256, nullptr, B, tr->d, ldd, tr->dtype};
    return validate_call(c, &vtr, &vq, k, C, out, false, need_pred);
}

// The train set of a host-buffer call on the device: reused across calls when the context
// caches train uploads (KNN_OPT_CACHE_TRAIN) and the buffer, shape and generation match.
knn_status train_device(knn_ctx* c, const knn_dataset* tr, hipStream_t st, knn_dataset* dtr) {
    const size_t es = (size_t)elem_size(tr->dtype);
    const int ldd = device_ld(tr->d, tr->dtype);
    auto& tc = c->tcache;
    const bool hit = c->cache_train && tc.valid && tc.feat == tr->feat && tc.labels == tr->labels && tc.n == tr->n &&
                     tc.d == tr->d && tc.ld == tr->ld && tc.dtype == tr->dtype && tc.gen == c->generation;
    if (!hit) {
        tc.valid = false;
        c->train_epoch++;  // the uploaded copy changes: the train-side filter operands of it are stale
        HIP_OR_FAIL(c, c->h_train.ensure(es * (size_t)ldd * tr->n));
        HIP_OR_FAIL(c, c->h_labels.ensure(sizeof(int32_t) * tr->n));
        HIP_OR_FAIL(c, hipMemcpy2DAsync(c->h_train.p, es * ldd, tr->feat, es * tr->ld, es * tr->d, tr->n,
                                        hipMemcpyHostToDevice, st));
        // (lists_host for regression has no classes: labels == NULL, and the pass runs with zeros)
        if (tr->labels)
            HIP_OR_FAIL(c, hipMemcpyAsync(c->h_labels.p, tr->labels, sizeof(int32_t) * tr->n, hipMemcpyHostToDevice, st));
        else
            HIP_OR_FAIL(c, hipMemsetAsync(c->h_labels.p, 0, sizeof(int32_t) * tr->n, st));
        c->stats[6] += (int64_t)(es * tr->d * tr->n + sizeof(int32_t) * tr->n);
        if (c->cache_train) {
            tc = {tr->feat, tr->labels, tr->n, tr->d, tr->ld, tr->dtype, ldd, c->generation, true};
        }
    }
    *dtr = knn_dataset{c->h_train.p, c->h_labels.as<int32_t>(), tr->n, tr->d, ldd, tr->dtype};
    return KNN_OK;
}

}  // namespace

// knn_arff.cpp's radius calls have no host-buffer entry point to go through: the host train set
// on the device by the host entry points' own upload path (train_device: cached under
// KNN_OPT_CACHE_TRAIN), enqueued on the context's stream
knn_status knn_ctx_train_device(knn_ctx* c, const knn_dataset* tr, knn_dataset* dtr) {
    if (!c || !tr || !dtr) return KNN_EINVAL;
    c->err.clear();
    knn_status s;
    if ((s = check_dataset(c, tr, "train", true)) != KNN_OK) return s;
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    if ((s = train_device(c, tr, c->stream, dtr)) != KNN_OK) {
        (void)hipStreamSynchronize(c->stream);
        c->tcache.valid = false;
    }
    return s;
}

extern "C" {

knn_status knn_predict_device(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int32_t k,
                              int32_t C, int32_t* pred, float* dist, int32_t* idx, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    QueryOut out{pred, dist, idx, nullptr, k, 0};
    return predict_core(c, tr, te, k, C, out, hip_stream, false);
}

knn_status knn_shard_topk_device(knn_ctx* c, const knn_dataset* shard, const knn_dataset* te, int32_t k,
                                 int32_t C, int64_t idx_base, int32_t* d_rec, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    if (te && te->n > 0 && !d_rec) return fail(c, KNN_EINVAL, "d_rec is NULL");
    QueryOut out{nullptr, reinterpret_cast<float*>(d_rec), d_rec ? d_rec + k : nullptr,
                 d_rec ? d_rec + 2 * (int64_t)k : nullptr, 3 * (int64_t)k, idx_base};
    return predict_core(c, shard, te, k, C, out, hip_stream, true);
}

knn_status knn_merge_vote_device(knn_ctx* c, int32_t nsrc, int64_t nq, int32_t k, int32_t C,
                                 const int32_t* d_rec, int32_t* d_pred, float* d_dist, int32_t* d_idx,
                                 void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    c->stages.clear();
    return knn_merge_vote_append(c, nsrc, nq, k, C, d_rec, d_pred, d_dist, d_idx, hip_stream);
}

}  // extern "C"

// the merge, with its stage appended to the context's profile (knn_predict_train_sharded
// keeps the shard's filter / rescore stages and the exchange beside it)
knn_status knn_merge_vote_append(knn_ctx* c, int32_t nsrc, int64_t nq, int32_t k, int32_t C, const int32_t* d_rec,
                                 int32_t* d_pred, float* d_dist, int32_t* d_idx, void* hip_stream) {
    if (nsrc < 1 || nq < 0 || k < 1 || k > 1024 || C < 1 || C > 16384)
        return fail(c, KNN_EINVAL, "merge: bad nsrc=%d nq=%lld k=%d C=%d", nsrc, (long long)nq, k, C);
    if (nq > 0 && (!d_rec || !d_pred)) return fail(c, KNN_EINVAL, "merge: d_rec / d_pred is NULL");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (nq == 0) return KNN_OK;
    HIP_OR_FAIL(c, reset_ctrl(c, st));
    MergeArgs m{};
    m.rec = d_rec; m.nsrc = nsrc; m.nq = nq; m.k = k; m.C = C;
    m.out = QueryOut{d_pred, d_dist, d_idx, nullptr, k, 0};
    m.status = c->ctrl.as<int32_t>();
    stage_begin(c, st, "merge_vote");
    HIP_OR_FAIL(c, knn_launch_merge(m, st));
    stage_end(c, st);
    return finish_call(c, st);
}

// ---------------------------------------------------------------------------------
// Consumers of the exact top-k lists: the k-sweep's vote (k_vote_sweep), the weighted vote
// (k_vote_weighted) and regression (k_regress_sweep; knn_amd.h "Regression").  A consumer is a
// ListConsumer, its texts and its *_enqueue function; the argument checks (list_check), the
// consumer alone on the caller's lists (lists_vote), the pass loop over device datasets
// (lists_core) and the batch loop over host arrays (lists_host) are shared.
// ---------------------------------------------------------------------------------
namespace {

// (LOF_SCORES runs its own kernels, lof_enqueue, behind a pass loop of its own: its scores need
// every row's list; it is a kind here for list_check and its texts)
enum ConsumerKind { VOTE_SWEEP = 0, VOTE_WEIGHTED = 1, REGRESS = 2, LOF_SCORES = 3 };

// What a call asks of its consumer.  Per query every element is 4 bytes wide (int32 labels and
// predictions for the class votes, float targets and predictions for regression) and every
// accumulator element 8 (int64 counts, double sums): the shared loops offset, stage and copy them
// without knowing which.
struct ListConsumer {
    ConsumerKind kind;
    int weights;           // knn_weight (VOTE_WEIGHTED, REGRESS)
    int row0;              // the first prefix row written: pred_all then points at that row
    const float* targets;  // REGRESS: the train targets
    const void* qside;     // the queries' labels or, REGRESS, targets [nq]
    void* pred_all;        // [kmax - row0] rows, pred_stride apart
    int64_t pred_stride;
    void* acc[2];          // per-k accumulators [kmax]: correct | sse, sae
    float* scores;         // VOTE_WEIGHTED: per-class scores [nq][C]
    float* dist_out;       // the lists the caller asked for, [nq][kmax]
    int32_t* idx_out;
};

ListConsumer sweep_consumer(const int32_t* qlabels, int32_t* pred_all, int64_t pred_stride, int64_t* correct,
                            float* dist_out, int32_t* idx_out) {
    return {VOTE_SWEEP, 0, 0, nullptr, qlabels, pred_all, pred_stride, {correct, nullptr}, nullptr, dist_out, idx_out};
}
ListConsumer weighted_consumer(int weights, int row0, const int32_t* qlabels, int32_t* pred_all, int64_t pred_stride,
                               int64_t* correct, float* scores, float* dist_out, int32_t* idx_out) {
    return {VOTE_WEIGHTED, weights, row0, nullptr, qlabels, pred_all, pred_stride, {correct, nullptr}, scores,
            dist_out, idx_out};
}
ListConsumer regress_consumer(int weights, int row0, const float* targets, const float* qtargets, float* pred_all,
                              int64_t pred_stride, double* sse, double* sae, float* dist_out, int32_t* idx_out) {
    return {REGRESS, weights, row0, targets, qtargets, pred_all, pred_stride, {sse, sae}, nullptr, dist_out, idx_out};
}

// the consumers' error texts, by kind.  bad_lists is lists_vote's printf format for (nq, kin,
// stride, C); regression has no classes and prints no C.
const struct {
    const char *prefix, *none_asked, *needs_side, *bad_lists, *null_lists;
} kConsumerText[] = {
    {"sweep", "query labels, pred_all and correct are all NULL", "correct needs the query labels",
     "vote sweep: bad nq=%lld kin=%d idx_stride=%lld C=%d", "vote sweep: d_idx / d_train_labels is NULL"},
    {"weighted vote", "query labels, pred_all, correct and scores are all NULL", "correct needs the query labels",
     "weighted vote: bad nq=%lld kin=%d stride=%lld C=%d", "weighted vote: d_idx / d_dist / d_train_labels is NULL"},
    {"regression", "pred_all, sse and sae are all NULL", "sse / sae need the query targets",
     "regression: bad nq=%lld kin=%d stride=%lld", "regression: d_idx / d_dist / d_train_targets is NULL"},
    {"lof", "kd, lrd and lof are all NULL", "", "lof: bad n=%lld kin=%d stride=%lld", "lof: d_idx / d_dist is NULL"},
};
// the local outlier factor's other texts
const struct {
    const char *bad_range, *bad_kin, *bad_self, *no_tables, *bad_index, *bad_dist, *too_few;
} kLofText = {
    "lof: k_lo=%d, k_hi=%d outside 1 <= k_lo <= k_hi <= 255",
    "lof: kin=%d is not k_hi=%d (+ 1 with self_base)",
    "lof: self_base=%lld must be 0 (row i is list i's own row) or negative (none)",
    "lof: the fitted kd / lrd tables and the output are needed",
    "lof: a list index is outside [0, n)",
    "lof: a neighbour distance is NaN or negative",
    "lof: a list is shorter than k_hi (fewer than k_hi other rows have a finite distance): NaN from that k on",
};

// what every entry point of a consumer checks: the kind of weights, the outputs asked for (the
// query labels count as one: a class vote's caller may want the status alone; regression's query
// targets do not) and the list length
knn_status list_check(knn_ctx* c, const ListConsumer& lc, int32_t kmax, int64_t self_base) {
    const char* p = kConsumerText[lc.kind].prefix;
    if (lc.kind != VOTE_SWEEP) {
        if (lc.weights != KNN_W_UNIFORM && lc.weights != KNN_W_INV_DIST && lc.weights != KNN_W_INV_SQDIST)
            return fail(c, KNN_EINVAL, "%s: unknown weights=%d", p, lc.weights);
        if (lc.weights == KNN_W_INV_SQDIST && c->metric != KNN_METRIC_SQEUCLIDEAN)
            return fail(c, KNN_EINVAL, "%s: KNN_W_INV_SQDIST needs the squared Euclidean metric (metric=%d)", p,
                        c->metric);
    }
    if (kmax < 1) return fail(c, KNN_EINVAL, "%s: kmax=%d must be >= 1", p, kmax);
    if (!(lc.kind != REGRESS && lc.qside) && !lc.pred_all && !lc.acc[0] && !lc.acc[1] && !lc.scores)
        return fail(c, KNN_EINVAL, "%s: %s", p, kConsumerText[lc.kind].none_asked);
    if ((lc.acc[0] || lc.acc[1]) && !lc.qside) return fail(c, KNN_EINVAL, "%s: %s", p, kConsumerText[lc.kind].needs_side);
    if (self_base >= 0 && kmax + 1 > 1024)
        return fail(c, KNN_EINVAL, "%s: kmax=%d + the self row exceeds the supported maximum 1024", p, kmax);
    return KNN_OK;
}

// The kernels' weight kind.  A non-Euclidean metric's distance is no square: KNN_W_INV_DIST is
// 1.0f / D there, the kernels' inverse-of-the-value kind (list_check refused KNN_W_INV_SQDIST).
int kernel_weights(const knn_ctx* c, int weights) {
    return (c->metric != KNN_METRIC_SQEUCLIDEAN && weights == KNN_W_INV_DIST) ? KNN_VOTE_W_INV_SQDIST : weights;
}

// the lists a consumer runs on, in device memory: the first kin entries of rows stride apart;
// check_dist: they are the caller's, not a pass's (a NaN or negative distance is an error)
struct Lists {
    const int32_t* idx;
    const float* dist;
    int64_t nq, stride;
    int kin;
    bool check_dist;
};

// k_vote_sweep on lists in device memory, enqueued on st (no synchronisation)
knn_status vote_sweep_enqueue(knn_ctx* c, const ListConsumer& lc, const Lists& L, int C, const int32_t* labels,
                              int64_t self_base, hipStream_t st) {
    VoteSweepArgs v{};
    v.idx = L.idx; v.idx_stride = L.stride; v.labels = labels;
    v.nq = L.nq; v.kin = L.kin; v.kmax = self_base >= 0 ? L.kin - 1 : L.kin; v.C = C; v.self_base = self_base;
    v.qlabels = static_cast<const int32_t*>(lc.qside);
    v.pred_all = static_cast<int32_t*>(lc.pred_all); v.pred_stride = lc.pred_stride;
    v.correct = static_cast<unsigned long long*>(lc.acc[0]);
    v.dist_in = L.dist; v.dist_out = L.dist ? lc.dist_out : nullptr; v.idx_out = lc.idx_out;
    v.status = c->ctrl.as<int32_t>();
    stage_begin(c, st, "vote_sweep");
    HIP_OR_FAIL(c, knn_launch_vote_sweep(v, st));
    stage_end(c, st);
    return KNN_OK;
}

// k_vote_weighted on lists in device memory, enqueued on st (no synchronisation); scores is
// zeroed here, ahead of the kernel on the same stream
knn_status vote_weighted_enqueue(knn_ctx* c, const ListConsumer& lc, const Lists& L, int C, const int32_t* labels,
                                 int64_t self_base, hipStream_t st) {
    VoteWeightedArgs v{};
    v.idx = L.idx; v.dist = L.dist; v.stride = L.stride; v.labels = labels;
    v.nq = L.nq; v.kin = L.kin; v.kmax = self_base >= 0 ? L.kin - 1 : L.kin; v.C = C;
    v.weights = kernel_weights(c, lc.weights);
    v.self_base = self_base;
    v.qlabels = static_cast<const int32_t*>(lc.qside);
    v.pred_all = static_cast<int32_t*>(lc.pred_all); v.pred_stride = lc.pred_stride; v.row0 = lc.row0;
    v.correct = static_cast<unsigned long long*>(lc.acc[0]);
    v.scores = lc.scores; v.dist_out = L.dist ? lc.dist_out : nullptr; v.idx_out = lc.idx_out;
    v.check_dist = L.check_dist ? 1 : 0;
    v.status = c->ctrl.as<int32_t>();
    stage_begin(c, st, "vote_weighted");
    if (lc.scores && L.nq > 0) HIP_OR_FAIL(c, hipMemsetAsync(lc.scores, 0, sizeof(float) * (size_t)L.nq * (size_t)C, st));
    HIP_OR_FAIL(c, knn_launch_vote_weighted(v, st));
    stage_end(c, st);
    return KNN_OK;
}

// k_regress_sweep (+ k_regress_reduce, which adds into sse / sae) on lists in device memory,
// enqueued on st (no synchronisation)
knn_status regress_enqueue(knn_ctx* c, const ListConsumer& lc, const Lists& L, int64_t self_base, hipStream_t st) {
    RegressArgs v{};
    v.idx = L.idx; v.dist = L.dist; v.stride = L.stride; v.targets = lc.targets;
    v.nq = L.nq; v.kin = L.kin; v.kmax = self_base >= 0 ? L.kin - 1 : L.kin;
    v.weights = kernel_weights(c, lc.weights);
    v.self_base = self_base;
    v.qtargets = static_cast<const float*>(lc.qside);
    v.pred_all = static_cast<float*>(lc.pred_all); v.pred_stride = lc.pred_stride; v.row0 = lc.row0;
    v.dist_out = L.dist ? lc.dist_out : nullptr; v.idx_out = lc.idx_out;
    v.check_dist = L.check_dist ? 1 : 0;
    v.status = c->ctrl.as<int32_t>();
    double *sse = static_cast<double*>(lc.acc[0]), *sae = static_cast<double*>(lc.acc[1]);
    if ((sse || sae) && L.nq > 0) {
        HIP_OR_FAIL(c, c->rg_part.ensure(sizeof(double) * 2 * (size_t)v.kmax * (size_t)knn_regress_chunks(L.nq)));
        v.part = c->rg_part.as<double>();
    }
    stage_begin(c, st, "regress");
    HIP_OR_FAIL(c, knn_launch_regress(v, st));
    if (v.part) HIP_OR_FAIL(c, knn_launch_regress_reduce(v.part, L.nq, v.kmax, lc.row0, sse, sae, st));
    stage_end(c, st);
    return KNN_OK;
}

knn_status consumer_enqueue(knn_ctx* c, const ListConsumer& lc, const Lists& L, int C, const int32_t* labels,
                            int64_t self_base, hipStream_t st) {
    switch (lc.kind) {
        case VOTE_SWEEP: return vote_sweep_enqueue(c, lc, L, C, labels, self_base, st);
        case VOTE_WEIGHTED: return vote_weighted_enqueue(c, lc, L, C, labels, self_base, st);
        case REGRESS: return regress_enqueue(c, lc, L, self_base, st);
        default: return fail(c, KNN_EINVAL, "%s: not a per-pass consumer", kConsumerText[lc.kind].prefix);
    }
}

// the context-owned all-zero label array of n entries the vote-less passes of callers without
// classes run with (regression, the local outlier factor)
knn_status zero_labels(knn_ctx* c, int64_t n, hipStream_t st, const int32_t** out) {
    const size_t need = sizeof(int32_t) * (size_t)std::max<int64_t>(n, 1);
    if (need > c->rg_zero.bytes || !c->rg_zero.p) {
        HIP_OR_FAIL(c, c->rg_zero.ensure(need));
        HIP_OR_FAIL(c, hipMemsetAsync(c->rg_zero.p, 0, need, st));
    }
    *out = c->rg_zero.as<int32_t>();
    return KNN_OK;
}

hipError_t zero_accumulators(const ListConsumer& lc, int32_t kmax, hipStream_t st) {
    for (void* a : lc.acc)
        if (a)
            if (hipError_t e = hipMemsetAsync(a, 0, 8 * (size_t)kmax, st)) return e;
    return hipSuccess;
}

// knn_vote_sweep_device, knn_vote_weighted_device and knn_regress_vote_device: the consumer alone
// on the caller's lists.  inputs: every array the kind reads is there.
knn_status lists_vote(knn_ctx* c, const ListConsumer& lc, const Lists& L, int32_t C, const int32_t* labels,
                      int64_t self_base, bool inputs, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    c->stages.clear();
    const int32_t kmax = self_base >= 0 ? L.kin - 1 : L.kin;
    if (L.nq < 0 || L.kin < 1 || L.kin > 1024 || L.stride < L.kin || C < 1 || C > 16384)
        return fail(c, KNN_EINVAL, kConsumerText[lc.kind].bad_lists, (long long)L.nq, L.kin, (long long)L.stride, C);
    knn_status s;
    if ((s = list_check(c, lc, kmax, self_base)) != KNN_OK) return s;
    if (L.nq > 0 && !inputs) return fail(c, KNN_EINVAL, "%s", kConsumerText[lc.kind].null_lists);
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIP_OR_FAIL(c, reset_ctrl(c, st));
    HIP_OR_FAIL(c, zero_accumulators(lc, kmax, st));
    if ((s = consumer_enqueue(c, lc, L, C, labels, self_base, st)) != KNN_OK) return s;
    return finish_call(c, st);
}

// The pass loop of every consumer over device datasets: one top-kin pass with no vote
// (QueryOut.pred == NULL) into the context's list workspace, the consumer behind it on the same
// stream, one finish_call.  The GEMM path runs more than c->ws_queries queries in passes, like
// predict_core; each pass ends in its own finish_call and adds into the accumulators, which are
// zeroed here first unless the caller has (lists_host, batch after batch).  Regression has no
// classes: its callers pass C = 1, and the pass runs on a context-owned all-zero label array.
// Its GEMM passes are cut at multiples of the reduce's span, so that sse / sae are the bits of a
// single pass.
knn_status lists_core(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int32_t kmax, int32_t C,
                      int64_t self_base, const ListConsumer& lc, bool zero_acc, hipStream_t st) {
    knn_status s;
    const bool regress = lc.kind == REGRESS;
    const int kin = kmax + (self_base >= 0 ? 1 : 0);
    knn_dataset trv;  // regression's train view
    if (regress) {
        if (!tr) return fail(c, KNN_EINVAL, "train dataset is NULL");
        trv = *tr;
        trv.labels = static_cast<const int32_t*>(tr->feat);  // (for the checks; the zero array replaces it below)
        tr = &trv;
    }
    QueryOut out{nullptr, nullptr, nullptr, nullptr, kin, 0};
    if ((s = validate_call(c, tr, te, kin, C, out, false, false)) != KNN_OK) return s;
    if (self_base >= 0 && self_base + te->n > tr->n)
        return fail(c, KNN_EINVAL, "%s: self rows [%lld, %lld) outside the %lld train rows",
                    regress ? "regression" : "sweep", (long long)self_base, (long long)(self_base + te->n),
                    (long long)tr->n);
    if (regress && te->n > 0 && !lc.targets) return fail(c, KNN_EINVAL, "regression: the train targets are NULL");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    if (zero_acc) HIP_OR_FAIL(c, zero_accumulators(lc, kmax, st));
    if (te->n == 0) {
        HIP_OR_FAIL(c, hipStreamSynchronize(st));
        return KNN_OK;
    }
    if (regress && (s = zero_labels(c, tr->n, st, &trv.labels)) != KNN_OK) return s;
    const int algo = choose_algo(c, tr->n, te->n, tr->d, kin, tr->dtype);
    const bool gemm = is_gemm(algo);
    const int64_t grain = regress ? (int64_t)KNN_REGRESS_CHUNK * KNN_REGRESS_SPAN : 1;
    int64_t pass = gemm ? std::max<int64_t>(1, c->ws_queries) : te->n;
    if (gemm && pass >= grain) pass -= pass % grain;
    const int64_t rows = std::min(pass, te->n);
    // (the weighted kinds read the distances whether or not the caller asked for them)
    const bool keep_dist = lc.kind != VOTE_SWEEP || lc.dist_out;
    HIP_OR_FAIL(c, c->sw_idx.ensure(sizeof(int32_t) * (size_t)rows * kin));
    if (keep_dist) HIP_OR_FAIL(c, c->sw_dist.ensure(sizeof(float) * (size_t)rows * kin));
    out.idx = c->sw_idx.as<int32_t>();
    out.dist = keep_dist ? c->sw_dist.as<float>() : nullptr;
    for (int64_t q0 = 0; q0 < te->n; q0 += pass) {
        const int64_t n = std::min(pass, te->n - q0);
        const knn_dataset tq = offset_rows(*te, q0, n);
        if ((s = predict_enqueue(c, tr, &tq, kin, C, out, st, algo, nullptr)) == KNN_OK) {
            ListConsumer pc = lc;  // the consumer's view of the queries from q0 on
            if (pc.qside) pc.qside = static_cast<const char*>(pc.qside) + 4 * q0;
            if (pc.pred_all) pc.pred_all = static_cast<char*>(pc.pred_all) + 4 * q0;
            if (pc.scores) pc.scores += q0 * C;
            if (pc.dist_out) pc.dist_out += q0 * kmax;
            if (pc.idx_out) pc.idx_out += q0 * kmax;
            s = consumer_enqueue(c, pc, Lists{out.idx, out.dist, n, kin, kin, false}, C, tr->labels,
                                 self_base >= 0 ? self_base + q0 : -1, st);
        }
        if (s != KNN_OK || (s = finish_call(c, st)) != KNN_OK) {
            if (s != KNN_EINVAL && s != KNN_ERANGE) c->tprep.valid = c->tpad.valid = false;  // a HIP failure: the operands may be partial
            return s;
        }
        pass_stats(c, c->ctrl_host, gemm);
    }
    return KNN_OK;
}

// knn_sweep_device, knn_sweep_weighted_device, knn_predict_weighted_device, knn_regress_sweep_device
// and knn_regress_device: the checks, then the pass loop on the caller's stream
knn_status lists_device(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int32_t kmax, int32_t C,
                        int64_t self_base, const ListConsumer& lc, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    knn_status s;
    if ((s = list_check(c, lc, kmax, self_base)) != KNN_OK) return s;
    reset_stats(c);
    return lists_core(c, tr, te, kmax, C, self_base, lc, true, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

// knn_sweep, knn_sweep_weighted and knn_regress_sweep: lc holds the caller's HOST arrays.  One
// batch after another (not pipelined): each is uploaded with its side input, run through
// lists_core, and its pred_all rows and scores are copied back.  The accumulators stay on the
// device, added into batch after batch, and come back once at the end.
knn_status lists_host(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int32_t kmax, int32_t C,
                      int64_t self_base, const ListConsumer& lc) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    knn_status s;
    const bool regress = lc.kind == REGRESS;
    if ((s = check_dataset(c, tr, "train", !regress)) != KNN_OK) return s;
    if ((s = check_dataset(c, te, "test", false)) != KNN_OK) return s;
    if ((s = list_check(c, lc, kmax, self_base)) != KNN_OK) return s;
    if (tr->d != te->d) return fail(c, KNN_EINVAL, "feature count mismatch: train d=%d test d=%d", tr->d, te->d);
    if (tr->dtype != te->dtype) return fail(c, KNN_EINVAL, "train and test dtypes differ");
    const int64_t nq = te->n;
    const int kin = kmax + (self_base >= 0 ? 1 : 0);
    if (kin > tr->n) return fail(c, KNN_EINVAL, "k=%d outside [1, n_train=%lld]", kin, (long long)tr->n);
    if (self_base >= 0 && self_base + nq > tr->n)
        return fail(c, KNN_EINVAL, "%s: self rows [%lld, %lld) outside the %lld train rows",
                    regress ? "regression" : "sweep", (long long)self_base, (long long)(self_base + nq),
                    (long long)tr->n);
    if (regress && tr->n > 0 && !lc.targets) return fail(c, KNN_EINVAL, "regression: the train targets are NULL");
    reset_stats(c);
    for (void* a : lc.acc)
        if (a) std::memset(a, 0, 8 * (size_t)kmax);
    if (nq == 0) return KNN_OK;
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int d = tr->d;
    const size_t es = (size_t)elem_size(tr->dtype);
    const int ldd = device_ld(d, tr->dtype);
    int64_t B = std::min<int64_t>(nq, c->batch_rows);
    if (regress) {
        // batches are cut at multiples of the reduce's span: the sums then are the bits
        // knn_regress_sweep_device gives for all queries
        const int64_t span = (int64_t)KNN_REGRESS_CHUNK * KNN_REGRESS_SPAN;
        B = std::min<int64_t>(nq, std::max<int64_t>(span, c->batch_rows - c->batch_rows % span));
    } else if (lc.scores && C >= 1) {
        B = std::min<int64_t>(B, std::max<int64_t>(1, ((int64_t)64 << 20) / C));  // a batch's scores stay under 256 MiB
    }
    if ((s = validate_host_shapes(c, tr, B, ldd, kin, C, QueryOut{nullptr, nullptr, nullptr, nullptr, kin, 0}, false)) !=
        KNN_OK)
        return s;
    // every error from here on drains the stream (no copy from or to the caller's buffers
    // outlives the call) and drops the train cache entry (its upload may not have run)
    auto abort_call = [&](knn_status e) {
        (void)hipStreamSynchronize(st);
        c->tcache.valid = false;
        c->tprep.valid = c->tpad.valid = false;
        return e;
    };
    knn_dataset trn = *tr, dtr;
    if (regress) trn.labels = nullptr;  // no classes: train_device uploads zeros
    if ((s = train_device(c, &trn, st, &dtr)) != KNN_OK) return abort_call(s);
    ListConsumer dc = lc;  // the consumer on the device copies of one batch
    if (regress) {
        HIP_OR_ABORT(c->rg_targets.ensure(sizeof(float) * (size_t)tr->n));
        HIP_OR_ABORT(hipMemcpyAsync(c->rg_targets.p, lc.targets, sizeof(float) * (size_t)tr->n, hipMemcpyHostToDevice, st));
        dc.targets = c->rg_targets.as<float>();
    }
    HIP_OR_ABORT(c->q_slot[0].ensure(es * (size_t)ldd * B));
    if (lc.pred_all) HIP_OR_ABORT(c->sw_pred.ensure(4 * (size_t)kmax * B));
    if (lc.qside) HIP_OR_ABORT(c->sw_qside.ensure(4 * (size_t)B));
    if (lc.scores) HIP_OR_ABORT(c->sw_scores.ensure(sizeof(float) * (size_t)B * (size_t)C));
    if (lc.acc[0] || lc.acc[1]) {
        HIP_OR_ABORT(c->sw_acc.ensure(8 * 2 * (size_t)kmax));
        HIP_OR_ABORT(hipMemsetAsync(c->sw_acc.p, 0, 8 * 2 * (size_t)kmax, st));
    }
    dc.pred_all = lc.pred_all ? c->sw_pred.p : nullptr;
    dc.qside = lc.qside ? c->sw_qside.p : nullptr;
    dc.scores = lc.scores ? c->sw_scores.as<float>() : nullptr;
    for (int i = 0; i < 2; i++) dc.acc[i] = lc.acc[i] ? c->sw_acc.as<char>() + 8 * (size_t)kmax * i : nullptr;
    for (int64_t q0 = 0; q0 < nq; q0 += B) {
        const int64_t n = std::min(B, nq - q0);
        const unsigned char* src = (const unsigned char*)te->feat + es * (size_t)q0 * (size_t)te->ld;
        HIP_OR_ABORT(hipMemcpy2DAsync(c->q_slot[0].p, es * ldd, src, es * te->ld, es * d, n, hipMemcpyHostToDevice, st));
        if (lc.qside)
            HIP_OR_ABORT(hipMemcpyAsync(c->sw_qside.p, static_cast<const char*>(lc.qside) + 4 * q0, 4 * (size_t)n,
                                        hipMemcpyHostToDevice, st));
        c->stats[7] += (int64_t)(es * d * n);
        const knn_dataset dq{c->q_slot[0].p, nullptr, n, d, ldd, te->dtype};
        dc.pred_stride = n;
        if ((s = lists_core(c, &dtr, &dq, kmax, C, self_base >= 0 ? self_base + q0 : -1, dc, false, st)) != KNN_OK)
            return abort_call(s);
        // (synchronous copies on the null stream: ordered after the context's blocking stream)
        if (lc.pred_all)
            HIP_OR_ABORT(hipMemcpy2D(static_cast<char*>(lc.pred_all) + 4 * q0, 4 * (size_t)nq, c->sw_pred.p, 4 * (size_t)n,
                                     4 * (size_t)n, kmax, hipMemcpyDeviceToHost));
        if (lc.scores)
            HIP_OR_ABORT(hipMemcpy(lc.scores + (size_t)q0 * (size_t)C, c->sw_scores.p, sizeof(float) * (size_t)n * (size_t)C,
                                   hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < 2; i++)
        if (lc.acc[i]) HIP_OR_ABORT(hipMemcpy(lc.acc[i], dc.acc[i], 8 * (size_t)kmax, hipMemcpyDeviceToHost));
    return KNN_OK;
}

}  // namespace

extern "C" {

knn_status knn_vote_sweep_device(knn_ctx* c, int64_t nq, int32_t kin, int32_t C, const int32_t* d_idx,
                                 int64_t idx_stride, const int32_t* d_train_labels, int64_t self_base,
                                 const int32_t* d_query_labels, int32_t* d_pred_all, int64_t* d_correct,
                                 void* hip_stream) {
    return lists_vote(c, sweep_consumer(d_query_labels, d_pred_all, nq, d_correct, nullptr, nullptr),
                      Lists{d_idx, nullptr, nq, idx_stride, kin, true}, C, d_train_labels, self_base,
                      d_idx && d_train_labels, hip_stream);
}

knn_status knn_sweep_device(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int32_t kmax, int32_t C,
                            int64_t self_base, const int32_t* d_query_labels, int32_t* d_pred_all,
                            int64_t* d_correct, float* d_topk_dist, int32_t* d_topk_idx, void* hip_stream) {
    return lists_device(c, tr, te, kmax, C, self_base,
                        sweep_consumer(d_query_labels, d_pred_all, te ? te->n : 0, d_correct, d_topk_dist, d_topk_idx),
                        hip_stream);
}

knn_status knn_sweep(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int32_t kmax, int32_t C,
                     int64_t self_base, const int32_t* query_labels, int32_t* out_pred_all, int64_t* out_correct) {
    return lists_host(c, tr, te, kmax, C, self_base,
                      sweep_consumer(query_labels, out_pred_all, 0, out_correct, nullptr, nullptr));
}

knn_status knn_vote_weighted_device(knn_ctx* c, int64_t nq, int32_t kin, int32_t C, const int32_t* d_idx,
                                    const float* d_dist, int64_t stride, const int32_t* d_train_labels,
                                    int32_t weights, int64_t self_base, const int32_t* d_query_labels,
                                    int32_t* d_pred_all, int64_t* d_correct, float* d_scores, void* hip_stream) {
    return lists_vote(c,
                      weighted_consumer(weights, 0, d_query_labels, d_pred_all, nq, d_correct, d_scores, nullptr, nullptr),
                      Lists{d_idx, d_dist, nq, stride, kin, true}, C, d_train_labels, self_base,
                      d_idx && d_train_labels && (d_dist || weights == KNN_W_UNIFORM), hip_stream);
}

knn_status knn_sweep_weighted_device(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int32_t kmax,
                                     int32_t C, int32_t weights, int64_t self_base, const int32_t* d_query_labels,
                                     int32_t* d_pred_all, int64_t* d_correct, float* d_scores, float* d_topk_dist,
                                     int32_t* d_topk_idx, void* hip_stream) {
    return lists_device(c, tr, te, kmax, C, self_base,
                        weighted_consumer(weights, 0, d_query_labels, d_pred_all, te ? te->n : 0, d_correct, d_scores,
                                          d_topk_dist, d_topk_idx),
                        hip_stream);
}

knn_status knn_predict_weighted_device(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int32_t k,
                                       int32_t C, int32_t weights, int32_t* d_pred, float* d_scores,
                                       float* d_topk_dist, int32_t* d_topk_idx, void* hip_stream) {
    // only row k - 1 of the prefix votes is staged and stored: d_pred is that row
    return lists_device(c, tr, te, k, C, -1,
                        weighted_consumer(weights, k - 1, nullptr, d_pred, te ? te->n : 0, nullptr, d_scores, d_topk_dist,
                                          d_topk_idx),
                        hip_stream);
}

knn_status knn_sweep_weighted(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int32_t kmax, int32_t C,
                              int32_t weights, int64_t self_base, const int32_t* query_labels, int32_t* out_pred_all,
                              int64_t* out_correct, float* out_scores) {
    return lists_host(c, tr, te, kmax, C, self_base,
                      weighted_consumer(weights, 0, query_labels, out_pred_all, 0, out_correct, out_scores, nullptr,
                                        nullptr));
}

knn_status knn_regress_vote_device(knn_ctx* c, int64_t nq, int32_t kin, const int32_t* d_idx, const float* d_dist,
                                   int64_t stride, const float* d_train_targets, int32_t weights, int64_t self_base,
                                   const float* d_query_targets, float* d_pred_all, double* d_sse, double* d_sae,
                                   void* hip_stream) {
    return lists_vote(c,
                      regress_consumer(weights, 0, d_train_targets, d_query_targets, d_pred_all, nq, d_sse, d_sae, nullptr,
                                       nullptr),
                      Lists{d_idx, d_dist, nq, stride, kin, true}, 1, nullptr, self_base,
                      d_idx && d_train_targets && (d_dist || weights == KNN_W_UNIFORM), hip_stream);
}

knn_status knn_regress_sweep_device(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te,
                                    const float* d_train_targets, int32_t kmax, int32_t weights, int64_t self_base,
                                    const float* d_query_targets, float* d_pred_all, double* d_sse, double* d_sae,
                                    float* d_topk_dist, int32_t* d_topk_idx, void* hip_stream) {
    return lists_device(c, tr, te, kmax, 1, self_base,
                        regress_consumer(weights, 0, d_train_targets, d_query_targets, d_pred_all, te ? te->n : 0, d_sse,
                                         d_sae, d_topk_dist, d_topk_idx),
                        hip_stream);
}

knn_status knn_regress_device(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, const float* d_train_targets,
                              int32_t k, int32_t weights, float* d_pred, float* d_topk_dist, int32_t* d_topk_idx,
                              void* hip_stream) {
    // only row k - 1 of the prefix predictions is staged and stored: d_pred is that row
    return lists_device(c, tr, te, k, 1, -1,
                        regress_consumer(weights, k - 1, d_train_targets, nullptr, d_pred, te ? te->n : 0, nullptr, nullptr,
                                         d_topk_dist, d_topk_idx),
                        hip_stream);
}

knn_status knn_regress_sweep(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, const float* train_targets,
                             int32_t kmax, int32_t weights, int64_t self_base, const float* query_targets,
                             float* out_pred_all, double* out_sse, double* out_sae) {
    return lists_host(c, tr, te, kmax, 1, self_base,
                      regress_consumer(weights, 0, train_targets, query_targets, out_pred_all, 0, out_sse, out_sae, nullptr,
                                       nullptr));
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// Local outlier factor (knn_amd.h "Local outlier factor"): k_lof_compact, k_lof_lrd, k_lof_score
// behind the vote-less top-k pass.  A row's score reads its neighbours' lists, so the kernels start
// after the LAST pass of the loop, over all rows: how the loop cuts the rows cannot change a bit.
// ---------------------------------------------------------------------------------
namespace {

struct LofOut {
    float* kd; double* lrd; float* lof; int64_t lof_stride;
};

knn_status lof_args_check(knn_ctx* c, int32_t k_lo, int32_t k_hi, int64_t self_base, const void* any_out) {
    if (k_lo < 1 || k_hi > KNN_LOF_MAX_K || k_lo > k_hi) return fail(c, KNN_EINVAL, kLofText.bad_range, k_lo, k_hi);
    return list_check(c,
                      ListConsumer{LOF_SCORES, KNN_W_UNIFORM, 0, nullptr, nullptr, const_cast<void*>(any_out), 0,
                                   {nullptr, nullptr}, nullptr, nullptr, nullptr},
                      k_hi, self_base);
}

// The three kernels on lists in device memory, enqueued on st (no synchronisation).  kd_fit /
// lrd_fit: the fitted tables of n_table rows (novelty: the lists are queries'); NULL: the lists are
// the table rows' own, and kd / lrd are computed (into the caller's arrays or workspace).
knn_status lof_enqueue(knn_ctx* c, const Lists& L, int64_t self_base, int64_t n_table, int k_lo, int k_hi,
                       const float* kd_fit, const double* lrd_fit, const LofOut& o, hipStream_t st) {
    const size_t Kr = (size_t)(k_hi - k_lo + 1), nq = (size_t)L.nq;
    const bool novelty = kd_fit != nullptr;
    HIP_OR_FAIL(c, c->lof_cidx.ensure(sizeof(int32_t) * nq * (size_t)k_hi));
    HIP_OR_FAIL(c, c->lof_delta.ensure(sizeof(float) * nq * (size_t)k_hi));
    float* kd = novelty ? nullptr : o.kd;
    if (!novelty && !kd) {
        HIP_OR_FAIL(c, c->lof_kd.ensure(sizeof(float) * nq * Kr));
        kd = c->lof_kd.as<float>();
    }
    LofCompactArgs a{};
    a.idx = L.idx; a.dist = L.dist; a.stride = L.stride;
    a.nq = L.nq; a.n_table = n_table; a.kin = L.kin; a.k_lo = k_lo; a.k_hi = k_hi; a.self_base = self_base;
    a.euclid = c->metric == KNN_METRIC_SQEUCLIDEAN ? 1 : 0;
    a.check_dist = L.check_dist ? 1 : 0;
    a.cidx = c->lof_cidx.as<int32_t>(); a.delta = c->lof_delta.as<float>(); a.kd = kd;
    a.status = c->ctrl.as<int32_t>();
    stage_begin(c, st, "lof");
    HIP_OR_FAIL(c, knn_launch_lof_compact(a, st));
    stage_end(c, st);
    if (!novelty && !o.lrd && !o.lof) return KNN_OK;
    double* lrd = novelty ? nullptr : o.lrd;
    if (!lrd) {
        DBuf& ws = novelty ? c->lof_qlrd : c->lof_lrd;
        HIP_OR_FAIL(c, ws.ensure(sizeof(double) * nq * Kr));
        lrd = ws.as<double>();
    }
    LofWalkArgs w{};
    w.cidx = a.cidx; w.delta = a.delta; w.nq = L.nq; w.k_lo = k_lo; w.k_hi = k_hi;
    w.kd_table = novelty ? kd_fit : kd; w.lrd_out = lrd;
    stage_begin(c, st, "lof");
    HIP_OR_FAIL(c, knn_launch_lof_lrd(w, st));
    stage_end(c, st);
    if (!o.lof) return KNN_OK;
    w.lrd_table = novelty ? lrd_fit : lrd; w.lrd_own = lrd; w.lof = o.lof; w.lof_stride = o.lof_stride;
    stage_begin(c, st, "lof");
    HIP_OR_FAIL(c, knn_launch_lof_score(w, st));
    stage_end(c, st);
    return KNN_OK;
}

// finish_call behind the LOF kernels: the status word's texts are this feature's
knn_status lof_finish(knn_ctx* c, hipStream_t st) {
    const knn_status s = finish_call(c, st);
    const int32_t status = c->ctrl_host[0];
    if (s == KNN_EINVAL && (status & KNN_STATUS_BAD_INDEX)) return fail(c, s, "%s", kLofText.bad_index);
    if (s == KNN_EINVAL && (status & KNN_STATUS_BAD_DIST)) return fail(c, s, "%s", kLofText.bad_dist);
    if (s == KNN_ERANGE) return fail(c, s, "%s", kLofText.too_few);
    return s;
}

// The vote-less top-kin pass of te against tr (context-owned zero labels, one class, choose_algo as
// it is; kin may exceed the rows: the lists then end in missing entries) into lists [te->n][kin],
// then the LOF kernels on ALL rows behind the last pass and one finish_call for both.  Earlier
// passes of the GEMM path end in their own finish_call, as in lists_core.
knn_status lof_core(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int kin, int64_t self_base, int k_lo,
                    int k_hi, const float* kd_fit, const double* lrd_fit, const LofOut& o, float* d_dist, int32_t* d_idx,
                    hipStream_t st) {
    knn_status s;
    if (!tr || !te) return fail(c, KNN_EINVAL, "%s dataset is NULL", tr ? "test" : "train");
    knn_dataset trv = *tr, tev = *te;
    trv.labels = static_cast<const int32_t*>(tr->feat);  // (for the checks; the zero array replaces it below)
    tev.labels = nullptr;
    QueryOut out{nullptr, nullptr, nullptr, nullptr, kin, 0};
    if ((s = validate_call(c, &trv, &tev, kin, 1, out, true, false)) != KNN_OK) return s;
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    reset_stats(c);
    const int64_t nq = tev.n;
    if (nq == 0) return KNN_OK;
    if ((s = zero_labels(c, trv.n, st, &trv.labels)) != KNN_OK) return s;
    if (!d_idx) {
        HIP_OR_FAIL(c, c->lof_idx.ensure(sizeof(int32_t) * (size_t)nq * kin));
        d_idx = c->lof_idx.as<int32_t>();
    }
    if (!d_dist) {
        HIP_OR_FAIL(c, c->lof_dist.ensure(sizeof(float) * (size_t)nq * kin));
        d_dist = c->lof_dist.as<float>();
    }
    out.idx = d_idx;
    out.dist = d_dist;
    const int algo = choose_algo(c, trv.n, nq, trv.d, kin, trv.dtype);
    const bool gemm = is_gemm(algo);
    const int64_t pass = gemm ? std::max<int64_t>(1, c->ws_queries) : nq;
    for (int64_t q0 = 0; q0 < nq; q0 += pass) {
        const int64_t n = std::min(pass, nq - q0);
        const bool last = q0 + n >= nq;
        const knn_dataset tq = offset_rows(tev, q0, n);
        s = predict_enqueue(c, &trv, &tq, kin, 1, offset_out(out, q0), st, algo, nullptr);
        if (s == KNN_OK && last)
            s = lof_enqueue(c, Lists{d_idx, d_dist, nq, kin, kin, false}, self_base, trv.n, k_lo, k_hi, kd_fit, lrd_fit, o,
                            st);
        if (s != KNN_OK || (s = last ? lof_finish(c, st) : finish_call(c, st)) != KNN_OK) {
            if (s != KNN_EINVAL && s != KNN_ERANGE) c->tprep.valid = c->tpad.valid = false;  // a HIP failure: the operands may be partial
            return s;
        }
        pass_stats(c, c->ctrl_host, gemm);
    }
    return KNN_OK;
}

}  // namespace

extern "C" {

knn_status knn_lof_fit_device(knn_ctx* c, const knn_dataset* tr, int32_t k_lo, int32_t k_hi, float* d_kd, double* d_lrd,
                              float* d_lof, float* d_dist, int32_t* d_idx, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    knn_status s;
    const void* any = d_kd ? (const void*)d_kd : d_lrd ? (const void*)d_lrd : (const void*)d_lof;
    if ((s = lof_args_check(c, k_lo, k_hi, 0, any)) != KNN_OK) return s;
    return lof_core(c, tr, tr, k_hi + 1, 0, k_lo, k_hi, nullptr, nullptr, LofOut{d_kd, d_lrd, d_lof, tr ? tr->n : 0}, d_dist,
                    d_idx, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

knn_status knn_lof_score_device(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, int32_t k_lo, int32_t k_hi,
                                const float* d_kd, const double* d_lrd, float* d_lof_out, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    knn_status s;
    if ((s = lof_args_check(c, k_lo, k_hi, -1, d_lof_out)) != KNN_OK) return s;
    if (te && te->n > 0 && (!d_kd || !d_lrd || !d_lof_out)) return fail(c, KNN_EINVAL, "%s", kLofText.no_tables);
    return lof_core(c, tr, te, k_hi, -1, k_lo, k_hi, d_kd, d_lrd, LofOut{nullptr, nullptr, d_lof_out, te ? te->n : 0},
                    nullptr, nullptr, hip_stream ? (hipStream_t)hip_stream : c->stream);
}

knn_status knn_lof_lists_device(knn_ctx* c, int64_t n, int32_t kin, const int32_t* d_idx, const float* d_dist,
                                int64_t stride, int64_t self_base, int32_t k_lo, int32_t k_hi, float* d_kd,
                                double* d_lrd, float* d_lof, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    c->stages.clear();
    knn_status s;
    const void* any = d_kd ? (const void*)d_kd : d_lrd ? (const void*)d_lrd : (const void*)d_lof;
    if ((s = lof_args_check(c, k_lo, k_hi, self_base, any)) != KNN_OK) return s;
    if (self_base > 0) return fail(c, KNN_EINVAL, kLofText.bad_self, (long long)self_base);
    if (kin != k_hi + (self_base >= 0 ? 1 : 0)) return fail(c, KNN_EINVAL, kLofText.bad_kin, kin, k_hi);
    if (n < 0 || n > 0x7fffffffLL || stride < kin)
        return fail(c, KNN_EINVAL, kConsumerText[LOF_SCORES].bad_lists, (long long)n, kin, (long long)stride);
    if (n > 0 && (!d_idx || !d_dist)) return fail(c, KNN_EINVAL, "%s", kConsumerText[LOF_SCORES].null_lists);
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (n == 0) return KNN_OK;
    HIP_OR_FAIL(c, reset_ctrl(c, st));
    if ((s = lof_enqueue(c, Lists{d_idx, d_dist, n, stride, kin, true}, self_base, n, k_lo, k_hi, nullptr, nullptr,
                         LofOut{d_kd, d_lrd, d_lof, n}, st)) != KNN_OK)
        return s;
    return lof_finish(c, st);
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// Radius neighbours (knn_amd.h "Radius neighbours"): k_radius_tile under the context's metric, or
// k_radius_gemm where radius_policy says so
// ---------------------------------------------------------------------------------
namespace {

// what the count and the fill pass check of their datasets and threshold
knn_status radius_check(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, float thr, int64_t self_base,
                        bool need_labels) {
    knn_status s;
    if ((s = check_dataset(c, tr, "train", need_labels)) != KNN_OK) return s;
    if ((s = check_dataset(c, te, "test", false)) != KNN_OK) return s;
    if (tr->d != te->d) return fail(c, KNN_EINVAL, "feature count mismatch: train d=%d test d=%d", tr->d, te->d);
    if (tr->dtype != te->dtype) return fail(c, KNN_EINVAL, "train and test dtypes differ");
    if (!(thr >= 0.0f && thr < FLT_MAX)) return fail(c, KNN_EINVAL, "radius: the threshold must be in [0, FLT_MAX)");
    if (tr->n > 0x7fffffffLL) return fail(c, KNN_EINVAL, "train row indices exceed 2^31-1");
    const int es = elem_size(tr->dtype);
    if (((int64_t)tr->ld * es) % 16 || ((int64_t)te->ld * es) % 16 || (((uintptr_t)tr->feat) & 15) ||
        (((uintptr_t)te->feat) & 15))
        return fail(c, KNN_EINVAL, "device rows must be 16-byte aligned (ld * element size %% 16 == 0)");
    if (self_base >= 0 && self_base + te->n > tr->n)
        return fail(c, KNN_EINVAL, "radius: self rows [%lld, %lld) outside the %lld train rows", (long long)self_base,
                    (long long)(self_base + te->n), (long long)tr->n);
    return KNN_OK;
}

knn_ctx::RadiusKey radius_key(const knn_ctx* c, const RadiusTileArgs& a) {
    uint32_t tb;
    std::memcpy(&tb, &a.thr, sizeof(tb));
    return {a.train, a.test, a.nt, a.nq, a.self_base, a.d, a.ld_t, a.ld_q, a.elem, c->metric, a.nseg, tb, true,
            a.seg_len};
}

// AUTO's floors of the MFMA form (knn_radius_policy): train rows and queries from which
// k_radius_gemm, operand build included, measured not slower than k_radius_tile (DESIGN.md
// "Radius neighbours", "Routing").  The row floor is top-k's (choose_algo).  Whole calls at 16,384
// rows, d = 64, uncached: 256 queries 0.148 ms against the direct form's 0.135 (beyond its 4.1 %
// spread, in every run), 512 queries 0.142 against 0.143, 1,024 0.143 against 0.170; d = 128 is
// faster from 1 query on.  Below the floors both forms are bounded by their launches.
static constexpr int64_t KNN_RADIUS_MFMA_MIN_ROWS = 16384;
static constexpr int64_t KNN_RADIUS_MFMA_MIN_QUERIES = 512;

// the form of a radius pass: 0 direct (k_radius_tile), 1 MFMA (k_radius_gemm)
int radius_policy(int metric, int d, int64_t nt, int64_t nq, int algo) {
    if (metric != KNN_METRIC_SQEUCLIDEAN || !knn_radius_gemm_supported(d)) return 0;
    if (nt < 1 || nq < 1) return 0;  // (nothing to filter: no operands are built)
    if (algo == KNN_ALGO_DIRECT || algo == KNN_ALGO_DIRECT_SCAN) return 0;
    if (algo == KNN_ALGO_GEMM_BF16) return 1;
    return nt >= KNN_RADIUS_MFMA_MIN_ROWS && nq >= KNN_RADIUS_MFMA_MIN_QUERIES ? 1 : 0;
}

// form = 1: k_radius_gemm's segments (multiples of 64 rows), which the direct form behind it
// (unsafe norms) shares, so either leaves the same per-segment counts
RadiusTileArgs radius_args(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, float thr, int64_t self_base,
                           int C, int form = 0) {
    RadiusTileArgs a{};
    a.train = tr->feat; a.labels = tr->labels; a.nt = tr->n; a.ld_t = tr->ld;
    a.test = te->feat; a.ld_q = te->ld; a.nq = te->n;
    a.d = tr->d; a.C = C; a.elem = tr->dtype;
    a.thr = thr; a.self_base = self_base;
    if (form) {
        int qb = 32 * KNN_RADIUS_GEMM_NW, occ = 1;
        if (knn_radius_gemm_units(tr->dtype, tr->d, &qb, &occ) != hipSuccess || occ < 1) occ = 1;
        a.nseg = c->train_splits > 0
                     ? std::min(32, c->train_splits)
                     : fill_segments(tr->n, te->n, (te->n + qb - 1) / qb, (int64_t)occ * c->num_cus, 12.0);
        a.seg_len = std::max<int64_t>(64, ((tr->n + a.nseg - 1) / a.nseg + 63) / 64 * 64);
    } else {
        a.nseg = c->train_splits > 0 ? std::min(32, c->train_splits)
                                     : choose_radius_segments(c, tr->n, te->n, tr->d, C, tr->dtype);
        a.seg_len = (tr->n + a.nseg - 1) / a.nseg;
    }
    a.status = c->ctrl.as<int32_t>();
    c->stats[2] = a.nseg;
    c->stats[13] = form;
    return a;
}

// The MFMA form's operands (the fused filter's, by its launchers, in buffers of this form's own)
// and its arguments from the direct form's.  Train side: norms and tile statistics (k_row_norms),
// their maxima, tile blocks of 64 rows over the 64-row grid -- kept across calls under
// KNN_OPT_CACHE_TRAIN[_DEVICE] like run_gemm's (stats[8] says so).  The train norms' share of the
// status word (KNN_STATUS_GEMM_UNSAFE) is kept with them and copied into this call's, which
// reset_ctrl left zero; the query norms add theirs.
knn_status radius_prep(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, const RadiusTileArgs& a,
                       hipStream_t st, RadiusGemmArgs* g) {
    const int64_t nt = tr->n, nq = te->n;
    const int d = tr->d, dtype = tr->dtype;
    const int64_t tiles = (nt + 63) / 64;
    const bool own_train = tr->feat == c->h_train.p;
    const bool may_cache = c->cache_train && (own_train || c->cache_train_device);
    const uint64_t ep = own_train ? c->train_epoch : 0;
    auto& rp = c->rmprep;
    const bool hit = may_cache && rp.valid && rp.feat == tr->feat && rp.n == nt && rp.d == d && rp.ld == tr->ld &&
                     rp.dtype == dtype && rp.gen == c->generation && rp.epoch == ep;
    rp.valid = false;
    HIP_OR_FAIL(c, c->rm_tctrl.ensure(4 * sizeof(int32_t)));
    HIP_OR_FAIL(c, c->rm_tsmax.ensure(sizeof(float4)));
    HIP_OR_FAIL(c, c->rm_qnorm.ensure(sizeof(float) * nq));
    HIP_OR_FAIL(c, c->rm_qstat.ensure(sizeof(float2) * (nq + 1)));
    HIP_OR_FAIL(c, c->rm_qop.ensure(sizeof(uint16_t) * (size_t)d * nq));
    if (!hit) {
        HIP_OR_FAIL(c, c->rm_tnorm.ensure(sizeof(float) * (tiles * 64)));
        HIP_OR_FAIL(c, c->rm_tmax.ensure(sizeof(float4) * (tiles + 1)));
        HIP_OR_FAIL(c, c->rm_tblk.ensure(knn_radius_gemm_tile_bytes(d) * (size_t)tiles));
    }
    stage_begin(c, st, "radius_norms");
    if (!hit) {
        HIP_OR_FAIL(c, hipMemsetAsync(c->rm_tctrl.p, 0, 4 * sizeof(int32_t), st));
        HIP_OR_FAIL(c, knn_launch_row_norms(tr->feat, dtype, nt, tr->ld, d, c->rm_tnorm.as<float>(),
                                            c->rm_tctrl.as<int32_t>(), nullptr, nullptr, 0.0f, st,
                                            c->rm_tmax.as<float4>()));
        HIP_OR_FAIL(c, knn_launch_tile_stat_max(c->rm_tmax.as<float4>(), tiles, c->rm_tsmax.as<float4>(), st));
    }
    HIP_OR_FAIL(c, hipMemcpyAsync(c->ctrl.p, c->rm_tctrl.p, 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    HIP_OR_FAIL(c, knn_launch_row_norms(te->feat, dtype, nq, te->ld, d, c->rm_qnorm.as<float>(), c->ctrl.as<int32_t>(),
                                        nullptr, nullptr, 0.0f, st, nullptr, nullptr, c->rm_qstat.as<float2>(), -2.0f));
    stage_end(c, st);
    stage_begin(c, st, "radius_operands");
    if (!hit)
        HIP_OR_FAIL(c, knn_launch_tn_rows(tr->feat, dtype, tiles * 64, nt, tr->ld, d, d, c->rm_tnorm.as<float>(), 1.0f,
                                          c->rm_tblk.p, c->rm_tmax.as<float4>(), 64, st));
    HIP_OR_FAIL(c, knn_launch_tn_rows(te->feat, dtype, nq, nq, te->ld, d, d, nullptr, -2.0f, c->rm_qop.p, nullptr, 0, st));
    stage_end(c, st);
    c->stats[8] = hit ? 1 : 0;
    if (may_cache) rp = {tr->feat, nt, d, tr->ld, dtype, c->generation, ep, true};

    RadiusGemmArgs r{};
    r.tblk = c->rm_tblk.p; r.qop = c->rm_qop.p; r.qnorm = c->rm_qnorm.as<float>();
    r.qstat = c->rm_qstat.as<float2>(); r.tsmax = c->rm_tsmax.as<float4>();
    r.train = a.train; r.labels = a.labels; r.nt = nt; r.ld_t = a.ld_t;
    r.test = a.test; r.ld_q = a.ld_q; r.nq = nq;
    r.d = d; r.C = a.C; r.elem = dtype;
    r.seg_len = a.seg_len; r.nseg = a.nseg;
    r.thr = a.thr; r.self_base = a.self_base;
    certificate_fused(d, dtype == KNN_F32, &r.coef, &r.eta);
    r.status = a.status;
    c->rm_counted = false;
    if (c->profile == 2) {
        HIP_OR_FAIL(c, c->rm_exact.ensure(sizeof(unsigned long long)));
        HIP_OR_FAIL(c, hipMemsetAsync(c->rm_exact.p, 0, sizeof(unsigned long long), st));
        r.exact_cnt = c->rm_exact.as<unsigned long long>();
        c->rm_counted = true;
    }
    *g = r;
    return KNN_OK;
}

// a radius call's last step: the synchronisation, then which form ran (stats[13]) and, under
// profile = 2, the pairs the MFMA form evaluated exactly (stats[14])
knn_status radius_finish(knn_ctx* c, hipStream_t st, int form) {
    const knn_status s = finish_call(c, st);
    if (!form) return s;
    if (s != KNN_OK && s != KNN_EINVAL && s != KNN_ERANGE) c->rmprep.valid = false;  // a HIP failure: the operands may be partial
    if (s == KNN_OK || s == KNN_EINVAL) {
        if (c->ctrl_host[0] & KNN_STATUS_GEMM_UNSAFE) c->stats[13] = 2;
        unsigned long long n = 0;
        if (c->rm_counted && hipMemcpy(&n, c->rm_exact.p, sizeof(n), hipMemcpyDeviceToHost) == hipSuccess)
            c->stats[14] = (int64_t)n;
    }
    return s;
}

knn_status weights_check(knn_ctx* c, const char* what, int32_t weights) {
    if (weights != KNN_W_UNIFORM && weights != KNN_W_INV_DIST && weights != KNN_W_INV_SQDIST)
        return fail(c, KNN_EINVAL, "%s: unknown weights=%d", what, weights);
    if (weights == KNN_W_INV_SQDIST && c->metric != KNN_METRIC_SQEUCLIDEAN)
        return fail(c, KNN_EINVAL, "%s: KNN_W_INV_SQDIST needs the squared Euclidean metric (metric=%d)", what,
                    c->metric);
    return KNN_OK;
}

}  // namespace

extern "C" {

knn_status knn_radius_count_device(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, float thr, int32_t C,
                                   int64_t self_base, int32_t outlier_label, const int32_t* d_query_labels,
                                   int32_t* d_count, int32_t* d_class_counts, int32_t* d_pred, int64_t* d_correct,
                                   int64_t* d_offsets, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    reset_stats(c);
    const bool classes = d_class_counts || d_pred || d_correct;
    knn_status s;
    if ((s = radius_check(c, tr, te, thr, self_base, classes)) != KNN_OK) return s;
    if (classes && (C < 1 || C > 16384)) return fail(c, KNN_EINVAL, "num_classes=%d outside [1, 16384]", C);
    if (d_correct && !d_query_labels) return fail(c, KNN_EINVAL, "radius count: correct needs the query labels");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const int64_t nq = te->n;
    if (d_correct) HIP_OR_FAIL(c, hipMemsetAsync(d_correct, 0, sizeof(int64_t), st));
    if (nq == 0) {
        if (d_offsets) HIP_OR_FAIL(c, hipMemsetAsync(d_offsets, 0, sizeof(int64_t), st));
        HIP_OR_FAIL(c, hipStreamSynchronize(st));
        return KNN_OK;
    }
    if (!d_count && !classes && !d_offsets)
        return fail(c, KNN_EINVAL, "radius count: count, class_counts, pred, correct and offsets are all NULL");
    HIP_OR_FAIL(c, reset_ctrl(c, st));
    const int form = radius_policy(c->metric, tr->d, tr->n, nq, c->algo);
    RadiusTileArgs a = radius_args(c, tr, te, thr, self_base, classes ? C : 0, form);
    RadiusGemmArgs g{};
    if (form) {
        if ((s = radius_prep(c, tr, te, a, st, &g)) != KNN_OK) return s;
        a.gate = a.status;
    }
    // (the MFMA form never votes itself: its members add into class_counts, and so does the gated
    // direct pass behind it, which is handed no pred / correct)
    const bool pass_votes = !form && classes && knn_radius_pass_votes(C, a.nseg);
    a.classes = classes ? 1 : 0;
    a.class_counts = d_class_counts;
    if (classes && !pass_votes) {
        // the pass adds into the class counts (and k_radius_argmax reads them): the caller's, or workspace
        if (!a.class_counts) {
            HIP_OR_FAIL(c, c->rd_cc.ensure(sizeof(int32_t) * (size_t)nq * (size_t)C));
            a.class_counts = c->rd_cc.as<int32_t>();
        }
        HIP_OR_FAIL(c, hipMemsetAsync(a.class_counts, 0, sizeof(int32_t) * (size_t)nq * (size_t)C, st));
    } else if (pass_votes) {
        a.pred = d_pred; a.qlabels = d_query_labels; a.outlier = outlier_label;
        a.correct = reinterpret_cast<unsigned long long*>(d_correct);
    }
    // one segment: its counts are the counts
    if (a.nseg == 1 && d_count) {
        a.seg_count = d_count;
    } else {
        c->rd_key.valid = false;
        HIP_OR_FAIL(c, c->rd_segcnt.ensure(sizeof(int32_t) * (size_t)nq * a.nseg));
        a.seg_count = c->rd_segcnt.as<int32_t>();
    }
    stage_begin(c, st, "radius_count");
    if (form) {
        g.classes = a.classes; g.class_counts = a.class_counts; g.seg_count = a.seg_count;
        HIP_OR_FAIL(c, knn_launch_radius_gemm(g, false, st));
    }
    HIP_OR_FAIL(c, knn_launch_radius_tile(a, c->metric, false, st));
    stage_end(c, st);
    if (d_offsets || (a.nseg > 1 && d_count)) {
        stage_begin(c, st, "radius_scan");
        HIP_OR_FAIL(c, knn_launch_radius_scan(a.seg_count, a.nseg, nq, d_count, d_offsets, st));
        stage_end(c, st);
    }
    if (classes && !pass_votes && (d_pred || d_correct)) {
        stage_begin(c, st, "radius_argmax");
        HIP_OR_FAIL(c, knn_launch_radius_argmax(a.class_counts, nq, C, outlier_label, d_query_labels, d_pred,
                                                reinterpret_cast<unsigned long long*>(d_correct), st));
        stage_end(c, st);
    }
    if ((s = radius_finish(c, st, form)) == KNN_OK && a.seg_count == c->rd_segcnt.as<int32_t>())
        c->rd_key = radius_key(c, a);
    return s;
}

knn_status knn_radius_fill_device(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te, float thr,
                                  int64_t self_base, const int64_t* d_offsets, int32_t* d_idx, float* d_dist,
                                  void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    reset_stats(c);
    knn_status s;
    if ((s = radius_check(c, tr, te, thr, self_base, false)) != KNN_OK) return s;
    if (te->n == 0) return KNN_OK;
    // (d_idx may be NULL only when the lists are empty, which the host cannot know: refuse)
    if (!d_offsets || !d_idx) return fail(c, KNN_EINVAL, "radius fill: d_offsets / d_idx is NULL");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    const int64_t nq = te->n;
    HIP_OR_FAIL(c, reset_ctrl(c, st));
    const int form = radius_policy(c->metric, tr->d, tr->n, nq, c->algo);
    RadiusTileArgs a = radius_args(c, tr, te, thr, self_base, 0, form);
    RadiusGemmArgs g{};
    if (form) {
        if ((s = radius_prep(c, tr, te, a, st, &g)) != KNN_OK) return s;
        a.gate = a.status;
    }
    a.offsets = d_offsets; a.idx = d_idx; a.dist = d_dist;
    a.base = d_offsets;
    if (a.nseg > 1) {
        // where each train segment's part of a query's list starts: the segments' own counts --
        // those the count call of this very pass left in workspace, else counted again (the count
        // call may have run with other segments) -- prefixed from the caller's offsets
        const bool counted = c->rd_key.same(radius_key(c, a));
        c->rd_key.valid = false;
        HIP_OR_FAIL(c, c->rd_segcnt.ensure(sizeof(int32_t) * (size_t)nq * a.nseg));
        HIP_OR_FAIL(c, c->rd_base.ensure(sizeof(int64_t) * (size_t)nq * a.nseg));
        a.seg_count = c->rd_segcnt.as<int32_t>();
        if (!counted) {
            stage_begin(c, st, "radius_count");
            if (form) {
                g.seg_count = a.seg_count;
                HIP_OR_FAIL(c, knn_launch_radius_gemm(g, false, st));
            }
            HIP_OR_FAIL(c, knn_launch_radius_tile(a, c->metric, false, st));
            stage_end(c, st);
        }
        stage_begin(c, st, "radius_scan");
        HIP_OR_FAIL(c, knn_launch_radius_bases(a.seg_count, a.nseg, nq, d_offsets, c->rd_base.as<int64_t>(), st));
        stage_end(c, st);
        a.base = c->rd_base.as<int64_t>();
    }
    stage_begin(c, st, "radius_fill");
    if (form) {
        g.base = a.base; g.offsets = a.offsets; g.idx = a.idx; g.dist = a.dist;
        HIP_OR_FAIL(c, knn_launch_radius_gemm(g, true, st));
    }
    HIP_OR_FAIL(c, knn_launch_radius_tile(a, c->metric, true, st));
    stage_end(c, st);
    if ((s = radius_finish(c, st, form)) == KNN_OK && a.nseg > 1) c->rd_key = radius_key(c, a);
    return s;
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// DBSCAN (knn_amd.h "DBSCAN"): the radius passes' RADIUS_LINK / RADIUS_BORDER modes and
// knn_dbscan.hip's kernels around them
// ---------------------------------------------------------------------------------
namespace {

struct DbscanBufs {
    int32_t *count, *parent, *root, *isroot, *cluster, *cand, *nb;
    int64_t *offs, *info;
    unsigned long long* unions;
};

// the tables of a call over n rows; count is the caller's when it asked for it.  nb is a spare
// status word (ctrl[3], zero at a call's start, read back and zeroed by k_finish): the host learns
// the number of border candidates without a copy of its own.
knn_status dbscan_bufs(knn_ctx* c, int64_t n, int32_t* d_count, hipStream_t st, DbscanBufs* b) {
    HIP_OR_FAIL(c, c->db_tab.ensure(sizeof(int32_t) * 5 * (size_t)n));
    HIP_OR_FAIL(c, c->db_offs.ensure(sizeof(int64_t) * ((size_t)n + 1)));
    HIP_OR_FAIL(c, c->db_info.ensure(sizeof(int64_t) * 8));
    if (!d_count) HIP_OR_FAIL(c, c->db_count.ensure(sizeof(int32_t) * (size_t)n));
    int32_t* t = c->db_tab.as<int32_t>();
    b->count = d_count ? d_count : c->db_count.as<int32_t>();
    b->parent = t; b->root = t + n; b->isroot = t + 2 * n; b->cluster = t + 3 * n; b->cand = t + 4 * n;
    b->nb = c->ctrl.as<int32_t>() + 3;
    b->offs = c->db_offs.as<int64_t>();
    b->info = c->db_info.as<int64_t>();
    b->unions = c->profile == 2 ? reinterpret_cast<unsigned long long*>(b->info + 4) : nullptr;
    HIP_OR_FAIL(c, hipMemsetAsync(b->info, 0, sizeof(int64_t) * 8, st));
    return KNN_OK;
}

// after the link step: every core row's root -> cluster numbers -> labels and the cluster table
knn_status dbscan_number(knn_ctx* c, const DbscanBufs& b, int64_t n, int32_t min_samples, int32_t* d_labels,
                         hipStream_t st) {
    stage_begin(c, st, "dbscan_labels");
    HIP_OR_FAIL(c, knn_launch_dbscan_flatten(b.parent, b.count, min_samples, n, b.root, b.isroot, c->ctrl.as<int32_t>(), st));
    HIP_OR_FAIL(c, knn_launch_radius_scan(b.isroot, 1, n, nullptr, b.offs, st));
    HIP_OR_FAIL(c, knn_launch_dbscan_labels(b.root, b.offs, n, d_labels, b.cluster, st));
    stage_end(c, st);
    return KNN_OK;
}

// the summary, the call's one synchronisation, and the counters
knn_status dbscan_end(knn_ctx* c, const DbscanBufs& b, int64_t n, int32_t min_samples, const int32_t* d_labels,
                      int64_t* d_summary, hipStream_t st, int form, bool passes) {
    stage_begin(c, st, "dbscan_labels");
    HIP_OR_FAIL(c, knn_launch_dbscan_summary(d_labels, b.count, min_samples, b.offs, n, b.info, st));
    if (d_summary) HIP_OR_FAIL(c, hipMemcpyAsync(d_summary, b.info, sizeof(int64_t) * 4, hipMemcpyDeviceToDevice, st));
    stage_end(c, st);
    const knn_status s = passes ? radius_finish(c, st, form) : finish_call(c, st);
    if (s == KNN_OK) {
        c->stats[18] = c->ctrl_host[3];
        unsigned long long u = 0;
        if (b.unions && hipMemcpy(&u, b.unions, sizeof(u), hipMemcpyDeviceToHost) == hipSuccess) c->stats[19] = (int64_t)u;
    }
    return s;
}

}  // namespace

extern "C" {

knn_status knn_dbscan_device(knn_ctx* c, const knn_dataset* tr, float thr, int32_t min_samples, int32_t* d_labels,
                             int32_t* d_count, int64_t* d_summary, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    reset_stats(c);
    knn_status s;
    if (min_samples < 1) return fail(c, KNN_EINVAL, "dbscan: min_samples=%d must be >= 1", min_samples);
    if ((s = radius_check(c, tr, tr, thr, -1, false)) != KNN_OK) return s;
    const int64_t n = tr->n;
    if (n > 0 && !d_labels) return fail(c, KNN_EINVAL, "dbscan: d_labels is NULL");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (n == 0) {
        if (d_summary) HIP_OR_FAIL(c, hipMemsetAsync(d_summary, 0, sizeof(int64_t) * 4, st));
        HIP_OR_FAIL(c, hipStreamSynchronize(st));
        return KNN_OK;
    }
    HIP_OR_FAIL(c, reset_ctrl(c, st));
    // the three passes share the count pass's form and segments: the link pass is routed on (n, n),
    // the border pass goes with it (its query count is known on the device alone)
    const int form = radius_policy(c->metric, tr->d, n, n, c->algo);
    RadiusTileArgs a = radius_args(c, tr, tr, thr, -1, 0, form);
    RadiusGemmArgs g{};
    if (form) {
        if ((s = radius_prep(c, tr, tr, a, st, &g)) != KNN_OK) return s;
        a.gate = a.status;
    }
    DbscanBufs b{};
    if ((s = dbscan_bufs(c, n, d_count, st, &b)) != KNN_OK) return s;
    c->rd_key.valid = false;
    if (a.nseg == 1) {
        a.seg_count = b.count;
    } else {
        HIP_OR_FAIL(c, c->rd_segcnt.ensure(sizeof(int32_t) * (size_t)n * a.nseg));
        a.seg_count = c->rd_segcnt.as<int32_t>();
    }
    stage_begin(c, st, "radius_count");
    if (form) {
        g.seg_count = a.seg_count;
        HIP_OR_FAIL(c, knn_launch_radius_gemm(g, RADIUS_COUNT, st));
    }
    HIP_OR_FAIL(c, knn_launch_radius_tile(a, c->metric, RADIUS_COUNT, st));
    stage_end(c, st);
    if (a.nseg > 1) {
        stage_begin(c, st, "radius_scan");
        HIP_OR_FAIL(c, knn_launch_radius_scan(a.seg_count, a.nseg, n, b.count, nullptr, st));
        stage_end(c, st);
    }
    stage_begin(c, st, "dbscan_labels");
    HIP_OR_FAIL(c, knn_launch_dbscan_init(b.parent, n, st));
    stage_end(c, st);

    a.db.dcount = b.count; a.db.min_samples = min_samples; a.db.parent = b.parent; a.db.unions = b.unions;
    a.db.cand = b.cand; a.db.nb = b.nb; a.db.cluster = b.cluster; a.db.out_labels = d_labels;
    g.db = a.db;
    stage_begin(c, st, "dbscan_link");
    if (form) HIP_OR_FAIL(c, knn_launch_radius_gemm(g, RADIUS_LINK, st));
    HIP_OR_FAIL(c, knn_launch_radius_tile(a, c->metric, RADIUS_LINK, st));
    stage_end(c, st);

    if ((s = dbscan_number(c, b, n, min_samples, d_labels, st)) != KNN_OK) return s;

    stage_begin(c, st, "dbscan_border");
    HIP_OR_FAIL(c, knn_launch_dbscan_candidates(b.count, min_samples, n, b.cand, b.nb, st));
    if (form) HIP_OR_FAIL(c, knn_launch_radius_gemm(g, RADIUS_BORDER, st));
    HIP_OR_FAIL(c, knn_launch_radius_tile(a, c->metric, RADIUS_BORDER, st));
    stage_end(c, st);

    return dbscan_end(c, b, n, min_samples, d_labels, d_summary, st, form, true);
}

knn_status knn_dbscan_lists_device(knn_ctx* c, int64_t n, const int64_t* d_offsets, const int32_t* d_idx,
                                   int32_t min_samples, int32_t* d_labels, int32_t* d_count, int64_t* d_summary,
                                   void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    reset_stats_keep_radius(c);
    if (min_samples < 1) return fail(c, KNN_EINVAL, "dbscan lists: min_samples=%d must be >= 1", min_samples);
    if (n < 0 || n > 0x7fffffffLL) return fail(c, KNN_EINVAL, "dbscan lists: n=%lld outside [0, 2^31-1]", (long long)n);
    // (d_idx may be NULL only when the lists are empty, which the host cannot know: refuse)
    if (n > 0 && (!d_offsets || !d_idx || !d_labels))
        return fail(c, KNN_EINVAL, "dbscan lists: d_offsets / d_idx / d_labels is NULL");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (n == 0) {
        if (d_summary) HIP_OR_FAIL(c, hipMemsetAsync(d_summary, 0, sizeof(int64_t) * 4, st));
        HIP_OR_FAIL(c, hipStreamSynchronize(st));
        return KNN_OK;
    }
    HIP_OR_FAIL(c, reset_ctrl(c, st));
    knn_status s;
    DbscanBufs b{};
    if ((s = dbscan_bufs(c, n, d_count, st, &b)) != KNN_OK) return s;
    int32_t* status = c->ctrl.as<int32_t>();
    stage_begin(c, st, "dbscan_labels");
    HIP_OR_FAIL(c, knn_launch_dbscan_lists_count(d_offsets, n, b.count, status, st));
    HIP_OR_FAIL(c, knn_launch_dbscan_init(b.parent, n, st));
    stage_end(c, st);
    stage_begin(c, st, "dbscan_link");
    HIP_OR_FAIL(c, knn_launch_dbscan_lists_link(d_offsets, d_idx, n, b.count, min_samples, b.parent, status, b.unions, st));
    stage_end(c, st);
    if ((s = dbscan_number(c, b, n, min_samples, d_labels, st)) != KNN_OK) return s;
    stage_begin(c, st, "dbscan_border");
    HIP_OR_FAIL(c, knn_launch_dbscan_candidates(b.count, min_samples, n, b.cand, b.nb, st));
    HIP_OR_FAIL(c, knn_launch_dbscan_lists_border(d_offsets, d_idx, n, b.count, b.cand, b.nb, b.cluster, d_labels, st));
    stage_end(c, st);
    return dbscan_end(c, b, n, min_samples, d_labels, d_summary, st, 0, false);
}

int32_t knn_radius_policy(int32_t metric, int32_t dtype, int32_t d, int64_t n_train, int64_t n_query, int32_t algo,
                          int32_t* form) {
    if (!form || d <= 0 || n_train < 0 || n_query < 0 || (dtype != KNN_F32 && dtype != KNN_BF16) ||
        metric < KNN_METRIC_SQEUCLIDEAN || metric > KNN_METRIC_CHEBYSHEV || algo < KNN_ALGO_AUTO || algo > KNN_ALGO_GEMM_I8)
        return KNN_EINVAL;
    *form = radius_policy(metric, d, n_train, n_query, algo);
    return KNN_OK;
}

int32_t knn_filter_policy(int32_t dtype, int32_t d, int32_t k, int64_t n_train, int64_t n_query, int32_t algo,
                          int32_t* form, int32_t* operand_width) {
    if (!form || !operand_width || d <= 0 || k < 1 || n_train < 0 || n_query < 0 ||
        (dtype != KNN_F32 && dtype != KNN_BF16) || algo < KNN_ALGO_AUTO || algo > KNN_ALGO_GEMM_I8)
        return KNN_EINVAL;
    *form = 0;
    *operand_width = 0;
    const int a = choose_algo(algo, KNN_METRIC_SQEUCLIDEAN, n_train, n_query, d, k, dtype);
    if (!is_gemm(a)) return KNN_OK;
    // run_gemm's choice between the fused kernel and k_gemm_filter: the bf16 operand classes run
    // fused wherever knn_fused_plan has a shape for (width, k) -- that does not depend on the
    // device or the query count, which only pick among the shapes
    const int fe = filter_elem(a, dtype), dp = filter_width(fe, d);
    const bool fused = (fe == ELEM_ROUND || fe == ELEM_BF16) && knn_fused_supported(dp) &&
                       knn_fused_plan(dp, k, n_query, 256, FusedForce{}, 1).nw > 0;
    *form = is_wide(fe, dp) ? 3 : fused ? 1 : 2;
    *operand_width = dp;
    return KNN_OK;
}

knn_status knn_radius_vote_device(knn_ctx* c, int64_t nq, int64_t n_train, const int64_t* d_offsets,
                                  const int32_t* d_idx, const float* d_dist, const int32_t* d_train_labels, int32_t C,
                                  int32_t weights, int32_t outlier_label, const int32_t* d_query_labels,
                                  int32_t* d_pred, int64_t* d_correct, float* d_scores, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    reset_stats_keep_radius(c);
    knn_status s;
    if (nq < 0 || n_train < 0 || n_train > 0x7fffffffLL || C < 1 || C > 16384)
        return fail(c, KNN_EINVAL, "radius vote: bad nq=%lld n_train=%lld C=%d", (long long)nq, (long long)n_train, C);
    if ((s = weights_check(c, "radius vote", weights)) != KNN_OK) return s;
    if (nq > 0 && !d_pred && !d_correct && !d_scores)
        return fail(c, KNN_EINVAL, "radius vote: pred, correct and scores are all NULL");
    if (d_correct && !d_query_labels) return fail(c, KNN_EINVAL, "radius vote: correct needs the query labels");
    // (d_idx / d_dist may be NULL when every list is empty, which the host cannot know: refuse)
    if (nq > 0 && (!d_offsets || !d_idx || !d_train_labels || (!d_dist && weights != KNN_W_UNIFORM)))
        return fail(c, KNN_EINVAL, "radius vote: d_offsets / d_idx / d_dist / d_train_labels is NULL");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (d_correct) HIP_OR_FAIL(c, hipMemsetAsync(d_correct, 0, sizeof(int64_t), st));
    if (nq == 0) {
        HIP_OR_FAIL(c, hipStreamSynchronize(st));
        return KNN_OK;
    }
    HIP_OR_FAIL(c, reset_ctrl(c, st));
    RadiusVoteArgs v{};
    v.offsets = d_offsets; v.idx = d_idx; v.dist = d_dist; v.nq = nq; v.n_train = n_train;
    v.labels = d_train_labels; v.C = C; v.weights = kernel_weights(c, weights); v.outlier = outlier_label;
    v.qlabels = d_query_labels; v.pred = d_pred; v.correct = reinterpret_cast<unsigned long long*>(d_correct);
    v.scores = d_scores;
    if (!v.scores) {
        HIP_OR_FAIL(c, c->rd_scores.ensure(sizeof(float) * (size_t)nq * (size_t)C));
        v.scores = c->rd_scores.as<float>();
    }
    v.status = c->ctrl.as<int32_t>();
    stage_begin(c, st, "radius_vote");
    HIP_OR_FAIL(c, hipMemsetAsync(v.scores, 0, sizeof(float) * (size_t)nq * (size_t)C, st));
    HIP_OR_FAIL(c, knn_launch_radius_vote(v, st));
    stage_end(c, st);
    return finish_call(c, st);
}

knn_status knn_radius_regress_device(knn_ctx* c, int64_t nq, int64_t n_train, const int64_t* d_offsets,
                                     const int32_t* d_idx, const float* d_dist, const float* d_train_targets,
                                     int32_t weights, float* d_pred, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    reset_stats_keep_radius(c);
    knn_status s;
    if (nq < 0 || n_train < 0 || n_train > 0x7fffffffLL)
        return fail(c, KNN_EINVAL, "radius regression: bad nq=%lld n_train=%lld", (long long)nq, (long long)n_train);
    if ((s = weights_check(c, "radius regression", weights)) != KNN_OK) return s;
    if (nq == 0) return KNN_OK;
    if (!d_pred) return fail(c, KNN_EINVAL, "radius regression: pred is NULL");
    if (!d_offsets || !d_idx || !d_train_targets || (!d_dist && weights != KNN_W_UNIFORM))
        return fail(c, KNN_EINVAL, "radius regression: d_offsets / d_idx / d_dist / d_train_targets is NULL");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIP_OR_FAIL(c, reset_ctrl(c, st));
    RadiusVoteArgs v{};
    v.offsets = d_offsets; v.idx = d_idx; v.dist = d_dist; v.nq = nq; v.n_train = n_train;
    v.weights = kernel_weights(c, weights);
    v.targets = d_train_targets; v.pred_f = d_pred;
    v.status = c->ctrl.as<int32_t>();
    stage_begin(c, st, "radius_regress");
    HIP_OR_FAIL(c, knn_launch_radius_regress(v, st));
    stage_end(c, st);
    return finish_call(c, st);
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// Radius sweep (knn_amd.h "Radius sweep"): R thresholds in one distance pass
// (k_radius_sweep_tile -> k_radius_sweep_finish), and the vote of every threshold on held lists
// (k_radius_vote_sweep)
// ---------------------------------------------------------------------------------
namespace {

// 1 <= R <= 32 thresholds, each in [0, FLT_MAX), non-decreasing
knn_status sweep_thresholds_check(knn_ctx* c, const char* what, const float* thr, int32_t R) {
    if (R < 1 || R > KNN_RADIUS_SWEEP_MAX_R)
        return fail(c, KNN_EINVAL, "%s: R=%d thresholds outside [1, %d]", what, R, KNN_RADIUS_SWEEP_MAX_R);
    if (!thr) return fail(c, KNN_EINVAL, "%s: thresholds is NULL", what);
    for (int r = 0; r < R; r++) {
        if (!(thr[r] >= 0.0f && thr[r] < FLT_MAX))
            return fail(c, KNN_EINVAL, "%s: threshold %d must be in [0, FLT_MAX)", what, r);
        if (r && thr[r] < thr[r - 1])
            return fail(c, KNN_EINVAL, "%s: thresholds %d and %d descend (the list must be non-decreasing)", what,
                        r - 1, r);
    }
    return KNN_OK;
}

// the bytes of workspace one call may take: what ws_queries queries of the GEMM path's candidate
// workspace take (a quarter of the free HBM at knn_create)
size_t workspace_budget(const knn_ctx* c) {
    return (size_t)std::max<int64_t>(1, c->ws_queries) * (12 * 64 * (size_t)KNN_RESCORE_CAPW + 64);
}

}  // namespace

extern "C" {

int64_t knn_radius_sweep_max_queries(const knn_ctx* c, int32_t R, int32_t C) {
    if (!c || R < 1 || R > KNN_RADIUS_SWEEP_MAX_R || C < 0 || C > 16384) return 0;
    return (int64_t)(workspace_budget(c) / ((size_t)(R + 1) * (size_t)(1 + C) * sizeof(int32_t)));
}

knn_status knn_radius_sweep_count_device(knn_ctx* c, const knn_dataset* tr, const knn_dataset* te,
                                         const float* thresholds, int32_t R, int32_t C, int64_t self_base,
                                         int32_t outlier_label, const int32_t* d_query_labels, int64_t ld_out,
                                         int32_t* d_count, int32_t* d_class_counts, int32_t* d_pred,
                                         int64_t* d_correct, int64_t* d_outliers, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    reset_stats(c);
    const bool classes = d_class_counts || d_pred || d_correct;
    knn_status s;
    if ((s = sweep_thresholds_check(c, "radius sweep", thresholds, R)) != KNN_OK) return s;
    if ((s = radius_check(c, tr, te, thresholds[R - 1], self_base, classes)) != KNN_OK) return s;
    if (classes && (C < 1 || C > 16384)) return fail(c, KNN_EINVAL, "num_classes=%d outside [1, 16384]", C);
    if (d_correct && !d_query_labels) return fail(c, KNN_EINVAL, "radius sweep: correct needs the query labels");
    const int64_t nq = te->n;
    if (ld_out < nq) return fail(c, KNN_EINVAL, "radius sweep: ld_out=%lld < nq=%lld", (long long)ld_out, (long long)nq);
    if (!d_count && !classes && !d_outliers)
        return fail(c, KNN_EINVAL, "radius sweep: count, class_counts, pred, correct and outliers are all NULL");
    if (nq == 0) return KNN_OK;
    // hist [nq][R + 1] | chist [nq][R + 1][C]
    const size_t per_q = (size_t)(R + 1) * (size_t)(1 + (classes ? C : 0)) * sizeof(int32_t);
    const int64_t fit = knn_radius_sweep_max_queries(c, R, classes ? C : 0);
    if (nq > fit)
        return fail(c, KNN_ERANGE,
                    "radius sweep: the histograms of nq=%lld queries (R=%d, num_classes=%d) exceed the workspace "
                    "budget; at most nq=%lld queries fit in one call",
                    (long long)nq, R, classes ? C : 0, (long long)fit);
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIP_OR_FAIL(c, reset_ctrl(c, st));
    HIP_OR_FAIL(c, c->rd_sweep.ensure(per_q * (size_t)nq));

    // the form a single-threshold pass of this shape takes (knn_radius_policy), with its segments
    const int form = radius_policy(c->metric, tr->d, tr->n, nq, c->algo);
    const RadiusTileArgs ta = radius_args(c, tr, te, thresholds[R - 1], self_base, classes ? C : 0, form);
    RadiusSweepArgs a{};
    a.train = tr->feat; a.labels = tr->labels; a.nt = tr->n; a.ld_t = tr->ld;
    a.test = te->feat; a.ld_q = te->ld; a.nq = nq;
    a.d = tr->d; a.C = classes ? C : 0; a.elem = tr->dtype;
    a.self_base = self_base;
    a.classes = classes ? 1 : 0; a.R = R;
    std::copy(thresholds, thresholds + R, a.thr);
    a.nseg = ta.nseg; a.seg_len = ta.seg_len;
    a.hist = c->rd_sweep.as<int32_t>();
    a.chist = classes ? a.hist + (size_t)nq * (R + 1) : nullptr;
    a.status = c->ctrl.as<int32_t>();
    RadiusSweepGemmArgs g{};
    if (form) {
        // k_radius_gemm's operands (radius_prep: cached like a single-threshold pass's) and certificate
        RadiusGemmArgs r{};
        if ((s = radius_prep(c, tr, te, ta, st, &r)) != KNN_OK) return s;
        g.tblk = r.tblk; g.qop = r.qop; g.qnorm = r.qnorm; g.qstat = r.qstat; g.tsmax = r.tsmax;
        g.train = r.train; g.labels = r.labels; g.nt = r.nt; g.ld_t = r.ld_t;
        g.test = r.test; g.ld_q = r.ld_q; g.nq = r.nq;
        g.d = r.d; g.C = a.C; g.elem = r.elem;
        g.seg_len = r.seg_len; g.nseg = r.nseg;
        g.self_base = self_base; g.coef = r.coef; g.eta = r.eta;
        g.classes = a.classes; g.R = R;
        g.hist = a.hist; g.chist = a.chist; g.status = r.status; g.exact_cnt = r.exact_cnt;
        std::copy(thresholds, thresholds + R, g.thr);
        a.gate = a.status;
    }

    stage_begin(c, st, "radius_sweep");
    HIP_OR_FAIL(c, hipMemsetAsync(c->rd_sweep.p, 0, per_q * (size_t)nq, st));
    if (form) HIP_OR_FAIL(c, knn_launch_radius_sweep_gemm(g, st));
    HIP_OR_FAIL(c, knn_launch_radius_sweep_tile(a, c->metric, st));
    stage_end(c, st);

    RadiusSweepFinishArgs f{};
    f.hist = a.hist; f.chist = a.chist; f.nq = nq; f.R = R; f.C = a.C; f.classes = a.classes;
    f.ld_out = ld_out; f.outlier = outlier_label; f.qlabels = d_query_labels;
    f.count = d_count; f.class_counts = d_class_counts; f.pred = d_pred;
    f.correct = reinterpret_cast<unsigned long long*>(d_correct);
    f.outliers = reinterpret_cast<unsigned long long*>(d_outliers);
    stage_begin(c, st, "radius_sweep_finish");
    HIP_OR_FAIL(c, knn_launch_radius_sweep_finish(f, st));
    stage_end(c, st);
    return radius_finish(c, st, form);
}

knn_status knn_radius_vote_sweep_device(knn_ctx* c, int64_t nq, int64_t n_train, const int64_t* d_offsets,
                                        const int32_t* d_idx, const float* d_dist, const int32_t* d_train_labels,
                                        int32_t C, int32_t weights, const float* thresholds, int32_t R,
                                        int32_t outlier_label, const int32_t* d_query_labels, int64_t ld_out,
                                        int32_t* d_pred, int64_t* d_correct, float* d_scores, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    reset_stats_keep_radius(c);
    knn_status s;
    if (nq < 0 || n_train < 0 || n_train > 0x7fffffffLL || C < 1 || C > 16384)
        return fail(c, KNN_EINVAL, "radius vote sweep: bad nq=%lld n_train=%lld C=%d", (long long)nq,
                    (long long)n_train, C);
    if ((s = weights_check(c, "radius vote sweep", weights)) != KNN_OK) return s;
    if ((s = sweep_thresholds_check(c, "radius vote sweep", thresholds, R)) != KNN_OK) return s;
    if (ld_out < nq)
        return fail(c, KNN_EINVAL, "radius vote sweep: ld_out=%lld < nq=%lld", (long long)ld_out, (long long)nq);
    if (!d_pred && !d_correct && !d_scores)
        return fail(c, KNN_EINVAL, "radius vote sweep: pred, correct and scores are all NULL");
    if (d_correct && !d_query_labels)
        return fail(c, KNN_EINVAL, "radius vote sweep: correct needs the query labels");
    if (nq == 0) return KNN_OK;
    // (the threshold filter reads the distances under every kind of weights)
    if (!d_offsets || !d_idx || !d_dist || !d_train_labels)
        return fail(c, KNN_EINVAL, "radius vote sweep: d_offsets / d_idx / d_dist / d_train_labels is NULL");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIP_OR_FAIL(c, reset_ctrl(c, st));
    RadiusVoteSweepArgs v{};
    v.offsets = d_offsets; v.idx = d_idx; v.dist = d_dist; v.nq = nq; v.n_train = n_train;
    v.labels = d_train_labels; v.C = C; v.weights = kernel_weights(c, weights); v.outlier = outlier_label;
    v.R = R; v.ld_out = ld_out;
    std::copy(thresholds, thresholds + R, v.thr);
    v.qlabels = d_query_labels; v.pred = d_pred; v.correct = reinterpret_cast<unsigned long long*>(d_correct);
    v.scores = d_scores;
    stage_begin(c, st, "radius_vote_sweep");
    if (!v.scores) {
        // (workspace of the caller's pitch: the kernel has one ld_out for pred and scores)
        HIP_OR_FAIL(c, c->rd_scores.ensure(sizeof(float) * (size_t)R * (size_t)ld_out * (size_t)C));
        v.scores = c->rd_scores.as<float>();
        HIP_OR_FAIL(c, hipMemsetAsync(v.scores, 0, sizeof(float) * (size_t)R * (size_t)ld_out * (size_t)C, st));
    } else {
        // the caller's [R][ld_out][C]: only this call's nq rows of every r are zeroed
        HIP_OR_FAIL(c, hipMemset2DAsync(v.scores, sizeof(float) * (size_t)ld_out * (size_t)C, 0,
                                        sizeof(float) * (size_t)nq * (size_t)C, (size_t)R, st));
    }
    v.status = c->ctrl.as<int32_t>();
    HIP_OR_FAIL(c, knn_launch_radius_vote_sweep(v, st));
    stage_end(c, st);
    return finish_call(c, st);
}

// The DBSCAN eps sweep (knn_amd.h "DBSCAN sweep"): the sweep's count pass as a self-join, walked in
// query blocks the histograms' budget takes -> k_dbscan_sweep_prepare (levels, candidates) ->
// k_dbscan_sweep_init -> the link pass (one union per pair, into the forest of the pair's level) ->
// per level k_dbscan_sweep_level and k_radius_scan -> the border pass -> k_dbscan_sweep_labels.
knn_status knn_dbscan_sweep_device(knn_ctx* c, const knn_dataset* tr, const float* thresholds, int32_t R,
                                   int32_t min_samples, int64_t ld_out, int32_t* d_labels, int32_t* d_count,
                                   int64_t* d_summary, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    reset_stats(c);
    knn_status s;
    if (min_samples < 1) return fail(c, KNN_EINVAL, "dbscan sweep: min_samples=%d must be >= 1", min_samples);
    if ((s = sweep_thresholds_check(c, "dbscan sweep", thresholds, R)) != KNN_OK) return s;
    if ((s = radius_check(c, tr, tr, thresholds[R - 1], -1, false)) != KNN_OK) return s;
    const int64_t n = tr->n;
    if (ld_out < n) return fail(c, KNN_EINVAL, "dbscan sweep: ld_out=%lld < n=%lld", (long long)ld_out, (long long)n);
    if (n > 0 && !d_labels) return fail(c, KNN_EINVAL, "dbscan sweep: d_labels is NULL");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (n == 0) {
        if (d_summary) HIP_OR_FAIL(c, hipMemsetAsync(d_summary, 0, sizeof(int64_t) * 4 * (size_t)R, st));
        HIP_OR_FAIL(c, hipStreamSynchronize(st));
        return KNN_OK;
    }
    // every buffer before the first launch: a failed allocation leaves the outputs untouched
    const size_t N = (size_t)n, RN = (size_t)R * N;
    const int64_t qblock = std::max<int64_t>(1, std::min<int64_t>(n, knn_radius_sweep_max_queries(c, R, 0)));
    HIP_OR_FAIL(c, c->dbs_tab.ensure(sizeof(int32_t) * (2 * N + 4 * RN)));
    HIP_OR_FAIL(c, c->dbs_offs.ensure(sizeof(int64_t) * (size_t)R * (N + 1)));
    HIP_OR_FAIL(c, c->dbs_info.ensure(sizeof(int64_t) * (4 * (size_t)R + 1)));
    if (!d_count) HIP_OR_FAIL(c, c->dbs_count.ensure(sizeof(int32_t) * RN));
    HIP_OR_FAIL(c, c->rd_sweep.ensure(sizeof(int32_t) * (size_t)(R + 1) * (size_t)qblock));
    int32_t* t = c->dbs_tab.as<int32_t>();
    int32_t *level = t, *cand = t + N, *parent = t + 2 * N, *root = parent + RN, *isroot = root + RN;
    uint32_t* best = reinterpret_cast<uint32_t*>(isroot + RN);
    int64_t* offs = c->dbs_offs.as<int64_t>();
    int64_t* info = c->dbs_info.as<int64_t>();
    int32_t* count = d_count ? d_count : c->dbs_count.as<int32_t>();
    const int64_t ldc = d_count ? ld_out : n;
    int32_t* status = c->ctrl.as<int32_t>();
    int32_t* nb = status + 3;  // (a spare status word: dbscan_bufs)
    unsigned long long* unions = c->profile == 2 ? reinterpret_cast<unsigned long long*>(info + 4 * R) : nullptr;

    HIP_OR_FAIL(c, reset_ctrl(c, st));
    HIP_OR_FAIL(c, hipMemsetAsync(info, 0, sizeof(int64_t) * (4 * (size_t)R + 1), st));
    c->rd_key.valid = false;
    // the three passes share the form and the segments of a single-threshold pass on (n, n)
    const int form = radius_policy(c->metric, tr->d, n, n, c->algo);
    const RadiusTileArgs ta = radius_args(c, tr, tr, thresholds[R - 1], -1, 0, form);
    DbscanSweepTileArgs a{};
    a.s.train = tr->feat; a.s.nt = n; a.s.ld_t = tr->ld;
    a.s.test = tr->feat; a.s.ld_q = tr->ld; a.s.nq = n;
    a.s.d = tr->d; a.s.elem = tr->dtype;
    a.s.self_base = -1; a.s.R = R;
    std::copy(thresholds, thresholds + R, a.s.thr);
    a.s.nseg = ta.nseg; a.s.seg_len = ta.seg_len;
    a.s.hist = c->rd_sweep.as<int32_t>();
    a.s.status = status;
    DbscanSweepGemmArgs g{};
    if (form) {
        RadiusGemmArgs r{};
        if ((s = radius_prep(c, tr, tr, ta, st, &r)) != KNN_OK) return s;
        g.s.tblk = r.tblk; g.s.qop = r.qop; g.s.qnorm = r.qnorm; g.s.qstat = r.qstat; g.s.tsmax = r.tsmax;
        g.s.train = r.train; g.s.nt = r.nt; g.s.ld_t = r.ld_t;
        g.s.test = r.test; g.s.ld_q = r.ld_q; g.s.nq = r.nq;
        g.s.d = r.d; g.s.elem = r.elem;
        g.s.seg_len = r.seg_len; g.s.nseg = r.nseg;
        g.s.self_base = -1; g.s.coef = r.coef; g.s.eta = r.eta;
        g.s.R = R;
        g.s.hist = a.s.hist; g.s.status = r.status; g.s.exact_cnt = r.exact_cnt;
        std::copy(thresholds, thresholds + R, g.s.thr);
        a.s.gate = a.s.status;
    }

    // 1. the count pass, one query block of the rows at a time over the whole train set
    const size_t es = (size_t)elem_size(tr->dtype);
    for (int64_t q0 = 0; q0 < n; q0 += qblock) {
        const int64_t nb_q = std::min(qblock, n - q0);
        RadiusSweepArgs ca = a.s;
        ca.test = static_cast<const char*>(tr->feat) + (size_t)q0 * (size_t)tr->ld * es;
        ca.nq = nb_q;
        stage_begin(c, st, "radius_sweep");
        HIP_OR_FAIL(c, hipMemsetAsync(ca.hist, 0, sizeof(int32_t) * (size_t)(R + 1) * (size_t)nb_q, st));
        if (form) {
            RadiusSweepGemmArgs cg = g.s;
            cg.test = ca.test; cg.nq = nb_q;
            cg.qop = static_cast<const char*>(g.s.qop) + (size_t)q0 * 2 * (size_t)tr->d;
            cg.qnorm = g.s.qnorm + q0; cg.qstat = g.s.qstat + q0;
            HIP_OR_FAIL(c, knn_launch_radius_sweep_gemm(cg, st));
        }
        HIP_OR_FAIL(c, knn_launch_radius_sweep_tile(ca, c->metric, st));
        stage_end(c, st);
        RadiusSweepFinishArgs f{};
        f.hist = ca.hist; f.nq = nb_q; f.R = R; f.ld_out = ldc; f.count = count + q0;
        stage_begin(c, st, "radius_sweep_finish");
        HIP_OR_FAIL(c, knn_launch_radius_sweep_finish(f, st));
        stage_end(c, st);
    }
    stage_begin(c, st, "dbscan_labels");
    HIP_OR_FAIL(c, knn_launch_dbscan_sweep_prepare(count, ldc, R, min_samples, n, level, cand, nb, st));
    HIP_OR_FAIL(c, knn_launch_dbscan_sweep_init(parent, best, R, n, st));
    stage_end(c, st);

    // 2. the link pass
    a.db.level = level; a.db.parent = parent; a.db.unions = unions;
    a.db.cand = cand; a.db.nb = nb; a.db.root = root; a.db.best = best;
    g.db = a.db;
    stage_begin(c, st, "dbscan_sweep_link");
    if (form) HIP_OR_FAIL(c, knn_launch_dbscan_sweep_gemm(g, DBSCAN_SWEEP_LINK, st));
    HIP_OR_FAIL(c, knn_launch_dbscan_sweep_tile(a, c->metric, DBSCAN_SWEEP_LINK, st));
    stage_end(c, st);

    // 3. the level chain and the cluster numbers of every level
    stage_begin(c, st, "dbscan_labels");
    for (int r = 0; r < R; r++) {
        HIP_OR_FAIL(c, knn_launch_dbscan_sweep_level(parent, level, r, R, n, root, isroot + (size_t)r * N, status, unions, st));
        HIP_OR_FAIL(c, knn_launch_radius_scan(isroot + (size_t)r * N, 1, n, nullptr, offs + (size_t)r * (N + 1), st));
    }
    stage_end(c, st);

    // 4. the border pass
    stage_begin(c, st, "dbscan_sweep_border");
    if (form) HIP_OR_FAIL(c, knn_launch_dbscan_sweep_gemm(g, DBSCAN_SWEEP_BORDER, st));
    HIP_OR_FAIL(c, knn_launch_dbscan_sweep_tile(a, c->metric, DBSCAN_SWEEP_BORDER, st));
    stage_end(c, st);

    // 5. labels, summary, and the call's one synchronisation
    stage_begin(c, st, "dbscan_labels");
    HIP_OR_FAIL(c, knn_launch_dbscan_sweep_labels(level, root, best, offs, R, n, ld_out, d_labels, info, st));
    if (d_summary)
        HIP_OR_FAIL(c, hipMemcpyAsync(d_summary, info, sizeof(int64_t) * 4 * (size_t)R, hipMemcpyDeviceToDevice, st));
    stage_end(c, st);
    s = radius_finish(c, st, form);
    if (s == KNN_OK) {
        c->stats[18] = c->ctrl_host[3];
        unsigned long long u = 0;
        if (unions && hipMemcpy(&u, unions, sizeof(u), hipMemcpyDeviceToHost) == hipSuccess) c->stats[19] = (int64_t)u;
    }
    return s;
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// The mutual-reachability spanning tree (knn_amd.h "Spanning tree"): the vote-less top-K pass of ALL
// rows (LOF's) -> k_mst_core -> Boruvka rounds (k_mst_resolve -> k_mst_tile -> pick / hook / flatten,
// one counter read-back each) -> the sort; and the cut on a tree the caller holds
// ---------------------------------------------------------------------------------
namespace {

// the lists hold max(min_samples, L) entries; L chosen among 0 / 16 / 32 (DESIGN.md "Spanning tree", "Measured")
constexpr int KNN_MST_LIST_L = 32;
constexpr int KNN_MST_MAX_MIN_SAMPLES = 256;

// finish_call behind the tree's kernels: the status word's texts are this feature's
knn_status mst_finish(knn_ctx* c, hipStream_t st, const char* what) {
    const knn_status s = finish_call(c, st);
    const int32_t status = c->ctrl_host[0];
    if (s == KNN_EHIP && (status & KNN_STATUS_UF_LIMIT))
        return fail(c, s, "%s: internal error: a union-find loop reached its iteration cap", what);
    if (s == KNN_EINVAL && (status & KNN_STATUS_BAD_INDEX)) return fail(c, s, "%s: an edge index is outside [0, n)", what);
    return s;
}

}  // namespace

extern "C" {

knn_status knn_mst_device(knn_ctx* c, const knn_dataset* tr, int32_t min_samples, float* d_w, int32_t* d_a, int32_t* d_b,
                          float* d_core, int64_t* d_summary, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    reset_stats(c);
    knn_status s;
    if (min_samples < 1 || min_samples > KNN_MST_MAX_MIN_SAMPLES)
        return fail(c, KNN_EINVAL, "mst: min_samples=%d outside [1, %d]", min_samples, KNN_MST_MAX_MIN_SAMPLES);
    if ((s = radius_check(c, tr, tr, 0.0f, -1, false)) != KNN_OK) return s;
    const int64_t n = tr->n;
    if (n > 0 && min_samples > n)
        return fail(c, KNN_EINVAL, "mst: min_samples=%d exceeds the %lld rows", min_samples, (long long)n);
    if (!d_summary) return fail(c, KNN_EINVAL, "mst: d_summary is NULL");
    if (n > 1 && (!d_w || !d_a || !d_b)) return fail(c, KNN_EINVAL, "mst: d_w / d_a / d_b is NULL");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (n == 0) {
        HIP_OR_FAIL(c, hipMemsetAsync(d_summary, 0, sizeof(int64_t) * 4, st));
        HIP_OR_FAIL(c, hipStreamSynchronize(st));
        return KNN_OK;
    }
    const int K = (int)std::min<int64_t>(std::max(min_samples, c->mst_list_l >= 0 ? c->mst_list_l : KNN_MST_LIST_L), n);
    knn_dataset trv = *tr;
    trv.labels = static_cast<const int32_t*>(tr->feat);  // (for the checks; the zero array replaces it below)
    QueryOut out{nullptr, nullptr, nullptr, nullptr, K, 0};
    if ((s = validate_call(c, &trv, &trv, K, 1, out, false, false)) != KNN_OK) return s;

    // every buffer before the first launch: a failed allocation leaves the outputs untouched
    const size_t N = (size_t)n;
    HIP_OR_FAIL(c, c->mst_idx.ensure(sizeof(int32_t) * N * K));
    HIP_OR_FAIL(c, c->mst_dist.ensure(sizeof(float) * N * K));
    HIP_OR_FAIL(c, c->mst_f.ensure(sizeof(float) * 2 * N));
    HIP_OR_FAIL(c, c->mst_i.ensure(sizeof(int32_t) * 4 * N));
    HIP_OR_FAIL(c, c->mst_u.ensure(sizeof(unsigned long long) * 3 * N));
    HIP_OR_FAIL(c, c->mst_w.ensure(sizeof(uint32_t) * N));
    HIP_OR_FAIL(c, c->mst_cnt.ensure(sizeof(unsigned long long) * MST_CNT_WORDS));
    HIP_OR_FAIL(c, c->mst_sort.ensure(knn_mst_sort_bytes(n - 1)));
    MstTables t{};
    t.idx = c->mst_idx.as<int32_t>(); t.dist = c->mst_dist.as<float>(); t.K = K;
    t.core = c->mst_f.as<float>(); t.dlast = t.core + N;
    t.parent = c->mst_i.as<int32_t>(); t.comp = t.parent + N; t.cand = t.comp + N;
    t.comphi = reinterpret_cast<uint32_t*>(t.cand + N);
    t.rowbest = c->mst_u.as<unsigned long long>(); t.compbest = t.rowbest + N; t.ekey = t.compbest + N;
    t.ew = c->mst_w.as<uint32_t>();
    t.cnt = c->mst_cnt.as<unsigned long long>();
    t.status = c->ctrl.as<int32_t>();

    // 1. the lists: LOF's vote-less pass with nothing removed (its own stage names), then c and dlast
    if ((s = zero_labels(c, n, st, &trv.labels)) != KNN_OK) return s;
    out.idx = c->mst_idx.as<int32_t>();
    out.dist = c->mst_dist.as<float>();
    const int algo = choose_algo(c, n, n, trv.d, K, trv.dtype);
    const bool gemm = is_gemm(algo);
    const int64_t pass = gemm ? std::max<int64_t>(1, c->ws_queries) : n;
    for (int64_t q0 = 0; q0 < n; q0 += pass) {
        const int64_t m = std::min(pass, n - q0);
        const knn_dataset tq = offset_rows(trv, q0, m);
        if ((s = predict_enqueue(c, &trv, &tq, K, 1, offset_out(out, q0), st, algo, nullptr)) == KNN_OK)
            s = finish_call(c, st);
        // (a row with fewer than K finite distances: its list ends in missing entries, c may be +inf)
        if (s == KNN_ERANGE) {
            c->err.clear();
            s = KNN_OK;
        }
        if (s != KNN_OK) {
            if (s != KNN_EINVAL) c->tprep.valid = c->tpad.valid = false;  // a HIP failure: the operands may be partial
            return s;
        }
        pass_stats(c, c->ctrl_host, gemm);
    }
    HIP_OR_FAIL(c, reset_ctrl(c, st));
    stage_begin(c, st, "mst_lists");
    HIP_OR_FAIL(c, hipMemsetAsync(t.cnt, 0, sizeof(unsigned long long) * MST_CNT_WORDS, st));
    HIP_OR_FAIL(c, knn_launch_mst_core(t, n, min_samples, d_core, st));
    stage_end(c, st);

    // 2. the rounds.  The pass has the radius pass's direct form and segments.
    RadiusTileArgs a = radius_args(c, &trv, &trv, 0.0f, -1, 0, 0);
    int max_rounds = 1;
    while (((int64_t)1 << (max_rounds - 1)) < n) max_rounds++;  // ceil(log2 n) + 1
    int64_t E = 0, rounds = 0, pass_rows = 0;
    while (E < n - 1) {
        if (rounds == max_rounds)
            return fail(c, KNN_EHIP, "mst: internal error: %d rounds did not finish the tree", max_rounds);
        stage_begin(c, st, "mst_resolve");
        HIP_OR_FAIL(c, hipMemsetAsync(t.cnt, 0, sizeof(unsigned long long) * MST_CNT_EDGES, st));
        HIP_OR_FAIL(c, hipMemsetAsync(t.rowbest, 0xff, sizeof(unsigned long long) * 2 * N, st));
        HIP_OR_FAIL(c, hipMemsetAsync(t.comphi, 0xff, sizeof(uint32_t) * N, st));
        HIP_OR_FAIL(c, knn_launch_mst_resolve(t, n, c->mst_lists, st));
        stage_end(c, st);
        stage_begin(c, st, "mst_pass");
        HIP_OR_FAIL(c, knn_launch_mst_tile(a, t, c->metric, st));
        stage_end(c, st);
        stage_begin(c, st, "mst_pick");
        HIP_OR_FAIL(c, knn_launch_mst_pick_hook(t, n, st));
        stage_end(c, st);
        unsigned long long cnt[MST_CNT_WORDS];
        HIP_OR_FAIL(c, hipMemcpyAsync(cnt, t.cnt, sizeof(cnt), hipMemcpyDeviceToHost, st));
        HIP_OR_FAIL(c, hipStreamSynchronize(st));
        rounds++;
        pass_rows += (int64_t)cnt[MST_CNT_NB];
        if (!cnt[MST_CNT_OFFERS]) break;  // no component has a candidate: the forest is complete
        if (!cnt[MST_CNT_HOOKS] || (int64_t)cnt[MST_CNT_EDGES] > n - 1)
            return fail(c, KNN_EHIP, "mst: internal error: a round with candidates hooked nothing");
        E = (int64_t)cnt[MST_CNT_EDGES];
    }

    // 3. the order (w, a, b), the summary and the last synchronisation
    stage_begin(c, st, "mst_sort");
    HIP_OR_FAIL(c, knn_launch_mst_sort(t, E, c->mst_sort.p, d_w, d_a, d_b, st));
    c->mst_summary[0] = E; c->mst_summary[1] = n - E; c->mst_summary[2] = rounds; c->mst_summary[3] = pass_rows;
    HIP_OR_FAIL(c, hipMemcpyAsync(d_summary, c->mst_summary, sizeof(int64_t) * 4, hipMemcpyHostToDevice, st));
    stage_end(c, st);
    s = mst_finish(c, st, "mst");
    c->stats[20] = rounds;
    c->stats[21] = pass_rows;
    return s;
}

knn_status knn_mst_cut_device(knn_ctx* c, int64_t n, int64_t n_edges, const float* d_w, const int32_t* d_a,
                              const int32_t* d_b, const float* d_core, const float* thresholds, int32_t R, int64_t ld_out,
                              int32_t* d_labels, int64_t* d_summary, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    c->stages.clear();
    knn_status s;
    if ((s = sweep_thresholds_check(c, "mst cut", thresholds, R)) != KNN_OK) return s;
    if (n < 0 || n > 0x7fffffffLL) return fail(c, KNN_EINVAL, "mst cut: n=%lld outside [0, 2^31-1]", (long long)n);
    if (n_edges < 0 || n_edges > std::max<int64_t>(n - 1, 0))
        return fail(c, KNN_EINVAL, "mst cut: n_edges=%lld outside [0, n - 1]", (long long)n_edges);
    if (ld_out < n) return fail(c, KNN_EINVAL, "mst cut: ld_out=%lld < n=%lld", (long long)ld_out, (long long)n);
    if (n > 0 && (!d_core || !d_labels)) return fail(c, KNN_EINVAL, "mst cut: d_core / d_labels is NULL");
    if (n_edges > 0 && (!d_w || !d_a || !d_b)) return fail(c, KNN_EINVAL, "mst cut: d_w / d_a / d_b is NULL");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (n == 0) {
        if (d_summary) HIP_OR_FAIL(c, hipMemsetAsync(d_summary, 0, sizeof(int64_t) * 3 * (size_t)R, st));
        HIP_OR_FAIL(c, hipStreamSynchronize(st));
        return KNN_OK;
    }
    const size_t N = (size_t)n;
    HIP_OR_FAIL(c, c->mst_cut.ensure(sizeof(int32_t) * 3 * N));
    HIP_OR_FAIL(c, c->mst_offs.ensure(sizeof(int64_t) * (N + 1)));
    HIP_OR_FAIL(c, c->mst_info.ensure(sizeof(unsigned long long) * 3));
    int32_t *parent = c->mst_cut.as<int32_t>(), *root = parent + N, *isroot = root + N;
    int64_t* offs = c->mst_offs.as<int64_t>();
    unsigned long long* info = c->mst_info.as<unsigned long long>();
    int32_t* status = c->ctrl.as<int32_t>();
    HIP_OR_FAIL(c, reset_ctrl(c, st));
    stage_begin(c, st, "mst_cut");
    HIP_OR_FAIL(c, knn_launch_dbscan_init(parent, n, st));
    // the levels are nested: one forest, carried over; level r adds the edges with thr[r - 1] < w <= thr[r]
    for (int r = 0; r < R; r++) {
        HIP_OR_FAIL(c, hipMemsetAsync(info, 0, sizeof(unsigned long long) * 3, st));
        HIP_OR_FAIL(c, knn_launch_mst_cut_link(d_w, d_a, d_b, n_edges, n, r ? thresholds[r - 1] : -1.0f, thresholds[r], parent,
                                               status, st));
        HIP_OR_FAIL(c, knn_launch_mst_cut_roots(parent, d_core, thresholds[r], n, root, isroot, info, status, st));
        HIP_OR_FAIL(c, knn_launch_radius_scan(isroot, 1, n, nullptr, offs, st));
        HIP_OR_FAIL(c, knn_launch_mst_cut_labels(root, offs, n, d_labels + (size_t)r * (size_t)ld_out, info, st));
        if (d_summary)
            HIP_OR_FAIL(c, hipMemcpyAsync(d_summary + 3 * (size_t)r, info, sizeof(int64_t) * 3, hipMemcpyDeviceToDevice, st));
    }
    stage_end(c, st);
    return mst_finish(c, st, "mst cut");
}

}  // extern "C"

extern "C" {

knn_status knn_predict(knn_ctx* c,const knn_dataset* tr, const knn_dataset* te, int32_t k, int32_t C,
                       int64_t q_begin, int64_t q_end, int32_t* out_pred, float* out_dist,
                       int32_t* out_idx) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    knn_status s;
    if ((s = check_dataset(c, tr, "train", true)) != KNN_OK) return s;
    if ((s = check_dataset(c, te, "test", false)) != KNN_OK) return s;
    if (q_begin < 0 || q_end < q_begin || q_end > te->n)
        return fail(c, KNN_EINVAL, "query range [%lld, %lld) outside [0, %lld)", (long long)q_begin,
                    (long long)q_end, (long long)te->n);
    if (tr->d != te->d) return fail(c, KNN_EINVAL, "feature count mismatch: train d=%d test d=%d", tr->d, te->d);
    if (tr->dtype != te->dtype) return fail(c, KNN_EINVAL, "train and test dtypes differ");
    if (k < 1 || k > tr->n) return fail(c, KNN_EINVAL, "k=%d outside [1, n_train=%lld]", k, (long long)tr->n);
    const int64_t nq = q_end - q_begin;
    reset_stats(c);
    if (nq == 0) return KNN_OK;
    if (!out_pred) return fail(c, KNN_EINVAL, "out_pred is NULL");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = c->stream, cs = c->cstream;
    const int d = tr->d;
    const size_t es = (size_t)elem_size(tr->dtype);
    const int ldd = device_ld(d, tr->dtype);
    const int algo = choose_algo(c, tr->n, nq, d, k, tr->dtype);
    const bool gemm = is_gemm(algo);
    // queries stream through two device slots: batch b+1 uploads (copy stream) while batch b
    // computes, and batch b's outputs download while b+1 computes
    int64_t B = std::min<int64_t>(nq, c->batch_rows);
    if (gemm) B = std::min<int64_t>(B, c->ws_queries);
    const int64_t nb = (nq + B - 1) / B;
    if ((s = validate_host_shapes(c, tr, B, ldd, k, C, QueryOut{out_pred, out_dist, out_idx, nullptr, k, 0}, true)) !=
        KNN_OK)
        return s;
    // from here on every error drains both streams (no DMA outlives the call) and drops the
    // train cache entry (its upload may not have run)
    auto abort_call = [&](knn_status e) {
        (void)hipStreamSynchronize(cs);
        (void)hipStreamSynchronize(st);
        c->tcache.valid = false;
        c->tprep.valid = c->tpad.valid = false;
        return e;
    };
    knn_dataset dtr;
    if ((s = train_device(c, tr, st, &dtr)) != KNN_OK) return abort_call(s);
    for (int i = 0; i < 2 && i < nb; i++) {
        HIP_OR_ABORT(c->q_slot[i].ensure(es * (size_t)ldd * B));
        HIP_OR_ABORT(c->pred_slot[i].ensure(sizeof(int32_t) * B));
        if (out_dist) HIP_OR_ABORT(c->dist_slot[i].ensure(sizeof(float) * B * k));
        if (out_idx) HIP_OR_ABORT(c->idx_slot[i].ensure(sizeof(int32_t) * B * k));
    }
    if (nb == 1) {
        // one batch (a call of config L's size): one stream and no events -- the upload, the pass,
        // k_finish's status hand-off (finish_call: the spin on its sequence word), then the
        // downloads.  The pipelined form below pays three cross-stream event waits and a status
        // copy per batch, which only pay off when batches overlap.
        const unsigned char* src = (const unsigned char*)te->feat + es * (size_t)q_begin * (size_t)te->ld;
        HIP_OR_ABORT(hipMemcpy2DAsync(c->q_slot[0].p, es * ldd, src, es * te->ld, es * d, nq, hipMemcpyHostToDevice, st));
        c->stats[7] += (int64_t)(es * d * nq);
        const knn_dataset dq{c->q_slot[0].p, nullptr, nq, d, ldd, te->dtype};
        const QueryOut o{c->pred_slot[0].as<int32_t>(), out_dist ? c->dist_slot[0].as<float>() : nullptr,
                         out_idx ? c->idx_slot[0].as<int32_t>() : nullptr, nullptr, k, 0};
        if ((s = predict_enqueue(c, &dtr, &dq, k, C, o, st, algo, nullptr)) != KNN_OK) return abort_call(s);
        if ((s = finish_call(c, st)) != KNN_OK) {
            if (s != KNN_EINVAL && s != KNN_ERANGE) return abort_call(s);
            return s;  // (a status error: every kernel of the call has completed)
        }
        // (synchronous copies on the null stream: ordered after the context's blocking stream)
        HIP_OR_ABORT(hipMemcpy(out_pred, c->pred_slot[0].p, sizeof(int32_t) * nq, hipMemcpyDeviceToHost));
        if (out_dist)
            HIP_OR_ABORT(hipMemcpy(out_dist, c->dist_slot[0].p, sizeof(float) * nq * k, hipMemcpyDeviceToHost));
        if (out_idx)
            HIP_OR_ABORT(hipMemcpy(out_idx, c->idx_slot[0].p, sizeof(int32_t) * nq * k, hipMemcpyDeviceToHost));
        pass_stats(c, c->ctrl_host, gemm);
        return KNN_OK;
    }
    while ((int64_t)c->ctrl_slots.size() < nb) {
        int32_t* p = nullptr;
        HIP_OR_ABORT(hipHostMalloc((void**)&p, 4 * sizeof(int32_t), hipHostMallocDefault));
        c->ctrl_slots.push_back(p);
    }
    auto rows = [&](int64_t b) { return std::min(B, nq - b * B); };
    auto upload = [&](int64_t b) -> knn_status {
        const int sl = (int)(b & 1);
        const unsigned char* src = (const unsigned char*)te->feat + es * (size_t)(q_begin + b * B) * (size_t)te->ld;
        HIP_OR_ABORT(hipMemcpy2DAsync(c->q_slot[sl].p, es * ldd, src, es * te->ld, es * d, rows(b),
                                        hipMemcpyHostToDevice, cs));
        HIP_OR_ABORT(hipEventRecord(c->ev_up[sl], cs));
        c->stats[7] += (int64_t)(es * d * rows(b));
        return KNN_OK;
    };
    if ((s = upload(0)) != KNN_OK) return abort_call(s);
    for (int64_t b = 0; b < nb; b++) {
        const int sl = (int)(b & 1);
        HIP_OR_ABORT(hipStreamWaitEvent(st, c->ev_up[sl], 0));
        if (b >= 2) HIP_OR_ABORT(hipStreamWaitEvent(st, c->ev_down[sl], 0));  // output slot downloaded
        const knn_dataset dq{c->q_slot[sl].p, nullptr, rows(b), d, ldd, te->dtype};
        const QueryOut o{c->pred_slot[sl].as<int32_t>(), out_dist ? c->dist_slot[sl].as<float>() : nullptr,
                         out_idx ? c->idx_slot[sl].as<int32_t>() : nullptr, nullptr, k, 0};
        if ((s = predict_enqueue(c, &dtr, &dq, k, C, o, st, algo, c->ctrl_slots[b])) != KNN_OK) return abort_call(s);
        HIP_OR_ABORT(hipEventRecord(c->ev_done[sl], st));
        if (b + 1 < nb) {
            if (b + 1 >= 2) HIP_OR_ABORT(hipStreamWaitEvent(cs, c->ev_done[(b + 1) & 1], 0));  // slot free
            if ((s = upload(b + 1)) != KNN_OK) return abort_call(s);
        }
        HIP_OR_ABORT(hipStreamWaitEvent(cs, c->ev_done[sl], 0));
        const int64_t q0 = b * B;
        HIP_OR_ABORT(hipMemcpyAsync(out_pred + q0, c->pred_slot[sl].p, sizeof(int32_t) * rows(b),
                                      hipMemcpyDeviceToHost, cs));
        if (out_dist)
            HIP_OR_ABORT(hipMemcpyAsync(out_dist + q0 * k, c->dist_slot[sl].p, sizeof(float) * rows(b) * k,
                                          hipMemcpyDeviceToHost, cs));
        if (out_idx)
            HIP_OR_ABORT(hipMemcpyAsync(out_idx + q0 * k, c->idx_slot[sl].p, sizeof(int32_t) * rows(b) * k,
                                          hipMemcpyDeviceToHost, cs));
        HIP_OR_ABORT(hipEventRecord(c->ev_down[sl], cs));
    }
    HIP_OR_ABORT(hipStreamSynchronize(cs));
    HIP_OR_ABORT(hipStreamSynchronize(st));
    collect_stages(c);
    for (int64_t b = 0; b < nb; b++) {
        if ((s = check_status(c, c->ctrl_slots[b])) != KNN_OK) return s;
        pass_stats(c, c->ctrl_slots[b], gemm);
    }
    return KNN_OK;
}

knn_status knn_set_metric(knn_ctx* c, int32_t metric) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    if (metric != KNN_METRIC_SQEUCLIDEAN && metric != KNN_METRIC_MANHATTAN && metric != KNN_METRIC_CHEBYSHEV)
        return fail(c, KNN_EINVAL, "unknown metric=%d", metric);
    if (metric != KNN_METRIC_SQEUCLIDEAN && c->algo != KNN_ALGO_AUTO && c->algo != KNN_ALGO_DIRECT)
        return fail(c, KNN_EINVAL, "metric=%d needs KNN_ALGO_AUTO or KNN_ALGO_DIRECT (context algo=%d)", metric, c->algo);
    c->metric = metric;
    return KNN_OK;
}

int32_t knn_get_metric(const knn_ctx* c) { return c ? c->metric : KNN_METRIC_SQEUCLIDEAN; }

knn_status knn_set_generation(knn_ctx* c, uint64_t generation) {
    if (!c) return KNN_EINVAL;
    c->generation = generation;
    c->rd_key.valid = false;
    return KNN_OK;
}

knn_status knn_alloc_pinned(size_t bytes, void** out) {
    if (!out) return KNN_EINVAL;
    *out = nullptr;
    if (bytes == 0) return KNN_OK;
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) {
        *out = nullptr;
        return KNN_ENOMEM;
    }
    return KNN_OK;
}

void knn_free_pinned(void* p) {
    if (p) (void)hipHostFree(p);
}

int32_t knn_stage_times(const knn_ctx* c, const char** names, float* ms, int32_t n) {
    if (!c) return 0;
    int32_t m = (int32_t)std::min<size_t>((size_t)std::max(n, 0), c->stage_ms.size());
    for (int32_t i = 0; i < m; i++) {
        if (names) names[i] = c->stage_names[i];
        if (ms) ms[i] = c->stage_ms[i];
    }
    return m;
}

int32_t knn_last_stats(const knn_ctx* c, int64_t* out, int32_t n) {
    if (!c || !out) return 0;
    int32_t m = std::min(n, 22);
    for (int32_t i = 0; i < m; i++) out[i] = c->stats[i];
    return m;
}

knn_status knn_generate(knn_ctx* c, void* d_feat, int32_t* d_labels, int64_t row0, int64_t n, int32_t d,
                        int32_t ld, int32_t dtype, int32_t kind, uint64_t seed, uint32_t stream,
                        int32_t C, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    if (n < 0 || d <= 0 || ld < d || (d_labels && C < 1) || (n > 0 && !d_feat) || kind < 0 || kind > 3 ||
        (dtype != KNN_F32 && dtype != KNN_BF16))
        return fail(c, KNN_EINVAL, "knn_generate: bad arguments");
    if (dtype == KNN_BF16 && kind != 1 && kind != 3)
        return fail(c, KNN_EINVAL, "bf16 output needs kind 1 or 3 (bf16-exact values)");
    if (kind >= 2 && C < 1) return fail(c, KNN_EINVAL, "clustered kinds need num_classes >= 1");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    GenerateArgs a{d_feat, d_labels, row0, n, d, ld, dtype == KNN_BF16, kind, seed, stream, C};
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIP_OR_FAIL(c, knn_launch_generate(a, st));
    HIP_OR_FAIL(c, hipStreamSynchronize(st));
    return KNN_OK;
}

knn_status knn_mfma_probe_bf16(knn_ctx* c, const uint16_t* d_a, const uint16_t* d_b, int32_t K, float* d_out,
                               void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    if (K <= 0 || K % 16 || !d_a || !d_b || !d_out) return fail(c, KNN_EINVAL, "mfma probe: K must be a positive multiple of 16");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIP_OR_FAIL(c, knn_launch_mfma_probe(d_a, d_b, K, d_out, st));
    HIP_OR_FAIL(c, hipStreamSynchronize(st));
    return KNN_OK;
}

knn_status knn_mfma_probe_i8(knn_ctx* c, const int8_t* d_a, const int8_t* d_b, int32_t K, int32_t* d_out,
                             void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    if (K <= 0 || K % 32 || !d_a || !d_b || !d_out) return fail(c, KNN_EINVAL, "mfma probe: K must be a positive multiple of 32");
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    HIP_OR_FAIL(c, knn_launch_mfma_probe_i8(d_a, d_b, K, d_out, st));
    HIP_OR_FAIL(c, hipStreamSynchronize(st));
    return KNN_OK;
}

// test hook (not in knn_amd.h): the seeds k_seed_thr published in the last pass of the last call
// on a profile = 2 context, one float per query of that pass (+inf: none); host_out takes
// min(n, queries).  Returns how many it wrote, 0 when that pass ran no seed, -1 on an error.
long long knn_debug_last_seed(knn_ctx* c, float* host_out, long long n) {
    if (!c || !host_out || n < 0) return -1;
    if (hipSetDevice(c->device) != hipSuccess) return -1;
    std::vector<float> seeds;
    if (!last_seeds(c, seeds)) return 0;
    const size_t m = std::min<size_t>((size_t)n, seeds.size());
    std::memcpy(host_out, seeds.data(), sizeof(float) * m);
    return (long long)m;
}

// test hook (not in knn_amd.h): the int8 operand class's step times mul (a factor in [1, 8]) on
// this context from now on; the cached scale and operands are dropped
knn_status knn_debug_set_i8_coarsen(knn_ctx* c, float mul) {
    if (!c || !(mul >= 1.0f && mul <= 8.0f)) return KNN_EINVAL;
    c->i8_coarsen = mul;
    c->i8c.valid = c->tprep.valid = false;
    return KNN_OK;
}

knn_status knn_confusion_matrix_device(knn_ctx* c, const int32_t* d_pred, const int32_t* d_labels, int64_t n,
                                       int32_t C, int32_t* d_cm, int64_t* d_correct, void* hip_stream) {
    if (!c) return KNN_EINVAL;
    c->err.clear();
    if (C < 1 || C > 16384 || n < 0 || !d_cm || (n > 0 && (!d_pred || !d_labels)))
        return fail(c, KNN_EINVAL, "confusion: bad arguments (n=%lld, C=%d)", (long long)n, C);
    HIP_OR_FAIL(c, hipSetDevice(c->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : c->stream;
    c->stages.clear();
    HIP_OR_FAIL(c, reset_ctrl(c, st));
    HIP_OR_FAIL(c, hipMemsetAsync(d_cm, 0, sizeof(int32_t) * (size_t)C * (size_t)C, st));
    unsigned long long* corr = reinterpret_cast<unsigned long long*>(d_correct);
    if (!corr) {
        HIP_OR_FAIL(c, c->scratch.ensure(sizeof(unsigned long long)));  // scratch word
        corr = c->scratch.as<unsigned long long>();
    }
    HIP_OR_FAIL(c, hipMemsetAsync(corr, 0, sizeof(unsigned long long), st));
    stage_begin(c, st, "confusion");
    HIP_OR_FAIL(c, knn_launch_confusion(d_pred, d_labels, n, C, d_cm, corr, c->ctrl.as<int32_t>(), st));
    stage_end(c, st);
    knn_status s = finish_call(c, st);
    if (s == KNN_EINVAL) return fail(c, KNN_EINVAL, "a label or prediction is outside [0, num_classes)");
    return s;
}

knn_status knn_confusion_matrix(const int32_t* pred, const int32_t* labels, int64_t n, int32_t C, int32_t* cm) {
    if (!cm || C < 1 || n < 0 || (n > 0 && (!pred || !labels))) return KNN_EINVAL;
    std::memset(cm, 0, sizeof(int32_t) * (size_t)C * (size_t)C);
    for (int64_t i = 0; i < n; i++) {
        int32_t t = labels[i], p = pred[i];
        if (t < 0 || t >= C || p < 0 || p >= C) return KNN_EINVAL;  // the reference writes out of bounds here
        cm[(int64_t)t * C + p]++;
    }
    return KNN_OK;
}

float knn_accuracy(const int32_t* cm, int32_t C, int64_t n) {
    int ok = 0;
    for (int32_t i = 0; i < C; i++) ok += cm[(int64_t)i * C + i];
    return ok / (float)n;
}

}  // extern "C"

void knn_ctx_stage_begin(knn_ctx* c, void* stream, const char* name) { stage_begin(c, (hipStream_t)stream, name); }
void knn_ctx_stage_end(knn_ctx* c, void* stream) { stage_end(c, (hipStream_t)stream); }
