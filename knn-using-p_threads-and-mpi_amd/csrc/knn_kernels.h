// knn_kernels.h -- kernel argument blocks and host launchers (internal to libknn_amd).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// device status word bits (one int32 per predict call)
#define KNN_STATUS_TOO_FEW 1       // a query has fewer than k finite distances
#define KNN_STATUS_BAD_LABEL 2     // a neighbour's label is outside [0, C)
#define KNN_STATUS_GEMM_UNSAFE 4   // a row norm is too large for the GEMM certificate
#define KNN_STATUS_UNSORTED 8      // k_merge_vote: a source list read was not ascending by (dist, idx)
#define KNN_STATUS_BAD_DIST 16     // k_vote_weighted: a caller-supplied distance is NaN or negative
#define KNN_STATUS_BAD_OFFSETS 32  // radius fill / vote: the CSR offsets do not belong to this call
#define KNN_STATUS_BAD_INDEX 64    // radius vote / regression: a list index is outside [0, n_train)
#define KNN_STATUS_UF_LIMIT 128    // DBSCAN: a union-find loop reached its iteration cap (an internal error)

// candidate-list capacity per query on the GEMM path (entries = 64 * CAPW)
#define KNN_RESCORE_CAPW 32

// feature element types (knn_dtype): rows are fp32 or bf16 bits; every distance is the
// reference's fp32 direct form on the (exactly) widened values
enum { ELEM_F32 = 0, ELEM_BF16 = 1 };
// filter-only operand type: fp32 rows split into bf16 [hi(d) | lo(d)] (k_split_rows), so
// q.t ~ hi.hi + hi.lo + lo.hi runs on the bf16 MFMA with an fp32-grade error bound
enum { ELEM_SPLIT = 2 };
// filter-only operand type: fp32 rows rounded to bf16 (k_round_rows, d elements per row);
// the filter runs the bf16 kernel on them under a certificate widened by the rounding
enum { ELEM_ROUND = 3 };

// Where a finished query's neighbours go.  pred may be NULL (train-shard mode: no vote);
// dist/idx/label may be NULL; entry e of query q is at [q * stride + e]; idx is reported
// as idx_base + local train row (train shards carry their global offset).
struct QueryOut {
    int32_t* pred; float* dist; int32_t* idx; int32_t* label;
    int64_t stride; int64_t idx_base;
};

struct ExactScanArgs {
    const void* train; const int32_t* labels; int64_t nt; int ld_t;
    const void* test; int ld_q; int64_t nq;
    int d; int k; int C; int elem;
    const int32_t* qlist; const int32_t* qcount;  // optional query list (device count)
    QueryOut out; int32_t* status;
    int q_lds_bytes;                              // set by the launcher
};

// one kept candidate of the GEMM filters: its train row and certified bounds L <= D <= U
// (one 12-byte store per kept row)
struct CandRec { int32_t idx; float L; float U; };

struct GemmFilterArgs {
    const void* train; int64_t nt; int ld_t;      // ld in elements
    const void* test; int64_t nq; int ld_q; int d;
    const float* tnorm; const float* tnp; const float* qnorm;  // tnorm/tnp padded with +inf to nt+64
    const uint32_t* tnmax;  // ordered bits of max tnorm
    int k; int64_t seg_len; int nseg; int n_qtiles;
    float coef; float eta;
    uint32_t* gthr;
    int32_t* cnt;  // [nseg][nq] kept rows per (segment, query)
    CandRec* cand; int cap; int cap_seg;  // [nq][cap] candidate records
    const float2* qstat;  // fused filter, per query: {|q|, |q - rq|} upper bounds (rq: the operand / -2)
    // fused filter schedule (knn_fused_schedule): p1_blocks whole query tiles, then g2 blocks
    // over the remaining w2 (query tile, 64-row unit) pairs; tiles64 units per query tile
    int p1_blocks; int g2; int64_t w2; int64_t tiles64;
    uint32_t* cursor;       // fused filter, optional: per XCD, the 64-row unit its blocks scan now
    // fused filter, register-list shapes with nseg > 1 (optional): each piece's threshold list
    // [nq][nseg][lshare_w] (U values, +inf where empty), shared between a query's pieces
    float* lshare; int lshare_w;
    // fused filter: the maxima over all 64-row tiles of the tile statistics {max tn, max |t - rt|,
    // max |rt|, 0} (k_tile_stat_max): the fast test's tile term, one per query group and piece
    const float4* tsmax;
    const int32_t* status;  // the call's status word: a set GEMM_UNSAFE bit skips the filter
    const int32_t* gate;    // optional: the filter runs only when *gate != 0 (AUTO's re-run)
    // fused filter, balanced schedule of one round of blocks (optional): per XCD {steps its running blocks have done,
    // running blocks}, zeroed before the launch -- a block ahead of its XCD's average waits a
    // bounded time (fused_pace), so the blocks of an XCD stream the same rows through its L2
    int32_t* pace;
    // int8 operand class (k_gemm_fused<..., I8>): s2 = fl(2 s s) of the train set's scale s; the
    // operand rows are int8, ld_t / ld_q in bytes; 0 for the bf16 operands
    float i8_s2;
    // fused filter, parked passes (optional, profile = 2): the records parked, added per flush
    unsigned long long* park_cnt;
};

struct RescoreArgs {
    const void* train; const int32_t* labels; int ld_t;
    const void* test; int ld_q; int64_t nq; int d; int k; int C; int elem;
    const int32_t* cnt; const CandRec* cand; int cap;
    int nseg; int cap_seg;
    QueryOut out; int32_t* status;
    int32_t* fb_list; int32_t* fb_count;
    const int32_t* gate;  // optional: runs only when *gate != 0 (AUTO's re-run)
    int su_cap;           // candidates staged in LDS per query (host: ~3x the expected count)
    // optional (the fused filter): per query, an upper bound on the k-th smallest U of its
    // candidates (ordered float bits, the filter's final thresholds): only candidates with
    // L <= it can survive, so the selection stages those alone
    const uint32_t* gthr;
    int q_lds_bytes; int c_lds_bytes; int wave_lds_bytes;  // set by the launcher
};

// Merge of per-shard neighbour lists.  rec: [nsrc][nq][3][k] int32 records (k dist bits,
// k global indices (-1 = none), k labels), each list ascending by (dist, idx).
// labels != NULL: the sources are segments of ONE train set (k_direct_tile): indices are
// its local rows, the vote and out.label read labels[idx] (finish_query).
struct MergeArgs {
    const int32_t* rec; int nsrc; int64_t nq; int k; int C;
    QueryOut out; int32_t* status;
    const int32_t* labels;
};

// k_vote_sweep: the vote over every prefix of a query's ascending neighbour list.
// idx: [nq][idx_stride] train rows (-1 = none), the first kin entries of a row are read;
// labels[idx] gives an entry's label.  self_base >= 0: the entry equal to self_base + q is
// skipped (none equal: the last is dropped), the effective list has kmax = kin - 1 entries;
// self_base < 0: kmax = kin.  pred_all (optional) [kmax][pred_stride >= nq]; correct (optional, needs
// qlabels) [kmax], zeroed by the caller; dist_in / dist_out / idx_out (optional): the lists
// after self-removal, [nq][kmax] (dist_in has idx's stride).
struct VoteSweepArgs {
    const int32_t* idx; int64_t idx_stride; const int32_t* labels;
    int64_t nq; int kin; int kmax; int C; int64_t self_base;
    const int32_t* qlabels; int32_t* pred_all; int64_t pred_stride; unsigned long long* correct;
    const float* dist_in; float* dist_out; int32_t* idx_out;
    int32_t* status;
    int qb;  // queries per LDS tile (set by the launcher)
};
hipError_t knn_launch_vote_sweep(const VoteSweepArgs& a, hipStream_t st);

// k_vote_weighted (knn_vote_weighted.hip): the distance-weighted vote and the per-class scores
// over every prefix.  idx / dist: [nq][stride] lists (dist may be NULL for the uniform kind),
// kin / kmax / self_base / labels / qlabels / dist_out / idx_out as VoteSweepArgs.  weights:
// knn_weight.  Only the prefixes k - 1 >= row0 are written: pred_all (optional) points at row
// row0 of [kmax][pred_stride]; correct (optional) is the whole [kmax], zeroed by the caller.
// scores (optional) [nq][C] fp32, zeroed by the caller.  check_dist: flag NaN / negative
// distances (KNN_STATUS_BAD_DIST).
#define KNN_VOTE_W_UNIFORM 0
#define KNN_VOTE_W_INV_DIST 1
#define KNN_VOTE_W_INV_SQDIST 2
struct VoteWeightedArgs {
    const int32_t* idx; const float* dist; int64_t stride; const int32_t* labels;
    int64_t nq; int kin; int kmax; int C; int weights; int64_t self_base;
    const int32_t* qlabels; int32_t* pred_all; int64_t pred_stride; int row0; unsigned long long* correct;
    float* scores; float* dist_out; int32_t* idx_out;
    int check_dist;
    int32_t* status;
    int qb;  // queries per LDS tile (set by the launcher)
};
hipError_t knn_launch_vote_weighted(const VoteWeightedArgs& a, hipStream_t st);

// k_regress_sweep (knn_regress.hip): the k-NN regression prediction over every prefix.  idx /
// dist / stride / kin / kmax / weights / self_base / row0 / dist_out / idx_out / check_dist as
// VoteWeightedArgs; targets[idx] is an entry's fp32 target.  pred_all (optional) fp32, points at
// row row0 of [kmax][pred_stride].  part (optional, needs qtargets): the error partials
// [2][kmax][knn_regress_chunks(nq)] binary64 -- [0]: the sum of e^2, [1]: of |e|, over the
// chunk's queries -- which k_regress_reduce adds INTO sse / sae [kmax] (each optional) in a fixed
// order: chunks of KNN_REGRESS_CHUNK queries ascending within spans of KNN_REGRESS_SPAN chunks,
// then the spans ascending.  The order depends on the query numbers alone, so a call on
// queries [0, n) followed by one on [n, n2) leaves the bits of one call on [0, n2) whenever n is
// a multiple of KNN_REGRESS_CHUNK * KNN_REGRESS_SPAN.
#define KNN_REGRESS_CHUNK 16
#define KNN_REGRESS_SPAN 256
struct RegressArgs {
    const int32_t* idx; const float* dist; int64_t stride; const float* targets;
    int64_t nq; int kin; int kmax; int weights; int64_t self_base;
    const float* qtargets; float* pred_all; int64_t pred_stride; int row0;
    double* part; float* dist_out; int32_t* idx_out;
    int check_dist;
    int32_t* status;
    int qb;  // queries per LDS tile (set by the launcher)
};
inline int64_t knn_regress_chunks(int64_t nq) { return (nq + KNN_REGRESS_CHUNK - 1) / KNN_REGRESS_CHUNK; }
hipError_t knn_launch_regress(const RegressArgs& a, hipStream_t st);
hipError_t knn_launch_regress_reduce(const double* part, int64_t nq, int kmax, int row0, double* sse, double* sae,
                                     hipStream_t st);

// Local outlier factor (knn_lof.hip; knn_amd.h "Local outlier factor"): LOF for every k in
// [k_lo, k_hi], 1 <= k_lo <= k_hi <= KNN_LOF_MAX_K, Kr = k_hi - k_lo + 1.
// k_lof_compact: lists idx / dist [nq][stride], the first kin = k_hi (+ 1 with self_base >= 0)
// entries of a row -> cidx / delta [nq][k_hi] after self-removal (delta binary32: sqrtf of the
// distance when euclid, else the distance; -1 / NaN where missing) and kd (optional) [nq][Kr], delta
// at positions k_lo - 1 .. k_hi - 1.  Indices are checked against [0, n_table) (KNN_STATUS_BAD_INDEX)
// and, with check_dist, distances for NaN / negative (KNN_STATUS_BAD_DIST); such entries are stored
// as missing.  A missing entry sets KNN_STATUS_TOO_FEW.
#define KNN_LOF_MAX_K 255
struct LofCompactArgs {
    const int32_t* idx; const float* dist; int64_t stride;
    int64_t nq; int64_t n_table; int kin; int k_lo; int k_hi; int64_t self_base;
    int euclid; int check_dist;
    int32_t* cidx; float* delta; float* kd;
    int32_t* status;
};
hipError_t knn_launch_lof_compact(const LofCompactArgs& a, hipStream_t st);
// k_lof_lrd: lrd_out [nq][Kr] binary64 from the rows' compacted lists and kd_table [n_table][Kr].
// k_lof_score: lof [Kr][lof_stride >= nq] binary32 from the lists, lrd_table [n_table][Kr] and the
// rows' own lrd_own [nq][Kr] (the table itself when the table's rows are scored).
struct LofWalkArgs {
    const int32_t* cidx; const float* delta; int64_t nq; int k_lo; int k_hi;
    const float* kd_table; double* lrd_out;
    const double* lrd_table; const double* lrd_own; float* lof; int64_t lof_stride;
};
hipError_t knn_launch_lof_lrd(const LofWalkArgs& a, hipStream_t st);
hipError_t knn_launch_lof_score(const LofWalkArgs& a, hipStream_t st);

// class counts up to this many live in a per-wave LDS table; above it the vote runs
// table-free (vote_ballot), so every path accepts any num_classes
#define KNN_VOTE_LDS_MAX_C 1024
// per-wave LDS words of k_merge_vote: class counts, or the k winners' labels + a counter
__host__ __device__ inline int merge_wave_words(int C, int k) {
    return C <= KNN_VOTE_LDS_MAX_C ? ((C + 3) & ~3) : ((k + 1 + 3) & ~3);
}

// k_direct_tile: DT_NW waves per block, 64 train rows per tile, rows staged in chunks of
// dc <= DT_MAX_DC dims (DT_MAXP 16-B staging registers per thread)
#define DT_NW 8
#define DT_MAX_DC 128
#define DT_MAXP (64 * (DT_MAX_DC / 4) / (64 * DT_NW))
struct DirectTileArgs {
    const void* train; const int32_t* labels; int64_t nt; int ld_t;
    const void* test; int ld_q; int64_t nq;
    int d; int k; int C; int elem;
    int64_t seg_len; int nseg; int n_qblocks;
    int dc; int stride;        // dims per staged chunk (multiple of 4), LDS row stride (floats)
    int vote_lds;              // per-wave LDS class counts (C <= KNN_VOTE_LDS_MAX_C)
    QueryOut out; int32_t* status;
    int32_t* rec;              // nseg > 1: segment records [nseg][nq][3][k] (local rows)
    // k_direct_rows with nseg > 1 (optional): per query group, the segments that finished
    // (zero between calls); the last wave of a group merges every segment's records and votes
    // in the same launch (no k_merge_vote pass)
    int32_t* arrive;
};
// k <= 64R selects the wave-list register count R
inline int knn_list_regs(int k) { return k <= 64 ? 1 : k <= 128 ? 2 : k <= 256 ? 4 : k <= 512 ? 8 : 16; }
// queries per k_direct_tile block for k (8 * QW, QW = max(1, 8 / list registers))
int knn_direct_tile_qb(int k);
// launch geometry: dims per staged chunk and the padded LDS row stride (floats), LDS bytes per
// block and blocks per CU at that LDS
void knn_direct_tile_geom(int d, int* dc, int* stride);
size_t knn_direct_tile_lds(int d, int C);
hipError_t knn_direct_tile_occupancy(int k, int elem, int d, int C, int* blocks_per_cu);
// work units of the direct form for (k, d): queries per unit and units resident per CU --
// k_direct_tile: a block of 8 waves; k_direct_rows (d <= 16, k <= 16): one wave
hipError_t knn_direct_units(int k, int elem, int d, int C, int* queries_per_unit, int* units_per_cu);
// fills dc / stride / vote_lds / n_qblocks from d, C, nq and launches nseg units per query
// unit (k_direct_tile: blocks; k_direct_rows for d <= 16, k <= 16: waves, four per block)
hipError_t knn_launch_direct_tile(DirectTileArgs a, hipStream_t st);
// whether (k, d) runs k_direct_rows (d <= 16, k <= 16), and its query groups for nq queries
bool knn_direct_rows_shape(int k, int d);
int64_t knn_direct_rows_groups(int64_t nq);

// distance metrics (knn_metric of knn_amd.h).  METRIC_SQEUCLIDEAN is every kernel above;
// the other two run k_metric_tile (knn_metric.hip): k_direct_tile's contract, block shape,
// LDS layout and segment records (DirectTileArgs, knn_direct_tile_qb / _geom / _lds) with the
// per-feature step sum = sum + |q_i - t_i| (Manhattan) or m = fmaxf(m, |q_i - t_i|) (Chebyshev).
// There is no rows form: every (k, d) runs the tile kernel, a block of 8 waves per unit.
enum { METRIC_SQEUCLIDEAN = 0, METRIC_MANHATTAN = 1, METRIC_CHEBYSHEV = 2 };
hipError_t knn_metric_units(int metric, int k, int elem, int d, int C, int* queries_per_unit, int* units_per_cu);
// fills dc / stride / vote_lds / n_qblocks and launches n_qblocks * nseg blocks
hipError_t knn_launch_metric_tile(DirectTileArgs a, int metric, hipStream_t st);

// Radius neighbours (knn_radius.hip; knn_amd.h "Radius neighbours").  k_radius_tile<M, E, MODE>:
// k_metric_tile's block shape, tile staging and geometry (knn_direct_tile_geom) for all three
// metrics, 8 queries per wave for every shape, the selection replaced by D <= thr.
#define KNN_RADIUS_QW 8
// class counts up to this many live in the count pass's per-wave LDS block [8][Cpad] (16 KiB a
// block at the limit, beside the tiles); above it they are integer atomics on class_counts
#define KNN_RADIUS_LDS_MAX_C 64
// what a distance pass does with a passing pair: count it, store it, or one of DBSCAN's two modes
// (knn_amd.h "DBSCAN"): LINK unions core rows q > t, BORDER takes the smallest cluster number among
// a candidate's core neighbours
enum { RADIUS_COUNT = 0, RADIUS_FILL = 1, RADIUS_LINK = 2, RADIUS_BORDER = 3 };
// the DBSCAN modes' tables (RadiusTileArgs / RadiusGemmArgs .db; a self-join: test == train, nq == nt)
struct RadiusDbscanArgs {
    const int32_t* dcount; int32_t min_samples;  // LINK: row i is core iff dcount[i] >= min_samples
    int32_t* parent;             // LINK: the union-find forest [nt]
    unsigned long long* unions;  // LINK, optional (profile = 2): += successful hooks, one add per wave
    // BORDER: query q is train row cand[q], q < *nb (blocks past it return at once); cluster [nt]
    // is a core row's cluster number and -1 for every other row; the minimum goes into
    // out_labels[cand[q]] with an unsigned atomicMin (-1 is the largest value)
    const int32_t* cand; const int32_t* nb; const int32_t* cluster; int32_t* out_labels;
};
struct RadiusTileArgs {
    const void* train; const int32_t* labels; int64_t nt; int ld_t;
    const void* test; int ld_q; int64_t nq;
    int d; int C; int elem;
    int64_t seg_len; int nseg; int n_qblocks;
    int dc; int stride;        // set by the launcher (knn_direct_tile_geom)
    float thr; int64_t self_base;  // self_base >= 0: train row self_base + q is no neighbour of q
    // count pass.  classes != 0: a class output is asked (the launcher turns it into 1: LDS counts,
    // 2: global atomics, and sets fuse_vote when the pass votes itself: LDS counts and nseg == 1)
    int classes; int fuse_vote;
    int32_t* seg_count;        // [nseg][nq]
    int32_t* class_counts;     // [nq][C]; optional with fuse_vote, else needed and zeroed by the caller
    int32_t* pred; const int32_t* qlabels; unsigned long long* correct; int32_t outlier;  // fuse_vote only
    // fill pass: base [nseg][nq] where a (segment, query) part starts (offsets itself when nseg == 1)
    const int64_t* base; const int64_t* offsets;
    int32_t* idx; float* dist;  // dist optional
    int32_t* status;
    // optional: a status word; the kernel runs only when it says KNN_STATUS_GEMM_UNSAFE (the pass
    // behind k_radius_gemm, which returns at once in that case)
    const int32_t* gate;
    RadiusDbscanArgs db;       // RADIUS_LINK / RADIUS_BORDER only
};
hipError_t knn_radius_units(int metric, int elem, int d, int C, int* queries_per_unit, int* units_per_cu);
// mode: RADIUS_COUNT / _FILL / _LINK / _BORDER
hipError_t knn_launch_radius_tile(RadiusTileArgs a, int metric, int mode, hipStream_t st);
// whether the count pass writes pred / correct itself (no k_radius_argmax behind it)
bool knn_radius_pass_votes(int C, int nseg);
// count (optional, may alias seg_count when nseg == 1) and the int64 exclusive scan offsets [nq + 1] (optional)
hipError_t knn_launch_radius_scan(const int32_t* seg_count, int nseg, int64_t nq, int32_t* count, int64_t* offsets,
                                  hipStream_t st);
hipError_t knn_launch_radius_bases(const int32_t* seg_count, int nseg, int64_t nq, const int64_t* offsets, int64_t* base,
                                   hipStream_t st);
hipError_t knn_launch_radius_argmax(const int32_t* class_counts, int64_t nq, int C, int32_t outlier,
                                    const int32_t* qlabels, int32_t* pred, unsigned long long* correct, hipStream_t st);
// k_radius_vote / k_radius_regress on CSR lists: segment q is [offsets[q], offsets[q + 1]) of idx /
// dist (dist optional for the uniform kind); weights: KNN_VOTE_W_*.  scores [nq][C] is needed and
// zeroed by the caller; pred / correct (needs qlabels) are optional.  Regression: targets, pred_f.
struct RadiusVoteArgs {
    const int64_t* offsets; const int32_t* idx; const float* dist; int64_t nq; int64_t n_train;
    const int32_t* labels; int C; int weights; int32_t outlier;
    const int32_t* qlabels; int32_t* pred; unsigned long long* correct; float* scores;
    const float* targets; float* pred_f;
    int32_t* status;
};
hipError_t knn_launch_radius_vote(const RadiusVoteArgs& a, hipStream_t st);
hipError_t knn_launch_radius_regress(const RadiusVoteArgs& a, hipStream_t st);

// The MFMA-filtered form of the radius pass (knn_radius_gemm.hip): k_radius_gemm<RB, E, MODE>,
// squared Euclidean, d in {64, 128, 256}.  8 waves a block, 32 queries a wave; train segments are
// multiples of 64 rows.  tblk: the fused filter's train tile blocks of 64 rows (knn_launch_tn_rows
// with bn = 64 over the 64-row grid), qop / qnorm / qstat its query operand, tsmax the maxima of the
// tile statistics; train / test the caller's rows (the exact distance of the band reads them).
#define KNN_RADIUS_GEMM_NW 8
struct RadiusGemmArgs {
    const void* tblk; const void* qop; const float* qnorm; const float2* qstat; const float4* tsmax;
    const void* train; const int32_t* labels; int64_t nt; int ld_t;
    const void* test; int ld_q; int64_t nq;
    int d; int C; int elem;
    int64_t seg_len; int nseg; int n_qblocks;  // n_qblocks: set by the launcher
    float thr; int64_t self_base;
    float coef; float eta;     // certificate_fused
    // count pass.  classes != 0: members add into class_counts [nq][C] (needed then, zeroed by the
    // caller) and every label of the train set is range-checked
    int classes;
    int32_t* seg_count;        // [nseg][nq]
    int32_t* class_counts;
    // fill pass: as RadiusTileArgs
    const int64_t* base; const int64_t* offsets;
    int32_t* idx; float* dist;
    int32_t* status;           // a set KNN_STATUS_GEMM_UNSAFE bit skips the pass
    unsigned long long* exact_cnt;  // optional (profile = 2): += the pairs given the exact evaluation
    RadiusDbscanArgs db;       // RADIUS_LINK / RADIUS_BORDER only
};
bool knn_radius_gemm_supported(int d);
// bytes of one 64-row tile block of the train operand
size_t knn_radius_gemm_tile_bytes(int d);
hipError_t knn_radius_gemm_units(int elem, int d, int* queries_per_unit, int* units_per_cu);
hipError_t knn_launch_radius_gemm(RadiusGemmArgs a, int mode, hipStream_t st);

// DBSCAN's small kernels (knn_dbscan.hip; knn_amd.h "DBSCAN").  count [n]: a row's neighbours, itself
// included; a row is core iff count >= min_samples.  parent / root / isroot / cluster / cand: int32
// [n] workspace, nb one int32 (zeroed by the caller), offsets the int64 exclusive scan of isroot
// (k_radius_scan, one segment), info int64 [4] {clusters, core, border, noise} (zeroed by the
// caller).  unions: optional, += successful hooks.
hipError_t knn_launch_dbscan_init(int32_t* parent, int64_t n, hipStream_t st);
hipError_t knn_launch_dbscan_flatten(int32_t* parent, const int32_t* count, int32_t min_samples, int64_t n, int32_t* root,
                                     int32_t* isroot, int32_t* status, hipStream_t st);
hipError_t knn_launch_dbscan_labels(const int32_t* root, const int64_t* offsets, int64_t n, int32_t* labels,
                                    int32_t* cluster, hipStream_t st);
hipError_t knn_launch_dbscan_candidates(const int32_t* count, int32_t min_samples, int64_t n, int32_t* cand, int32_t* nb,
                                        hipStream_t st);
hipError_t knn_launch_dbscan_summary(const int32_t* labels, const int32_t* count, int32_t min_samples,
                                     const int64_t* offsets, int64_t n, int64_t* info, hipStream_t st);
// the same clustering on CSR lists [list_offsets[i], list_offsets[i + 1]) of idx
hipError_t knn_launch_dbscan_lists_count(const int64_t* list_offsets, int64_t n, int32_t* count, int32_t* status,
                                         hipStream_t st);
hipError_t knn_launch_dbscan_lists_link(const int64_t* list_offsets, const int32_t* idx, int64_t n, const int32_t* count,
                                        int32_t min_samples, int32_t* parent, int32_t* status, unsigned long long* unions,
                                        hipStream_t st);
hipError_t knn_launch_dbscan_lists_border(const int64_t* list_offsets, const int32_t* idx, int64_t n, const int32_t* count,
                                          const int32_t* cand, const int32_t* nb, const int32_t* cluster, int32_t* labels,
                                          hipStream_t st);

// The radius sweep (knn_radius_sweep.hip; knn_amd.h "Radius sweep"): R <= 32 non-decreasing
// thresholds in one distance pass.  k_radius_sweep_tile<M, E> has k_radius_tile's block shape,
// geometry and segments; a pair counts into its bucket (the smallest r with D <= thr[r]) of
// hist [nq][R + 1] and, with classes, of chist [nq][R + 1][C] -- both zeroed by the caller, added
// to with integer atomics by every train segment.  The thresholds travel by value.
#define KNN_RADIUS_SWEEP_MAX_R 32
struct RadiusSweepArgs {
    const void* train; const int32_t* labels; int64_t nt; int ld_t;
    const void* test; int ld_q; int64_t nq;
    int d; int C; int elem;
    int64_t seg_len; int nseg; int n_qblocks;
    int dc; int stride;        // set by the launcher (knn_direct_tile_geom)
    int64_t self_base;
    int classes; int R;
    int32_t* hist; int32_t* chist;
    int32_t* status;
    // optional: a status word; the kernel runs only when it says KNN_STATUS_GEMM_UNSAFE (the pass
    // behind k_radius_sweep_gemm, which returns at once in that case)
    const int32_t* gate;
    float thr[KNN_RADIUS_SWEEP_MAX_R];  // [R..31]: set by the launcher to thr[R - 1]
};
// k_radius_sweep_gemm<RB, E>: the MFMA-filtered form of the sweep pass -- RadiusGemmArgs' operands
// and certificate (squared Euclidean, d in {64, 128, 256}; segments are multiples of 64 rows), the
// same histograms.
struct RadiusSweepGemmArgs {
    const void* tblk; const void* qop; const float* qnorm; const float2* qstat; const float4* tsmax;
    const void* train; const int32_t* labels; int64_t nt; int ld_t;
    const void* test; int ld_q; int64_t nq;
    int d; int C; int elem;
    int64_t seg_len; int nseg; int n_qblocks;  // n_qblocks: set by the launcher
    int64_t self_base;
    float coef; float eta;     // certificate_fused
    int classes; int R;
    int32_t* hist; int32_t* chist;
    int32_t* status;           // a set KNN_STATUS_GEMM_UNSAFE bit skips the pass
    unsigned long long* exact_cnt;  // optional (profile = 2): += the pairs given the exact evaluation
    float thr[KNN_RADIUS_SWEEP_MAX_R];  // [R..31]: set by the launcher to thr[R - 1]
};
hipError_t knn_launch_radius_sweep_gemm(RadiusSweepGemmArgs a, hipStream_t st);
hipError_t knn_launch_radius_sweep_tile(RadiusSweepArgs a, int metric, hipStream_t st);
// k_radius_sweep_finish: the prefix over buckets.  count / pred [R][ld_out], class_counts
// [R][ld_out][C] (each optional; the class outputs need classes != 0); correct / outliers [R] are
// ADDED to.  chist is overwritten with its own prefix.
struct RadiusSweepFinishArgs {
    const int32_t* hist; int32_t* chist; int64_t nq; int R; int C; int classes;
    int64_t ld_out; int32_t outlier; const int32_t* qlabels;
    int32_t* count; int32_t* class_counts; int32_t* pred;
    unsigned long long* correct; unsigned long long* outliers;
};
hipError_t knn_launch_radius_sweep_finish(const RadiusSweepFinishArgs& a, hipStream_t st);
// k_radius_vote_sweep: k_radius_vote on the sub-lists dist <= thr[r] of CSR lists (dist needed for
// every kind).  scores [R][ld_out][C] is needed and zeroed by the caller; pred [R][ld_out] and
// correct [R] (added to; needs qlabels) are optional.
struct RadiusVoteSweepArgs {
    const int64_t* offsets; const int32_t* idx; const float* dist; int64_t nq; int64_t n_train;
    const int32_t* labels; int C; int weights; int32_t outlier; int R; int64_t ld_out;
    const int32_t* qlabels; int32_t* pred; unsigned long long* correct; float* scores;
    int32_t* status;
    float thr[KNN_RADIUS_SWEEP_MAX_R];
};
hipError_t knn_launch_radius_vote_sweep(const RadiusVoteSweepArgs& a, hipStream_t st);

// The DBSCAN eps sweep (knn_dbscan_sweep.hip; knn_amd.h "DBSCAN sweep"): the link and the border
// pass of all R thresholds at once, over a self-join (test == train, nq == nt) with the sweep
// pass's arguments (hist / chist / classes / labels unused), and the integer kernels around them.
//   level [nt]      c(i): the smallest r at which row i is a core row, R when there is none
//   parent [R][nt]  LINK: one union-find forest per level, each started as the identity
//   cand / nb       BORDER: query q is train row cand[q], q < *nb (blocks past it return at once)
//   root [nt][R]    BORDER: a row's root at every level at which it is a core row, else -1
//   best [R][nt]    BORDER: unsigned atomicMin of the offered roots (0xffffffff: none)
enum { DBSCAN_SWEEP_LINK = 0, DBSCAN_SWEEP_BORDER = 1 };
struct DbscanSweepArgs {
    const int32_t* level;
    int32_t* parent;
    unsigned long long* unions;  // LINK, optional (profile = 2): += successful hooks, one add per wave
    const int32_t* cand; const int32_t* nb;
    const int32_t* root;
    uint32_t* best;
};
struct DbscanSweepTileArgs { RadiusSweepArgs s; DbscanSweepArgs db; };
struct DbscanSweepGemmArgs { RadiusSweepGemmArgs s; DbscanSweepArgs db; };
hipError_t knn_launch_dbscan_sweep_tile(DbscanSweepTileArgs a, int metric, int mode, hipStream_t st);
hipError_t knn_launch_dbscan_sweep_gemm(DbscanSweepGemmArgs a, int mode, hipStream_t st);
// count [R][ldc] (the sweep's) -> level [n] and the border candidates cand[0 .. *nb) (nb zeroed by the caller)
hipError_t knn_launch_dbscan_sweep_prepare(const int32_t* count, int64_t ldc, int R, int32_t min_samples, int64_t n,
                                           int32_t* level, int32_t* cand, int32_t* nb, hipStream_t st);
hipError_t knn_launch_dbscan_sweep_init(int32_t* parent, uint32_t* best, int R, int64_t n, hipStream_t st);
// level r of the chain, to be launched for r = 0 .. R - 1 in this order: root[.][r], isroot_r [n],
// and every core row of level r joined to its root in forest r + 1
hipError_t knn_launch_dbscan_sweep_level(int32_t* parent, const int32_t* level, int r, int R, int64_t n, int32_t* root,
                                         int32_t* isroot_r, int32_t* status, unsigned long long* unions, hipStream_t st);
// offs [R][n + 1]: per level the exclusive scan of isroot (k_radius_scan); labels [R][ld_out];
// info int64 [R][4] {clusters, core, border, noise}, zeroed by the caller
hipError_t knn_launch_dbscan_sweep_labels(const int32_t* level, const int32_t* root, const uint32_t* best,
                                          const int64_t* offs, int R, int64_t n, int64_t ld_out, int32_t* labels,
                                          int64_t* info, hipStream_t st);

// The mutual-reachability spanning tree (knn_mst.hip; knn_amd.h "Spanning tree"): Boruvka rounds over
// a self-join (test == train, nq == nt).  A candidate of row q is a row t of another component with
// D(q, t) < FLT_MAX; its key is bits(w) << 32 | t, w = fmaxf(fmaxf(core[q], core[t]), D), and
// 0xffff...f means "none".
//   lists idx / dist [n][K]  the rows' plain top-K lists (the row itself included; idx -1: missing)
//   core / dlast [n]         c(i); the list's last distance, +inf for a list that holds every
//                            candidate the row has (K == n, or a missing entry)
//   parent / comp [n]        the union-find forest and its flattened image, comp[i] = root of i
//   rowbest [n]              the smallest key of a row: stored by k_mst_resolve, atomicMin by the pass
//   compbest / comphi [n]    per component root: the smallest (bits(w) << 32 | lo) and, among the rows
//                            that offer it, the smallest hi
//   cnt int64 [MST_CNT_WORDS] the counters below, on the device
// (a round zeroes the first three; the edges add up over the rounds)
enum { MST_CNT_NB = 0, MST_CNT_OFFERS = 1, MST_CNT_HOOKS = 2, MST_CNT_EDGES = 3, MST_CNT_WORDS = 4 };
struct MstTables {
    const int32_t* idx; const float* dist; int K;
    float* core; float* dlast;
    int32_t* parent; int32_t* comp;
    unsigned long long* rowbest; unsigned long long* compbest; uint32_t* comphi;
    int32_t* cand;
    unsigned long long* ekey; uint32_t* ew;  // the edges in hook order: a << 32 | b (a < b), bits(w)
    unsigned long long* cnt;
    int32_t* status;
};
// c(i) = entry min_samples - 1 of row i's list, dlast; parent[i] = comp[i] = i
hipError_t knn_launch_mst_core(const MstTables& t, int64_t n, int32_t min_samples, float* core_out, hipStream_t st);
// one round's list walk: rowbest of the resolved rows, the others into cand[0 .. cnt[MST_CNT_NB]);
// use_lists = 0: every row is a candidate.  Zeroes nothing: the caller resets rowbest / compbest /
// comphi (all ones) and cnt[NB / OFFERS / HOOKS] first.
hipError_t knn_launch_mst_resolve(const MstTables& t, int64_t n, int use_lists, hipStream_t st);
// the pass over the candidates (RadiusTileArgs' geometry fields: train / nt / ld_t / d / elem / seg_len /
// nseg; test / nq / ld_q are set to the train set's here)
hipError_t knn_launch_mst_tile(RadiusTileArgs a, const MstTables& t, int metric, hipStream_t st);
// pick (two steps), hook (a successful union appends its edge), flatten
hipError_t knn_launch_mst_pick_hook(const MstTables& t, int64_t n, hipStream_t st);
// the E edges sorted by (w, a, b) into w / a / b; temp: knn_mst_sort_bytes(E) bytes
size_t knn_mst_sort_bytes(int64_t E);
hipError_t knn_launch_mst_sort(const MstTables& t, int64_t E, void* temp, float* w, int32_t* a, int32_t* b, hipStream_t st);
// The cut.  link: the edges with lo < w <= hi (lo < 0: no lower bound) are joined in parent; an index
// outside [0, n) sets KNN_STATUS_BAD_INDEX and is not followed.  number: root / isroot of the rows with
// core <= thr (-1 / 0 for the others), and info[1] += those rows (info int64 [3], zeroed by the caller)
hipError_t knn_launch_mst_cut_link(const float* w, const int32_t* a, const int32_t* b, int64_t E, int64_t n, float lo,
                                   float hi, int32_t* parent, int32_t* status, hipStream_t st);
hipError_t knn_launch_mst_cut_roots(int32_t* parent, const float* core, float thr, int64_t n, int32_t* root,
                                    int32_t* isroot, unsigned long long* info, int32_t* status, hipStream_t st);
// labels [n] from root and the scan of isroot; info[0] = clusters, info[2] = n - info[1]
hipError_t knn_launch_mst_cut_labels(const int32_t* root, const int64_t* offsets, int64_t n, int32_t* labels,
                                     unsigned long long* info, hipStream_t st);

struct GenerateArgs {
    void* out; int32_t* labels; int64_t row0; int64_t n; int d; int ld;
    int bf16_out; int kind; uint64_t seed; uint32_t stream; int C;
};

hipError_t knn_launch_exact_scan(const ExactScanArgs& a, int grid, hipStream_t st);
size_t knn_exact_scan_lds(int d, int k, int C);
// tstat (optional, train rows of the fused filter): per 64-row tile [ceil(n / 64)]
//   {max ||x||^2, max ||x - rx||, max ||rx||, 0}, rx = rn_bf16(x) (upper bounds)
// i8s > 0 (the int8 operand class, scale i8s): rx = i8s knn_i8_quant(x, i8s) in tstat and qstat
//   (oscale is not used), and tstat's fourth word is max |tn - s2 knn_i8_norm_q(tn, s2)|
// qstat (optional, query rows of the fused filter): per row {||x||, ||x - rx||} upper bounds,
//   rx = rn_bf16(oscale x) / oscale (the operand the filter multiplies, unscaled)
// gate (optional): the stage runs only when *gate != 0 (device-side control of AUTO's re-run)
hipError_t knn_launch_row_norms(const void* x, int elem, int64_t n, int ld, int d, float* out,
                                int32_t* status, uint32_t* maxo, float* outp, float c1, hipStream_t st,
                                float4* tstat = nullptr, const int32_t* gate = nullptr,
                                float2* qstat = nullptr, float oscale = 1.0f, float i8s = 0.0f);
// out (one word, zeroed by the caller) = max over the n x d fp32 elements of the bits of |x|
// (the bits of non-negative floats order like the floats; NaN and inf end up >= 0x7f800000)
hipError_t knn_launch_absmax(const float* x, int64_t n, int ld, int d, uint32_t* out, hipStream_t st);
// row_bytes = d * element size: 128, 256 or 512
bool knn_gemm_filter_supported(int elem, int row_bytes);
// block shape of the filter for (element type, row bytes, k): waves per block, query
// groups per wave, row groups per tile, min waves per SIMD (launch bounds), tile buffers,
// queries per block, LDS bytes per block
struct FilterPlan {
    int nw, qg, rg, minw, nbuf, bm;
    size_t lds;
    int kr = 0;  // fused: register-list shape (16, 32, 104; 0 = LDS heaps)
    int ls = 0;  // fused: the kernel exchanges threshold lists between a query's pieces
    int i8 = 0;   // fused: int8 operand rows of d bytes on v_mfma_i32_32x32x32_i8 (d = 128, k <= 32)
    int park = 0;  // fused, int8: passing tiles are parked in LDS and visited in batches (lds holds the ring)
};
FilterPlan knn_gemm_filter_plan(int elem, int row_bytes, int k);
hipError_t knn_launch_gemm_filter(const GemmFilterArgs& a, int elem, int row_bytes, hipStream_t st);
size_t knn_gemm_filter_lds(int elem, int row_bytes, int k);
hipError_t knn_gemm_filter_occupancy(int elem, int row_bytes, int k, int* blocks_per_cu);
// fp32 rows [n][ld] of d elements -> bf16 rows [n][2 dp]: hi = rn(x), lo = rn(x - hi), each half
// dp >= d elements wide (dp % 4 == 0) with zero bits in columns d .. dp-1
hipError_t knn_launch_split_rows(const float* x, int64_t n, int ld, int d, int dp, uint16_t* out, hipStream_t st,
                                 const int32_t* gate = nullptr);
// fp32 rows [n][ld] of d elements -> bf16 rows [n][dp] rn(x), dp >= d, dp % 4 == 0: columns d .. dp-1
// are zero bits, and no load touches column d or beyond
hipError_t knn_launch_round_rows(const float* x, int64_t n, int ld, int d, int dp, uint16_t* out, hipStream_t st,
                                 const int32_t* gate = nullptr);
hipError_t knn_launch_fill_u32(uint32_t* p, int64_t n, uint32_t v, const int32_t* gate, hipStream_t st);
// host_mapped[0..n) = ctrl[0..n) (a mapped pinned host buffer), then ctrl[0..n) = 0
hipError_t knn_launch_finish(int32_t* ctrl, int32_t* host_mapped, int n, uint32_t seq, hipStream_t st);
// AUTO's re-run decision on the device: ctrl[3] = !unsafe && ctrl[1] > limit (and ctrl[1] = 0 then)
hipError_t knn_launch_rerun_decide(int32_t* ctrl, int64_t limit, hipStream_t st);
hipError_t knn_launch_rescore(const RescoreArgs& a, hipStream_t st);
// fused-norm filter (knn_fused.hip), d in {64, 128, 256}: train as tile blocks [bn rows rn(t) |
// bn fp32 norms | tile statistics] (k_tn_rows), each accumulator starting from the norms
bool knn_fused_supported(int d);
// Test hooks of the fused plan (the product plan is knn_fused_plan's rule; a context snapshots
// these once, at knn_create, from KNN_FUSED_QG / KNN_FUSED_HEAPS / KNN_FUSED_PARK / KNN_FUSED_SEED so the tests can
// run every shape): qg 1|2 forces the queries per wave, heaps the LDS-heap shape for 32 < k <= 104
// at d = 256, park 0|1 the int8 shapes' parked passes off / on.  0 / false / -1: the rule.
struct FusedForce {
    int qg = 0;
    bool heaps = false;
    int park = -1;  // KNN_FUSED_PARK=0|1: the int8 shapes' parked passes off / on; -1: the rule
    int seed = 1;   // KNN_FUSED_SEED=0|1: the int8 shapes' seeded thresholds (k_seed_thr) off / on; not part of the plan
};
// nw == 0: k too large.  nq, num_cus and max_pieces (the most pieces a query's candidate list
// allows) pick the queries per wave (register-list shapes): 64 on 32-row tiles when the
// 512-query blocks, at most max_pieces per query tile, fill 80 % of a round of CUs, else 32 on
// 64-row tiles (fewer pieces per query tile).  run_gemm computes the plan once per pass and sizes the
// operands, the occupancy, the schedule and the launch from that one plan.
// i8: the int8 operand class (rows of d bytes; d = 128 and k <= 32 only: nw == 0 otherwise)
FilterPlan knn_fused_plan(int d, int k, int64_t nq, int num_cus, const FusedForce& force, int max_pieces,
                          bool i8 = false);
hipError_t knn_fused_occupancy(int d, const FilterPlan& f, int* blocks_per_cu);
// whether the library holds a kernel for plan f (no GPU call)
bool knn_fused_has_kernel(int d, const FilterPlan& f);
// out = component maxima of n tile statistics (the fused filter's a.tsmax)
hipError_t knn_launch_tile_stat_max(const float4* tstat, int64_t n, float4* out, hipStream_t st);
// candidate sub-slices per segment (piece) of the GEMM filters: one per lane half
static constexpr int KNN_FILTER_SUBSLICES = 2;
// whether plan f's kernel exchanges threshold lists between a query's pieces (a.lshare, lshare_w floats per piece)
int knn_fused_list_share_width(const FilterPlan& f);
// fills a.p1_blocks / g2 / w2 / tiles64 for the balanced schedule over `slots` resident
// blocks; returns the grid, *nseg = the most pieces one query tile gets.  (a.g2 = -1 and
// a.seg_len / nseg instead: the segment schedule, n_qtiles * nseg blocks.)
int knn_fused_schedule(GemmFilterArgs& a, int slots, int* nseg);
// f: the plan run_gemm sized the grid and operands with (knn_fused_plan)
hipError_t knn_launch_fused(const GemmFilterArgs& a, const FilterPlan& f, hipStream_t st);
// the fused filter's operands: x -> queries [n][dp] bf16 rn(scale x) (norms == NULL),
// or train blocks of bn rows [bn][dp] bf16 | bn fp32 norms | tstat of the enclosing 64-row tile.
// d: the caller's row width, dp >= d (dp % 4 == 0) the operand's: columns d .. dp-1 are zero bits
hipError_t knn_launch_tn_rows(const void* x, int elem, int64_t n, int64_t n_valid, int ld, int d, int dp,
                              const float* norms, float scale, void* out, const float4* tstat, int bn, hipStream_t st,
                              const int32_t* gate = nullptr);
// K-chunked filter for wide rows (knn_wide.hip, k_gemm_wide): bf16 operand rows of dp = d rounded up
// to a multiple of 128 features, 256 < d <= 4096, cut into chunks of 128; k_gemm_filter's
// protocol (GemmFilterArgs with d = ld_t = ld_q = dp, CandRec / cnt / gthr), k <= 128.
// knn_wide_width: dp, or 0 when the kernel does not take d.  The train operand covers the grid of
// knn_wide_group_rows()-row groups with zero rows, tnorm / tnp with +inf; seg_len is a multiple of it.
int knn_wide_width(int d);
int knn_wide_group_rows();
FilterPlan knn_wide_plan(int k);
hipError_t knn_wide_occupancy(int k, int* blocks_per_cu);
hipError_t knn_launch_wide(const GemmFilterArgs& a, hipStream_t st);
// the int8 operand class (fp32 x, scale s; knn_i8_quant): queries [n][d] int8 (norms == NULL), or
// train blocks of bn rows [bn][d] int8 | bn int32 -knn_i8_norm_q(tn, s2) | tstat of the enclosing
// 64-row tile; pad rows: zero features and -2^30
hipError_t knn_launch_i8_rows(const float* x, int64_t n, int64_t n_valid, int ld, int d, const float* norms, float s,
                              void* out, const float4* tstat, int bn, hipStream_t st);
// s2 = fl(2 s s) of scale s, as the kernels round it (knn_i8_s2, knn_device.h)
float knn_i8_s2_of(float s);
// Seeded thresholds of the int8 fused filter (knn_seed.hip, k_seed_thr; DESIGN.md "Seeded
// thresholds"): a pass over a strided sample of the train tile blocks that lowers gthr[q] from
// +inf to an upper bound of the query's k-th distance, so the filter's pieces start warm.
// The sample (no GPU call): tile block i (stride) of the train set's bn-row tile blocks, i < ns;
// each of `slices` blocks per query tile takes every slices-th of them and publishes its own bound.
// ns == 0: no seed for this shape.
struct SeedSample {
    int ns = 0;
    int64_t stride = 0;
    int slices = 1;
};
SeedSample knn_seed_sample(int64_t nt, int bn, int64_t nq, int num_cus);
struct SeedArgs {
    const void* tblk; int bn;      // the filter's train operand (k_i8_rows), bn = 32 or 64
    int64_t pad_blk;               // a tile block of it that holds pad rows only (the operand's last)
    const void* qop; int64_t nq;   // int8 query rows [nq][128]
    const float* qnorm; const float2* qstat; const float4* tsmax;
    float coef, eta, i8_s2;
    int k;                         // <= 32
    SeedSample sample;
    uint32_t* gthr;                // ordered bits; lowered with atomicMin
    uint32_t* seed_out;            // optional (profile = 2): the same bound, into a buffer of ordered(+inf)
    const int32_t* status;         // a set KNN_STATUS_GEMM_UNSAFE bit skips the pass
    const int32_t* gate;           // optional: the pass runs only when *gate != 0
};
hipError_t knn_launch_seed_thr(const SeedArgs& a, hipStream_t st);
// the int8 filter's MFMA chain on [32][K] int8 operands (K % 32 == 0): out [32][32] int32
hipError_t knn_launch_mfma_probe_i8(const int8_t* a, const int8_t* b, int K, int32_t* out, hipStream_t st);
hipError_t knn_launch_merge(const MergeArgs& a, hipStream_t st);
hipError_t knn_launch_generate(const GenerateArgs& a, hipStream_t st);
// the bf16 filter's MFMA chain on [32][K] bf16 operands (certificate self-test)
hipError_t knn_launch_mfma_probe(const uint16_t* a, const uint16_t* b, int K, float* out, hipStream_t st);
hipError_t knn_launch_confusion(const int32_t* pred, const int32_t* labels, int64_t n, int C, int32_t* cm,
                                unsigned long long* correct, int32_t* status, hipStream_t st);
