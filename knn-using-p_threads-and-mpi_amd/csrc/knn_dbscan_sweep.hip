// knn_dbscan_sweep.hip -- the DBSCAN eps sweep (include/knn_amd.h "DBSCAN sweep"; the argument is in
// DESIGN.md "DBSCAN sweep"): DBSCAN's labels at every one of R <= 32 non-decreasing thresholds from
// three distance passes over the train set against itself.  The count pass is the radius sweep's
// (knn_radius_sweep.hip); here are the two passes behind it and the integer steps around them:
//
//   k_dbscan_sweep_prepare      level[i] = c(i), the smallest r at which row i is a core row (R: none),
//                               and the border candidates cand[0 .. *nb)
//   k_dbscan_sweep_init         parent[r][i] = i, best[r][i] = "none"
//   k_dbscan_sweep_tile<M, E, MODE>   the link / border pass, k_radius_sweep_tile's skeleton
//   k_dbscan_sweep_gemm<RB, E, MODE>  its MFMA-filtered form, k_radius_sweep_gemm's skeleton
//   k_dbscan_sweep_level        level r of the chain: root[i][r], isroot[r][i], and the row joined
//                               to its root in forest r + 1
//   k_dbscan_sweep_labels       labels [R][ld_out] and info [R][4]
//
// A pair of rows t < q that are core rows at some level first becomes a core-core edge at level
// a = max(bucket(q, t), c(q), c(t)): the link pass makes ONE union, into forest a.  The level chain
// carries the components of level r into forest r + 1.  Every step is integer; the distances are
// k_radius_tile's, bit for bit (the same flags, the same chain).
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include "knn_kernels.h"

#include "knn_device.h"

#pragma clang fp contract(off)
#include "knn_radius_dev.h"  // radius_step<M>, load4q, RadiusGemmTile<RB>, radius_exact<E>
#include "knn_dbscan_dev.h"  // uf_find, uf_union

namespace {

constexpr uint32_t DBS_NONE = 0xffffffffu;

// best[r][q] = min(best[r][q], root[t][r]) for r in [lo, hi): the smallest root among the core
// neighbours of candidate q at every level at which q is no core row yet.  Values only fall, so a
// word that is already small enough (however stale the read) needs no atomic.
__device__ __forceinline__ void border_offer(const DbscanSweepArgs& db, int64_t nt, int R, int64_t q, int64_t t, int lo,
                                             int hi) {
    for (int r = lo; r < hi; r++) {
        const uint32_t v = (uint32_t)db.root[t * R + r];
        uint32_t* p = db.best + (int64_t)r * nt + q;
        if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v) atomicMin(p, v);
    }
}

}  // namespace

// ---------------------------------------------------------------------------------
// k_dbscan_sweep_tile<M, E, MODE> (DbscanSweepTileArgs: the sweep pass's arguments and the tables).
// Blocks, waves, tiles, chunks, query operands, the accumulator and the bucket of a pair are
// k_radius_sweep_tile's; the scan limits are k_radius_tile's RADIUS_LINK / RADIUS_BORDER modes'.
//  * MODE = DBSCAN_SWEEP_LINK: query q is train row q; only a query with c(q) < R takes part, the
//    scan ends at the block's last query, a block without such a query returns and a wave without
//    one only stages tiles.  A pair with D <= thr[R - 1], t < q and c(t) < R makes
//    uf_union(parent + a * nt, q, t) at a = max(bucket, c(q), c(t)) when a < R.
//  * MODE = DBSCAN_SWEEP_BORDER: query q is train row cand[q] (q < *nb; blocks past it return).  A
//    pair with D <= thr[R - 1] and c(t) < R offers root[t][r] to best[r][cand[q]] for every r in
//    [max(bucket, c(t)), c(q)) -- the levels at which t is a core row within thr[r] of a row that
//    is none yet.  (The self pair has an empty range.)
// LDS: 2 tile buffers [64][stride] f32.
// ---------------------------------------------------------------------------------
template <int M, typename E, int MODE>
__global__ __launch_bounds__(64 * DT_NW, 4) void k_dbscan_sweep_tile(DbscanSweepTileArgs aa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const RadiusSweepArgs& a = aa.s;
    const DbscanSweepArgs& db = aa.db;
    // (the pass behind k_dbscan_sweep_gemm: only when a norm made the certificate unsafe)
    if (a.gate && !(*a.gate & KNN_STATUS_GEMM_UNSAFE)) return;
    constexpr bool LINK = MODE == DBSCAN_SWEEP_LINK, BORDER = MODE == DBSCAN_SWEEP_BORDER;
    constexpr int NT = 64 * DT_NW;
    constexpr int QW = KNN_RADIUS_QW;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile_floats = 64 * a.stride;
    float* bufs = reinterpret_cast<float*>(smem);
    const int qb = blockIdx.x % a.n_qblocks;
    const int seg = blockIdx.x / a.n_qblocks;
    const int64_t row_begin = (int64_t)seg * a.seg_len;
    int64_t row_end = min(a.nt, row_begin + a.seg_len);
    int64_t nq = a.nq;
    if constexpr (BORDER) {
        nq = *db.nb;
        if ((int64_t)qb * (DT_NW * QW) >= nq) return;
    }
    if constexpr (LINK) row_end = min(row_end, min(nq, (int64_t)(qb + 1) * (DT_NW * QW)));
    const E* __restrict__ train = reinterpret_cast<const E*>(a.train);
    const E* __restrict__ test = reinterpret_cast<const E*>(a.test);
    const int d = a.d;
    const int R = a.R;
    const float thr_top = a.thr[KNN_RADIUS_SWEEP_MAX_R - 1];  // == thr[R - 1]

    int64_t qr[QW];     // the query's train row
    const E* qrow[QW];
    int qlev[QW];       // c(query); a query that takes no part: LINK R, BORDER 0
    bool wave_any = false;
    [[maybe_unused]] unsigned long long nun = 0;  // (LINK) successful hooks
#pragma unroll
    for (int i = 0; i < QW; i++) {
        const int64_t qi = (int64_t)qb * (DT_NW * QW) + wave * QW + i;
        if constexpr (BORDER) {
            qr[i] = qi < nq ? db.cand[qi] : 0;
            qlev[i] = qi < nq ? db.level[qr[i]] : 0;
            if (qlev[i] > 0) wave_any = true;
        } else {
            qr[i] = qi < nq ? qi : nq - 1;
            qlev[i] = qi < nq ? db.level[qi] : R;
            if (qlev[i] < R) wave_any = true;
        }
        qrow[i] = test + qr[i] * (int64_t)a.ld_q;
    }
    // a block none of whose queries takes part has nothing to do; a wave without one only stages tiles
    if (!__syncthreads_or(wave_any ? 1 : 0)) return;

    const int ngr = (d + 3) >> 2;          // 4-dim groups per row
    const int gpc = a.dc >> 2;             // groups per chunk
    const int nchunk = (ngr + gpc - 1) / gpc;
    const int pieces = 64 * gpc;           // 4-element pieces per staged chunk
    const int64_t nrows = row_end > row_begin ? row_end - row_begin : 0;
    const int64_t nsteps = ((nrows + 63) >> 6) * nchunk;

    float4 st[DT_MAXP];
    auto load_chunk = [&](int64_t s) __attribute__((always_inline)) {
        const int64_t r0 = row_begin + (s / nchunk) * 64;
        const int c0 = (int)(s % nchunk) * a.dc;
#pragma unroll
        for (int j = 0; j < DT_MAXP; j++) {
            const int p = threadIdx.x + j * NT;
            const int row = p / gpc, g = p - row * gpc;
            if (p < pieces && c0 + 4 * g < 4 * ngr) {
                const int64_t t = min(r0 + row, row_end - 1);
                st[j] = load4(train + t * a.ld_t + c0 + 4 * g);
            }
        }
    };
    auto store_chunk = [&](int64_t s) __attribute__((always_inline)) {
        float* b = bufs + (s & 1) * tile_floats;
        const int c0 = (int)(s % nchunk) * a.dc;
#pragma unroll
        for (int j = 0; j < DT_MAXP; j++) {
            const int p = threadIdx.x + j * NT;
            const int row = p / gpc, g = p - row * gpc;
            if (p < pieces && c0 + 4 * g < 4 * ngr) *reinterpret_cast<float4*>(b + row * a.stride + 4 * g) = st[j];
        }
    };

    float acc[QW];
#pragma unroll
    for (int i = 0; i < QW; i++) acc[i] = 0.0f;
    if (nsteps > 0) {
        load_chunk(0);
        store_chunk(0);
    }
    __syncthreads();
    for (int64_t s = 0; s < nsteps; s++) {
        if (s + 1 < nsteps) load_chunk(s + 1);  // in flight during this chunk's compute
        const int ch = (int)(s % nchunk);
        const int c0 = ch * a.dc;
        const float* tb = bufs + (s & 1) * tile_floats + lane * a.stride;
        const int gend = wave_any ? min(gpc, ngr - ch * gpc) : 0;
        for (int g = 0; g < gend; g++) {
            const float4 t = *reinterpret_cast<const float4*>(tb + 4 * g);
            const int col = c0 + 4 * g;
            if (col + 4 <= d) {
#pragma unroll
                for (int i = 0; i < QW; i++) {
                    const float4 qv = load4q(qrow[i] + col);  // wave-uniform: scalar loads
                    float s0 = acc[i];
                    s0 = radius_step<M>(s0, qv.x, t.x);
                    s0 = radius_step<M>(s0, qv.y, t.y);
                    s0 = radius_step<M>(s0, qv.z, t.z);
                    s0 = radius_step<M>(s0, qv.w, t.w);
                    acc[i] = s0;
                }
            } else {
                const int rem = d - col;  // 1..3 trailing dims
#pragma unroll
                for (int i = 0; i < QW; i++) {
                    const float4 qv = load4q(qrow[i] + col);
                    float s0 = acc[i];
                    s0 = radius_step<M>(s0, qv.x, t.x);
                    if (rem > 1) s0 = radius_step<M>(s0, qv.y, t.y);
                    if (rem > 2) s0 = radius_step<M>(s0, qv.z, t.z);
                    acc[i] = s0;
                }
            }
        }
        if (ch == nchunk - 1 && wave_any) {
            // the tile's distances are final: the threshold tests
            const int64_t row = row_begin + (s / nchunk) * 64 + lane;
            const bool valid = row < row_end;
            // c(t) of this lane's row: one word per tile and lane
            const int tl = valid ? db.level[row] : R;
#pragma unroll
            for (int i = 0; i < QW; i++) {
                const float D = acc[i];
                acc[i] = 0.0f;  // every metric restarts from +0
                bool pass = tl < R && D <= thr_top;
                if constexpr (LINK) pass = pass && qlev[i] < R && row < qr[i];
                else pass = pass && tl < qlev[i];
                if (!__ballot(pass)) continue;
                int b = 0;
#pragma unroll
                for (int r = 0; r < KNN_RADIUS_SWEEP_MAX_R; r++) b += D <= a.thr[r] ? 0 : 1;
                if (!pass) continue;
                if constexpr (LINK) {
                    const int lv = max(b, max(qlev[i], tl));
                    if (lv < R && uf_union(db.parent + (int64_t)lv * a.nt, (int32_t)qr[i], (int32_t)row, a.nt, a.status))
                        nun++;
                } else {
                    border_offer(db, a.nt, R, qr[i], row, max(b, tl), qlev[i]);
                }
            }
        }
        if (s + 1 < nsteps) store_chunk(s + 1);
        __syncthreads();
    }
    if constexpr (LINK) {
        if (db.unions) {  // (profile = 2) one 64-bit add per wave
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) nun += __shfl_xor(nun, o);
            if (lane == 0 && nun) atomicAdd(db.unions, nun);
        }
    }
}

// ---------------------------------------------------------------------------------
// k_dbscan_sweep_gemm<RB, E, MODE> (DbscanSweepGemmArgs).  Blocks, waves, the query fragments, the
// tile images, the MFMA loop, the certificate and the bracket [bl, bu] of a pair's bucket are
// k_radius_sweep_gemm's; the scan limits and the masks are k_radius_gemm's RADIUS_LINK /
// RADIUS_BORDER modes': the tile's rows with c(t) < R (one word per lane and tile, a ballot) and,
// for LINK, the rows below the query are masked BEFORE the band is resolved.
//  * The largest threshold that can matter to a query: LINK thr[R - 1]; BORDER thr[c(q) - 1] (a
//    pair matters only at a level below c(q)).  The fast test and the "surely out" test use it.
//  * A pair whose bracket decides the bucket (bl == bu) never touches the rows.  Of the others, a
//    pair with bu <= m needs no exact distance either -- m = max(c(q), c(t)) for LINK, c(t) for
//    BORDER: the thresholds below m cannot change the level the pair acts at.  Every other pair
//    gets radius_exact once and the bucket of that D.
//  * LINK: uf_union into forest max(bucket, c(q), c(t)) when that is below R.  BORDER: the offers
//    of k_dbscan_sweep_tile.
// The kernel returns at once when the status word says KNN_STATUS_GEMM_UNSAFE; k_dbscan_sweep_tile,
// gated the other way, runs instead.  LDS: 2 tile images.
// ---------------------------------------------------------------------------------
template <int RB, typename E, int MODE>
__global__ __launch_bounds__(64 * KNN_RADIUS_GEMM_NW) void k_dbscan_sweep_gemm(DbscanSweepGemmArgs aa) {
    typedef RadiusGemmTile<RB> RT;
    const RadiusSweepGemmArgs& a = aa.s;
    const DbscanSweepArgs& db = aa.db;
    constexpr bool LINK = MODE == DBSCAN_SWEEP_LINK, BORDER = MODE == DBSCAN_SWEEP_BORDER;
    constexpr int NW = KNN_RADIUS_GEMM_NW, NT = 64 * NW;
    constexpr int NS = RB / 32;                      // k-steps: d / 16
    constexpr int D = RB / 2;
    constexpr int STRIDE = RT::STRIDE, HDR = RT::HDR, TILE = RT::TILE, SPR = RT::SPR;
    constexpr int NL = 64 * SPR / NT;                // row staging registers (16 bytes) per thread
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (*a.status & KNN_STATUS_GEMM_UNSAFE) return;  // (block-uniform, before any barrier)

    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int qb = blockIdx.x % a.n_qblocks;
    const int seg = blockIdx.x / a.n_qblocks;
    const int64_t row_begin = (int64_t)seg * a.seg_len;
    int64_t row_end = min(a.nt, row_begin + a.seg_len);
    int64_t nq = a.nq;
    if constexpr (BORDER) {
        nq = *db.nb;
        if ((int64_t)qb * (32 * NW) >= nq) return;  // (block-uniform, before any barrier)
    }
    if constexpr (LINK) row_end = min(row_end, (min(nq, (int64_t)(qb + 1) * (32 * NW)) + 63) & ~(int64_t)63);
    const int ntiles = row_end > row_begin ? (int)((row_end - row_begin + 63) >> 6) : 0;
    const int R = a.R;
    const float thrv = a.thr[lane & (KNN_RADIUS_SWEEP_MAX_R - 1)];
    const float coef = a.coef, eta = a.eta;
    const float INF = __uint_as_float(0x7f800000u);
    const E* __restrict__ train = reinterpret_cast<const E*>(a.train);

    // this lane's query (both lane halves hold the same query, different rows)
    const int64_t q = (int64_t)qb * (32 * NW) + wave * 32 + j;
    const bool qvalid = q < nq;
    int64_t qx = qvalid ? q : 0;  // the train row its operands are read from
    if constexpr (BORDER) qx = qvalid ? db.cand[q] : 0;
    const int cq = qvalid ? db.level[qx] : (LINK ? R : 0);
    const bool qlive = LINK ? cq < R : cq > 0;
    // the largest threshold that matters to this query (every lane is active here)
    float thr = a.thr[KNN_RADIUS_SWEEP_MAX_R - 1];  // == thr[R - 1]
    if constexpr (BORDER) thr = __shfl(thrv, max(cq - 1, 0));
    const E* qrow = reinterpret_cast<const E*>(a.test) + qx * (int64_t)a.ld_q;
    uint4 qf[NS];
    {
        const unsigned char* qop = reinterpret_cast<const unsigned char*>(a.qop) + qx * (int64_t)RB;
#pragma unroll
        for (int s = 0; s < NS; s++)
            qf[s] = qvalid ? *reinterpret_cast<const uint4*>(qop + 32 * s + 16 * h) : make_uint4(0u, 0u, 0u, 0u);
    }
    const float qn = qvalid ? a.qnorm[qx] : 0.0f;
    float qe2 = 0.0f, eq2 = 0.0f;  // 2 |q| and 2 |q - rq|, rounded up
    if (qvalid) {
        const float2 qs = a.qstat[qx];
        qe2 = 2.0f * qs.x * (1.0f + 0x1p-17f);
        eq2 = 2.0f * qs.y * (1.0f + 0x1p-17f);
    }
    // the fast test's threshold (k_radius_gemm's, from the query's largest threshold)
    float tf = -INF;
    if (qlive) {
        const float4 smax = *a.tsmax;
        const float tk = fmaf(coef + 0x1p-18f, smax.x, fmaf(qe2, smax.y, eq2 * smax.z));
        tf = ((thr - qn) + fmaf(coef, qn, eta)) + 0x1p-18f * (fabsf(thr) + qn + eta) + tk;
    }
    const bool wave_live = __ballot(qlive) != 0ull;
    unsigned long long nexact = 0;  // pairs given radius_exact
    [[maybe_unused]] unsigned long long nun = 0;  // (LINK) successful hooks

    // thr[r] for the whole wave
    auto thr_at = [&](int r) __attribute__((always_inline)) {
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(thrv), r));
    };

    // ---- tile blocks: global -> registers (in flight during the tile before) -> LDS
    const unsigned char* tsrc = reinterpret_cast<const unsigned char*>(a.tblk) + (row_begin >> 6) * RT::TB;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    static_assert((64 * SPR) % NT == 0 && RT::HS <= NT, "tile rows: whole staging rounds");
    u32x4 stg[NL];
    u32x4 hdr = {0u, 0u, 0u, 0u};
    const bool hdr_lane = threadIdx.x < RT::HS;
    auto load_tile = [&](int t) __attribute__((always_inline)) {
        const u32x4* src = reinterpret_cast<const u32x4*>(tsrc + (int64_t)t * RT::TB);
#pragma unroll
        for (int i = 0; i < NL; i++) stg[i] = src[threadIdx.x + i * NT];
        if (hdr_lane) hdr = src[64 * SPR + threadIdx.x];
    };
    auto store_tile = [&](int t) __attribute__((always_inline)) {
        unsigned char* img = smem + (t & 1) * TILE;
#pragma unroll
        for (int i = 0; i < NL; i++) {
            const int P = threadIdx.x + i * NT;
            *reinterpret_cast<u32x4*>(img + (P / SPR) * STRIDE + 16 * (P % SPR)) = stg[i];
        }
        if (hdr_lane) *reinterpret_cast<u32x4*>(img + HDR + 16 * threadIdx.x) = hdr;
    };

    if (ntiles > 0) {
        load_tile(0);
        store_tile(0);
    }
    __syncthreads();
    for (int t = 0; t < ntiles; t++) {
        if (t + 1 < ntiles) load_tile(t + 1);
        const unsigned char* tile = smem + (t & 1) * TILE;
        const int64_t r0 = row_begin + (int64_t)t * 64;
        if (wave_live) {
            floatx16 X[2];
#pragma unroll
            for (int rg = 0; rg < 2; rg++) {
#pragma unroll
                for (int g4 = 0; g4 < 4; g4++) {
                    const float4 v = *reinterpret_cast<const float4*>(tile + fused_norm_off(HDR, h, rg, g4));
                    X[rg][4 * g4] = v.x;
                    X[rg][4 * g4 + 1] = v.y;
                    X[rg][4 * g4 + 2] = v.z;
                    X[rg][4 * g4 + 3] = v.w;
                }
            }
#pragma unroll
            for (int s = 0; s < NS; s++) {
#pragma unroll
                for (int rg = 0; rg < 2; rg++) {
                    const uint4 A = *reinterpret_cast<const uint4*>(tile + fused_frag_off(32 * rg + j, h, s, STRIDE));
                    X[rg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A),
                                                                    __builtin_bit_cast(bf16x8, qf[s]), X[rg], 0, 0, 0);
                }
            }
            float mn = INF;
#pragma unroll
            for (int r = 0; r < 16; r++) mn = fminf(mn, fminf(X[0][r], X[1][r]));
            if (__ballot(mn <= tf) != 0ull) {
                // the tile's statistics and this query's band against it (bounds() of knn_fused.hip)
                const float4 w = *reinterpret_cast<const float4*>(tile + HDR + 4 * 64);
                const float rho = fmaf(qe2, w.y, eq2 * w.z);
                const float dl = fmaf(coef, qn + w.x, eta) + rho;
                // rows of the segment that are core rows at some level; LINK: below the query
                const int64_t trow = r0 + lane;
                const int tlv = trow < row_end ? db.level[trow] : R;
                u64 vm = __ballot(tlv < R);
                if constexpr (LINK) {
                    const int64_t below = q - r0;  // rows of the tile with an index under q's
                    if (below < 64) vm &= below > 0 ? (1ull << below) - 1ull : 0ull;
                }
                if (!qlive) vm = 0ull;
                // Pass 1, per value: its 7-bit code -- the bucket where the bracket decides it,
                // UNDECIDED | bu otherwise -- packed nine to a 64-bit word at the value's fixed place.
                constexpr u64 UNDECIDED = 64;
                u64 todo = 0;           // rows with a code, bit = tile row
                u64 code[4] = {0, 0, 0, 0};
#pragma unroll
                for (int c = 0; c < 2; c++) {
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const float G = qn + X[c][r];
                        const float L = G - dl;
                        const float U = G + dl;
                        const int b = 32 * c + (r & 3) + 8 * (r >> 2) + 4 * h;
                        if (!(L > thr) && ((vm >> b) & 1ull)) {
                            int bl = 0, bu = 0;
                            for (int k = 0; k < R; k++) {
                                const float tk = thr_at(k);
                                bl += L > tk ? 1 : 0;
                                bu += U <= tk ? 0 : 1;
                            }
                            const int s = 16 * c + r;  // (a constant once unrolled)
                            code[s / 9] |= (bl == bu ? (u64)bl : UNDECIDED | (u64)bu) << (7 * (s % 9));
                            todo |= 1ull << b;
                        }
                    }
                }
                // Pass 2, every lane's next row together
                while (todo) {
                    const int b = __ffsll((long long)todo) - 1;
                    todo &= todo - 1ull;
                    const int s = 16 * (b >> 5) + (b & 3) + 4 * ((b & 31) >> 3);  // the value of row b
                    const int w9 = s / 9;
                    const u64 cw = w9 == 0 ? code[0] : w9 == 1 ? code[1] : w9 == 2 ? code[2] : code[3];
                    int bk = (int)((cw >> (7 * (s - 9 * w9))) & 127ull);
                    const int64_t tr = r0 + b;
                    const int ct = db.level[tr];  // (< R: the mask)
                    const int m = LINK ? max(cq, ct) : ct;
                    if (bk & (int)UNDECIDED) {
                        bk &= 63;  // bu: the bucket is at most this
                        if (bk > m) {
                            const float Dx = radius_exact<E>(qrow, train + tr * (int64_t)a.ld_t, D);
                            nexact++;
                            bk = 0;
                            for (int k = 0; k < R; k++) bk += Dx <= thr_at(k) ? 0 : 1;
                        }
                    }
                    const int lv = max(bk, m);
                    if constexpr (LINK) {
                        if (lv < R && uf_union(db.parent + (int64_t)lv * a.nt, (int32_t)q, (int32_t)tr, a.nt, a.status))
                            nun++;
                    } else {
                        border_offer(db, a.nt, R, qx, tr, lv, cq);
                    }
                }
            }
        }
        if (t + 1 < ntiles) store_tile(t + 1);
        __syncthreads();
    }
    if constexpr (LINK) {
        if (db.unions) {  // (profile = 2) one 64-bit add per wave
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) nun += __shfl_xor(nun, o);
            if (lane == 0 && nun) atomicAdd(db.unions, nun);
        }
    }
    if (a.exact_cnt) {  // (profile = 2) one 64-bit add per wave
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nexact += __shfl_xor(nexact, o);
        if (lane == 0 && nexact) atomicAdd(a.exact_cnt, nexact);
    }
}
#pragma clang fp contract(on)

namespace {

// level[i] = the number of r with count[r][i] < min_samples (the counts are nested: that is the
// smallest r at which the row is a core row, R when there is none).  A candidate is a row that is
// no core row at level 0 and has a neighbour besides itself at its last level as a non-core row.
// cand in no particular order (every offer is an atomicMin on the row's own words); one atomic add
// per wave.
__global__ __launch_bounds__(256) void k_dbscan_sweep_prepare(const int32_t* __restrict__ count, int64_t ldc, int R,
                                                              int32_t min_samples, int64_t n, int32_t* __restrict__ level,
                                                              int32_t* __restrict__ cand, int32_t* nb) {
    const int lane = lane_id();
    const int64_t n64 = (n + 63) & ~(int64_t)63;  // whole waves stay in the loop: the ballot is wave-wide
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n64; i += (int64_t)gridDim.x * 256) {
        bool is = false;
        if (i < n) {
            int c = 0;
            for (int r = 0; r < R; r++) c += count[r * ldc + i] < min_samples ? 1 : 0;
            level[i] = c;
            is = c >= 1 && count[(int64_t)(c - 1) * ldc + i] >= 2;
        }
        const u64 m = __ballot(is);
        if (!m) continue;
        int base = 0;
        if (lane == 0) base = atomicAdd(nb, (int32_t)__popcll(m));
        base = __builtin_amdgcn_readfirstlane(base);
        if (is) cand[base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)i;
    }
}

__global__ __launch_bounds__(256) void k_dbscan_sweep_init(int32_t* __restrict__ parent, uint32_t* __restrict__ best, int R,
                                                           int64_t n) {
    const int64_t total = n * R;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        parent[e] = (int32_t)(e % n);
        best[e] = DBS_NONE;
    }
}

// Level r of the chain (launched in ascending r; forest r is final: every union into it came from
// the link pass or from level r - 1).  A row with c(i) <= r: root[i][r] = find(i) in forest r, and
// the row joins its root in forest r + 1, which so receives level r's components.  Every other
// row: root[i][r] = -1.
__global__ __launch_bounds__(256) void k_dbscan_sweep_level(int32_t* parent_r, int32_t* parent_next,
                                                            const int32_t* __restrict__ level, int r, int R, int64_t n,
                                                            int32_t* __restrict__ root, int32_t* __restrict__ isroot_r,
                                                            int32_t* status, unsigned long long* unions) {
    const int lane = lane_id();
    unsigned long long nun = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int32_t rt = -1;
        if (level[i] <= r) {
            int64_t budget = n + 8;
            rt = uf_find(parent_r, (int32_t)i, budget);
            if (rt < 0) atomicOr(status, KNN_STATUS_UF_LIMIT);
            else if (parent_next && rt != (int32_t)i && uf_union(parent_next, (int32_t)i, rt, n, status)) nun++;
        }
        root[i * R + r] = rt;
        isroot_r[i] = rt == (int32_t)i ? 1 : 0;
    }
    if (unions) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nun += __shfl_xor(nun, o);
        if (lane == 0 && nun) atomicAdd(unions, nun);
    }
}

// labels[r][i] (blockIdx.y = r): a core row its root's cluster number, a row with an offer that
// root's number, every other row -1; offs[r] is the exclusive scan of isroot[r] (n + 1 words), so
// offs[r][root] is the number of roots below it.  info [R][4]: clusters, core, border, noise
// (zeroed by the caller).
__global__ __launch_bounds__(256) void k_dbscan_sweep_labels(const int32_t* __restrict__ level,
                                                             const int32_t* __restrict__ root,
                                                             const uint32_t* __restrict__ best,
                                                             const int64_t* __restrict__ offs, int R, int64_t n,
                                                             int64_t ld_out, int32_t* __restrict__ labels,
                                                             unsigned long long* info) {
    const int lane = lane_id();
    const int r = blockIdx.y;
    const int64_t* of = offs + (int64_t)r * (n + 1);
    unsigned long long core = 0, border = 0, noise = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int32_t v = -1;
        if (level[i] <= r) {
            const int32_t rt = root[i * R + r];
            if (rt >= 0) v = (int32_t)of[rt];
            core++;
        } else {
            const uint32_t b = best[(int64_t)r * n + i];
            if (b != DBS_NONE && (int64_t)b < n) {
                v = (int32_t)of[b];
                border++;
            } else {
                noise++;
            }
        }
        labels[(int64_t)r * ld_out + i] = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        core += __shfl_xor(core, o);
        border += __shfl_xor(border, o);
        noise += __shfl_xor(noise, o);
    }
    if (lane == 0) {
        if (core) atomicAdd(info + 4 * r + 1, core);
        if (border) atomicAdd(info + 4 * r + 2, border);
        if (noise) atomicAdd(info + 4 * r + 3, noise);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) info[4 * r] = (unsigned long long)of[n];
}

template <int M, typename E>
const void* dbs_tile_mode(int mode) {
    return mode == DBSCAN_SWEEP_LINK ? reinterpret_cast<const void*>(&k_dbscan_sweep_tile<M, E, DBSCAN_SWEEP_LINK>)
           : mode == DBSCAN_SWEEP_BORDER ? reinterpret_cast<const void*>(&k_dbscan_sweep_tile<M, E, DBSCAN_SWEEP_BORDER>)
                                         : nullptr;
}
template <int M>
const void* dbs_tile_fn(bool bf, int mode) {
    return bf ? dbs_tile_mode<M, bf16_t>(mode) : dbs_tile_mode<M, float>(mode);
}
// nullptr: no such metric or mode
const void* dbs_tile_ptr(int metric, int elem, int mode) {
    const bool bf = elem == ELEM_BF16;
    switch (metric) {
        case METRIC_SQEUCLIDEAN: return dbs_tile_fn<METRIC_SQEUCLIDEAN>(bf, mode);
        case METRIC_MANHATTAN: return dbs_tile_fn<METRIC_MANHATTAN>(bf, mode);
        case METRIC_CHEBYSHEV: return dbs_tile_fn<METRIC_CHEBYSHEV>(bf, mode);
        default: return nullptr;
    }
}

template <int RB, typename E>
const void* dbs_gemm_mode(int mode) {
    return mode == DBSCAN_SWEEP_LINK ? reinterpret_cast<const void*>(&k_dbscan_sweep_gemm<RB, E, DBSCAN_SWEEP_LINK>)
           : mode == DBSCAN_SWEEP_BORDER ? reinterpret_cast<const void*>(&k_dbscan_sweep_gemm<RB, E, DBSCAN_SWEEP_BORDER>)
                                         : nullptr;
}
template <int RB>
const void* dbs_gemm_fn(int elem, int mode) {
    return elem == ELEM_BF16 ? dbs_gemm_mode<RB, bf16_t>(mode) : dbs_gemm_mode<RB, float>(mode);
}

// the thresholds a kernel may take: 1 <= R <= 32, each in [0, FLT_MAX), non-decreasing
bool dbs_thresholds_ok(const float* thr, int R) {
    if (R < 1 || R > KNN_RADIUS_SWEEP_MAX_R) return false;
    for (int r = 0; r < R; r++)
        if (!(thr[r] >= 0.0f && thr[r] < FLT_MAX) || (r && thr[r] < thr[r - 1])) return false;
    return true;
}

// the tables of a mode, over a self-join of nt <= 2^31 - 1 rows
bool dbs_tables_ok(const DbscanSweepArgs& db, int mode, int64_t nt, int64_t nq, const void* train, const void* test) {
    if (nq != nt || test != train || nt > 0x7fffffffLL || !db.level) return false;
    if (mode == DBSCAN_SWEEP_LINK) return db.parent != nullptr;
    return mode == DBSCAN_SWEEP_BORDER && db.cand && db.nb && db.root && db.best;
}

}  // namespace

// ---------------------------------------------------------------------------------
// Launchers (host side)
// ---------------------------------------------------------------------------------
hipError_t knn_launch_dbscan_sweep_tile(DbscanSweepTileArgs aa, int metric, int mode, hipStream_t st) {
    RadiusSweepArgs& a = aa.s;
    if (a.nq <= 0) return hipSuccess;
    const void* fn = dbs_tile_ptr(metric, a.elem, mode);
    if (!fn || a.nseg < 1 || a.d < 1 || !a.status || !dbs_thresholds_ok(a.thr, a.R) ||
        !dbs_tables_ok(aa.db, mode, a.nt, a.nq, a.train, a.test))
        return hipErrorInvalidValue;
    for (int r = a.R; r < KNN_RADIUS_SWEEP_MAX_R; r++) a.thr[r] = a.thr[a.R - 1];
    knn_direct_tile_geom(a.d, &a.dc, &a.stride);
    const int qb = DT_NW * KNN_RADIUS_QW;
    a.n_qblocks = (int)((a.nq + qb - 1) / qb);
    const dim3 grid((unsigned)((int64_t)a.n_qblocks * a.nseg));
    void* args[] = {&aa};
    const hipError_t e = hipLaunchKernel(fn, grid, dim3(64 * DT_NW), args, 2 * 64 * (size_t)a.stride * 4, st);
    if (e != hipSuccess) return e;
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_dbscan_sweep_gemm(DbscanSweepGemmArgs aa, int mode, hipStream_t st) {
    RadiusSweepGemmArgs& a = aa.s;
    if (a.nq <= 0) return hipSuccess;
    const void* fn = a.d == 64 ? dbs_gemm_fn<128>(a.elem, mode) : a.d == 128 ? dbs_gemm_fn<256>(a.elem, mode)
                     : a.d == 256 ? dbs_gemm_fn<512>(a.elem, mode) : nullptr;
    if (!fn || a.nseg < 1 || a.seg_len < 64 || a.seg_len % 64 || !a.status || !a.tblk || !a.qop || !a.qnorm ||
        !a.qstat || !a.tsmax || !a.train || !a.test || !dbs_thresholds_ok(a.thr, a.R) ||
        !dbs_tables_ok(aa.db, mode, a.nt, a.nq, a.train, a.test))
        return hipErrorInvalidValue;
    for (int r = a.R; r < KNN_RADIUS_SWEEP_MAX_R; r++) a.thr[r] = a.thr[a.R - 1];
    const int qb = 32 * KNN_RADIUS_GEMM_NW;
    a.n_qblocks = (int)((a.nq + qb - 1) / qb);
    const dim3 grid((unsigned)((int64_t)a.n_qblocks * a.nseg));
    const size_t lds = 2 * (64 * (size_t)(2 * a.d + 16) + 16 * (64 / 4 + 1));  // 2 RadiusGemmTile<2 d>::TILE
    void* args[] = {&aa};
    const hipError_t e = hipLaunchKernel(fn, grid, dim3(64 * KNN_RADIUS_GEMM_NW), args, lds, st);
    if (e != hipSuccess) return e;
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_dbscan_sweep_prepare(const int32_t* count, int64_t ldc, int R, int32_t min_samples, int64_t n,
                                           int32_t* level, int32_t* cand, int32_t* nb, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!count || ldc < n || R < 1 || R > KNN_RADIUS_SWEEP_MAX_R || !level || !cand || !nb) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dbscan_sweep_prepare, dim3(elementwise_grid(n)), dim3(256), 0, st, count, ldc, R, min_samples, n,
                       level, cand, nb);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_dbscan_sweep_init(int32_t* parent, uint32_t* best, int R, int64_t n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!parent || !best || R < 1 || R > KNN_RADIUS_SWEEP_MAX_R || n > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dbscan_sweep_init, dim3(elementwise_grid(n * R)), dim3(256), 0, st, parent, best, R, n);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_dbscan_sweep_level(int32_t* parent, const int32_t* level, int r, int R, int64_t n, int32_t* root,
                                         int32_t* isroot_r, int32_t* status, unsigned long long* unions, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!parent || !level || !root || !isroot_r || !status || r < 0 || r >= R || R > KNN_RADIUS_SWEEP_MAX_R)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dbscan_sweep_level, dim3(elementwise_grid(n)), dim3(256), 0, st, parent + (int64_t)r * n,
                       r + 1 < R ? parent + (int64_t)(r + 1) * n : nullptr, level, r, R, n, root, isroot_r, status, unions);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_dbscan_sweep_labels(const int32_t* level, const int32_t* root, const uint32_t* best,
                                          const int64_t* offs, int R, int64_t n, int64_t ld_out, int32_t* labels,
                                          int64_t* info, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!level || !root || !best || !offs || !labels || !info || R < 1 || R > KNN_RADIUS_SWEEP_MAX_R || ld_out < n)
        return hipErrorInvalidValue;
    const unsigned gx = std::min<unsigned>(elementwise_grid(n), 4096u);
    hipLaunchKernelGGL(k_dbscan_sweep_labels, dim3(gx, (unsigned)R), dim3(256), 0, st, level, root, best, offs, R, n, ld_out,
                       labels, reinterpret_cast<unsigned long long*>(info));
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}
