// knn_radius_sweep.hip -- the radius sweep (include/knn_amd.h, "Radius sweep"): the counts and the
// uniform vote of every one of R <= 32 non-decreasing thresholds from one distance pass, and the
// weighted vote of every threshold on CSR lists the caller holds.
//
//   k_radius_sweep_tile<M, E>  the distance pass: k_radius_tile's skeleton (knn_radius.hip); a pair's
//                              bucket (the smallest r with D <= thr[r]) counts into integer
//                              histograms hist [nq][R + 1] and chist [nq][R + 1][C]
//   k_radius_sweep_gemm<RB, E> the MFMA-filtered form of that pass (squared Euclidean, d = 64 / 128 /
//                              256): k_radius_gemm's operands and certificate (knn_radius_gemm.hip)
//                              bracket a pair's bucket; only an undecided pair gets the exact D
//   k_radius_sweep_finish      the prefix over buckets -> count / class_counts / pred [R][ld_out],
//                              correct [R], outliers [R]
//   k_radius_vote_sweep        k_radius_vote on the sub-list dist <= thr[r], one (query, r) per wave
//
// Neighbourhoods are nested (thr is non-decreasing), so everything a threshold's own pass returns
// is a prefix sum over buckets.  The distances are k_radius_tile's, bit for bit (the same flags,
// the same chain); the counters are integers, and every floating-point sum of the vote is one
// thread's chain in list order: the same call returns the same bits every time.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include "knn_kernels.h"

#include "knn_device.h"

#pragma clang fp contract(off)
#include "knn_radius_dev.h"

// ---------------------------------------------------------------------------------
// k_radius_sweep_tile<M, E> (RadiusSweepArgs; the launcher fills dc / stride / n_qblocks and pads
// thr[R..31] with thr[R - 1]).  Blocks, waves, tiles, chunks, query operands and the accumulator:
// k_radius_tile's.  After a tile's last chunk, per query:
//  * pass = valid && D <= thr[R - 1] && row != self; a wave with no passing lane goes on (one
//    ballot, as in k_radius_tile -- in a sparse sweep almost no tile has a member);
//  * a passing lane's bucket is the number of the 32 padded thresholds with !(D <= thr[r]), which
//    is below R for it (the thresholds are wave-uniform kernel arguments: scalar operands);
//  * per distinct bucket of the wave, one lane adds the popcount to hist[q][bucket]; with classes
//    every passing lane adds 1 to chist[q][bucket][label] (integer atomics on global memory, as
//    k_radius_tile's classes == 2 path: an [8][8][R][Cpad] LDS block does not fit four blocks a CU).
// The tile's labels are loaded one per lane and every one is range-checked.  Train segments add
// into the same histograms.  LDS: 2 tile buffers [64][stride] f32.
// ---------------------------------------------------------------------------------
template <int M, typename E>
__global__ __launch_bounds__(64 * DT_NW, 4) void k_radius_sweep_tile(RadiusSweepArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // (the pass behind k_radius_sweep_gemm: only when a norm made the certificate unsafe)
    if (a.gate && !(*a.gate & KNN_STATUS_GEMM_UNSAFE)) return;
    constexpr int NT = 64 * DT_NW;
    constexpr int QW = KNN_RADIUS_QW;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile_floats = 64 * a.stride;
    float* bufs = reinterpret_cast<float*>(smem);
    const int qb = blockIdx.x % a.n_qblocks;
    const int seg = blockIdx.x / a.n_qblocks;
    const int64_t row_begin = (int64_t)seg * a.seg_len;
    const int64_t row_end = min(a.nt, row_begin + a.seg_len);
    const E* __restrict__ train = reinterpret_cast<const E*>(a.train);
    const E* __restrict__ test = reinterpret_cast<const E*>(a.test);
    const int d = a.d;
    const int R = a.R;
    const int R1 = R + 1;
    const float thr_top = a.thr[KNN_RADIUS_SWEEP_MAX_R - 1];  // == thr[R - 1]

    int64_t qi[QW];
    const E* qrow[QW];
    int64_t self[QW];
#pragma unroll
    for (int i = 0; i < QW; i++) {
        qi[i] = (int64_t)qb * (DT_NW * QW) + wave * QW + i;
        qrow[i] = test + (qi[i] < a.nq ? qi[i] : a.nq - 1) * (int64_t)a.ld_q;
        // (a query past the end tests against row -2: nothing passes)
        self[i] = qi[i] < a.nq ? (a.self_base >= 0 ? a.self_base + qi[i] : -1) : -2;
    }

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
        const int gend = min(gpc, ngr - ch * gpc);
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
        if (ch == nchunk - 1) {
            // the tile's distances are final: the threshold tests
            const int64_t row = row_begin + (s / nchunk) * 64 + lane;
            const bool valid = row < row_end;
            int lab = -1;
            if (a.classes && valid) {
                lab = a.labels[row];
                if (lab < 0 || lab >= a.C) {
                    atomicOr(a.status, KNN_STATUS_BAD_LABEL);
                    lab = -1;
                }
            }
#pragma unroll
            for (int i = 0; i < QW; i++) {
                const float D = acc[i];
                acc[i] = 0.0f;  // every metric restarts from +0
                const bool pass = valid && D <= thr_top && row != self[i] && self[i] != -2;
                if (!__ballot(pass)) continue;
                int b = 0;
#pragma unroll
                for (int r = 0; r < KNN_RADIUS_SWEEP_MAX_R; r++) b += D <= a.thr[r] ? 0 : 1;
                if (!pass) b = -1;
                u64 pend = __ballot(pass);
                while (pend) {
                    const int be = __builtin_amdgcn_readlane(b, __ffsll(pend) - 1);
                    const u64 m = __ballot(b == be);
                    pend &= ~m;
                    if (lane == 0) atomicAdd(&a.hist[qi[i] * R1 + be], __popcll(m));
                }
                if (pass && lab >= 0) atomicAdd(&a.chist[(qi[i] * R1 + b) * a.C + lab], 1);
            }
        }
        if (s + 1 < nsteps) store_chunk(s + 1);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------
// k_radius_sweep_gemm<RB, E> (RadiusSweepGemmArgs; RB = 2 d operand bytes per row).  Blocks, waves,
// the query fragments, the tile images, the MFMA loop and the certificate are k_radius_gemm's
// (knn_radius_gemm.hip): y = tn - 2 rn(q).rn(t), G = qn + y, L = G - dl <= D <= U = G + dl.
//  * Fast test: as k_radius_gemm, with tf from thr[R - 1] -- a tile none of whose rows can be
//    within the largest threshold of any of the wave's queries is skipped.
//  * Otherwise, for each of the lane's 32 values that is not surely out of every neighbourhood
//    (!(L > thr[R - 1]); a valid row, not the self row):
//      bl = the number of thresholds with L > thr[r]   (D > thr[r] there: the bucket is >= bl),
//      bu = the number with !(U <= thr[r])             (D <= thr[bu]: the bucket is <= bu);
//    bl == bu decides the bucket without touching the rows.  The others (a NaN bound is among
//    them: never sure, always maybe) get radius_exact once, in a second pass that takes every
//    lane's next row together, and the bucket of that D.  The thresholds sit in one VGPR, lane l
//    holding thr[l & 31]; v_readlane hands thr[r] to the wave.
//  * A member adds 1 to hist[q][bucket] and, with classes, to chist[q][bucket][label] (integer
//    atomics; members are rare where this form runs).  Wave 0 of query block 0 range-checks every
//    label of the segment.
// The kernel returns at once when the status word says KNN_STATUS_GEMM_UNSAFE; k_radius_sweep_tile,
// gated the other way, runs instead.  LDS: 2 tile images.
// ---------------------------------------------------------------------------------
template <int RB, typename E>
__global__ __launch_bounds__(64 * KNN_RADIUS_GEMM_NW) void k_radius_sweep_gemm(RadiusSweepGemmArgs a) {
    typedef RadiusGemmTile<RB> RT;
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
    const int64_t row_end = min(a.nt, row_begin + a.seg_len);
    const int ntiles = row_end > row_begin ? (int)((row_end - row_begin + 63) >> 6) : 0;
    const int R = a.R, R1 = a.R + 1;
    const float thrv = a.thr[lane & (KNN_RADIUS_SWEEP_MAX_R - 1)];
    const float thr = a.thr[KNN_RADIUS_SWEEP_MAX_R - 1];  // == thr[R - 1]
    const float coef = a.coef, eta = a.eta;
    const float INF = __uint_as_float(0x7f800000u);
    const E* __restrict__ train = reinterpret_cast<const E*>(a.train);

    // this lane's query (both lane halves hold the same query, different rows)
    const int64_t q = (int64_t)qb * (32 * NW) + wave * 32 + j;
    const bool qvalid = q < a.nq;
    const E* qrow = reinterpret_cast<const E*>(a.test) + (qvalid ? q : 0) * (int64_t)a.ld_q;
    const int64_t self = (qvalid && a.self_base >= 0) ? a.self_base + q : -1;
    uint4 qf[NS];
    {
        const unsigned char* qop = reinterpret_cast<const unsigned char*>(a.qop) + (qvalid ? q : 0) * (int64_t)RB;
#pragma unroll
        for (int s = 0; s < NS; s++)
            qf[s] = qvalid ? *reinterpret_cast<const uint4*>(qop + 32 * s + 16 * h) : make_uint4(0u, 0u, 0u, 0u);
    }
    const float qn = qvalid ? a.qnorm[q] : 0.0f;
    float qe2 = 0.0f, eq2 = 0.0f;  // 2 |q| and 2 |q - rq|, rounded up
    if (qvalid) {
        const float2 qs = a.qstat[q];
        qe2 = 2.0f * qs.x * (1.0f + 0x1p-17f);
        eq2 = 2.0f * qs.y * (1.0f + 0x1p-17f);
    }
    // the fast test's threshold (k_radius_gemm's, from the largest threshold)
    float tf = -INF;
    if (qvalid) {
        const float4 smax = *a.tsmax;
        const float tk = fmaf(coef + 0x1p-18f, smax.x, fmaf(qe2, smax.y, eq2 * smax.z));
        tf = ((thr - qn) + fmaf(coef, qn, eta)) + 0x1p-18f * (fabsf(thr) + qn + eta) + tk;
    }
    const bool wave_live = __ballot(qvalid) != 0ull;
    unsigned long long nexact = 0;  // pairs given radius_exact

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
        // every label of the segment is range-checked, neighbour or not
        if (a.classes && qb == 0 && wave == 0 && r0 + lane < row_end) {
            const int lab = a.labels[r0 + lane];
            if (lab < 0 || lab >= a.C) atomicOr(a.status, KNN_STATUS_BAD_LABEL);
        }
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
                // rows of the segment, without the self row; nothing for a query past the end
                const int64_t nv = row_end - r0;
                u64 vm = nv >= 64 ? ~0ull : ((1ull << nv) - 1ull);
                if (self >= r0 && self < r0 + 64) vm &= ~(1ull << (int)(self - r0));
                if (!qvalid) vm = 0ull;
                // Pass 1, per value: its 6-bit code -- the bucket where the bracket decides it,
                // UNDECIDED otherwise -- packed ten to a 64-bit word at the value's fixed place.
                constexpr u64 UNDECIDED = 63;
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
                            // (bl == bu is below R: L > thr[R - 1] fails)
                            const int s = 16 * c + r;  // (a constant once unrolled)
                            code[s / 10] |= (bl == bu ? (u64)bl : UNDECIDED) << (6 * (s % 10));
                            todo |= 1ull << b;
                        }
                    }
                }
                // Pass 2, every lane's next row together: the exact D of an undecided row and its
                // bucket; a member adds 1 to its bucket's counters.
                while (todo) {
                    const int b = __ffsll((long long)todo) - 1;
                    todo &= todo - 1ull;
                    const int s = 16 * (b >> 5) + (b & 3) + 4 * ((b & 31) >> 3);  // the value of row b
                    const int w10 = s / 10;
                    const u64 cw = w10 == 0 ? code[0] : w10 == 1 ? code[1] : w10 == 2 ? code[2] : code[3];
                    int bk = (int)((cw >> (6 * (s - 10 * w10))) & 63ull);
                    if (bk == (int)UNDECIDED) {
                        const float Dx = radius_exact<E>(qrow, train + (r0 + b) * (int64_t)a.ld_t, D);
                        nexact++;
                        bk = 0;
                        for (int k = 0; k < R; k++) bk += Dx <= thr_at(k) ? 0 : 1;
                    }
                    if (bk < R) {
                        atomicAdd(&a.hist[q * R1 + bk], 1);
                        if (a.classes) {
                            const int lab = a.labels[r0 + b];
                            if (lab >= 0 && lab < a.C) atomicAdd(&a.chist[(q * R1 + bk) * a.C + lab], 1);
                        }
                    }
                }
            }
        }
        if (t + 1 < ntiles) store_tile(t + 1);
        __syncthreads();
    }
    if (a.exact_cnt) {  // (profile = 2) one 64-bit add per wave
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nexact += __shfl_xor(nexact, o);
        if (lane == 0 && nexact) atomicAdd(a.exact_cnt, nexact);
    }
}
#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------
// k_radius_sweep_finish (RadiusSweepFinishArgs), one wave per query.
//  * count[r][q] = the inclusive prefix over buckets of hist[q][.]; a query with count[r][q] == 0
//    is one of outliers[r].
//  * With classes: per class, the prefix over buckets of chist[q][.][c], written back in place
//    (and to class_counts[r][q][c] when asked); then per r the argmax over c of that row, ties to
//    the smallest label, outlier where the count is 0 -> pred[r][q], correct[r].  A lane reads in
//    the second step only what it wrote itself in the first (c = lane, lane + 64, ...).
//  * correct / outliers: LDS integer counters per block, one global integer atomic per block and r.
//    They are ADDED to: the caller zeroes them (query blocks accumulate).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_radius_sweep_finish(RadiusSweepFinishArgs a) {
    __shared__ unsigned ok_s[KNN_RADIUS_SWEEP_MAX_R], out_s[KNN_RADIUS_SWEEP_MAX_R];
    const int lane = lane_id();
    const int R = a.R, R1 = a.R + 1;
    if (threadIdx.x < KNN_RADIUS_SWEEP_MAX_R) {
        ok_s[threadIdx.x] = 0;
        out_s[threadIdx.x] = 0;
    }
    __syncthreads();
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < a.nq; q += (int64_t)gridDim.x * 4) {
        const int32_t* h = a.hist + q * R1;
        if (a.classes) {
            int32_t* ch = a.chist + q * R1 * a.C;
            for (int c = lane; c < a.C; c += 64) {
                int run = 0;
                for (int r = 0; r < R; r++) {
                    run += ch[(int64_t)r * a.C + c];
                    ch[(int64_t)r * a.C + c] = run;
                    if (a.class_counts) a.class_counts[((int64_t)r * a.ld_out + q) * a.C + c] = run;
                }
            }
        }
        int cnt = 0;
        for (int r = 0; r < R; r++) {
            cnt += h[r];
            if (lane == 0) {
                if (a.count) a.count[(int64_t)r * a.ld_out + q] = cnt;
                if (a.outliers && cnt == 0) atomicAdd(&out_s[r], 1u);
            }
            if (!a.classes || (!a.pred && !a.correct)) continue;
            const int32_t* cc = a.chist + (q * R1 + r) * a.C;
            u64 best = 0;
            for (int c = lane; c < a.C; c += 64)
                best = umax64(best, ((u64)(uint32_t)cc[c] << 32) | (u64)(0xffffffffu - (uint32_t)c));
#pragma unroll
            for (int j = 32; j > 0; j >>= 1) best = umax64(best, __shfl_xor(best, j));
            const int32_t p = (best >> 32) ? (int32_t)(0xffffffffu - (uint32_t)(best & 0xffffffffull)) : a.outlier;
            if (lane == 0) {
                if (a.pred) a.pred[(int64_t)r * a.ld_out + q] = p;
                if (a.correct && p == a.qlabels[q]) atomicAdd(&ok_s[r], 1u);
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < R) {
        if (a.correct && ok_s[threadIdx.x]) atomicAdd(&a.correct[threadIdx.x], (unsigned long long)ok_s[threadIdx.x]);
        if (a.outliers && out_s[threadIdx.x])
            atomicAdd(&a.outliers[threadIdx.x], (unsigned long long)out_s[threadIdx.x]);
    }
}

#pragma clang fp contract(off)
// ---------------------------------------------------------------------------------
// k_radius_vote_sweep (RadiusVoteSweepArgs): k_radius_vote (knn_radius.hip) on the sub-list of the
// entries with dist <= thr[r], one (query, r) unit per wave over the same CSR segment.
//  * Pass 1 runs the checks on EVERY entry of the segment (index, label, distance: the status a
//    single-threshold vote of the whole list sets), and finds the zero rule among the entries of
//    the sub-list alone.
//  * Pass 2 skips the entries with dist > thr[r]; the others add their weight to S_c in ascending
//    list position, one thread's chain of binary32 adds per class, as in k_radius_vote.
//  * The vote: the argmax of (bits(S_c), -c); an empty sub-list gives the outlier label and leaves
//    its score row +0.
// scores [R][ld_out][C] (the caller's, or workspace) is zeroed by the launcher's caller; pred is
// [R][ld_out]; correct [R] is added to.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_radius_vote_sweep(RadiusVoteSweepArgs a) {
    __shared__ unsigned ok_s[KNN_RADIUS_SWEEP_MAX_R];
    const int lane = lane_id();
    const int R = a.R;
    if (threadIdx.x < KNN_RADIUS_SWEEP_MAX_R) ok_s[threadIdx.x] = 0;
    __syncthreads();
    const int64_t units = a.nq * R;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += (int64_t)gridDim.x * 4) {
        const int64_t q = u / R;
        const int r = (int)(u - q * R);
        const float thr = a.thr[r];
        const int64_t o0 = a.offsets[q], o1 = a.offsets[q + 1];
        float* S = a.scores + ((int64_t)r * a.ld_out + q) * a.C;
        bool bad = false;
        if (o0 < 0 || o1 < o0) {
            if (lane == 0) atomicOr(a.status, KNN_STATUS_BAD_OFFSETS);
            bad = true;
        }
        bool zero_mode = false, any = false;
        for (int64_t e0 = o0; !bad && e0 < o1; e0 += 64) {
            const int64_t e = e0 + lane;
            bool z = false, in = false;
            if (e < o1) {
                const int32_t t = a.idx[e];
                if (t < 0 || t >= a.n_train) atomicOr(a.status, KNN_STATUS_BAD_INDEX);
                else if (a.labels[t] < 0 || a.labels[t] >= a.C) atomicOr(a.status, KNN_STATUS_BAD_LABEL);
                const float dd = a.dist[e];
                if (!(dd >= 0.0f)) atomicOr(a.status, KNN_STATUS_BAD_DIST);
                in = dd <= thr;
                z = in && dd == 0.0f;
            }
            if (__ballot(in)) any = true;
            if (a.weights != KNN_VOTE_W_UNIFORM && __ballot(z)) zero_mode = true;
        }
        for (int64_t e0 = o0; any && e0 < o1; e0 += 64) {
            const int64_t e = e0 + lane;
            int lab = -1;
            float w = 0.0f;
            if (e < o1) {
                const float dd = a.dist[e];
                const int32_t t = a.idx[e];
                if (dd <= thr && t >= 0 && t < a.n_train) {
                    const int l = a.labels[t];
                    if (l >= 0 && l < a.C) lab = l;
                }
                w = vote_weight(a.weights, zero_mode, dd);
            }
            u64 pend = __ballot(lab >= 0);
            while (pend) {
                const int le = __builtin_amdgcn_readlane(lab, __ffsll(pend) - 1);
                u64 m = __ballot(lab == le);
                pend &= ~m;
                float run = 0.0f;
                if (lane == 0) run = S[le];
                run = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(run)));
                while (m) {
                    const int b = __ffsll(m) - 1;
                    m &= m - 1;
                    run = run + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), b));
                }
                if (lane == 0) S[le] = run;
            }
        }
        // lane 0's stores, read by every lane
        __threadfence();
        __builtin_amdgcn_wave_barrier();
        u64 best = 0;
        if (any)
            for (int c = lane; c < a.C; c += 64)
                best = umax64(best, ((u64)__float_as_uint(S[c]) << 32) | (u64)(0xffffffffu - (uint32_t)c));
#pragma unroll
        for (int j = 32; j > 0; j >>= 1) best = umax64(best, __shfl_xor(best, j));
        const int32_t p = any ? (int32_t)(0xffffffffu - (uint32_t)(best & 0xffffffffull)) : a.outlier;
        if (lane == 0) {
            if (a.pred) a.pred[(int64_t)r * a.ld_out + q] = p;
            if (a.correct && p == a.qlabels[q]) atomicAdd(&ok_s[r], 1u);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < R && a.correct && ok_s[threadIdx.x])
        atomicAdd(&a.correct[threadIdx.x], (unsigned long long)ok_s[threadIdx.x]);
}
#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------
// Launchers (host side)
// ---------------------------------------------------------------------------------
template <int M>
static const void* sweep_tile_fn(bool bf) {
    return bf ? reinterpret_cast<const void*>(&k_radius_sweep_tile<M, bf16_t>)
              : reinterpret_cast<const void*>(&k_radius_sweep_tile<M, float>);
}
// nullptr: no such metric
static const void* sweep_tile_ptr(int metric, int elem) {
    const bool bf = elem == ELEM_BF16;
    switch (metric) {
        case METRIC_SQEUCLIDEAN: return sweep_tile_fn<METRIC_SQEUCLIDEAN>(bf);
        case METRIC_MANHATTAN: return sweep_tile_fn<METRIC_MANHATTAN>(bf);
        case METRIC_CHEBYSHEV: return sweep_tile_fn<METRIC_CHEBYSHEV>(bf);
        default: return nullptr;
    }
}

static size_t sweep_tile_lds(int d) {
    int dc, stride;
    knn_direct_tile_geom(d, &dc, &stride);
    return 2 * 64 * (size_t)stride * 4;
}

// the thresholds a kernel may take: 1 <= R <= 32, each in [0, FLT_MAX), non-decreasing
static bool sweep_thresholds_ok(const float* thr, int R) {
    if (R < 1 || R > KNN_RADIUS_SWEEP_MAX_R) return false;
    for (int r = 0; r < R; r++)
        if (!(thr[r] >= 0.0f && thr[r] < FLT_MAX) || (r && thr[r] < thr[r - 1])) return false;
    return true;
}

hipError_t knn_launch_radius_sweep_tile(RadiusSweepArgs a, int metric, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    const void* fn = sweep_tile_ptr(metric, a.elem);
    if (!fn || a.nseg < 1 || a.d < 1 || !a.status || !a.hist || !sweep_thresholds_ok(a.thr, a.R))
        return hipErrorInvalidValue;
    if (a.classes) {
        if (a.C < 1 || !a.labels || !a.chist) return hipErrorInvalidValue;
        a.classes = 1;
    }
    for (int r = a.R; r < KNN_RADIUS_SWEEP_MAX_R; r++) a.thr[r] = a.thr[a.R - 1];
    knn_direct_tile_geom(a.d, &a.dc, &a.stride);
    const int qb = DT_NW * KNN_RADIUS_QW;
    a.n_qblocks = (int)((a.nq + qb - 1) / qb);
    const dim3 grid((unsigned)((int64_t)a.n_qblocks * a.nseg));
    void* args[] = {&a};
    const hipError_t e = hipLaunchKernel(fn, grid, dim3(64 * DT_NW), args, sweep_tile_lds(a.d), st);
    if (e != hipSuccess) return e;
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

template <int RB>
static const void* sweep_gemm_fn(int elem) {
    return elem == ELEM_BF16 ? reinterpret_cast<const void*>(&k_radius_sweep_gemm<RB, bf16_t>)
                             : reinterpret_cast<const void*>(&k_radius_sweep_gemm<RB, float>);
}

hipError_t knn_launch_radius_sweep_gemm(RadiusSweepGemmArgs a, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    const void* fn = a.d == 64 ? sweep_gemm_fn<128>(a.elem) : a.d == 128 ? sweep_gemm_fn<256>(a.elem)
                     : a.d == 256 ? sweep_gemm_fn<512>(a.elem) : nullptr;
    if (!fn || a.nseg < 1 || a.seg_len < 64 || a.seg_len % 64 || !a.status || !a.tblk || !a.qop || !a.qnorm ||
        !a.qstat || !a.tsmax || !a.train || !a.test || !a.hist || !sweep_thresholds_ok(a.thr, a.R))
        return hipErrorInvalidValue;
    if (a.classes && (a.C < 1 || !a.labels || !a.chist)) return hipErrorInvalidValue;
    for (int r = a.R; r < KNN_RADIUS_SWEEP_MAX_R; r++) a.thr[r] = a.thr[a.R - 1];
    const int qb = 32 * KNN_RADIUS_GEMM_NW;
    a.n_qblocks = (int)((a.nq + qb - 1) / qb);
    const dim3 grid((unsigned)((int64_t)a.n_qblocks * a.nseg));
    const size_t lds = 2 * (64 * (size_t)(2 * a.d + 16) + 16 * (64 / 4 + 1));  // 2 RadiusGemmTile<2 d>::TILE
    void* args[] = {&a};
    const hipError_t e = hipLaunchKernel(fn, grid, dim3(64 * KNN_RADIUS_GEMM_NW), args, lds, st);
    if (e != hipSuccess) return e;
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_radius_sweep_finish(const RadiusSweepFinishArgs& a, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    if (!a.hist || a.R < 1 || a.R > KNN_RADIUS_SWEEP_MAX_R || a.ld_out < a.nq) return hipErrorInvalidValue;
    if (a.classes && (a.C < 1 || !a.chist)) return hipErrorInvalidValue;
    if (!a.classes && (a.class_counts || a.pred || a.correct)) return hipErrorInvalidValue;
    if (a.correct && !a.qlabels) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<int64_t>((a.nq + 3) / 4, 1024);
    hipLaunchKernelGGL(k_radius_sweep_finish, dim3(grid), dim3(256), 0, st, a);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_radius_vote_sweep(const RadiusVoteSweepArgs& a, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    if (!a.offsets || !a.idx || !a.dist || !a.labels || !a.scores || !a.status || a.C < 1 || a.n_train < 0 ||
        a.weights < KNN_VOTE_W_UNIFORM || a.weights > KNN_VOTE_W_INV_SQDIST || (a.correct && !a.qlabels) ||
        a.ld_out < a.nq || !sweep_thresholds_ok(a.thr, a.R))
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<int64_t>((a.nq * a.R + 3) / 4, 8192);
    hipLaunchKernelGGL(k_radius_vote_sweep, dim3(grid), dim3(256), 0, st, a);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}
