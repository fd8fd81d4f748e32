// knn_radius_gemm.hip -- the MFMA-filtered form of the radius distance pass (include/knn_amd.h,
// "Radius neighbours"; DESIGN.md "Radius neighbours", "The MFMA form"): squared Euclidean, d in
// {64, 128, 256}, fp32 or bf16 rows.
//
//   k_radius_gemm<RB, E, MODE>  the fused filter's operands and certificate (knn_fused.hip) against
//                               a threshold that is known before the scan
//
// Operands (built by the fused filter's own launchers): train as tile blocks of 64 rows,
//   [64][d] bf16 rn(t) | 64 fp32 norms tn | {max tn, max |t - rt|, max |rt|, 0},
// queries as [nq][d] bf16 rn(-2 q) with their norms qn and statistics {|q|, |q - rq|}.  Each
// accumulator starts from its rows' norms, so d/16 steps of v_mfma_f32_32x32x16_bf16 leave
//   y = tn - 2 rn(q).rn(t),
// and the certificate of k_gemm_fused (bounds(), certificate_fused) brackets the reference's
// direct-form distance D:  G = qn + y,  dl = coef (qn + tmax_tile) + eta + rho(q, tile),
//   L = G - dl <= D <= U = G + dl.
// A fixed threshold uses both sides: U <= thr puts the row in, L > thr puts it out, and only the
// rows between get D itself -- radius_exact, the bits of k_radius_tile's radius_step chain -- and
// the membership test D <= thr on that value.  Every output is therefore what k_radius_tile gives.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include "knn_kernels.h"

#include "knn_device.h"

#pragma clang fp contract(off)
#include "knn_radius_dev.h"  // RadiusGemmTile<RB>, radius_exact<E>
#include "knn_dbscan_dev.h"  // uf_union

// ---------------------------------------------------------------------------------
// k_radius_gemm<RB, E, MODE> (RadiusGemmArgs; RB = 2 d operand bytes per row, E the caller's
// element).  A block of 8 waves owns 256 queries, 32 per wave, against one train segment (a
// multiple of 64 rows); lane (j, h) holds its query's B fragments in VGPRs for the whole scan.
//  * Train tile blocks go global -> registers -> LDS, two buffers, one barrier per tile; the LDS
//    image and the fragment / norm reads are k_gemm_fused's (fused_frag_off, fused_norm_off).
//  * Register r of accumulator c is tile row 32 c + (r & 3) + 8 (r >> 2) + 4 h against query j.
//  * Fast test: the tile is skipped for the wave when no lane has min y <= tf, tf = thr - qn +
//    coef qn + eta + the maxima of the tile terms over all tiles + slack -- implied by `maybe`.
//  * Otherwise each lane classifies its 32 values (sure = U <= thr, maybe = !(L > thr): a NaN is
//    never sure and always maybe), masks rows past the segment's end and the self row, resolves
//    its maybe-but-not-sure rows with radius_exact, and ORs its 64-bit member mask with its
//    partner's (lane ^ 32): both then hold the query's members of the tile.
//  * MODE = RADIUS_COUNT: the running count grows by popcount; members add 1 to class_counts[q][label]
//    (integer atomics; members are rare where this form runs).  Wave 0 of query block 0 range-checks
//    every label of the segment, one 256-byte load per tile.  At the end seg_count[seg][q].
//  * MODE = RADIUS_FILL: member row b stores at base + count + popcount(mask & rows below b), inside the
//    part [base[seg][q], base[seg + 1][q]) and below offsets[q + 1], with D when dist is asked
//    (radius_exact for a sure row; a band member's D is the one that classified it); a count that does not end at the part's length sets KNN_STATUS_BAD_OFFSETS.
//  * MODE = RADIUS_LINK / RADIUS_BORDER, DBSCAN's two passes (RadiusDbscanArgs; knn_amd.h "DBSCAN"):
//    the valid-row mask also drops the tile's non-core rows (one word per lane and tile, a ballot)
//    and, for LINK, the rows not below the query, BEFORE the band is resolved -- no exact distance
//    is spent on a pair that cannot matter.  LINK: a lane whose query is no core row takes no part,
//    the scan ends at the tile of the block's last query, and each member calls uf_union.  BORDER:
//    lane's query is train row cand[q] (operands, norms and rows are read through it; blocks past *nb
//    return), each member offers its cluster number, and the minimum of both lane halves goes into
//    out_labels with an integer atomicMin.
// The kernel returns at once when the status word says KNN_STATUS_GEMM_UNSAFE (a norm that is NaN,
// inf or >= 2^125: the certificate does not hold; k_radius_tile, gated the other way, runs instead).
// LDS: 2 tile images.
// ---------------------------------------------------------------------------------
template <int RB, typename E, int MODE>
__global__ __launch_bounds__(64 * KNN_RADIUS_GEMM_NW) void k_radius_gemm(RadiusGemmArgs a) {
    typedef RadiusGemmTile<RB> RT;
    constexpr bool COUNT = MODE == RADIUS_COUNT, FILL = MODE == RADIUS_FILL;
    constexpr bool LINK = MODE == RADIUS_LINK, BORDER = MODE == RADIUS_BORDER;
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
    // (BORDER: the candidates, counted on the device; the grid is sized for every row)
    int64_t nq = a.nq;
    if constexpr (BORDER) {
        nq = *a.db.nb;
        if ((int64_t)qb * (32 * NW) >= nq) return;  // (block-uniform, before any barrier)
    }
    // (LINK: only rows below the query make a union, so the scan ends at the 64-row tile that
    // holds the block's last query)
    if constexpr (LINK) row_end = min(row_end, (min(nq, (int64_t)(qb + 1) * (32 * NW)) + 63) & ~(int64_t)63);
    const int ntiles = row_end > row_begin ? (int)((row_end - row_begin + 63) >> 6) : 0;
    const float thr = a.thr, coef = a.coef, eta = a.eta;
    const float INF = __uint_as_float(0x7f800000u);
    const E* __restrict__ train = reinterpret_cast<const E*>(a.train);

    // this lane's query (both lane halves hold the same query, different rows)
    const int64_t q = (int64_t)qb * (32 * NW) + wave * 32 + j;
    const bool qvalid = q < nq;
    // the row its operands are read from: q itself, or (BORDER) the candidate's train row
    int64_t qx = qvalid ? q : 0;
    if constexpr (BORDER) qx = qvalid ? a.db.cand[q] : 0;
    // whether the query takes part in the scan: (LINK) only a core row does
    bool qlive = qvalid;
    if constexpr (LINK) qlive = qvalid && a.db.dcount[q] >= a.db.min_samples;
    const E* qrow = reinterpret_cast<const E*>(a.test) + qx * (int64_t)a.ld_q;
    const int64_t self = (qvalid && a.self_base >= 0) ? a.self_base + q : -1;
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
    // The fast test's threshold, constant for the scan: with the maxima over all tiles of the tile
    // statistics (tsmax) every tile's dl is <= coef qn + eta + tk, so !(L > thr), i.e. y <= thr -
    // qn + dl up to the roundings of G, L and of tf itself (<= 2^-21 of the magnitudes involved),
    // implies y <= tf.  A passing y is never NaN here: the pass runs only with every norm finite
    // and below 2^125, where every partial sum of the MFMA chain is finite.
    float tf = -INF;
    if (qlive) {
        const float4 smax = *a.tsmax;
        const float tk = fmaf(coef + 0x1p-18f, smax.x, fmaf(qe2, smax.y, eq2 * smax.z));
        tf = ((thr - qn) + fmaf(coef, qn, eta)) + 0x1p-18f * (fabsf(thr) + qn + eta) + tk;
    }
    const bool wave_live = __ballot(qlive) != 0ull;
    [[maybe_unused]] uint32_t best = 0xffffffffu;  // (BORDER) the smallest cluster number so far
    [[maybe_unused]] unsigned long long nun = 0;   // (LINK) successful hooks

    int run = 0;        // the query's members so far (the same in both lane halves)
    int64_t base = 0;   // (FILL) where this segment's part of the query's list starts
    int room = 0;       // (FILL) and how many entries it may take
    if constexpr (FILL) {
        if (qvalid) {
            const int64_t end = a.offsets[q + 1];
            const int64_t next = seg + 1 < a.nseg ? a.base[(int64_t)(seg + 1) * a.nq + q] : end;
            base = a.base[(int64_t)seg * a.nq + q];
            const int64_t r = min(next, end) - base;
            room = base >= a.offsets[q] ? (int)max((int64_t)0, min(r, (int64_t)0x7fffffff)) : 0;
        }
    }
    unsigned long long nexact = 0;  // pairs given radius_exact

    // ---- tile blocks: global -> registers (in flight during the tile before) -> LDS
    const unsigned char* tsrc = reinterpret_cast<const unsigned char*>(a.tblk) + (row_begin >> 6) * RT::TB;
    // Rows: 64 SPR slots, whole rounds of the block's NT threads; the HS header slots take one more
    // load of the first HS threads alone.  (A native vector type: an array of HIP's uint4 structs
    // stayed in scratch here.)
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
        if constexpr (COUNT) {
            // every label of the segment is range-checked, neighbour or not
            if (a.classes && qb == 0 && wave == 0 && r0 + lane < row_end) {
                const int lab = a.labels[r0 + lane];
                if (lab < 0 || lab >= a.C) atomicOr(a.status, KNN_STATUS_BAD_LABEL);
            }
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
                u64 mb = 0, sb = 0;  // maybe / sure, bit = tile row - 4 h
#pragma unroll
                for (int c = 0; c < 2; c++) {
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const float G = qn + X[c][r];
                        const float L = G - dl;
                        const float U = G + dl;
                        const u64 bit = 1ull << (32 * c + (r & 3) + 8 * (r >> 2));
                        if (!(L > thr)) mb |= bit;
                        if (U <= thr) sb |= bit;
                    }
                }
                // rows of the segment, without the self row; nothing for a query past the end
                const int64_t nv = row_end - r0;
                u64 vm = nv >= 64 ? ~0ull : ((1ull << nv) - 1ull);
                if (self >= r0 && self < r0 + 64) vm &= ~(1ull << (int)(self - r0));
                if (!qlive) vm = 0ull;
                if constexpr (LINK || BORDER) {
                    // the tile's core rows, one word per lane (LINK: the neighbour count against
                    // min_samples; BORDER: a cluster number); LINK keeps the rows below the query
                    const int64_t tr = r0 + lane;
                    bool tc = false;
                    if constexpr (LINK) tc = tr < row_end && a.db.dcount[tr] >= a.db.min_samples;
                    else tc = tr < row_end && a.db.cluster[tr] >= 0;
                    vm &= __ballot(tc);
                    if constexpr (LINK) {
                        const int64_t below = q - r0;  // rows of the tile with an index under q's
                        if (below < 64) vm &= below > 0 ? (1ull << below) - 1ull : 0ull;
                    }
                }
                mb = (mb << (4 * h)) & vm;
                sb = (sb << (4 * h)) & vm;
                u64 band = mb & ~sb;
                u64 bmem = 0ull;  // band rows found to be members
                // (FILL) the distances of the lane's first four of them, kept for the store
                [[maybe_unused]] float kd0 = 0.0f, kd1 = 0.0f, kd2 = 0.0f, kd3 = 0.0f;
                while (band) {
                    const int b = __ffsll((long long)band) - 1;
                    band &= band - 1ull;
                    const float Dx = radius_exact<E>(qrow, train + (r0 + b) * (int64_t)a.ld_t, D);
                    nexact++;
                    if (Dx <= thr) {
                        if constexpr (FILL) {
                            const int jn = __popcll(bmem);
                            if (jn == 0) kd0 = Dx;
                            else if (jn == 1) kd1 = Dx;
                            else if (jn == 2) kd2 = Dx;
                            else if (jn == 3) kd3 = Dx;
                        }
                        bmem |= 1ull << b;
                    }
                }
                u64 mem = sb | bmem;
                if constexpr (LINK) {
                    while (mem) {
                        const int b = __ffsll((long long)mem) - 1;
                        mem &= mem - 1ull;
                        if (uf_union(a.db.parent, (int32_t)q, (int32_t)(r0 + b), a.nt, a.status)) nun++;
                    }
                } else if constexpr (BORDER) {
                    while (mem) {
                        const int b = __ffsll((long long)mem) - 1;
                        mem &= mem - 1ull;
                        best = min(best, (uint32_t)a.db.cluster[r0 + b]);
                    }
                }
                [[maybe_unused]] u64 m64 = 0ull;
                if constexpr (COUNT || FILL) m64 = mem | lane_xor64(mem, 32);
                if constexpr (FILL) {
                    while (mem) {
                        const int b = __ffsll((long long)mem) - 1;
                        mem &= mem - 1ull;
                        const int p = run + __popcll(m64 & ((1ull << b) - 1ull));
                        if (p < room) {
                            a.idx[base + p] = (int32_t)(r0 + b);
                            if (a.dist) {
                                // a band member's D was computed above; a sure row's, or a fifth band
                                // member's, is computed here
                                const int jn = ((bmem >> b) & 1ull) ? __popcll(bmem & ((1ull << b) - 1ull)) : 4;
                                float Dv;
                                if (jn < 4) {
                                    Dv = jn == 0 ? kd0 : jn == 1 ? kd1 : jn == 2 ? kd2 : kd3;
                                } else {
                                    Dv = radius_exact<E>(qrow, train + (r0 + b) * (int64_t)a.ld_t, D);
                                    nexact++;
                                }
                                a.dist[base + p] = Dv;
                            }
                        }
                    }
                } else if (COUNT && a.classes) {
                    while (mem) {
                        const int b = __ffsll((long long)mem) - 1;
                        mem &= mem - 1ull;
                        const int lab = a.labels[r0 + b];
                        if (lab >= 0 && lab < a.C) atomicAdd(&a.class_counts[q * a.C + lab], 1);
                    }
                }
                run += __popcll(m64);
            }
        }
        if (t + 1 < ntiles) store_tile(t + 1);
        __syncthreads();
    }

    if constexpr (LINK) {
        if (a.db.unions) {  // (profile = 2) one 64-bit add per wave
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) nun += __shfl_xor(nun, o);
            if (lane == 0 && nun) atomicAdd(a.db.unions, nun);
        }
    } else if constexpr (BORDER) {
        // both lane halves' minima, then the train segments' through an integer atomicMin
        // (unsigned: -1, "none yet", is the largest value)
        best = min(best, lane_xor(best, 32));
        if (qvalid && h == 0 && best != 0xffffffffu)
            atomicMin(reinterpret_cast<unsigned int*>(a.db.out_labels) + qx, best);
    } else if (qvalid && h == 0) {
        if constexpr (FILL) {
            const int64_t end = a.offsets[q + 1];
            const int64_t next = seg + 1 < a.nseg ? a.base[(int64_t)(seg + 1) * a.nq + q] : end;
            if (next - base != (int64_t)run || base < a.offsets[q] || next > end)
                atomicOr(a.status, KNN_STATUS_BAD_OFFSETS);
        } else {
            a.seg_count[(int64_t)seg * a.nq + q] = run;
        }
    }
    if (a.exact_cnt) {  // (profile = 2) one 64-bit add per wave
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nexact += __shfl_xor(nexact, o);
        if (lane == 0 && nexact) atomicAdd(a.exact_cnt, nexact);
    }
}
#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------
// Launchers (host side)
// ---------------------------------------------------------------------------------
template <int RB, typename E>
static const void* radius_gemm_mode(int mode) {
    switch (mode) {
        case RADIUS_COUNT: return reinterpret_cast<const void*>(&k_radius_gemm<RB, E, RADIUS_COUNT>);
        case RADIUS_FILL: return reinterpret_cast<const void*>(&k_radius_gemm<RB, E, RADIUS_FILL>);
        case RADIUS_LINK: return reinterpret_cast<const void*>(&k_radius_gemm<RB, E, RADIUS_LINK>);
        case RADIUS_BORDER: return reinterpret_cast<const void*>(&k_radius_gemm<RB, E, RADIUS_BORDER>);
        default: return nullptr;
    }
}
template <int RB>
static const void* radius_gemm_fn(int elem, int mode) {
    return elem == ELEM_BF16 ? radius_gemm_mode<RB, bf16_t>(mode) : radius_gemm_mode<RB, float>(mode);
}
// nullptr: no such shape or mode
static const void* radius_gemm_ptr(int d, int elem, int fill) {
    switch (d) {
        case 64: return radius_gemm_fn<128>(elem, fill);
        case 128: return radius_gemm_fn<256>(elem, fill);
        case 256: return radius_gemm_fn<512>(elem, fill);
        default: return nullptr;
    }
}

bool knn_radius_gemm_supported(int d) { return d == 64 || d == 128 || d == 256; }

size_t knn_radius_gemm_tile_bytes(int d) { return 64 * (size_t)(2 * d) + 16 * (64 / 4 + 1); }

static size_t radius_gemm_lds(int d) { return 2 * (64 * (size_t)(2 * d + 16) + 16 * (64 / 4 + 1)); }

hipError_t knn_radius_gemm_units(int elem, int d, int* queries_per_unit, int* units_per_cu) {
    const void* fn = radius_gemm_ptr(d, elem, false);
    if (!fn) return hipErrorInvalidValue;
    int occ = 1;
    const hipError_t e =
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 64 * KNN_RADIUS_GEMM_NW, radius_gemm_lds(d));
    *queries_per_unit = 32 * KNN_RADIUS_GEMM_NW;
    *units_per_cu = std::max(occ, 1);
    return e;
}

hipError_t knn_launch_radius_gemm(RadiusGemmArgs a, int mode, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    const void* fn = radius_gemm_ptr(a.d, a.elem, mode);
    if (!fn || a.nseg < 1 || a.seg_len < 64 || a.seg_len % 64 || !a.status || !a.tblk || !a.qop || !a.qnorm ||
        !a.qstat || !a.tsmax || !a.train || !a.test)
        return hipErrorInvalidValue;
    const bool fill = mode == RADIUS_FILL, count = mode == RADIUS_COUNT;
    if (fill && (!a.base || !a.offsets || !a.idx)) return hipErrorInvalidValue;
    if (count && !a.seg_count) return hipErrorInvalidValue;
    if (count && a.classes && (a.C < 1 || !a.labels || !a.class_counts)) return hipErrorInvalidValue;
    // the DBSCAN modes are self-joins over tables of nt rows
    if (mode == RADIUS_LINK && (a.nq != a.nt || a.test != a.train || !a.db.dcount || !a.db.parent || a.nt > 0x7fffffffLL))
        return hipErrorInvalidValue;
    if (mode == RADIUS_BORDER &&
        (a.nq != a.nt || a.test != a.train || !a.db.cand || !a.db.nb || !a.db.cluster || !a.db.out_labels))
        return hipErrorInvalidValue;
    const int qb = 32 * KNN_RADIUS_GEMM_NW;
    a.n_qblocks = (int)((a.nq + qb - 1) / qb);
    const dim3 grid((unsigned)((int64_t)a.n_qblocks * a.nseg));
    void* args[] = {&a};
    const hipError_t e = hipLaunchKernel(fn, grid, dim3(64 * KNN_RADIUS_GEMM_NW), args, radius_gemm_lds(a.d), st);
    if (e != hipSuccess) return e;
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}
