// knn_radius.hip -- radius neighbours (include/knn_amd.h, "Radius neighbours"): which train rows
// lie within a fixed threshold of a query, how many, and what they vote.
//
//   k_radius_tile<M, E, MODE>  the distance pass: k_metric_tile's skeleton (knn_metric.hip) with
//                              the selection replaced by `D <= thr`, a ballot and a popcount
//   k_radius_scan              per-(segment, query) counts -> count [nq], int64 offsets [nq + 1]
//   k_radius_bases             a caller's offsets + the counts -> where each segment's part starts
//   k_radius_argmax            class counts -> pred / correct (when the pass did not vote itself)
//   k_radius_vote              the weighted vote over a CSR segment, in list order
//   k_radius_regress           the weighted mean of the targets over a CSR segment, in list order
//
// D is the value k_direct_tile / k_metric_tile compute, bit for bit: i ascending, IEEE binary32,
// one rounding per operation (no FMA: the file is built with contraction off and no fast-math
// flag), subnormals kept.  Nothing here adds floating-point numbers with atomics: the counts are
// integers, and every floating-point sum runs in one wave in list order.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include "knn_kernels.h"

#include "knn_device.h"

#pragma clang fp contract(off)
#include "knn_radius_dev.h"  // radius_step<M>, load4q
#include "knn_dbscan_dev.h"  // uf_union

// set bits of m below this lane
__device__ __forceinline__ int lanes_below(u64 m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// ---------------------------------------------------------------------------------
// k_radius_tile<M, E, MODE> (RadiusTileArgs; the launcher fills dc / stride / n_qblocks).  A block
// of DT_NW = 8 waves owns 64 queries, 8 per wave (there are no list registers to make room for);
// lane l of every wave computes the distances of train row r0 + l to its wave's 8 queries.
//  * Train tiles, query operands, chunks and the accumulator: as k_metric_tile.
//  * After a tile's last chunk, per query: pass = valid && acc <= thr && row != self (a NaN or
//    inf distance is never <= thr < FLT_MAX), m = ballot(pass), and the query's wave-uniform
//    counter grows by popcount(m).
//  * MODE = RADIUS_COUNT, the count pass: passing lanes add 1 to their label's class count -- in the
//    wave's LDS block [8][Cpad] (classes == 1) or straight in class_counts (classes == 2, integer
//    atomics).  The tile's 64 labels are loaded once per wave, one per lane, and every one is
//    range-checked.  At the end seg_count[seg][q] is written; the LDS counts go to class_counts
//    (stores when nseg == 1, integer atomic adds of the non-zero ones otherwise), and with
//    fuse_vote (nseg == 1, LDS counts) the wave votes: argmax of the counts, ties to the smallest
//    label, outlier when the query has no neighbour.
//  * MODE = RADIUS_FILL, the fill pass: the part of query q's CSR segment that belongs to this train
//    segment starts at base[seg][q] and ends where the next one starts (offsets[q + 1] for the last);
//    a passing lane stores its row (and distance) at base + counter + (passing lanes below it),
//    only inside that part and below offsets[q + 1].  A counter that does not end at the part's
//    length sets KNN_STATUS_BAD_OFFSETS.
//  * MODE = RADIUS_LINK / RADIUS_BORDER, DBSCAN's two passes over the train set against itself
//    (RadiusDbscanArgs; knn_amd.h "DBSCAN").  LINK: a passing pair of core rows with row < query
//    calls uf_union; the scan ends at the block's last query, a block without a core query returns
//    and a wave without one only stages tiles.  BORDER: query q is train row cand[q] (q < *nb; blocks
//    past it return), a passing core row offers its cluster number, each lane keeps its minimum per
//    query, and the wave's minimum goes into out_labels with an integer atomicMin.
// LDS: 2 tile buffers [64][stride] f32 | per-wave class counts [8 waves][8 queries][Cpad] (classes == 1)
// ---------------------------------------------------------------------------------
template <int M, typename E, int MODE>
__global__ __launch_bounds__(64 * DT_NW, 4) void k_radius_tile(RadiusTileArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // (the pass behind k_radius_gemm: only when a norm made the certificate unsafe)
    if (a.gate && !(*a.gate & KNN_STATUS_GEMM_UNSAFE)) return;
    constexpr bool COUNT = MODE == RADIUS_COUNT, FILL = MODE == RADIUS_FILL;
    constexpr bool LINK = MODE == RADIUS_LINK, BORDER = MODE == RADIUS_BORDER;
    constexpr int NT = 64 * DT_NW;
    constexpr int QW = KNN_RADIUS_QW;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile_floats = 64 * a.stride;
    float* bufs = reinterpret_cast<float*>(smem);
    const int Cpad = (a.C + 3) & ~3;
    int* counts = reinterpret_cast<int*>(smem + 2 * (size_t)tile_floats * 4) + wave * QW * Cpad;
    const int qb = blockIdx.x % a.n_qblocks;
    const int seg = blockIdx.x / a.n_qblocks;
    const int64_t row_begin = (int64_t)seg * a.seg_len;
    int64_t row_end = min(a.nt, row_begin + a.seg_len);
    // (BORDER: the candidates, counted on the device; the grid is sized for every row)
    int64_t nq = a.nq;
    if constexpr (BORDER) {
        nq = *a.db.nb;
        if ((int64_t)qb * (DT_NW * QW) >= nq) return;
    }
    // (LINK: D is symmetric, so the pair (q, t) with t < q makes the union: no row past the
    // block's last query is scanned)
    if constexpr (LINK) row_end = min(row_end, min(nq, (int64_t)(qb + 1) * (DT_NW * QW)));
    const E* __restrict__ train = reinterpret_cast<const E*>(a.train);
    const E* __restrict__ test = reinterpret_cast<const E*>(a.test);
    const int d = a.d;
    const float thr = a.thr;
    const bool lds_counts = COUNT && a.classes == 1;

    int64_t qi[QW];
    const E* qrow[QW];
    int64_t self[QW];
    int run[QW];
    int64_t base[QW];
    int room[QW];
    [[maybe_unused]] int64_t qr[QW];        // (BORDER) the candidate's train row
    [[maybe_unused]] uint32_t best[QW];     // (BORDER) this lane's smallest cluster number per query
    [[maybe_unused]] bool wave_any = true;  // (LINK) one of the wave's queries is a core row
    [[maybe_unused]] unsigned long long nun = 0;  // (LINK) successful hooks
    if constexpr (LINK) wave_any = false;
#pragma unroll
    for (int i = 0; i < QW; i++) {
        qi[i] = (int64_t)qb * (DT_NW * QW) + wave * QW + i;
        if constexpr (BORDER) {
            qr[i] = qi[i] < nq ? a.db.cand[qi[i]] : 0;
            best[i] = 0xffffffffu;
            qrow[i] = test + qr[i] * (int64_t)a.ld_q;
        } else {
            qrow[i] = test + (qi[i] < nq ? qi[i] : nq - 1) * (int64_t)a.ld_q;
        }
        // (a query past the end tests against row -2: nothing passes)
        self[i] = qi[i] < nq ? (a.self_base >= 0 ? a.self_base + qi[i] : -1) : -2;
        if constexpr (LINK) {
            // (nor for a query that is no core row)
            if (qi[i] < nq && a.db.dcount[qi[i]] >= a.db.min_samples) wave_any = true;
            else self[i] = -2;
        }
        run[i] = 0;
        base[i] = 0;
        room[i] = 0;
        if constexpr (FILL) {
            if (qi[i] < a.nq) {
                const int64_t end = a.offsets[qi[i] + 1];
                const int64_t next = seg + 1 < a.nseg ? a.base[(int64_t)(seg + 1) * a.nq + qi[i]] : end;
                base[i] = a.base[(int64_t)seg * a.nq + qi[i]];
                const int64_t r = min(next, end) - base[i];
                room[i] = base[i] >= a.offsets[qi[i]] ? (int)max((int64_t)0, min(r, (int64_t)0x7fffffff)) : 0;
            }
        }
    }
    if constexpr (LINK) {
        // a block without a core query has nothing to link; a wave without one only stages tiles
        if (!__syncthreads_or(wave_any ? 1 : 0)) return;
    }
    if (lds_counts)
        for (int c = lane; c < QW * Cpad; c += 64) counts[c] = 0;

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
            // the tile's distances are final: the threshold test
            const int64_t row = row_begin + (s / nchunk) * 64 + lane;
            const bool valid = row < row_end;
            int lab = -1;
            if constexpr (COUNT) {
                if (a.classes && valid) {
                    lab = a.labels[row];
                    if (lab < 0 || lab >= a.C) {
                        atomicOr(a.status, KNN_STATUS_BAD_LABEL);
                        lab = -1;
                    }
                }
            }
            // (LINK) whether this lane's row is a core row; (BORDER) its cluster number, -1 for
            // a row that is none: one word per tile and lane, where COUNT loads its label
            [[maybe_unused]] int tword = -1;
            if constexpr (LINK) tword = valid && a.db.dcount[row] >= a.db.min_samples ? 0 : -1;
            if constexpr (BORDER) tword = valid ? a.db.cluster[row] : -1;
#pragma unroll
            for (int i = 0; i < QW; i++) {
                const bool pass = valid && acc[i] <= thr && row != self[i] && self[i] != -2;
                if constexpr (LINK) {
                    if (pass && tword >= 0 && row < qi[i] &&
                        uf_union(a.db.parent, (int32_t)qi[i], (int32_t)row, a.nt, a.status))
                        nun++;
                } else if constexpr (BORDER) {
                    if (pass && tword >= 0) best[i] = min(best[i], (uint32_t)tword);
                } else {
                    const u64 m = __ballot(pass);
                    if constexpr (FILL) {
                        const int p = run[i] + lanes_below(m);
                        if (pass && p < room[i]) {
                            a.idx[base[i] + p] = (int32_t)row;
                            if (a.dist) a.dist[base[i] + p] = acc[i];
                        }
                    } else {
                        if (pass && lab >= 0) {
                            if (lds_counts) atomicAdd(&counts[i * Cpad + lab], 1);
                            else atomicAdd(&a.class_counts[qi[i] * a.C + lab], 1);
                        }
                    }
                    run[i] += __popcll(m);
                }
                acc[i] = 0.0f;  // every metric restarts from +0
            }
        }
        if (s + 1 < nsteps) store_chunk(s + 1);
        __syncthreads();
    }

    if constexpr (LINK) {
        if (a.db.unions) {  // (profile = 2) one 64-bit add per wave
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) nun += __shfl_xor(nun, o);
            if (lane == 0 && nun) atomicAdd(a.db.unions, nun);
        }
    } else if constexpr (BORDER) {
        // the smallest cluster number among the core neighbours in this train segment; the
        // segments meet in an integer atomicMin (unsigned: -1, "none yet", is the largest value)
#pragma unroll
        for (int i = 0; i < QW; i++) {
            uint32_t b = best[i];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) b = min(b, (uint32_t)__shfl_xor((int)b, o));
            if (lane == 0 && qi[i] < nq && b != 0xffffffffu)
                atomicMin(reinterpret_cast<unsigned int*>(a.db.out_labels) + qr[i], b);
        }
    } else if constexpr (FILL) {
#pragma unroll
        for (int i = 0; i < QW; i++) {
            if (qi[i] >= a.nq) continue;
            const int64_t end = a.offsets[qi[i] + 1];
            const int64_t next = seg + 1 < a.nseg ? a.base[(int64_t)(seg + 1) * a.nq + qi[i]] : end;
            if (lane == 0 && (next - base[i] != (int64_t)run[i] || base[i] < a.offsets[qi[i]] || next > end))
                atomicOr(a.status, KNN_STATUS_BAD_OFFSETS);
        }
    } else {
        int ok = 0;
#pragma unroll
        for (int i = 0; i < QW; i++) {
            if (qi[i] >= a.nq) continue;
            const int64_t q = qi[i];
            if (lane == 0) a.seg_count[(int64_t)seg * a.nq + q] = run[i];
            if (!lds_counts) continue;
            const int* cnt = counts + i * Cpad;
            u64 best = 0;
            for (int c = lane; c < a.C; c += 64) {
                const int v = cnt[c];
                if (a.nseg == 1) {
                    if (a.class_counts) a.class_counts[q * a.C + c] = v;
                } else if (v) {
                    atomicAdd(&a.class_counts[q * a.C + c], v);
                }
                best = umax64(best, ((u64)(uint32_t)v << 32) | (u64)(0xffffffffu - (uint32_t)c));
            }
            if (a.fuse_vote) {
#pragma unroll
                for (int j = 32; j > 0; j >>= 1) best = umax64(best, __shfl_xor(best, j));
                const int32_t p = (best >> 32) ? (int32_t)(0xffffffffu - (uint32_t)(best & 0xffffffffull)) : a.outlier;
                if (lane == 0 && a.pred) a.pred[q] = p;
                if (a.correct && p == a.qlabels[q]) ok++;
            }
        }
        if (a.fuse_vote && a.correct && lane == 0 && ok) atomicAdd(a.correct, (unsigned long long)ok);
    }
}
#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------
// k_radius_scan: one block.  count[q] = the sum over segments of seg_count[s][q] (optional; it may
// be seg_count itself when nseg == 1), offsets[q] = the exclusive int64 scan of the counts,
// offsets[nq] the total (optional).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_radius_scan(const int32_t* __restrict__ seg_count, int nseg, int64_t nq,
                                                      int32_t* count, int64_t* __restrict__ offsets) {
    __shared__ long long wsum[16];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    long long carry = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += 1024) {
        const int64_t q = q0 + threadIdx.x;
        int c = 0;
        if (q < nq) {
            for (int s = 0; s < nseg; s++) c += seg_count[(int64_t)s * nq + q];
            if (count) count[q] = c;
        }
        long long v = c;
#pragma unroll
        for (int j = 1; j < 64; j <<= 1) {
            const long long o = __shfl_up(v, j);
            if (lane >= j) v += o;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        long long pre = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            if (w < wave) pre += wsum[w];
            tot += wsum[w];
        }
        if (offsets && q < nq) offsets[q] = carry + pre + v - c;
        carry += tot;
        __syncthreads();
    }
    if (offsets && threadIdx.x == 0) offsets[nq] = carry;
}

// base[s][q] = offsets[q] + the counts of q's segments below s: a query's segments land in
// ascending train index order
__global__ __launch_bounds__(256) void k_radius_bases(const int32_t* __restrict__ seg_count, int nseg, int64_t nq,
                                                      const int64_t* __restrict__ offsets, int64_t* __restrict__ base) {
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
        int64_t b = offsets[q];
        for (int s = 0; s < nseg; s++) {
            base[(int64_t)s * nq + q] = b;
            b += seg_count[(int64_t)s * nq + q];
        }
    }
}

// pred[q] = the argmax over c of class_counts[q][c], ties to the smallest label; outlier when every
// count is zero.  correct += the queries with pred == qlabels.  One wave per query.
__global__ __launch_bounds__(256) void k_radius_argmax(const int32_t* __restrict__ cc, int64_t nq, int C, int32_t outlier,
                                                       const int32_t* __restrict__ qlabels, int32_t* __restrict__ pred,
                                                       unsigned long long* correct) {
    const int lane = lane_id();
    int ok = 0;
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < nq; q += (int64_t)gridDim.x * 4) {
        u64 best = 0;
        for (int c = lane; c < C; c += 64)
            best = umax64(best, ((u64)(uint32_t)cc[q * C + c] << 32) | (u64)(0xffffffffu - (uint32_t)c));
#pragma unroll
        for (int j = 32; j > 0; j >>= 1) best = umax64(best, __shfl_xor(best, j));
        const int32_t p = (best >> 32) ? (int32_t)(0xffffffffu - (uint32_t)(best & 0xffffffffull)) : outlier;
        if (lane == 0 && pred) pred[q] = p;
        if (correct && p == qlabels[q]) ok++;
    }
    if (correct && lane == 0 && ok) atomicAdd(correct, (unsigned long long)ok);
}

#pragma clang fp contract(off)
// ---------------------------------------------------------------------------------
// k_radius_vote: the weighted vote over CSR segments (RadiusVoteArgs), one wave per query.
//  * Pass 1 over the segment: the checks (an index outside [0, n_train) is not followed, a label
//    outside [0, C), a NaN or negative distance) and, for the weighted kinds, whether any entry
//    has d == 0 (the zero rule: those entries weigh 1 and all others 0).
//  * Pass 2, 64 entries at a time in list order: one round per distinct label of the batch; the
//    round reads S_c from the query's score row, adds the label's weights one after the other in
//    ascending list position (v_readlane hands a weight to the whole wave), and writes S_c back.
//    Lane 0 alone loads and stores the row, so each S_c is one thread's chain of binary32 adds.
//  * The vote: the argmax over c of (bits(S_c), -c); S >= +0, so its bits order like its value.
//    An empty segment gives the outlier label and leaves its score row +0.
// scores [nq][C] is zeroed by the launcher's caller.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_radius_vote(RadiusVoteArgs a) {
    const int lane = lane_id();
    int ok = 0;
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < a.nq; q += (int64_t)gridDim.x * 4) {
        const int64_t o0 = a.offsets[q], o1 = a.offsets[q + 1];
        float* S = a.scores + q * a.C;
        bool bad = false;
        if (o0 < 0 || o1 < o0) {
            if (lane == 0) atomicOr(a.status, KNN_STATUS_BAD_OFFSETS);
            bad = true;
        }
        bool zero_mode = false;
        for (int64_t e0 = o0; !bad && e0 < o1; e0 += 64) {
            const int64_t e = e0 + lane;
            bool z = false;
            if (e < o1) {
                const int32_t t = a.idx[e];
                if (t < 0 || t >= a.n_train) atomicOr(a.status, KNN_STATUS_BAD_INDEX);
                else if (a.labels[t] < 0 || a.labels[t] >= a.C) atomicOr(a.status, KNN_STATUS_BAD_LABEL);
                if (a.dist) {
                    const float dd = a.dist[e];
                    if (!(dd >= 0.0f)) atomicOr(a.status, KNN_STATUS_BAD_DIST);
                    z = dd == 0.0f;
                }
            }
            if (a.weights != KNN_VOTE_W_UNIFORM && __ballot(z)) zero_mode = true;
        }
        for (int64_t e0 = o0; !bad && e0 < o1; e0 += 64) {
            const int64_t e = e0 + lane;
            int lab = -1;
            float w = 0.0f;
            if (e < o1) {
                const int32_t t = a.idx[e];
                if (t >= 0 && t < a.n_train) {
                    const int l = a.labels[t];
                    if (l >= 0 && l < a.C) lab = l;
                }
                w = vote_weight(a.weights, zero_mode, a.dist ? a.dist[e] : 0.0f);
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
        if (o1 > o0 && !bad)
            for (int c = lane; c < a.C; c += 64)
                best = umax64(best, ((u64)__float_as_uint(S[c]) << 32) | (u64)(0xffffffffu - (uint32_t)c));
#pragma unroll
        for (int j = 32; j > 0; j >>= 1) best = umax64(best, __shfl_xor(best, j));
        const int32_t p = (o1 > o0 && !bad) ? (int32_t)(0xffffffffu - (uint32_t)(best & 0xffffffffull)) : a.outlier;
        if (lane == 0 && a.pred) a.pred[q] = p;
        if (a.correct && p == a.qlabels[q]) ok++;
    }
    if (a.correct && lane == 0 && ok) atomicAdd(a.correct, (unsigned long long)ok);
}

// ---------------------------------------------------------------------------------
// k_radius_regress: pred[q] = (float)(N / Dn), N = N + (double)w_j (double)y_j and Dn = Dn +
// (double)w_j in list order (binary64; the product of two widened binary32 values is exact), the
// weights and the zero rule of k_radius_vote.  An empty segment predicts NaN (0.0 / 0.0).
// One wave per query; every lane runs the same chain on broadcast values.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_radius_regress(RadiusVoteArgs a) {
    const int lane = lane_id();
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < a.nq; q += (int64_t)gridDim.x * 4) {
        const int64_t o0 = a.offsets[q], o1 = a.offsets[q + 1];
        bool bad = false;
        if (o0 < 0 || o1 < o0) {
            if (lane == 0) atomicOr(a.status, KNN_STATUS_BAD_OFFSETS);
            bad = true;
        }
        bool zero_mode = false;
        for (int64_t e0 = o0; !bad && e0 < o1; e0 += 64) {
            const int64_t e = e0 + lane;
            bool z = false;
            if (e < o1) {
                const int32_t t = a.idx[e];
                if (t < 0 || t >= a.n_train) atomicOr(a.status, KNN_STATUS_BAD_INDEX);
                if (a.dist) {
                    const float dd = a.dist[e];
                    if (!(dd >= 0.0f)) atomicOr(a.status, KNN_STATUS_BAD_DIST);
                    z = dd == 0.0f;
                }
            }
            if (a.weights != KNN_VOTE_W_UNIFORM && __ballot(z)) zero_mode = true;
        }
        double N = 0.0, Dn = 0.0;
        for (int64_t e0 = o0; !bad && e0 < o1; e0 += 64) {
            const int64_t e = e0 + lane;
            float w = 0.0f, y = 0.0f;
            if (e < o1) {
                const int32_t t = a.idx[e];
                if (t >= 0 && t < a.n_train) y = a.targets[t];
                w = vote_weight(a.weights, zero_mode, a.dist ? a.dist[e] : 0.0f);
            }
            const int n = (int)min((int64_t)64, o1 - e0);
            for (int b = 0; b < n; b++) {
                const double wb = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), b));
                const double yb = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(y), b));
                N = N + wb * yb;
                Dn = Dn + wb;
            }
        }
        if (lane == 0) a.pred_f[q] = (float)(N / Dn);
    }
}
#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------
// Launchers (host side): k_direct_tile's geometry, one kernel per (metric, element type, pass)
// ---------------------------------------------------------------------------------
template <int M, typename E>
static const void* radius_tile_fn(int mode) {
    switch (mode) {
        case RADIUS_COUNT: return reinterpret_cast<const void*>(&k_radius_tile<M, E, RADIUS_COUNT>);
        case RADIUS_FILL: return reinterpret_cast<const void*>(&k_radius_tile<M, E, RADIUS_FILL>);
        case RADIUS_LINK: return reinterpret_cast<const void*>(&k_radius_tile<M, E, RADIUS_LINK>);
        case RADIUS_BORDER: return reinterpret_cast<const void*>(&k_radius_tile<M, E, RADIUS_BORDER>);
        default: return nullptr;
    }
}
// nullptr: no such metric or mode
static const void* radius_tile_ptr(int metric, int elem, int fill) {
    const bool bf = elem == ELEM_BF16;
    switch (metric) {
        case METRIC_SQEUCLIDEAN:
            return bf ? radius_tile_fn<METRIC_SQEUCLIDEAN, bf16_t>(fill) : radius_tile_fn<METRIC_SQEUCLIDEAN, float>(fill);
        case METRIC_MANHATTAN:
            return bf ? radius_tile_fn<METRIC_MANHATTAN, bf16_t>(fill) : radius_tile_fn<METRIC_MANHATTAN, float>(fill);
        case METRIC_CHEBYSHEV:
            return bf ? radius_tile_fn<METRIC_CHEBYSHEV, bf16_t>(fill) : radius_tile_fn<METRIC_CHEBYSHEV, float>(fill);
        default: return nullptr;
    }
}

// the tile buffers, and the per-wave class counts of the count pass where they fit beside them
size_t knn_radius_tile_lds(int d, int C, bool lds_counts) {
    int dc, stride;
    knn_direct_tile_geom(d, &dc, &stride);
    return 2 * 64 * (size_t)stride * 4 + (lds_counts ? (size_t)DT_NW * KNN_RADIUS_QW * ((C + 3) & ~3) * 4 : 0);
}

hipError_t knn_radius_units(int metric, int elem, int d, int C, int* queries_per_unit, int* units_per_cu) {
    const void* fn = radius_tile_ptr(metric, elem, false);
    if (!fn) return hipErrorInvalidValue;
    int occ = 1;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &occ, fn, 64 * DT_NW, knn_radius_tile_lds(d, C, C >= 1 && C <= KNN_RADIUS_LDS_MAX_C));
    *queries_per_unit = DT_NW * KNN_RADIUS_QW;
    *units_per_cu = std::max(occ, 1);
    return e;
}

hipError_t knn_launch_radius_tile(RadiusTileArgs a, int metric, int mode, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    const void* fn = radius_tile_ptr(metric, a.elem, mode);
    if (!fn || a.nseg < 1 || a.d < 1 || !a.status) return hipErrorInvalidValue;
    const bool fill = mode == RADIUS_FILL, count = mode == RADIUS_COUNT;
    if (fill && (!a.base || !a.offsets || !a.idx)) return hipErrorInvalidValue;
    if (count && !a.seg_count) return hipErrorInvalidValue;
    // the DBSCAN modes are self-joins over tables of nt rows
    if (mode == RADIUS_LINK && (a.nq != a.nt || a.test != a.train || !a.db.dcount || !a.db.parent || a.nt > 0x7fffffffLL))
        return hipErrorInvalidValue;
    if (mode == RADIUS_BORDER &&
        (a.nq != a.nt || a.test != a.train || !a.db.cand || !a.db.nb || !a.db.cluster || !a.db.out_labels))
        return hipErrorInvalidValue;
    if (count && a.classes) {
        if (a.C < 1 || !a.labels) return hipErrorInvalidValue;
        a.classes = a.C <= KNN_RADIUS_LDS_MAX_C ? 1 : 2;
        a.fuse_vote = a.classes == 1 && a.nseg == 1;
        // (the pass that does not vote itself adds into class_counts: zeroed by the caller)
        if (!a.fuse_vote && !a.class_counts) return hipErrorInvalidValue;
        if (a.correct && !a.qlabels) return hipErrorInvalidValue;
    } else {
        a.classes = 0;
        a.fuse_vote = 0;
    }
    knn_direct_tile_geom(a.d, &a.dc, &a.stride);
    const int qb = DT_NW * KNN_RADIUS_QW;
    a.n_qblocks = (int)((a.nq + qb - 1) / qb);
    const dim3 grid((unsigned)((int64_t)a.n_qblocks * a.nseg));
    void* args[] = {&a};
    const hipError_t e =
        hipLaunchKernel(fn, grid, dim3(64 * DT_NW), args, knn_radius_tile_lds(a.d, a.C, a.classes == 1), st);
    if (e != hipSuccess) return e;
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

bool knn_radius_pass_votes(int C, int nseg) { return C <= KNN_RADIUS_LDS_MAX_C && nseg == 1; }

hipError_t knn_launch_radius_scan(const int32_t* seg_count, int nseg, int64_t nq, int32_t* count, int64_t* offsets,
                                  hipStream_t st) {
    if (nq < 0 || nseg < 1 || !seg_count) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_radius_scan, dim3(1), dim3(1024), 0, st, seg_count, nseg, nq, count, offsets);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_radius_bases(const int32_t* seg_count, int nseg, int64_t nq, const int64_t* offsets, int64_t* base,
                                   hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_radius_bases, dim3(elementwise_grid(nq)), dim3(256), 0, st, seg_count, nseg, nq, offsets, base);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_radius_argmax(const int32_t* class_counts, int64_t nq, int C, int32_t outlier,
                                    const int32_t* qlabels, int32_t* pred, unsigned long long* correct, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    if (!class_counts || C < 1 || (correct && !qlabels)) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<int64_t>((nq + 3) / 4, 8192);
    hipLaunchKernelGGL(k_radius_argmax, dim3(grid), dim3(256), 0, st, class_counts, nq, C, outlier, qlabels, pred, correct);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_radius_vote(const RadiusVoteArgs& a, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    if (!a.offsets || !a.idx || !a.labels || !a.scores || !a.status || a.C < 1 || a.n_train < 0 ||
        a.weights < KNN_VOTE_W_UNIFORM || a.weights > KNN_VOTE_W_INV_SQDIST ||
        (a.weights != KNN_VOTE_W_UNIFORM && !a.dist) || (a.correct && !a.qlabels))
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<int64_t>((a.nq + 3) / 4, 8192);
    hipLaunchKernelGGL(k_radius_vote, dim3(grid), dim3(256), 0, st, a);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_radius_regress(const RadiusVoteArgs& a, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    if (!a.offsets || !a.idx || !a.targets || !a.pred_f || !a.status || a.n_train < 0 ||
        a.weights < KNN_VOTE_W_UNIFORM || a.weights > KNN_VOTE_W_INV_SQDIST ||
        (a.weights != KNN_VOTE_W_UNIFORM && !a.dist))
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<int64_t>((a.nq + 3) / 4, 8192);
    hipLaunchKernelGGL(k_radius_regress, dim3(grid), dim3(256), 0, st, a);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}
