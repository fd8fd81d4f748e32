// knn_vote_weighted.hip -- k_vote_weighted: the distance-weighted vote, and the per-class
// scores, for every prefix of a neighbour list (gfx950).  The uniform-vote sibling is
// k_vote_sweep (knn_kernels.hip); the rules are in include/knn_amd.h ("Weighted vote").
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "knn_kernels.h"

#include "knn_device.h"

// every weight and every sum below is one IEEE binary32 operation: no contraction, and the
// default correctly rounded 1.0f / x and sqrtf (no fast-math flag on this file)
// (the weight itself is vote_weight, knn_device.h: k_regress_sweep uses the same values)
#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------
// k_vote_weighted<R>: k_vote_sweep's skeleton -- one wave per query, element e = 64 r + lane
// in register r, labels read as labels[idx], the same self-skip (list_skip), the [k][query] tile staged
// in LDS (row stride qb + 1) and stored coalesced, correct[k - 1] counted per thread -- with
// the popcount of a label's occurrences replaced by the score the rules define:
//   S_c(k) = the fp32 sum of w_j over j < k with label_j == c, added in ascending j.
//  * w_j: 1 (uniform), 1 / sqrtf(d_j), or 1 / d_j.  When the first entry left after
//    self-removal has d == 0 (sklearn's rule) a weighted kind gives 1 to every d == 0 entry
//    and 0 to the rest.
//  * One round per DISTINCT label, as in k_vote_sweep.  The round's chain is sequential: the
//    set bits of the label's occurrence masks are walked in list order, the bit's lane hands
//    its weight to the whole wave (v_readlane: the lane number is a scalar), every lane adds
//    it to the same running sum, and the occurrence's lane keeps the sum so far.  The walks
//    of all rounds together are kmax adds per query; the chains of different labels are
//    independent, and so are the queries of the four waves.
//  * The prediction for k is the label in the maximum over j < k of the key
//    (bits(S_j) << 32) | (0xffffffff - label_j), an inclusive prefix-max scan.  S >= +0, so
//    its bits order like its value (inf included); a label's sums never decrease along the
//    list, so its last occurrence inside a prefix carries its score there and its earlier
//    ones carry no more: the maximum over elements is the maximum over labels of
//    (score, -label).  A top score of +0 (every weight 0) ties with every absent class: 0.
//  * scores [nq][C] (optional, zeroed by the launcher's caller): the round's final sum is
//    S_c(kmax); lane 0 stores it.  A query whose list reaches a missing entry keeps its zeros.
//  * row0: only the prefixes k - 1 >= row0 are staged, stored (pred_all points at row row0)
//    and counted; the single-k predict entry passes row0 = kmax - 1 and a [nq] vector.
//  * check_dist (lists the caller supplies): a non-missing entry whose distance is NaN or
//    negative sets KNN_STATUS_BAD_DIST.
// LDS: tile [kmax - row0][qb + 1] i32 | query labels [qb] i32
// ---------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(256) void k_vote_weighted(VoteWeightedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int S = a.qb + 1;
    const int nrows = a.kmax - a.row0;
    int32_t* tile = reinterpret_cast<int32_t*>(smem);
    int32_t* ql = tile + (size_t)nrows * S;
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int64_t ntiles = (a.nq + a.qb - 1) / a.qb;
    unsigned long long ok[4] = {0, 0, 0, 0};  // prefix k - 1 = threadIdx.x + 256 i

    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t q0 = t * a.qb;
        const int nqv = (int)std::min<int64_t>(a.qb, a.nq - q0);
        if (a.qlabels)
            for (int j = threadIdx.x; j < nqv; j += 256) ql[j] = a.qlabels[q0 + j];
        for (int j = wave; j < nqv; j += 4) {
            const int64_t q = q0 + j;
            const int32_t* __restrict__ row = a.idx + q * a.stride;
            const float* __restrict__ drow = a.dist ? a.dist + q * a.stride : nullptr;
            const int skip = list_skip<R>(row, a.kin, a.self_base, q, lane);
            const bool zero_mode = list_zero_mode(a.weights, row, drow, skip);
            int lab[R];
            float w[R];
            int first_missing = a.kmax;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int e = 64 * r + lane;
                lab[r] = -1;
                w[r] = 0.0f;
                bool miss = false;
                if (e < a.kmax) {
                    const int src = e + (e >= skip ? 1 : 0);
                    const int32_t idx = row[src];
                    const float d = drow ? drow[src] : 0.0f;
                    if (idx >= 0) {
                        const int l = a.labels[idx];
                        if (l >= 0 && l < a.C) lab[r] = l;
                        else atomicOr(a.status, KNN_STATUS_BAD_LABEL);
                        if (a.check_dist && !(d >= 0.0f)) atomicOr(a.status, KNN_STATUS_BAD_DIST);
                        w[r] = vote_weight(a.weights, zero_mode, d);
                    } else {
                        miss = true;
                    }
                    if (a.idx_out) a.idx_out[q * a.kmax + e] = idx;
                    if (a.dist_out) a.dist_out[q * a.kmax + e] = d;
                }
                const u64 mm = __ballot(miss);
                if (mm && first_missing == a.kmax) first_missing = 64 * r + __ffsll(mm) - 1;
            }
            // running sums, one round per distinct label
            float sum[R];
            u64 pend[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                sum[r] = 0.0f;
                pend[r] = __ballot(lab[r] >= 0);
            }
            for (;;) {
                int re = -1;
                u64 pm = 0;
#pragma unroll
                for (int r = R - 1; r >= 0; r--)
                    if (pend[r]) { re = r; pm = pend[r]; }
                if (re < 0) break;
                int le = lab[0];
#pragma unroll
                for (int r = 1; r < R; r++)
                    if (r == re) le = lab[r];
                le = __builtin_amdgcn_readlane(le, __ffsll(pm) - 1);
                float run = 0.0f;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    u64 m = __ballot(lab[r] == le);
                    pend[r] &= ~m;
                    while (m) {
                        const int b = __ffsll(m) - 1;
                        m &= m - 1;
                        run = run + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w[r]), b));
                        if (lane == b) sum[r] = run;
                    }
                }
                if (a.scores && first_missing >= a.kmax && lane == 0) a.scores[q * a.C + le] = run;
            }
            // prefix max of the keys, carried from register to register
            u64 carry = 0;
#pragma unroll
            for (int r = 0; r < R; r++) {
                u64 key = lab[r] >= 0 ? ((u64)__float_as_uint(sum[r]) << 32) | (u64)(0xffffffffu - (uint32_t)lab[r]) : 0;
#pragma unroll
                for (int s = 1; s < 64; s <<= 1) {
                    const u64 o = __shfl_up(key, s);
                    if (lane >= s) key = umax64(key, o);
                }
                key = umax64(key, carry);
                carry = __shfl(key, 63);
                const int e = 64 * r + lane;
                if (e >= a.row0 && e < a.kmax)
                    tile[(e - a.row0) * S + j] =
                        (e < first_missing && (key >> 32)) ? (int32_t)(0xffffffffu - (uint32_t)(key & 0xffffffffull)) : 0;
            }
            if (lane == 0 && first_missing < a.kmax) atomicOr(a.status, KNN_STATUS_TOO_FEW);
        }
        __syncthreads();
        if (a.pred_all) {
            for (int i = threadIdx.x; i < nrows * nqv; i += 256) {
                const int k = i / nqv, jj = i - k * nqv;
                a.pred_all[(int64_t)k * a.pred_stride + q0 + jj] = tile[k * S + jj];
            }
        }
        if (a.correct) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int k = threadIdx.x + 256 * i;
                if (k >= a.row0 && k < a.kmax) {
                    int c = 0;
                    for (int jj = 0; jj < nqv; jj++) c += tile[(k - a.row0) * S + jj] == ql[jj];
                    ok[i] += (unsigned long long)c;
                }
            }
        }
        __syncthreads();
    }
    if (a.correct) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k = threadIdx.x + 256 * i;
            if (k >= a.row0 && k < a.kmax && ok[i]) atomicAdd(&a.correct[k], ok[i]);
        }
    }
}

// queries per tile as launch_vote_sweep_r: about 4096 tile words, halved while the tiles would
// not give every CU a block or two
template <int R>
static hipError_t launch_vote_weighted_r(const VoteWeightedArgs& a0, hipStream_t st) {
    VoteWeightedArgs a = a0;
    a.qb = std::max(4, 64 / R);
    while (a.qb > 4 && (a.nq + a.qb - 1) / a.qb < 512) a.qb >>= 1;
    const int64_t ntiles = (a.nq + a.qb - 1) / a.qb;
    const size_t lds = sizeof(int32_t) * ((size_t)(a.kmax - a.row0) * (a.qb + 1) + a.qb);
    hipLaunchKernelGGL(k_vote_weighted<R>, dim3((unsigned)std::min<int64_t>(ntiles, 4096)), dim3(256), lds, st, a);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_vote_weighted(const VoteWeightedArgs& a, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    if (a.kin < 1 || a.kin > 1024 || a.kmax < 1 || a.kmax > a.kin || a.stride < a.kin || a.row0 < 0 ||
        a.row0 >= a.kmax || a.weights < KNN_VOTE_W_UNIFORM || a.weights > KNN_VOTE_W_INV_SQDIST ||
        (a.weights != KNN_VOTE_W_UNIFORM && !a.dist) || (a.self_base >= 0 && a.kmax != a.kin - 1))
        return hipErrorInvalidValue;
    const int regs = a.kin <= 64 ? 1 : a.kin <= 128 ? 2 : a.kin <= 256 ? 4 : a.kin <= 512 ? 8 : 16;
    switch (regs) {
        case 1: return launch_vote_weighted_r<1>(a, st);
        case 2: return launch_vote_weighted_r<2>(a, st);
        case 4: return launch_vote_weighted_r<4>(a, st);
        case 8: return launch_vote_weighted_r<8>(a, st);
        default: return launch_vote_weighted_r<16>(a, st);
    }
}
