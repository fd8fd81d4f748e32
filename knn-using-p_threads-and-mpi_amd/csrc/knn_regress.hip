// knn_regress.hip -- k_regress_sweep: the k-NN regression prediction for every prefix of a
// neighbour list, and the per-k error sums against the query targets (gfx950).  The class-vote
// siblings are k_vote_sweep (knn_kernels.hip) and k_vote_weighted (knn_vote_weighted.hip); the
// rules are in include/knn_amd.h ("Regression").
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "knn_kernels.h"

#include "knn_device.h"

// the weights are vote_weight's binary32 values and every sum below is one IEEE binary64
// operation per step: no contraction (the one fused step is written as fma(), on an exact
// product), and the default correctly rounded divisions (no fast-math flag on this file)
#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------
// k_regress_sweep<R>: k_vote_weighted's skeleton -- one wave per query, element e = 64 r + lane
// in register r, the same self-skip and zero rule (list_skip, list_zero_mode: knn_device.h),
// first_missing, check_dist and idx_out / dist_out copy, the [k][query] tile staged in LDS (row
// stride qb + 1) and stored coalesced --
// with the per-class rounds replaced by ONE chain per query:
//   N_k = N_{k-1} + (double)w_j (double)y_j,  D_k = D_{k-1} + (double)w_j,  j = k - 1 ascending.
//  * The list is walked in order; the entry's lane hands (w, y) to the wave (v_readlane: the
//    lane number is the loop counter, a scalar), every lane adds into the same two binary64
//    running sums, and the entry's lane keeps (N, D) as they stand.  The product of two
//    binary32 values is exact in binary64, so fma() rounds once, exactly as multiply-then-add.
//  * After the walk each lane divides its own pair once: pred_k = (float)(N_k / D_k).  A prefix
//    that reaches a missing entry is NaN from there on (KNN_STATUS_TOO_FEW).
//  * A block owns one CHUNK of KNN_REGRESS_CHUNK consecutive queries, in tiles of qb.  The
//    thread owning prefix k adds the chunk's errors e = (double)pred - (double)yq in ascending
//    query order, e * e and |e| in binary64, and stores the two sums to part[m][k][chunk]:
//    the chunks are cut by query number alone, so the partials do not depend on the launch.
//  * row0: only the prefixes k - 1 >= row0 are staged, stored (pred_all points at row row0)
//    and summed; the single-k entry passes row0 = kmax - 1 and a [nq] vector.
// LDS: tile [kmax - row0][qb + 1] f32 | query targets [qb] f32
// ---------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(256) void k_regress_sweep(RegressArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int S = a.qb + 1;
    const int nrows = a.kmax - a.row0;
    float* tile = reinterpret_cast<float*>(smem);
    float* yq = tile + (size_t)nrows * S;
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int64_t chunk = blockIdx.x;
    const int64_t nchunks = gridDim.x;
    double se[4] = {0.0, 0.0, 0.0, 0.0}, sa[4] = {0.0, 0.0, 0.0, 0.0};  // prefix k - 1 = threadIdx.x + 256 i

    for (int t = 0; t < KNN_REGRESS_CHUNK / a.qb; t++) {
        const int64_t q0 = chunk * KNN_REGRESS_CHUNK + (int64_t)t * a.qb;
        if (q0 >= a.nq) break;
        const int nqv = (int)std::min<int64_t>(a.qb, a.nq - q0);
        if (a.qtargets)
            for (int j = threadIdx.x; j < nqv; j += 256) yq[j] = a.qtargets[q0 + j];
        for (int j = wave; j < nqv; j += 4) {
            const int64_t q = q0 + j;
            const int32_t* __restrict__ row = a.idx + q * a.stride;
            const float* __restrict__ drow = a.dist ? a.dist + q * a.stride : nullptr;
            const int skip = list_skip<R>(row, a.kin, a.self_base, q, lane);
            const bool zero_mode = list_zero_mode(a.weights, row, drow, skip);
            float w[R], y[R];
            int first_missing = a.kmax;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int e = 64 * r + lane;
                w[r] = 0.0f;
                y[r] = 0.0f;
                bool miss = false;
                if (e < a.kmax) {
                    const int src = e + (e >= skip ? 1 : 0);
                    const int32_t idx = row[src];
                    const float d = drow ? drow[src] : 0.0f;
                    if (idx >= 0) {
                        if (a.check_dist && !(d >= 0.0f)) atomicOr(a.status, KNN_STATUS_BAD_DIST);
                        w[r] = vote_weight(a.weights, zero_mode, d);
                        y[r] = a.targets[idx];
                    } else {
                        miss = true;
                    }
                    if (a.idx_out) a.idx_out[q * a.kmax + e] = idx;
                    if (a.dist_out) a.dist_out[q * a.kmax + e] = d;
                }
                const u64 mm = __ballot(miss);
                if (mm && first_missing == a.kmax) first_missing = 64 * r + __ffsll(mm) - 1;
            }
            // the one chain: list position by list position, up to the first missing entry
            double N = 0.0, D = 0.0;
            double Nk[R], Dk[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                Nk[r] = 0.0;
                Dk[r] = 0.0;
                const int nb = std::min(64, first_missing - 64 * r);
                for (int b = 0; b < nb; b++) {
                    const double wb = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(w[r]), b));
                    const double yb = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(y[r]), b));
                    N = fma(wb, yb, N);
                    D = D + wb;
                    if (lane == b) {
                        Nk[r] = N;
                        Dk[r] = D;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int e = 64 * r + lane;
                if (e >= a.row0 && e < a.kmax)
                    tile[(e - a.row0) * S + j] = e < first_missing ? (float)(Nk[r] / Dk[r]) : __int_as_float(0x7fc00000);
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
        if (a.part) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int k = threadIdx.x + 256 * i;
                if (k >= a.row0 && k < a.kmax) {
                    for (int jj = 0; jj < nqv; jj++) {
                        const double e = (double)tile[(k - a.row0) * S + jj] - (double)yq[jj];
                        se[i] = se[i] + e * e;
                        sa[i] = sa[i] + fabs(e);
                    }
                }
            }
        }
        __syncthreads();
    }
    if (a.part) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k = threadIdx.x + 256 * i;
            if (k >= a.row0 && k < a.kmax) {
                a.part[(size_t)k * nchunks + chunk] = se[i];
                a.part[((size_t)a.kmax + k) * nchunks + chunk] = sa[i];
            }
        }
    }
}

// ---------------------------------------------------------------------------------
// k_regress_reduce: out[k] += the chunk partials of prefix k, in a fixed order that depends on
// the query numbers alone.  Block (k, m) -- m = 0: sse, 1: sae -- cuts the chunks into spans of
// KNN_REGRESS_SPAN; thread t adds one span's chunks in ascending order, then thread 0 adds the
// span sums to out[k] in ascending order.  No atomics: the same inputs give the same bits, and
// a call that continues on the next KNN_REGRESS_SPAN * KNN_REGRESS_CHUNK queries (a later
// batch, a later pass) continues the same chain.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_regress_reduce(const double* __restrict__ part, int64_t nchunks, int kmax,
                                                        int row0, double* sse, double* sae) {
    __shared__ double span[256];
    const int k = row0 + blockIdx.x, m = blockIdx.y;
    double* out = m ? sae : sse;
    if (!out) return;
    const double* __restrict__ p = part + ((size_t)m * kmax + k) * nchunks;
    const int64_t nspans = (nchunks + KNN_REGRESS_SPAN - 1) / KNN_REGRESS_SPAN;
    double total = threadIdx.x == 0 ? out[k] : 0.0;
    for (int64_t s0 = 0; s0 < nspans; s0 += 256) {
        const int64_t s = s0 + threadIdx.x;
        double acc = 0.0;
        if (s < nspans) {
            const int64_t c1 = std::min<int64_t>((s + 1) * KNN_REGRESS_SPAN, nchunks);
            for (int64_t c = s * KNN_REGRESS_SPAN; c < c1; c++) acc = acc + p[c];
        }
        span[threadIdx.x] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int n = (int)std::min<int64_t>(256, nspans - s0);
            for (int i = 0; i < n; i++) total = total + span[i];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = total;
}

// queries per tile: the chunk, or fewer while the tile would pass about 4096 words
template <int R>
static hipError_t launch_regress_r(const RegressArgs& a0, hipStream_t st) {
    RegressArgs a = a0;
    a.qb = std::min(KNN_REGRESS_CHUNK, std::max(4, 64 / R));
    const int64_t nchunks = knn_regress_chunks(a.nq);
    if (nchunks > 0x7fffffffLL) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * ((size_t)(a.kmax - a.row0) * (a.qb + 1) + a.qb);
    hipLaunchKernelGGL(k_regress_sweep<R>, dim3((unsigned)nchunks), dim3(256), lds, st, a);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_regress(const RegressArgs& a, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    if (a.kin < 1 || a.kin > 1024 || a.kmax < 1 || a.kmax > a.kin || a.stride < a.kin || a.row0 < 0 ||
        a.row0 >= a.kmax || a.weights < KNN_VOTE_W_UNIFORM || a.weights > KNN_VOTE_W_INV_SQDIST ||
        (a.weights != KNN_VOTE_W_UNIFORM && !a.dist) || (a.self_base >= 0 && a.kmax != a.kin - 1) ||
        (a.part && !a.qtargets) || !a.targets)
        return hipErrorInvalidValue;
    const int regs = a.kin <= 64 ? 1 : a.kin <= 128 ? 2 : a.kin <= 256 ? 4 : a.kin <= 512 ? 8 : 16;
    switch (regs) {
        case 1: return launch_regress_r<1>(a, st);
        case 2: return launch_regress_r<2>(a, st);
        case 4: return launch_regress_r<4>(a, st);
        case 8: return launch_regress_r<8>(a, st);
        default: return launch_regress_r<16>(a, st);
    }
}

hipError_t knn_launch_regress_reduce(const double* part, int64_t nq, int kmax, int row0, double* sse, double* sae,
                                     hipStream_t st) {
    if (nq <= 0 || (!sse && !sae)) return hipSuccess;
    if (!part || kmax < 1 || row0 < 0 || row0 >= kmax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_regress_reduce, dim3((unsigned)(kmax - row0), 2), dim3(256), 0, st, part,
                       knn_regress_chunks(nq), kmax, row0, sse, sae);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}
