// knn_lof.hip -- local outlier factor for every k in [k_lo, k_hi] from one set of ordered
// neighbour lists (gfx950): k_lof_compact, k_lof_lrd, k_lof_score.  The rules are in
// include/knn_amd.h ("Local outlier factor"); the other list consumers are k_vote_sweep
// (knn_kernels.hip), k_vote_weighted (knn_vote_weighted.hip) and k_regress_sweep (knn_regress.hip).
// Unlike them a row's score depends on its NEIGHBOURS' lists: two gather rounds over tables the
// size of the lists, so the three kernels run one after the other over all rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "knn_kernels.h"

#include "knn_device.h"

// every value below is one IEEE operation per step: binary32 sqrtf and fmaxf, binary64 sums,
// divisions and the one conversion at the end; no contraction, and the default correctly rounded
// sqrtf and divisions (no fast-math flag on this file)
#pragma clang fp contract(off)

namespace {

constexpr int LOF_WAVES = 4;      // waves per block, one row per wave at a time
constexpr int LOF_INFLIGHT = 4;   // neighbour rows a wave keeps in flight
constexpr int LOF_QB = 16;        // rows per block and LDS tile of k_lof_score

__device__ __forceinline__ float lof_nan32() { return __int_as_float(0x7fc00000); }
__device__ __forceinline__ double lof_nan64() { return __longlong_as_double(0x7ff8000000000000ll); }

// ---------------------------------------------------------------------------------
// k_lof_compact<R>: one wave per row, list element e = 64 r + lane (kin <= 64 R).  Applies
// list_skip once and writes the row's self-removed list cidx / delta [nq][k_hi], delta the
// binary32 distance (sqrtf of the reported squared distance under the Euclidean metric), and kd
// [nq][Kr] = delta at list positions k_lo - 1 .. k_hi - 1.  Every index is checked here, before any
// gather: -1 is a missing entry (cidx -1, delta NaN; KNN_STATUS_TOO_FEW), any other value outside
// [0, n_table) sets KNN_STATUS_BAD_INDEX and is stored as missing, and with check_dist a distance
// that is NaN or negative sets KNN_STATUS_BAD_DIST and is stored as missing too.  The two kernels
// behind it read only cidx: they never see an unchecked index.
// ---------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(64 * LOF_WAVES) void k_lof_compact(LofCompactArgs a) {
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int Kr = a.k_hi - a.k_lo + 1;
    for (int64_t q = (int64_t)blockIdx.x * LOF_WAVES + wave; q < a.nq; q += (int64_t)gridDim.x * LOF_WAVES) {
        const int32_t* __restrict__ row = a.idx + q * a.stride;
        const float* __restrict__ drow = a.dist + q * a.stride;
        const int skip = list_skip<R>(row, a.kin, a.self_base, q, lane);
        int flags = 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int e = 64 * r + lane;
            if (e < a.k_hi) {
                const int src = e + (e >= skip ? 1 : 0);
                const int32_t idx = row[src];
                const float d = drow[src];
                int32_t ci = -1;
                float dl = lof_nan32();
                if (idx == -1) {
                    flags |= KNN_STATUS_TOO_FEW;
                } else if (idx < 0 || (int64_t)idx >= a.n_table) {
                    flags |= KNN_STATUS_BAD_INDEX;
                } else if (a.check_dist && !(d >= 0.0f)) {
                    flags |= KNN_STATUS_BAD_DIST;
                } else {
                    ci = idx;
                    dl = a.euclid ? sqrtf(d) : d;
                }
                a.cidx[q * a.k_hi + e] = ci;
                a.delta[q * a.k_hi + e] = dl;
                if (a.kd && e >= a.k_lo - 1) a.kd[q * Kr + (e - (a.k_lo - 1))] = dl;
            }
        }
        if (flags) atomicOr(a.status, flags);
    }
}

// the row's preloaded list (element e = 64 r + lane) and the number of entries ahead of its first
// missing one
template <int R>
__device__ __forceinline__ int lof_load_row(const LofWalkArgs& a, int64_t q, int lane, int32_t (&ci)[R], float (&dl)[R]) {
    int first_missing = a.k_hi;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int e = 64 * r + lane;
        ci[r] = -1;
        dl[r] = 0.0f;
        if (e < a.k_hi) {
            ci[r] = a.cidx[q * a.k_hi + e];
            dl[r] = a.delta[q * a.k_hi + e];
        }
        const u64 mm = __ballot(e < a.k_hi && ci[r] < 0);
        if (mm && first_missing == a.k_hi) first_missing = 64 * r + __ffsll(mm) - 1;
    }
    return first_missing;
}

// The walk both gather kernels share: list positions j = 0 .. nwalk - 1 in order.  o_j and
// delta(i, o_j) are wave-uniform (v_readlane from the preloaded registers; the lane number is the
// loop counter), the wave loads row o_j of the table [.][Kr] as one coalesced segment per register
// (element e = 64 r + lane), and step(j, delta, row) runs in ascending j.  The loads of
// LOF_INFLIGHT positions are issued before the first of their steps: the kernels are latency-bound
// gathers, and the order of the steps, not of the loads, is the definition.
template <int R, typename T, typename F>
__device__ __forceinline__ void lof_walk(const int32_t (&ci)[R], const float (&dl)[R], int nwalk,
                                         const T* __restrict__ table, int Kr, int lane, F&& step) {
    for (int j0 = 0; j0 < nwalk; j0 += LOF_INFLIGHT) {
        T v[LOF_INFLIGHT][R];
        float dj[LOF_INFLIGHT];
#pragma unroll
        for (int u = 0; u < LOF_INFLIGHT; u++) {
            const int j = j0 + u;
            dj[u] = 0.0f;
#pragma unroll
            for (int r = 0; r < R; r++) v[u][r] = T(0);
            if (j < nwalk) {
                int32_t cs = ci[0];
                float ds = dl[0];
#pragma unroll
                for (int r = 1; r < R; r++)
                    if (r == (j >> 6)) {
                        cs = ci[r];
                        ds = dl[r];
                    }
                const int o = __builtin_amdgcn_readlane(cs, j & 63);
                dj[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ds), j & 63));
                const T* __restrict__ trow = table + (int64_t)o * Kr;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int e = 64 * r + lane;
                    if (e < Kr) v[u][r] = trow[e];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < LOF_INFLIGHT; u++)
            if (j0 + u < nwalk) step(j0 + u, dj[u], v[u]);
    }
}

// ---------------------------------------------------------------------------------
// k_lof_lrd<R>: one wave per row, lane <-> k: element e = 64 r + lane of the range, k = k_lo + e,
// in register r (k_hi <= 64 R bounds both the list and the range).  The walk reads kd[o_j][.];
// lanes whose k > j add (double)fmaxf(kd_k(o_j), delta(i, o_j)) to their binary64 sum, in
// ascending j.  A neighbour whose own list has no k-th entry (kd NaN) makes the sum NaN (fmaxf
// alone would drop it).  lrd_k = 1.0 / (S_k / (double)k + 1e-10); NaN from the row's first missing
// entry on.
// ---------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(64 * LOF_WAVES) void k_lof_lrd(LofWalkArgs a) {
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int Kr = a.k_hi - a.k_lo + 1;
    for (int64_t q = (int64_t)blockIdx.x * LOF_WAVES + wave; q < a.nq; q += (int64_t)gridDim.x * LOF_WAVES) {
        int32_t ci[R];
        float dl[R];
        const int first_missing = lof_load_row<R>(a, q, lane, ci, dl);
        double S[R];
#pragma unroll
        for (int r = 0; r < R; r++) S[r] = 0.0;
        lof_walk<R, float>(ci, dl, first_missing, a.kd_table, Kr, lane, [&](int j, float dj, const float(&v)[R]) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int e = 64 * r + lane;
                float reach = fmaxf(v[r], dj);
                if (v[r] != v[r]) reach = v[r];
                if (e < Kr && j < a.k_lo + e) S[r] = S[r] + (double)reach;
            }
        });
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int e = 64 * r + lane;
            if (e < Kr) {
                const int k = a.k_lo + e;
                a.lrd_out[q * Kr + e] = k <= first_missing ? 1.0 / (S[r] / (double)k + 1e-10) : lof_nan64();
            }
        }
    }
}

// ---------------------------------------------------------------------------------
// k_lof_score<R>: the same walk over lrd[o_j][.] (binary64), L_k = sum of lrd_k(o_j) over j < k in
// ascending j, then LOF_k = (float)(L_k / ((double)k * lrd_k(i))): one rounding to binary32.  A
// block owns LOF_QB consecutive rows; the [k][row] tile is staged in LDS (row stride LOF_QB + 1)
// and stored to lof [Kr][lof_stride] coalesced.  lrd_own is the rows' own lrd [nq][Kr]: the table
// itself when the train rows are scored, the queries' (k_lof_lrd on their lists against the
// fitted kd) for novelty.
// ---------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(64 * LOF_WAVES) void k_lof_score(LofWalkArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* tile = reinterpret_cast<float*>(smem);
    constexpr int S = LOF_QB + 1;
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int Kr = a.k_hi - a.k_lo + 1;
    for (int64_t q0 = (int64_t)blockIdx.x * LOF_QB; q0 < a.nq; q0 += (int64_t)gridDim.x * LOF_QB) {
        const int nqv = (int)std::min<int64_t>(LOF_QB, a.nq - q0);
        for (int jq = wave; jq < nqv; jq += LOF_WAVES) {
            const int64_t q = q0 + jq;
            int32_t ci[R];
            float dl[R];
            const int first_missing = lof_load_row<R>(a, q, lane, ci, dl);
            double L[R];
#pragma unroll
            for (int r = 0; r < R; r++) L[r] = 0.0;
            lof_walk<R, double>(ci, dl, first_missing, a.lrd_table, Kr, lane, [&](int j, float, const double(&v)[R]) {
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int e = 64 * r + lane;
                    if (e < Kr && j < a.k_lo + e) L[r] = L[r] + v[r];
                }
            });
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int e = 64 * r + lane;
                if (e < Kr) {
                    const int k = a.k_lo + e;
                    const double own = a.lrd_own[q * Kr + e];
                    tile[e * S + jq] = k <= first_missing ? (float)(L[r] / ((double)k * own)) : lof_nan32();
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < Kr * nqv; i += 64 * LOF_WAVES) {
            const int k = i / nqv, jj = i - k * nqv;
            a.lof[(int64_t)k * a.lof_stride + q0 + jj] = tile[k * S + jj];
        }
        __syncthreads();
    }
}

unsigned lof_grid(int64_t nq, int rows_per_block) {
    return (unsigned)std::min<int64_t>((nq + rows_per_block - 1) / rows_per_block, (int64_t)1 << 20);
}

bool lof_range_ok(int k_lo, int k_hi) { return k_lo >= 1 && k_lo <= k_hi && k_hi <= KNN_LOF_MAX_K; }

}  // namespace

hipError_t knn_launch_lof_compact(const LofCompactArgs& a, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    const int kin_want = a.k_hi + (a.self_base >= 0 ? 1 : 0);
    if (!lof_range_ok(a.k_lo, a.k_hi) || a.kin != kin_want || a.stride < a.kin || a.n_table < 0 || !a.idx || !a.dist ||
        !a.cidx || !a.delta || !a.status)
        return hipErrorInvalidValue;
    const dim3 grid(lof_grid(a.nq, LOF_WAVES)), block(64 * LOF_WAVES);
    switch (knn_list_regs(a.kin)) {
        case 1: hipLaunchKernelGGL(k_lof_compact<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(k_lof_compact<2>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(k_lof_compact<4>, grid, block, 0, st, a); break;
    }
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_lof_lrd(const LofWalkArgs& a, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    if (!lof_range_ok(a.k_lo, a.k_hi) || !a.cidx || !a.delta || !a.kd_table || !a.lrd_out) return hipErrorInvalidValue;
    const dim3 grid(lof_grid(a.nq, LOF_WAVES)), block(64 * LOF_WAVES);
    switch (knn_list_regs(a.k_hi)) {
        case 1: hipLaunchKernelGGL(k_lof_lrd<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(k_lof_lrd<2>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(k_lof_lrd<4>, grid, block, 0, st, a); break;
    }
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_lof_score(const LofWalkArgs& a, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    if (!lof_range_ok(a.k_lo, a.k_hi) || !a.cidx || !a.delta || !a.lrd_table || !a.lrd_own || !a.lof ||
        a.lof_stride < a.nq)
        return hipErrorInvalidValue;
    const dim3 grid(lof_grid(a.nq, LOF_QB)), block(64 * LOF_WAVES);
    const size_t lds = sizeof(float) * (size_t)(a.k_hi - a.k_lo + 1) * (LOF_QB + 1);
    switch (knn_list_regs(a.k_hi)) {
        case 1: hipLaunchKernelGGL(k_lof_score<1>, grid, block, lds, st, a); break;
        case 2: hipLaunchKernelGGL(k_lof_score<2>, grid, block, lds, st, a); break;
        default: hipLaunchKernelGGL(k_lof_score<4>, grid, block, lds, st, a); break;
    }
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}
