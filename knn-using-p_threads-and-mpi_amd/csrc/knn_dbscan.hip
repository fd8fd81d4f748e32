// knn_dbscan.hip -- DBSCAN's small kernels (gfx950; the rules are in include/knn_amd.h "DBSCAN",
// the argument in DESIGN.md "DBSCAN").  The distance work is k_radius_tile's and k_radius_gemm's
// RADIUS_LINK / RADIUS_BORDER modes; here are the steps around them, all integer:
//
//   k_dbscan_init           parent[i] = i
//   k_dbscan_flatten        root[i] = find(i) for a core row, isroot[i]
//   (k_radius_scan)         the exclusive scan of isroot: a root's cluster number
//   k_dbscan_labels         labels / cluster: a core row's cluster number, -1 for every other row
//   k_dbscan_candidates     the rows that may be border rows: !core && count >= 2
//   k_dbscan_summary        {clusters, core, border, noise}
//
// and the same clustering on CSR lists a caller holds (knn_dbscan_lists_device):
//
//   k_dbscan_lists_count    count[i] = offsets[i + 1] - offsets[i]
//   k_dbscan_lists_link     one wave per row: every index checked, a core row unions with its core entries
//   k_dbscan_lists_border   one wave per candidate: the smallest cluster number among its core entries
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "knn_kernels.h"

#include "knn_device.h"
#include "knn_dbscan_dev.h"

namespace {

constexpr int DB_WAVES = 4;  // waves per block of the wave-per-row kernels

__global__ __launch_bounds__(256) void k_dbscan_init(int32_t* __restrict__ parent, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) parent[i] = (int32_t)i;
}

// The link pass is over: every root is its component's smallest row.  A walk takes at most n
// steps (each moves to a smaller index).
__global__ __launch_bounds__(256) void k_dbscan_flatten(int32_t* parent, const int32_t* __restrict__ count,
                                                        int32_t min_samples, int64_t n, int32_t* __restrict__ root,
                                                        int32_t* __restrict__ isroot, int32_t* status) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int32_t r = -1;
        if (count[i] >= min_samples) {
            int64_t budget = n + 8;
            r = uf_find(parent, (int32_t)i, budget);
            if (r < 0) atomicOr(status, KNN_STATUS_UF_LIMIT);
        }
        root[i] = r;
        isroot[i] = r == (int32_t)i ? 1 : 0;
    }
}

// offsets: the exclusive scan of isroot, so offsets[r] is the number of roots below root r -- the
// clusters in ascending order of their smallest row
__global__ __launch_bounds__(256) void k_dbscan_labels(const int32_t* __restrict__ root, const int64_t* __restrict__ offsets,
                                                       int64_t n, int32_t* __restrict__ labels,
                                                       int32_t* __restrict__ cluster) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t r = root[i];
        const int32_t v = r >= 0 ? (int32_t)offsets[r] : -1;
        labels[i] = v;
        cluster[i] = v;
    }
}

// cand[0 .. *nb): the rows that are no core rows but have a neighbour besides themselves, in no
// particular order (each writes its own label, so the order changes no output).  One atomic add
// per wave.
__global__ __launch_bounds__(256) void k_dbscan_candidates(const int32_t* __restrict__ count, int32_t min_samples,
                                                           int64_t n, int32_t* __restrict__ cand, int32_t* nb) {
    const int lane = lane_id();
    const int64_t n64 = (n + 63) & ~(int64_t)63;  // whole waves stay in the loop: the ballot is wave-wide
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n64; i += (int64_t)gridDim.x * 256) {
        const bool is = i < n && count[i] < min_samples && count[i] >= 2;
        const u64 m = __ballot(is);
        if (!m) continue;
        int base = 0;
        if (lane == 0) base = atomicAdd(nb, (int32_t)__popcll(m));
        base = __builtin_amdgcn_readfirstlane(base);
        if (is) cand[base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)i;
    }
}

// info: [0] clusters, [1] core rows, [2] border rows, [3] noise rows (zeroed by the caller)
__global__ __launch_bounds__(256) void k_dbscan_summary(const int32_t* __restrict__ labels, const int32_t* __restrict__ count,
                                                        int32_t min_samples, const int64_t* __restrict__ offsets, int64_t n,
                                                        unsigned long long* info) {
    const int lane = lane_id();
    unsigned long long core = 0, border = 0, noise = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (count[i] >= min_samples) core++;
        else if (labels[i] >= 0) border++;
        else noise++;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        core += __shfl_xor(core, o);
        border += __shfl_xor(border, o);
        noise += __shfl_xor(noise, o);
    }
    if (lane == 0) {
        if (core) atomicAdd(info + 1, core);
        if (border) atomicAdd(info + 2, border);
        if (noise) atomicAdd(info + 3, noise);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) info[0] = (unsigned long long)offsets[n];
}

__global__ __launch_bounds__(256) void k_dbscan_lists_count(const int64_t* __restrict__ offsets, int64_t n,
                                                            int32_t* __restrict__ count, int32_t* status) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t o0 = offsets[i], o1 = offsets[i + 1];
        int64_t c = o1 - o0;
        if (o0 < 0 || c < 0) {
            atomicOr(status, KNN_STATUS_BAD_OFFSETS);
            c = 0;
        }
        count[i] = (int32_t)std::min<int64_t>(c, 0x7fffffff);
    }
}

// One wave per row walks the row's segment.  Every index is checked against [0, n) before any
// table is read with it; a core row unions with each of its core entries.
__global__ __launch_bounds__(64 * DB_WAVES) void k_dbscan_lists_link(const int64_t* __restrict__ offsets,
                                                                      const int32_t* __restrict__ idx, int64_t n,
                                                                      const int32_t* __restrict__ count,
                                                                      int32_t min_samples, int32_t* parent, int32_t* status,
                                                                      unsigned long long* unions) {
    const int lane = lane_id();
    unsigned long long nun = 0;
    for (int64_t q = (int64_t)blockIdx.x * DB_WAVES + (threadIdx.x >> 6); q < n; q += (int64_t)gridDim.x * DB_WAVES) {
        const int64_t o0 = offsets[q];
        const int64_t o1 = o0 + count[q];  // (count is 0 for offsets that are not in order)
        const bool qcore = count[q] >= min_samples;
        for (int64_t e = o0 + lane; e < o1; e += 64) {
            const int32_t t = idx[e];
            if (t < 0 || (int64_t)t >= n) {
                atomicOr(status, KNN_STATUS_BAD_INDEX);
            } else if (qcore && t != (int32_t)q && count[t] >= min_samples) {
                if (uf_union(parent, (int32_t)q, t, n, status)) nun++;
            }
        }
    }
    if (unions) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nun += __shfl_xor(nun, o);
        if (lane == 0 && nun) atomicAdd(unions, nun);
    }
}

// One wave per candidate (cand[0 .. *nb)); the link kernel has checked every index.
__global__ __launch_bounds__(64 * DB_WAVES) void k_dbscan_lists_border(const int64_t* __restrict__ offsets,
                                                                        const int32_t* __restrict__ idx, int64_t n,
                                                                        const int32_t* __restrict__ count,
                                                                        const int32_t* __restrict__ cand, const int32_t* nb,
                                                                        const int32_t* __restrict__ cluster,
                                                                        int32_t* __restrict__ labels) {
    const int lane = lane_id();
    const int64_t m = *nb;
    for (int64_t c = (int64_t)blockIdx.x * DB_WAVES + (threadIdx.x >> 6); c < m; c += (int64_t)gridDim.x * DB_WAVES) {
        const int32_t q = cand[c];
        const int64_t o0 = offsets[q];
        const int64_t o1 = o0 + count[q];
        uint32_t best = 0xffffffffu;
        for (int64_t e = o0 + lane; e < o1; e += 64) {
            const int32_t t = idx[e];
            if (t >= 0 && (int64_t)t < n) best = min(best, (uint32_t)cluster[t]);  // (-1: the largest value)
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, o));
        if (lane == 0) labels[q] = (int32_t)best;
    }
}

unsigned rows_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + DB_WAVES - 1) / DB_WAVES, 8192)); }

}  // namespace

// ---------------------------------------------------------------------------------
// Launchers (host side)
// ---------------------------------------------------------------------------------
hipError_t knn_launch_dbscan_init(int32_t* parent, int64_t n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!parent || n > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dbscan_init, dim3(elementwise_grid(n)), dim3(256), 0, st, parent, n);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_dbscan_flatten(int32_t* parent, const int32_t* count, int32_t min_samples, int64_t n, int32_t* root,
                                     int32_t* isroot, int32_t* status, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!parent || !count || !root || !isroot || !status) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dbscan_flatten, dim3(elementwise_grid(n)), dim3(256), 0, st, parent, count, min_samples, n, root,
                       isroot, status);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_dbscan_labels(const int32_t* root, const int64_t* offsets, int64_t n, int32_t* labels,
                                    int32_t* cluster, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!root || !offsets || !labels || !cluster) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dbscan_labels, dim3(elementwise_grid(n)), dim3(256), 0, st, root, offsets, n, labels, cluster);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_dbscan_candidates(const int32_t* count, int32_t min_samples, int64_t n, int32_t* cand, int32_t* nb,
                                        hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!count || !cand || !nb) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dbscan_candidates, dim3(elementwise_grid(n)), dim3(256), 0, st, count, min_samples, n, cand, nb);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_dbscan_summary(const int32_t* labels, const int32_t* count, int32_t min_samples,
                                     const int64_t* offsets, int64_t n, int64_t* info, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!labels || !count || !offsets || !info) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dbscan_summary, dim3(elementwise_grid(n)), dim3(256), 0, st, labels, count, min_samples, offsets, n,
                       reinterpret_cast<unsigned long long*>(info));
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_dbscan_lists_count(const int64_t* offsets, int64_t n, int32_t* count, int32_t* status,
                                         hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!offsets || !count || !status) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dbscan_lists_count, dim3(elementwise_grid(n)), dim3(256), 0, st, offsets, n, count, status);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_dbscan_lists_link(const int64_t* offsets, const int32_t* idx, int64_t n, const int32_t* count,
                                        int32_t min_samples, int32_t* parent, int32_t* status, unsigned long long* unions,
                                        hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!offsets || !idx || !count || !parent || !status || n > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dbscan_lists_link, dim3(rows_grid(n)), dim3(64 * DB_WAVES), 0, st, offsets, idx, n, count,
                       min_samples, parent, status, unions);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_dbscan_lists_border(const int64_t* offsets, const int32_t* idx, int64_t n, const int32_t* count,
                                          const int32_t* cand, const int32_t* nb, const int32_t* cluster, int32_t* labels,
                                          hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!offsets || !idx || !count || !cand || !nb || !cluster || !labels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dbscan_lists_border, dim3(rows_grid(n)), dim3(64 * DB_WAVES), 0, st, offsets, idx, n, count, cand,
                       nb, cluster, labels);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}
