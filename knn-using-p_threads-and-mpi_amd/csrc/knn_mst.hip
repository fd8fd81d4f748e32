// knn_mst.hip -- the minimum spanning tree of the mutual-reachability graph and its cut (gfx950; the
// rules are in include/knn_amd.h "Spanning tree", the argument in DESIGN.md "Spanning tree").
// Boruvka rounds over the train set against itself, every reduction an integer minimum:
//
//   k_mst_core          c(i) and dlast(i) from the rows' top-K lists; parent[i] = comp[i] = i
//   k_mst_resolve       per round: a row's smallest key among its LISTED rows of other components;
//                       the rows the list cannot decide are compacted into cand
//   k_mst_tile<M, E>    the distance pass over the candidates: k_radius_tile's skeleton
//                       (knn_radius.hip) with `D <= thr` replaced by the minimum key per query
//   k_mst_pick_lo / _hi the component's smallest edge under (w, lo, hi), two integer atomicMin steps
//   k_mst_hook          one union per component root; the call that hooked appends the edge
//   k_mst_flatten       comp[i] = find(i)
//   k_mst_unpack        the sorted records (rocPRIM's radix sort, stable: on (a, b), then on bits(w))
//                       -> w / a / b
//   k_mst_cut_link / _roots / _labels   the cut: one union-find carried over the levels
//
// D is k_radius_tile's, bit for bit (the same steps, the same flags); w = fmaxf(fmaxf(c, c), D) is
// exact.  Nothing here adds floating-point numbers with atomics.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "knn_kernels.h"

#include "knn_device.h"

#pragma clang fp contract(off)
#include "knn_radius_dev.h"  // radius_step<M>, load4q
#include "knn_dbscan_dev.h"  // uf_find, uf_union

namespace {

constexpr u64 MST_NONE = ~0ull;
constexpr int MST_SUB = 16;  // lanes per row of the list walk

__device__ __forceinline__ u64 mst_key(float w, uint32_t t) { return ((u64)__float_as_uint(w) << 32) | (u64)t; }
__device__ __forceinline__ int mst_lanes_below(u64 m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// a list entry that names a row: the missing marker is -1, and a distance a pass reports is < FLT_MAX
__device__ __forceinline__ bool mst_entry(int32_t t, float dd, int64_t n) {
    return t >= 0 && (int64_t)t < n && dd < FLT_MAX;
}

__global__ __launch_bounds__(256) void k_mst_core(MstTables t, int64_t n, int32_t min_samples, float* core_out) {
    const int K = t.K;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t* ix = t.idx + i * K;
        const float* ds = t.dist + i * K;
        int v = 0;
        for (int j = 0; j < K; j++) v += mst_entry(ix[j], ds[j], n) ? 1 : 0;
        const int m = min_samples - 1;
        const float c = m < K && mst_entry(ix[m], ds[m], n) ? ds[m] : __builtin_inff();
        t.core[i] = c;
        if (core_out) core_out[i] = c;
        t.dlast[i] = (v < K || (int64_t)K >= n) ? __builtin_inff() : ds[K - 1];
        t.parent[i] = (int32_t)i;
        t.comp[i] = (int32_t)i;
    }
}

// MST_SUB lanes walk one row's list; the group's first lane decides.  A row is resolved when its
// list holds every candidate it has (dlast = +inf) or a listed candidate has w < dlast STRICTLY: an
// unlisted row has D >= dlast, so w >= dlast, and only the strict test excludes a tie that the
// (w, t) order could give to an unlisted row of smaller index.
__global__ __launch_bounds__(256) void k_mst_resolve(MstTables t, int64_t n, int use_lists) {
    const int lane = lane_id(), sub = lane & (MST_SUB - 1);
    constexpr int RPB = 256 / MST_SUB;  // rows per block and step
    const int64_t nr = (n + RPB - 1) / RPB * RPB;  // whole waves stay in the loop: the ballot is wave-wide
    for (int64_t i = (int64_t)blockIdx.x * RPB + threadIdx.x / MST_SUB; i < nr; i += (int64_t)gridDim.x * RPB) {
        const bool row = i < n;
        u64 best = MST_NONE;
        bool unresolved = row;
        if (use_lists) {
            float ci = 0.0f, dl = 0.0f;
            int32_t mine = -1;
            if (row) {
                ci = t.core[i];
                dl = t.dlast[i];
                mine = t.comp[i];
                for (int j = sub; j < t.K; j += MST_SUB) {
                    const int32_t r = t.idx[i * t.K + j];
                    const float dd = t.dist[i * t.K + j];
                    if (!mst_entry(r, dd, n) || t.comp[r] == mine) continue;
                    best = umin64(best, mst_key(__builtin_fmaxf(__builtin_fmaxf(ci, t.core[r]), dd), (uint32_t)r));
                }
            }
#pragma unroll
            for (int o = MST_SUB / 2; o > 0; o >>= 1) best = umin64(best, __shfl_xor(best, o));
            const bool complete = dl == __builtin_inff();
            const bool resolved = complete || (best != MST_NONE && __uint_as_float((uint32_t)(best >> 32)) < dl);
            unresolved = row && !resolved;
            if (row && resolved && sub == 0 && best != MST_NONE) t.rowbest[i] = best;
        }
        const u64 m = __ballot(unresolved && sub == 0);
        if (!m) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(t.cnt + MST_CNT_NB, (unsigned long long)__popcll(m));
        base = __shfl(base, 0);
        if (unresolved && sub == 0) t.cand[base + mst_lanes_below(m)] = (int32_t)i;
    }
}

// ---------------------------------------------------------------------------------
// k_mst_tile<M, E>: k_radius_tile's block (8 waves, 8 queries a wave, lane l of every wave against
// train row r0 + l), tiles, chunks and accumulator.  Query q is train row cand[q], q < cnt[NB]
// (counted on the device; blocks past it return).  Per tile and lane one load each of comp[row] and
// core[row]; after the tile's last chunk ok = valid && D < FLT_MAX && comp[row] != comp[q], and the
// lane keeps its smallest key per query.  At the end a wave minimum by shuffles and one 64-bit
// integer atomicMin into rowbest[q], where the train segments meet.
// LDS: 2 tile buffers [64][stride] f32
// ---------------------------------------------------------------------------------
template <int M, typename E>
__global__ __launch_bounds__(64 * DT_NW, 4) void k_mst_tile(RadiusTileArgs a, MstTables mt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
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
    const int64_t nq = min((int64_t)mt.cnt[MST_CNT_NB], a.nt);
    if ((int64_t)qb * (DT_NW * QW) >= nq) return;
    const E* __restrict__ train = reinterpret_cast<const E*>(a.train);
    const int d = a.d;

    int64_t qi[QW];
    const E* qrow[QW];
    int32_t qr[QW], qcomp[QW];
    float qcore[QW];
    u64 best[QW];
#pragma unroll
    for (int i = 0; i < QW; i++) {
        qi[i] = (int64_t)qb * (DT_NW * QW) + wave * QW + i;
        int32_t r = qi[i] < nq ? mt.cand[qi[i]] : 0;
        if (r < 0 || (int64_t)r >= a.nt) r = 0;  // (cand is this library's own; never followed out of range)
        qr[i] = r;
        qrow[i] = train + (int64_t)r * a.ld_t;
        qcomp[i] = mt.comp[r];
        qcore[i] = mt.core[r];
        best[i] = MST_NONE;
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
            // the tile's distances are final: one component and one core distance per lane
            const int64_t row = row_begin + (s / nchunk) * 64 + lane;
            const bool valid = row < row_end;
            int32_t tcomp = -1;
            float tcore = 0.0f;
            if (valid) {
                tcomp = mt.comp[row];
                tcore = mt.core[row];
            }
#pragma unroll
            for (int i = 0; i < QW; i++) {
                const bool ok = valid && acc[i] < FLT_MAX && tcomp != qcomp[i];
                if (ok)
                    best[i] = umin64(best[i], mst_key(__builtin_fmaxf(__builtin_fmaxf(qcore[i], tcore), acc[i]), (uint32_t)row));
                acc[i] = 0.0f;  // every metric restarts from +0
            }
        }
        if (s + 1 < nsteps) store_chunk(s + 1);
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < QW; i++) {
        u64 b = best[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) b = umin64(b, __shfl_xor(b, o));
        if (lane == 0 && qi[i] < nq && b != MST_NONE) atomicMin(mt.rowbest + qr[i], b);
    }
}
#pragma clang fp contract(on)

// The component's smallest edge under (w, lo, hi).  A row's smallest key under (w, t) is its
// smallest edge under (w, lo, hi) too, and the component's smallest edge is some row's smallest.
__global__ __launch_bounds__(256) void k_mst_pick_lo(MstTables t, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const u64 key = t.rowbest[i];
        if (key == MST_NONE) continue;
        const uint32_t o = (uint32_t)key, lo = min(o, (uint32_t)i);
        atomicMin(t.compbest + t.comp[i], (key & 0xffffffff00000000ull) | (u64)lo);
    }
}
__global__ __launch_bounds__(256) void k_mst_pick_hi(MstTables t, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const u64 key = t.rowbest[i];
        if (key == MST_NONE) continue;
        const uint32_t o = (uint32_t)key, lo = min(o, (uint32_t)i), hi = max(o, (uint32_t)i);
        const int32_t r = t.comp[i];
        if (((key & 0xffffffff00000000ull) | (u64)lo) == t.compbest[r]) atomicMin(t.comphi + r, hi);
    }
}

// One thread per component root.  The strict order makes the chosen edges cycle-free, so an edge
// chosen from both sides hooks exactly once: the call that hooked appends it.
__global__ __launch_bounds__(256) void k_mst_hook(MstTables t, int64_t n) {
    const int lane = lane_id();
    const int64_t n64 = (n + 63) & ~(int64_t)63;  // whole waves stay in the loop: the ballots are wave-wide
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n64; i += (int64_t)gridDim.x * 256) {
        bool offer = false, hooked = false;
        uint32_t lo = 0, hi = 0, wb = 0;
        if (i < n && t.comp[i] == (int32_t)i) {
            const u64 cb = t.compbest[i];
            hi = t.comphi[i];
            lo = (uint32_t)cb;
            wb = (uint32_t)(cb >> 32);
            offer = cb != MST_NONE && (int64_t)hi < n && lo < hi;
        }
        if (offer) hooked = uf_union(t.parent, (int32_t)lo, (int32_t)hi, n, t.status);
        const u64 mo = __ballot(offer), mh = __ballot(hooked);
        if (!mo) continue;
        unsigned long long base = 0;
        if (lane == 0) {
            atomicAdd(t.cnt + MST_CNT_OFFERS, (unsigned long long)__popcll(mo));
            if (mh) {
                atomicAdd(t.cnt + MST_CNT_HOOKS, (unsigned long long)__popcll(mh));
                base = atomicAdd(t.cnt + MST_CNT_EDGES, (unsigned long long)__popcll(mh));
            }
        }
        base = __shfl(base, 0);
        const int64_t slot = (int64_t)base + mst_lanes_below(mh);
        if (hooked && slot < n - 1) {  // (a forest has at most n - 1 edges)
            t.ekey[slot] = ((u64)lo << 32) | (u64)hi;
            t.ew[slot] = wb;
        }
    }
}

__global__ __launch_bounds__(256) void k_mst_flatten(MstTables t, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int64_t budget = n + 8;
        const int32_t r = uf_find(t.parent, (int32_t)i, budget);
        if (r < 0) atomicOr(t.status, KNN_STATUS_UF_LIMIT);
        else t.comp[i] = r;
    }
}

__global__ __launch_bounds__(256) void k_mst_unpack(const u64* __restrict__ ekey, const uint32_t* __restrict__ ew, int64_t E,
                                                    float* __restrict__ w, int32_t* __restrict__ a, int32_t* __restrict__ b) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) {
        w[e] = __uint_as_float(ew[e]);
        a[e] = (int32_t)(ekey[e] >> 32);
        b[e] = (int32_t)(uint32_t)ekey[e];
    }
}

// Every index is checked against [0, n) before any table is read with it.
__global__ __launch_bounds__(256) void k_mst_cut_link(const float* __restrict__ w, const int32_t* __restrict__ a,
                                                      const int32_t* __restrict__ b, int64_t E, int64_t n, float lo, float hi,
                                                      int32_t* parent, int32_t* status) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) {
        const int32_t x = a[e], y = b[e];
        if (x < 0 || (int64_t)x >= n || y < 0 || (int64_t)y >= n) {
            atomicOr(status, KNN_STATUS_BAD_INDEX);
            continue;
        }
        const float we = w[e];
        if ((lo < 0.0f || we > lo) && we <= hi) uf_union(parent, x, y, n, status);
    }
}

// An edge with w <= thr joins two rows with c <= w <= thr, so a core row's component holds core rows
// only and its root, the smallest of them, is a core row.
__global__ __launch_bounds__(256) void k_mst_cut_roots(int32_t* parent, const float* __restrict__ core, float thr, int64_t n,
                                                       int32_t* __restrict__ root, int32_t* __restrict__ isroot,
                                                       unsigned long long* info, int32_t* status) {
    const int lane = lane_id();
    unsigned long long ncore = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int32_t r = -1;
        if (core[i] <= thr) {
            int64_t budget = n + 8;
            r = uf_find(parent, (int32_t)i, budget);
            if (r < 0) atomicOr(status, KNN_STATUS_UF_LIMIT);
            ncore++;
        }
        root[i] = r;
        isroot[i] = r == (int32_t)i ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ncore += __shfl_xor(ncore, o);
    if (lane == 0 && ncore) atomicAdd(info + 1, ncore);
}

__global__ __launch_bounds__(256) void k_mst_cut_labels(const int32_t* __restrict__ root, const int64_t* __restrict__ offsets,
                                                        int64_t n, int32_t* __restrict__ labels, unsigned long long* info) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t r = root[i];
        labels[i] = r >= 0 ? (int32_t)offsets[r] : -1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        info[0] = (unsigned long long)offsets[n];
        info[2] = (unsigned long long)n - info[1];  // (k_mst_cut_roots, an earlier kernel, finished info[1])
    }
}

template <typename E>
const void* mst_tile_fn(int metric) {
    switch (metric) {
        case METRIC_SQEUCLIDEAN: return reinterpret_cast<const void*>(&k_mst_tile<METRIC_SQEUCLIDEAN, E>);
        case METRIC_MANHATTAN: return reinterpret_cast<const void*>(&k_mst_tile<METRIC_MANHATTAN, E>);
        case METRIC_CHEBYSHEV: return reinterpret_cast<const void*>(&k_mst_tile<METRIC_CHEBYSHEV, E>);
        default: return nullptr;
    }
}

bool mst_tables_ok(const MstTables& t) {
    return t.idx && t.dist && t.K >= 1 && t.core && t.dlast && t.parent && t.comp && t.rowbest && t.compbest &&
           t.comphi && t.cand && t.ekey && t.ew && t.cnt && t.status;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

// ---------------------------------------------------------------------------------
// Launchers (host side)
// ---------------------------------------------------------------------------------
hipError_t knn_launch_mst_core(const MstTables& t, int64_t n, int32_t min_samples, float* core_out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!mst_tables_ok(t) || n > 0x7fffffffLL || min_samples < 1 || min_samples > t.K) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mst_core, dim3(elementwise_grid(n)), dim3(256), 0, st, t, n, min_samples, core_out);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_mst_resolve(const MstTables& t, int64_t n, int use_lists, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!mst_tables_ok(t) || n > 0x7fffffffLL) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 15) / 16, 16384));
    hipLaunchKernelGGL(k_mst_resolve, dim3(grid), dim3(256), 0, st, t, n, use_lists);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_mst_tile(RadiusTileArgs a, const MstTables& t, int metric, hipStream_t st) {
    if (a.nt <= 0) return hipSuccess;
    const void* fn = a.elem == ELEM_BF16 ? mst_tile_fn<bf16_t>(metric) : mst_tile_fn<float>(metric);
    if (!fn || !mst_tables_ok(t) || !a.train || a.nseg < 1 || a.seg_len < 1 || a.d < 1 || a.nt > 0x7fffffffLL)
        return hipErrorInvalidValue;
    a.test = a.train; a.nq = a.nt; a.ld_q = a.ld_t;
    knn_direct_tile_geom(a.d, &a.dc, &a.stride);
    const int qb = DT_NW * KNN_RADIUS_QW;
    a.n_qblocks = (int)((a.nq + qb - 1) / qb);
    const dim3 grid((unsigned)((int64_t)a.n_qblocks * a.nseg));
    MstTables tt = t;
    void* args[] = {&a, &tt};
    const hipError_t e = hipLaunchKernel(fn, grid, dim3(64 * DT_NW), args, 2 * 64 * (size_t)a.stride * 4, st);
    if (e != hipSuccess) return e;
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_mst_pick_hook(const MstTables& t, int64_t n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!mst_tables_ok(t) || n > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid(elementwise_grid(n));
    hipLaunchKernelGGL(k_mst_pick_lo, grid, dim3(256), 0, st, t, n);
    KNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mst_pick_hi, grid, dim3(256), 0, st, t, n);
    KNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mst_hook, grid, dim3(256), 0, st, t, n);
    KNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mst_flatten, grid, dim3(256), 0, st, t, n);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

// temp: [E] u64 keys | [E] u32 weights (the first sort's outputs) | rocPRIM's own storage
static size_t mst_rocprim_bytes(int64_t E) {
    size_t b1 = 0, b2 = 0;
    u64* k64 = nullptr;
    uint32_t* k32 = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, b1, k64, k64, k32, k32, (size_t)E, 0, 64, (hipStream_t) nullptr) != hipSuccess ||
        rocprim::radix_sort_pairs(nullptr, b2, k32, k32, k64, k64, (size_t)E, 0, 32, (hipStream_t) nullptr) != hipSuccess)
        return 0;
    return std::max<size_t>(std::max(b1, b2), 16);
}
size_t knn_mst_sort_bytes(int64_t E) {
    if (E <= 0) return 0;
    return align256(8 * (size_t)E) + align256(4 * (size_t)E) + mst_rocprim_bytes(E);
}

hipError_t knn_launch_mst_sort(const MstTables& t, int64_t E, void* temp, float* w, int32_t* a, int32_t* b, hipStream_t st) {
    if (E <= 0) return hipSuccess;
    if (!t.ekey || !t.ew || !temp || !w || !a || !b) return hipErrorInvalidValue;
    unsigned char* p = static_cast<unsigned char*>(temp);
    u64* key2 = reinterpret_cast<u64*>(p);
    uint32_t* w2 = reinterpret_cast<uint32_t*>(p + align256(8 * (size_t)E));
    void* rp = p + align256(8 * (size_t)E) + align256(4 * (size_t)E);
    size_t bytes = mst_rocprim_bytes(E);
    if (!bytes) return hipErrorInvalidValue;
    // stable: on (a, b), then on bits(w) -- the order (w, a, b); the second sort lands in ekey / ew
    hipError_t e = rocprim::radix_sort_pairs(rp, bytes, t.ekey, key2, t.ew, w2, (size_t)E, 0, 64, st);
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(rp, bytes, w2, t.ew, key2, t.ekey, (size_t)E, 0, 32, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mst_unpack, dim3(elementwise_grid(E)), dim3(256), 0, st, t.ekey, t.ew, E, w, a, b);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_mst_cut_link(const float* w, const int32_t* a, const int32_t* b, int64_t E, int64_t n, float lo,
                                   float hi, int32_t* parent, int32_t* status, hipStream_t st) {
    if (E <= 0 || n <= 0) return hipSuccess;
    if (!w || !a || !b || !parent || !status || n > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mst_cut_link, dim3(elementwise_grid(E)), dim3(256), 0, st, w, a, b, E, n, lo, hi, parent, status);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_mst_cut_roots(int32_t* parent, const float* core, float thr, int64_t n, int32_t* root,
                                    int32_t* isroot, unsigned long long* info, int32_t* status, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!parent || !core || !root || !isroot || !info || !status) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mst_cut_roots, dim3(elementwise_grid(n)), dim3(256), 0, st, parent, core, thr, n, root, isroot, info,
                       status);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t knn_launch_mst_cut_labels(const int32_t* root, const int64_t* offsets, int64_t n, int32_t* labels,
                                     unsigned long long* info, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!root || !offsets || !labels || !info) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mst_cut_labels, dim3(elementwise_grid(n)), dim3(256), 0, st, root, offsets, n, labels, info);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}
