// knn_metric.hip -- the direct form under the non-Euclidean metrics (include/knn_amd.h,
// "Metrics"): k_metric_tile<M, QW, R, E, SH>, k_direct_tile's skeleton (knn_kernels.hip) with
// the per-feature step of metric M.
//
//   Manhattan  D = sum_i |q_i - t_i|:  sum = +0;  df = fl(q_i - t_i);  sum = fl(sum + |df|)
//   Chebyshev  D = max_i |q_i - t_i|:  m = +0;    m = fmaxf(m, |fl(q_i - t_i)|)
//
// i ascending, IEEE binary32, no FMA, no reordering, subnormals kept.  fmaxf returns its other
// operand when one is NaN, so a NaN difference leaves the Chebyshev maximum as it was
// (numpy.fmax); under Manhattan a NaN difference makes the sum NaN, which never qualifies.
// Both values are >= +0, so they order by their bits like the squared Euclidean distance and
// everything behind the distance (the wave lists, finish_query, the segment records that
// k_merge_vote merges) is shared with k_direct_tile unchanged.
//
// This file is built with no fast-math flag and with contraction off (Makefile): `-x` and |x|
// are source modifiers of the add / max, so a feature costs v_sub_f32 + v_add_f32 |x|
// (Manhattan) or v_sub_f32 + half a v_max3_f32 |x| |y| (Chebyshev), against k_direct_tile's
// v_sub, v_mul, v_add.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include "knn_kernels.h"

#include "knn_device.h"

#pragma clang fp contract(off)
// one feature of metric M: the accumulator after (q_i, t_i)
template <int M>
__device__ __forceinline__ float metric_step(float acc, float q, float t) {
    const float df = q - t;
    if constexpr (M == METRIC_MANHATTAN)
        return acc + __builtin_fabsf(df);
    else
        return __builtin_fmaxf(acc, __builtin_fabsf(df));
}

// ---------------------------------------------------------------------------------
// k_metric_tile<M, QW, R, E, SH>: k_direct_tile for metric M (DirectTileArgs; the launcher
// fills dc / stride / vote_lds / n_qblocks).  A block of DT_NW = 8 waves owns 8*QW queries;
// lane l of every wave computes the distances of train row r0 + l to its wave's QW queries.
//  * Train tiles (64 rows x dc <= DT_MAX_DC dims, widened to fp32) are staged once per block
//    in LDS, double-buffered, rows padded to an odd number of 16-B slots; rows wider than dc
//    carry their accumulator over the chunks in ascending feature order.
//  * Query values are wave-uniform (scalar loads feeding the v_sub).
//  * After a tile's last chunk each query tests its 64 new distances against its running k-th
//    distance (strict '<' from the FLT_MAX sentinel: inf, NaN and >= FLT_MAX never pass), then
//    inserts by lane shift (SH: k <= 16, at most DT_SHIFT_MAX passing rows) or by topk_merge,
//    and the accumulator restarts from +0.
//  * nseg == 1 ends in finish_query; nseg > 1 writes the segment records [nseg][nq][3][k]
//    (dist bits, local row, label) that k_merge_vote merges.
// LDS: 2 tile buffers [64][stride] f32 | per-wave class counts [8][Cpad] (vote_lds)
// ---------------------------------------------------------------------------------
template <int M, int QW, int R, typename E, bool SH>
__global__ __launch_bounds__(64 * DT_NW, 4) void k_metric_tile(DirectTileArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NT = 64 * DT_NW;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile_floats = 64 * a.stride;
    float* bufs = reinterpret_cast<float*>(smem);
    int* counts = a.vote_lds ? reinterpret_cast<int*>(smem + 2 * (size_t)tile_floats * 4) + wave * ((a.C + 3) & ~3)
                             : nullptr;
    const int qb = blockIdx.x % a.n_qblocks;
    const int seg = blockIdx.x / a.n_qblocks;
    const int64_t row_begin = (int64_t)seg * a.seg_len;
    const int64_t row_end = min(a.nt, row_begin + a.seg_len);
    const E* __restrict__ train = reinterpret_cast<const E*>(a.train);
    const E* __restrict__ test = reinterpret_cast<const E*>(a.test);
    const int d = a.d, k = a.k;

    int64_t qi[QW];
    const E* qrow[QW];
    u64 T[QW][R];
    float thr[QW];
#pragma unroll
    for (int i = 0; i < QW; i++) {
        qi[i] = (int64_t)qb * (DT_NW * QW) + wave * QW + i;
        qrow[i] = test + (qi[i] < a.nq ? qi[i] : a.nq - 1) * (int64_t)a.ld_q;
#pragma unroll
        for (int r = 0; r < R; r++) T[i][r] = KEY_NONE;
        thr[i] = FLT_MAX;
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
                    const float4 qv = load4(qrow[i] + col);  // wave-uniform: scalar loads
                    float s0 = acc[i];
                    s0 = metric_step<M>(s0, qv.x, t.x);
                    s0 = metric_step<M>(s0, qv.y, t.y);
                    s0 = metric_step<M>(s0, qv.z, t.z);
                    s0 = metric_step<M>(s0, qv.w, t.w);
                    acc[i] = s0;
                }
            } else {
                const int rem = d - col;  // 1..3 trailing dims
#pragma unroll
                for (int i = 0; i < QW; i++) {
                    const float4 qv = load4(qrow[i] + col);
                    float s0 = acc[i];
                    s0 = metric_step<M>(s0, qv.x, t.x);
                    if (rem > 1) s0 = metric_step<M>(s0, qv.y, t.y);
                    if (rem > 2) s0 = metric_step<M>(s0, qv.z, t.z);
                    acc[i] = s0;
                }
            }
        }
        if (ch == nchunk - 1) {
            // the tile's distances are final: selection
            const int64_t row = row_begin + (s / nchunk) * 64 + lane;
            const bool valid = row < row_end;
#pragma unroll
            for (int i = 0; i < QW; i++) {
                const bool pass = valid && acc[i] < thr[i];
                u64 m = __ballot(pass);
                if (m) {
                    if (SH && __popcll(m) <= DT_SHIFT_MAX) {
                        // one row at a time, ascending: each re-tested against the threshold
                        // the previous insertions left
                        const uint32_t row0 = (uint32_t)(row - lane);
                        do {
                            const int b = __builtin_ctzll(m);
                            m &= m - 1;
                            const float x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc[i]), b));
                            if (x < thr[i]) {
                                shift_insert(T[i][0], ((u64)__float_as_uint(x) << 32) | (u64)(row0 + (uint32_t)b),
                                             lane < k);
                                thr[i] = kth_dist(T[i][0], k);
                            }
                        } while (m);
                    } else {
                        topk_merge<R>(T[i], pass ? make_key(acc[i], (uint32_t)row) : KEY_NONE);
                        if constexpr (SH) {
                            thr[i] = kth_dist(T[i][0], k);
                        } else {
                            const u64 kth = list_at(T[i], k - 1);
                            thr[i] = kth == KEY_NONE ? FLT_MAX : __uint_as_float((uint32_t)(kth >> 32));
                        }
                    }
                }
                acc[i] = 0.0f;  // both metrics restart from +0
            }
        }
        if (s + 1 < nsteps) store_chunk(s + 1);
        __syncthreads();
    }
    if (a.nseg == 1) {
#pragma unroll
        for (int i = 0; i < QW; i++)
            if (qi[i] < a.nq) finish_query<R>(T[i], k, a.C, a.labels, counts, qi[i], a.out, a.status);
        return;
    }
    // segment records: k (dist bits, local row, label), ascending (KEY_NONE: FLT_MAX, -1, -1)
#pragma unroll
    for (int i = 0; i < QW; i++) {
        if (qi[i] >= a.nq) continue;
        int32_t* rec = a.rec + ((int64_t)seg * a.nq + qi[i]) * 3 * (int64_t)k;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int e = 64 * r + lane;
            if (e < k) {
                const u64 key = T[i][r];
                const bool none = key == KEY_NONE;
                const int32_t idx = (int32_t)(uint32_t)(key & 0xffffffffull);
                rec[e] = none ? (int32_t)__float_as_uint(FLT_MAX) : (int32_t)(uint32_t)(key >> 32);
                rec[k + e] = none ? -1 : idx;
                rec[2 * k + e] = none ? -1 : a.labels[idx];
            }
        }
    }
}
#pragma clang fp contract(on)

// ---------------------------------------------------------------------------------
// Launcher (host side): k_direct_tile's geometry, one kernel per (metric, list registers,
// element type)
// ---------------------------------------------------------------------------------
template <int M, int QW, int R, typename E, bool SH = false>
static const void* metric_tile_fn() { return reinterpret_cast<const void*>(&k_metric_tile<M, QW, R, E, SH>); }

template <int M, typename E>
static const void* metric_tile_fn_e(int k) {
    switch (knn_list_regs(k)) {
        case 1: return k <= 16 ? metric_tile_fn<M, 8, 1, E, true>() : metric_tile_fn<M, 8, 1, E>();
        case 2: return metric_tile_fn<M, 4, 2, E>();
        case 4: return metric_tile_fn<M, 2, 4, E>();
        case 8: return metric_tile_fn<M, 1, 8, E>();
        default: return metric_tile_fn<M, 1, 16, E>();
    }
}
// nullptr: not a metric of this kernel
static const void* metric_tile_ptr(int metric, int k, int elem) {
    const bool bf = elem == ELEM_BF16;
    switch (metric) {
        case METRIC_MANHATTAN:
            return bf ? metric_tile_fn_e<METRIC_MANHATTAN, bf16_t>(k) : metric_tile_fn_e<METRIC_MANHATTAN, float>(k);
        case METRIC_CHEBYSHEV:
            return bf ? metric_tile_fn_e<METRIC_CHEBYSHEV, bf16_t>(k) : metric_tile_fn_e<METRIC_CHEBYSHEV, float>(k);
        default: return nullptr;
    }
}

hipError_t knn_metric_units(int metric, int k, int elem, int d, int C, int* queries_per_unit, int* units_per_cu) {
    const void* fn = metric_tile_ptr(metric, k, elem);
    if (!fn) return hipErrorInvalidValue;
    int occ = 1;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 64 * DT_NW, knn_direct_tile_lds(d, C));
    *queries_per_unit = knn_direct_tile_qb(k);
    *units_per_cu = std::max(occ, 1);
    return e;
}

hipError_t knn_launch_metric_tile(DirectTileArgs a, int metric, hipStream_t st) {
    if (a.nq <= 0) return hipSuccess;
    const void* fn = metric_tile_ptr(metric, a.k, a.elem);
    if (!fn || a.nseg < 1 || (a.nseg > 1 && !a.rec) || a.d < 1 || a.k < 1 || a.k > 1024) return hipErrorInvalidValue;
    knn_direct_tile_geom(a.d, &a.dc, &a.stride);
    a.vote_lds = a.C <= KNN_VOTE_LDS_MAX_C;
    a.arrive = nullptr;
    const int qb = knn_direct_tile_qb(a.k);
    a.n_qblocks = (int)((a.nq + qb - 1) / qb);
    const dim3 grid((unsigned)((int64_t)a.n_qblocks * a.nseg));
    void* args[] = {&a};
    const hipError_t e = hipLaunchKernel(fn, grid, dim3(64 * DT_NW), args, knn_direct_tile_lds(a.d, a.C), st);
    if (e != hipSuccess) return e;
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}
