// knn_fused.hip -- the GEMM-form candidate filter on the bf16 MFMA with the train norm
// folded into the MFMA (gfx950).  DESIGN.md "k_gemm_fused".
//
// Train operand: tile blocks (k_tn_rows), one per tile of bn rows,
//   [ bn rows x d bf16 rn(t) | bn fp32 norms tn = ||t||^2 | {max tn, max |t - rt|, max |rt|, 0} ]
// -- exactly the bytes one tile's LDS-DMA copies.  Query operand: [nq][d] bf16 rn(-2 q).
// Each accumulator starts from its rows' norms (the first MFMA's C operand), so one chain of
// v_mfma_f32_32x32x16_bf16 over d/16 k-steps leaves
//   y = tn - 2 rn(q).rn(t)
// in the accumulators: the fast test is a v_min3 chain over the 16 values of an
// accumulator against one per-(query, tile) threshold, with no per-value norm read or
// fma; the slow path takes each lane's passing values, computes the certificate bounds
//   G = qn + y,  Delta = coef (qn + tmax_tile) + eta + rho,  L = G - Delta <= D <= U = G + Delta
// (D: the reference's direct-form distance, main.cpp:14-23) and keeps (row, L, U) for
// the exact rescore (k_rescore).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "knn_device.h"
#include "knn_kernels.h"

// Constants of the filter (each measured against its alternatives; DESIGN.md "Filter studies")
static constexpr int FUSED_PF = 6;            // A-fragment prefetch depth, in MFMAs
static constexpr int FUSED_DEFER_EVERY = 64;  // 8-wave heap shapes: tiles between flushes of the queued values
static constexpr int FUSED_SHARE_EVERY = 64;  // tiles between threshold exchanges of a query's pieces (gthr)
static constexpr int FUSED_RQ = 4;            // queued passing values per lane (heap shapes)
static constexpr int FUSED_LIST_FIRST = 31;   // first list exchange after this tile (then doubling: tiles 32, 64, 128, ...)
// ... and after every this many tiles: never in practice (tile 2^30 - 1 is a doubling point
// too), but the compiler does not see that, and without the term the list-exchange kernels lose
// four instructions -- kept so that removing the study hooks left every kernel's code unchanged
static constexpr int FUSED_LIST_EVERY = 1 << 30;
// parked passes on the int8 shapes unless KNN_FUSED_PARK says otherwise (knn_fused_plan)
static constexpr bool FUSED_PARK_DEFAULT = true;

// ---------------------------------------------------------------------------------
// k_tn_rows<E>: operand rows of the filter (no augmented columns).
//   queries (norms == NULL): [n][dp] bf16 = rn(scale * x)
//   train: blocks of bn rows, [bn][dp] bf16 = rn(x) | bn fp32 norms | {max tn, max |t - rt|,
//   max |rt|, 0} of the enclosing 64-row tile (k_row_norms) -- the image one tile's LDS-DMA
//   copies, header included.  Rows n_valid .. n-1 (padding past the tile grid): zero features
//   and norm 0x1.fep127, so y = tn - 2 q.t never passes a fast test.  n % bn == 0.
// d: the caller's row width; dp >= d (dp % 4 == 0): the operand's.  Columns d .. dp-1 are zero
// bits (a zero product adds nothing to the MFMA chain); no load touches column d or beyond --
// whole quads inside the row are one load, the row's last partial quad is read by element (the
// caller's buffer may end at (n - 1) ld + d elements, and a view's pad columns hold anything).
// ---------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(256) void k_tn_rows(const E* __restrict__ x, int64_t n, int64_t n_valid, int ld, int d,
                                                 int dp, const float* __restrict__ norms, float scale,
                                                 unsigned char* __restrict__ out, const float4* __restrict__ tstat,
                                                 int bn, const int32_t* __restrict__ gate) {
    if (gate && *gate == 0) return;
    const int per_row = dp >> 2;
    auto quad = [&](int64_t r, int c) -> uint2 {
        if (r >= n_valid) return make_uint2(0u, 0u);
        return operand_quad(x + r * ld, c, d, scale);
    };
    if (!norms) {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * per_row; i += (int64_t)gridDim.x * 256) {
            const int64_t r = i / per_row;
            const int c = (int)(i - r * per_row) * 4;
            *reinterpret_cast<uint2*>(out + (r * dp + c) * 2) = quad(r, c);
        }
        return;
    }
    const int64_t per_tile = (int64_t)bn * per_row + bn + 1;
    const int64_t tb = (int64_t)bn * dp * 2 + 4 * bn + 16;
    const int64_t nvt = (n_valid + 63) >> 6;  // 64-row tiles with statistics
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (n / bn) * per_tile; i += (int64_t)gridDim.x * 256) {
        const int64_t T = i / per_tile;
        const int64_t l = i - T * per_tile;
        const int64_t r0 = T * bn;
        unsigned char* blk = out + T * tb;
        if (l < (int64_t)bn * per_row) {
            const int rr = (int)(l / per_row);
            const int c = (int)(l - (int64_t)rr * per_row) * 4;
            *reinterpret_cast<uint2*>(blk + ((int64_t)rr * dp + c) * 2) = quad(r0 + rr, c);
        } else if (l < (int64_t)bn * per_row + bn) {
            const int rr = (int)(l - (int64_t)bn * per_row);
            const int64_t r = r0 + rr;
            *reinterpret_cast<float*>(blk + (int64_t)bn * dp * 2 + 4 * rr) = r < n_valid ? norms[r] : 0x1.fep127f;
        } else {
            const int64_t t64 = r0 >> 6;
            *reinterpret_cast<float4*>(blk + (int64_t)bn * dp * 2 + 4 * bn) =
                t64 < nvt ? tstat[t64] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
}

hipError_t knn_launch_tn_rows(const void* x, int elem, int64_t n, int64_t n_valid, int ld, int d, int dp,
                              const float* norms, float scale, void* out, const float4* tstat, int bn, hipStream_t st,
                              const int32_t* gate) {
    if (n <= 0) return hipSuccess;
    if (d < 1 || dp < d || dp % 4 || ld % 4 || (norms && (bn <= 0 || n % bn))) return hipErrorInvalidValue;
    const int64_t total = norms ? (n / bn) * ((int64_t)bn * (dp / 4) + bn + 1) : n * (dp / 4);
    const dim3 grid(gated_grid(elementwise_grid(total), gate));
    if (elem == ELEM_BF16)
        hipLaunchKernelGGL(k_tn_rows<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)x, n, n_valid, ld, d, dp, norms,
                           scale, (unsigned char*)out, tstat, bn, gate);
    else
        hipLaunchKernelGGL(k_tn_rows<float>, grid, dim3(256), 0, st, (const float*)x, n, n_valid, ld, d, dp, norms,
                           scale, (unsigned char*)out, tstat, bn, gate);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

// Host view of the operand rows (no GPU call; tests/test_filter_width_cpu.py): out [n][dp] bf16 =
// the rows k_tn_rows' query form and k_round_rows (scale 1) write for x [n][ld] of d elements --
// operand_quad as the kernels run it, but for the load: on the host every quad takes the per-element
// branch, on the device a whole quad inside the row is one load4.  elem: ELEM_F32 or ELEM_BF16.
extern "C" int knn_debug_operand_rows(const void* x, int elem, long long n, int ld, int d, int dp, float scale,
                                      uint16_t* out) {
    if (!x || !out || n < 0 || d < 1 || dp < d || dp % 4 || ld < d || (elem != ELEM_F32 && elem != ELEM_BF16)) return -1;
    for (long long r = 0; r < n; r++)
        for (int c = 0; c < dp; c += 4) {
            const uint2 q = elem == ELEM_BF16 ? operand_quad((const bf16_t*)x + r * ld, c, d, scale)
                                              : operand_quad((const float*)x + r * ld, c, d, scale);
            uint16_t* o = out + r * dp + c;
            o[0] = (uint16_t)q.x; o[1] = (uint16_t)(q.x >> 16); o[2] = (uint16_t)q.y; o[3] = (uint16_t)(q.y >> 16);
        }
    return 0;
}

// ---------------------------------------------------------------------------------
// k_i8_rows: operand rows of the int8 operand class (fp32 x, the train set's scale s).
//   queries (norms == NULL): [n][d] int8 = knn_i8_quant(x, s)
//   train: blocks of bn rows, [bn][d] int8 | bn int32 -knn_i8_norm_q(tn, s2) (the accumulators'
//   start) | the enclosing 64-row tile's statistics (k_row_norms with i8s = s) -- the same image
//   shape as k_tn_rows at half the row bytes.  Rows n_valid .. n-1: zero features and -2^30, below
//   every valid row's term (run_gemm admits a train set only when max tn / s2 < 2^30), and their
//   indices are past row_end.  n % bn == 0.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_i8_rows(const float* __restrict__ x, int64_t n, int64_t n_valid, int ld, int d,
                                                 const float* __restrict__ norms, float s,
                                                 unsigned char* __restrict__ out, const float4* __restrict__ tstat,
                                                 int bn) {
    const int per_row = d >> 2;
    auto quad = [&](int64_t r, int c) -> uint32_t {
        if (r >= n_valid) return 0u;
        const float4 v = load4(x + r * ld + c);
        return ((uint32_t)knn_i8_quant(v.x, s) & 0xffu) | (((uint32_t)knn_i8_quant(v.y, s) & 0xffu) << 8) |
               (((uint32_t)knn_i8_quant(v.z, s) & 0xffu) << 16) | (((uint32_t)knn_i8_quant(v.w, s) & 0xffu) << 24);
    };
    if (!norms) {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * per_row; i += (int64_t)gridDim.x * 256) {
            const int64_t r = i / per_row;
            const int c = (int)(i - r * per_row) * 4;
            *reinterpret_cast<uint32_t*>(out + r * d + c) = quad(r, c);
        }
        return;
    }
    const float s2 = knn_i8_s2(s);
    const int64_t per_tile = (int64_t)bn * per_row + bn + 1;
    const int64_t tb = (int64_t)bn * d + 4 * bn + 16;
    const int64_t nvt = (n_valid + 63) >> 6;  // 64-row tiles with statistics
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (n / bn) * per_tile; i += (int64_t)gridDim.x * 256) {
        const int64_t T = i / per_tile;
        const int64_t l = i - T * per_tile;
        const int64_t r0 = T * bn;
        unsigned char* blk = out + T * tb;
        if (l < (int64_t)bn * per_row) {
            const int rr = (int)(l / per_row);
            const int c = (int)(l - (int64_t)rr * per_row) * 4;
            *reinterpret_cast<uint32_t*>(blk + (int64_t)rr * d + c) = quad(r0 + rr, c);
        } else if (l < (int64_t)bn * per_row + bn) {
            const int rr = (int)(l - (int64_t)bn * per_row);
            const int64_t r = r0 + rr;
            *reinterpret_cast<int32_t*>(blk + (int64_t)bn * d + 4 * rr) = r < n_valid ? -knn_i8_norm_q(norms[r], s2) : -(1 << 30);
        } else {
            const int64_t t64 = r0 >> 6;
            *reinterpret_cast<float4*>(blk + (int64_t)bn * d + 4 * bn) =
                t64 < nvt ? tstat[t64] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
}

hipError_t knn_launch_i8_rows(const float* x, int64_t n, int64_t n_valid, int ld, int d, const float* norms, float s,
                              void* out, const float4* tstat, int bn, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (d % 16 || ld % 4 || !(s > 0.0f) || (norms && (bn <= 0 || n % bn))) return hipErrorInvalidValue;
    const int64_t total = norms ? (n / bn) * ((int64_t)bn * (d / 4) + bn + 1) : n * (d / 4);
    hipLaunchKernelGGL(k_i8_rows, dim3(elementwise_grid(total)), dim3(256), 0, st, x, n, n_valid, ld, d, norms, s,
                       (unsigned char*)out, tstat, bn);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

float knn_i8_s2_of(float s) { return knn_i8_s2(s); }

// host views of the int8 operand rule (knn_device.h), for tests/test_i8_quant_cpu.py.  No GPU call.
extern "C" int knn_i8_debug_quant(const float* x, long long n, float s, signed char* out) {
    for (long long i = 0; i < n; i++) out[i] = (signed char)knn_i8_quant(x[i], s);
    return 0;
}
// out[3 i] = {knn_i8_norm_q(tn, s2), the bits of knn_i8_norm_res(tn, s2, that), knn_i8_fast_thr(tf, s2)}
extern "C" int knn_i8_debug_fast(const float* tn, const float* tf, const float* s2, long long n, int* out) {
    for (long long i = 0; i < n; i++) {
        const int32_t nr = knn_i8_norm_q(tn[i], s2[i]);
        const float res = knn_i8_norm_res(tn[i], s2[i], nr);
        uint32_t bits;
        memcpy(&bits, &res, 4);
        out[3 * i] = nr;
        out[3 * i + 1] = (int)bits;
        out[3 * i + 2] = knn_i8_fast_thr(tf[i], s2[i]);
    }
    return 0;
}

// ---------------------------------------------------------------------------------
// k_tile_stat_max: out = {max tn, max |t - rt|, max |rt|, max |tn - s2 n| (int8 operands)} over the n 64-row tile statistics
// (k_row_norms' tstat): the fused filter's fast-test tile term (a.tsmax).  One block.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tile_stat_max(const float4* __restrict__ t, int64_t n, float4* __restrict__ out) {
    __shared__ float4 part[4];
    float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // (the statistics are >= 0)
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const float4 v = t[i];
        m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m.x = fmaxf(m.x, __shfl_xor(m.x, o)); m.y = fmaxf(m.y, __shfl_xor(m.y, o)); m.z = fmaxf(m.z, __shfl_xor(m.z, o));
        m.w = fmaxf(m.w, __shfl_xor(m.w, o));
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float4 r = part[0];
        for (int w = 1; w < 4; w++) { r.x = fmaxf(r.x, part[w].x); r.y = fmaxf(r.y, part[w].y); r.z = fmaxf(r.z, part[w].z); r.w = fmaxf(r.w, part[w].w); }
        *out = r;
    }
}

hipError_t knn_launch_tile_stat_max(const float4* tstat, int64_t n, float4* out, hipStream_t st) {
    if (n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tile_stat_max, dim3(1), dim3(256), 0, st, tstat, n, out);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

// ---------------------------------------------------------------------------------
// k_gemm_fused<RB, MINW, NBUF, NW, RG>: the filter (RB = bytes per operand row,
// 2d; d for the int8 class).  Block = NW waves x 32 queries; a train tile has BN = 32 RG rows, copied
// global -> LDS by LDS-DMA (NBUF buffers, one barrier per tile, pieces issued between
// the MFMAs) with each row padded to RB + 16 bytes (conflict-free ds_read_b128 of the A
// fragments).  Lane (j, h) holds 16 bytes of its query's row per k-step in
// VGPRs (the B fragment) for the whole scan; register r of accumulator c holds train
// row 32c + (r & 3) + 8 (r >> 2) + 4h of the tile against query j.  Per tile each wave
// issues the MFMAs of tile it into X while the fast test of tile it-1 (Y) runs in
// between (software pipelining).
//
// Fast test: the tile passes for query q when min_r y_r <= tf(q, tile), with
//   tf = (thr - qn) + coef qn + eta + 2^-18 (|thr| + qn) + (coef + 2^-18) tmax_tile,
// tmax_tile >= tn of every row of the tile (k_row_norms' per-64-row maxima): a superset
// of the exact test L <= thr (2^-18 (...) covers the few fp32 roundings between the two
// forms, <= 2^-21 of the same magnitudes).
// Threshold thr: the k-th smallest U among rows this block kept (per-query 4-ary
// max-heap in LDS, as k_gemm_filter), or a smaller bound published by another segment
// (gthr).  Every row of the exact top-k has L <= D <= D_(k) <= thr, so it is kept.
// ---------------------------------------------------------------------------------
// fused_piece: one piece of work -- query tile qt against train rows [row_begin, row_end),
// piece (segment) id seg of that query tile (its candidate sub-slices, 2 seg + h)

// Pacing of the blocks of one XCD (a.pace; the balanced schedule): every FUSED_SHARE_EVERY tiles
// a block adds a step to its XCD's sum, and while it is more than FUSED_PACE_LEAD steps ahead of
// the average of the XCD's running blocks it sleeps -- at most FUSED_PACE_POLLS times, then
// goes on regardless.  Only blocks that are running are counted (each registers itself at its
// start, at the XCD's average then, and takes its steps out at its end), so nothing is assumed
// about which blocks are resident; the kernel's time is its slowest block's, which is never held.  Thread 0 only: the
// other waves wait for it at the next group barrier.
static constexpr int FUSED_PACE_LEAD = 1;
static constexpr int FUSED_PACE_POLLS = 32;
__device__ __forceinline__ void fused_pace(int32_t* p, int steps) {
    __hip_atomic_fetch_add(p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int poll = 0; poll < FUSED_PACE_POLLS; poll++) {
        const int sum = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int n = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n <= 0 || (steps - FUSED_PACE_LEAD) * n <= sum) break;
        __builtin_amdgcn_s_sleep(127);
    }
}

// The 16 compares of a lane's accumulator values against one operand, each folded into a mask by
// an add-with-carry (the lane scans of fused_piece's slow path; CMP: the element's compare)
#define KNN_FUSED_SCAN16(CMP)                                                                   \
    CMP " vcc, %17, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"                            \
    CMP " vcc, %16, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"                            \
    CMP " vcc, %15, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"                            \
    CMP " vcc, %14, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"                            \
    CMP " vcc, %13, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"                            \
    CMP " vcc, %12, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"                            \
    CMP " vcc, %11, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"                            \
    CMP " vcc, %10, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"                            \
    CMP " vcc, %9, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"                             \
    CMP " vcc, %8, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"                             \
    CMP " vcc, %7, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"                             \
    CMP " vcc, %6, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"                             \
    CMP " vcc, %5, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"                             \
    CMP " vcc, %4, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"                             \
    CMP " vcc, %3, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"                             \
    CMP " vcc, %2, %1\n\tv_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
#define KNN_FUSED_SCAN16_Y(Y) "v"(Y[0]), "v"(Y[1]), "v"(Y[2]), "v"(Y[3]), "v"(Y[4]), "v"(Y[5]), "v"(Y[6]), "v"(Y[7]), \
    "v"(Y[8]), "v"(Y[9]), "v"(Y[10]), "v"(Y[11]), "v"(Y[12]), "v"(Y[13]), "v"(Y[14]), "v"(Y[15])

// I8: the int8 operand class (DESIGN.md "int8 filter operands"): rows of RB = d int8 bytes on
// v_mfma_i32_32x32x32_i8 (K = 32 per k-step, the same 16 bytes per lane and k-step), the tile
// header's BN words int32 -n_r (n_r ~ tn / s2), integer accumulators
//   a = nq . nt - n_r,    y* = tn - s2 nq . nt = (tn - s2 n_r) - s2 a,   |tn - s2 n_r| <= nu,
// the fast test max_r a_r >= ti (ti: knn_i8_fast_thr of the same tf, which carries nu) and the
// slow path's G = qn - s2 float(a) with nu in the band.  Three sites differ from the bf16 form:
// the MFMA, the accumulators' start, the fast test and its scans' compares.
//
// PARK (the int8 register-list shapes; DESIGN.md "Parked passes"): a tile that passes the fast
// test is not visited at once.  Its passing lanes copy their accumulator into a slot of their own
// in LDS (fused_park_off) and the wave goes on with the next tile's MFMAs; every
// FUSED_SHARE_EVERY tiles, before a list exchange and at the end of the piece all lanes take their
// parked records through the slow path together (flush_ring).  A tile whose passing lanes do not
// all have a free slot takes the immediate path, as without PARK.
template <int RB, int NBUF, int NW, int QG, int RG, int KR, bool I8, bool PARK>
__device__ __forceinline__ void fused_piece(const GemmFilterArgs& a, const int qt, const int seg,
                                            const int64_t row_begin, const int64_t row_end,
                                            const int64_t rot_units, int& steps) {
    typedef typename std::conditional<I8, int, float>::type AccT;  // an accumulator value
    typedef AccT accx16 __attribute__((ext_vector_type(16)));
    typedef typename std::conditional<I8, int4, float4>::type accx4;  // one header read of four accumulator starts
    typedef int intx4 __attribute__((ext_vector_type(4)));
    constexpr int EB = I8 ? 1 : 2;  // bytes per operand element
    // train tiles carry their rows' norms in a header, and each accumulator starts from them (the
    // MFMA's C operand)
    static_assert(RB % 64 == 0, "operand rows: whole k-steps");
    constexpr int HS = 32 * RG / 4 + 1;  // header slots: BN fp32 norms + the statistics
    // QG 32-query groups per wave (QG = 2: 64 queries per wave on 32-row tiles, the register-list
    // shapes only): accumulator c holds row group c % RG against query group c / RG, so each A
    // fragment read from LDS feeds QG MFMAs and each tile copy serves 32 QG NW queries
    typedef FilterTile<RB, NW, QG, RG, HS> FT;
    constexpr int NACC = FT::NACC, BN = FT::BN, BM = FT::BM, STRIDE = FT::STRIDE;
    constexpr int DMA_INS = FT::DMA_INS, TILE = FT::TILE, HDR = FT::HDR;
    // bytes of one tile in the train operand (a block of rows + header)
    constexpr int64_t TB = (int64_t)BN * RB + 16 * HS;
    constexpr int NT = 64 * NW;
    constexpr int DMA_PER_WAVE = (DMA_INS + NW - 1) / NW;
    constexpr int NS = RB / 32;                  // k-steps: d/16 feature steps
    constexpr int VPS = (16 + NS - 1) / NS;      // fast-test values per k-step per accumulator
    static_assert(NBUF == 2 || NBUF == 4 || NBUF == 8 || NBUF == 16, "tile buffers: two, four (pairs), eight (quads), 16 (octets)");
    // NBUF = 4: tiles go in pairs -- one barrier per pair; the DMA of tile it + 2 is issued
    // during step it into the buffer tile it - 2 used (read before this pair's barrier)
    // NBUF = 8: quads -- one barrier per four tiles; NBUF = 16: octets (the QG = 2 default,
    // knn_fused_plan: eight 32-row tiles per barrier; the code of eight static tile places is
    // ~50 KB)
    constexpr int GRP = NBUF >= 4 ? NBUF / 2 : 1;  // tiles per barrier
    constexpr bool PAIR = GRP > 1;
    constexpr int AHEAD = PAIR ? GRP : NBUF - 1;  // tiles between a step and the tile it DMAs
    static_assert(RG == 1 || RG == 2, "row groups");
    static_assert(KR == 0 || KR == 8 || KR == 32 || KR == 104, "register lists: k <= 16, 32, 104, or LDS heaps");
    constexpr bool RL = KR > 0;                   // thresholds from per-lane register lists (else LDS heaps)
    // (QG = 2 on 64-row tiles, four accumulators, was tried at d = 64: 1.5 KB of scratch spills)
    static_assert(QG == 1 || (QG == 2 && RG == 1 && RL), "64-query waves: 32-row tiles, register lists");
    static_assert(!I8 || (RL && KR <= 32 && PAIR),
                  "int8 operands: the register-list shapes, the global tile term");
    static_assert(!PARK || (I8 && NW == 8 && QG * RG == 2), "parked passes: the int8 shapes, two accumulators");
    constexpr int LL = KR == 104 ? 52 : KR == 8 ? 8 : 16;  // register list length (one per lane half)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* tiles = smem;                                     // [NBUF][TILE]
    const int hs = heap_stride(a.k);
    float* topU = reinterpret_cast<float*>(smem + NBUF * TILE);      // [BM][hs] max-heaps of U
    const int cap_sub = a.cap_seg / 2;  // candidate sub-slice of one lane half (h) of a query

    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31;
    const int h = lane >> 5;
    const int k = a.k;
    const float INF = __uint_as_float(0x7f800000u);
    const float coef = a.coef, eta = a.eta;
    const int64_t ldb = (int64_t)a.ld_t * EB;  // train row pitch, bytes
    [[maybe_unused]] const float s2 = a.i8_s2;  // (I8)
    const unsigned char* trainb = reinterpret_cast<const unsigned char*>(a.train);

    if constexpr (!RL) {
        for (int i = threadIdx.x; i < BM * hs; i += NT) {
            const int e = i % hs;
            topU[i] = (e == hs - 1 || e <= k - 2) ? INF : -INF;  // root, nodes 1..k-1: +inf
        }
    }

    // this lane's queries, one per query group g (both lane halves hold the same queries,
    // different rows): query jl[g] of the block
    int jl[QG];
    int64_t q[QG];
    bool qvalid[QG];
    uint4 qf[QG][NS];
    float qn[QG], thr[QG], published[QG];
    int ccnt[QG];  // candidates this lane half kept, per query
#pragma unroll
    for (int g = 0; g < QG; g++) {
        jl[g] = (wave * QG + g) * 32 + j;
        q[g] = (int64_t)qt * BM + jl[g];
        qvalid[g] = q[g] < a.nq;
        const unsigned char* qrow = reinterpret_cast<const unsigned char*>(a.test) +
                                    (qvalid[g] ? q[g] : 0) * (int64_t)a.ld_q * EB;
#pragma unroll
        for (int s = 0; s < NS; s++)
            qf[g][s] = qvalid[g] ? *reinterpret_cast<const uint4*>(qrow + 32 * s + 16 * h)
                                 : make_uint4(0u, 0u, 0u, 0u);
        qn[g] = qvalid[g] ? a.qnorm[q[g]] : 0.0f;
        thr[g] = qvalid[g] ? o2f(a.gthr[q[g]]) : -INF;
        published[g] = thr[g];
        ccnt[g] = 0;
    }
    // a wave whose queries all lie past nq (the last query tile; a few-query call's seven other
    // waves) keeps the block's tile DMAs and barriers but runs no MFMAs or tests, so its SIMD
    // partner has the matrix pipe to itself
    bool any_q = false;
#pragma unroll
    for (int g = 0; g < QG; g++) any_q = any_q || qvalid[g];
    const bool wave_live = __ballot(any_q) != 0ull;
    float root = INF;  // (heap shapes, QG = 1) this query's heap root, mirrored in both lanes
    float qe2[QG], eq2[QG];  // 2 |q| and 2 |q - rq|, rounded up
#pragma unroll
    for (int g = 0; g < QG; g++) {
        qe2[g] = eq2[g] = 0.0f;
        if (qvalid[g]) {
            const float2 qs = a.qstat[q[g]];
            qe2[g] = 2.0f * qs.x * (1.0f + 0x1p-17f);
            eq2[g] = 2.0f * qs.y * (1.0f + 0x1p-17f);
        }
    }
    // Fast-test tile term (round 6, TFG): from the maxima over ALL tiles of the tile statistics
    // (a.tsmax = {max tn, max |t - rt|, max |rt|} over the train set's 64-row tiles) instead of
    // each tile's own: one threshold tfc per query group, rebuilt only when the threshold moves
    // (make_tfb) -- no header read and two FMAs per group and tile.  The maxima bound every
    // tile's, so the test passes a superset of what the per-tile test passed (the 2^-18 slack
    // covers the reordered additions); the slow path still bounds L, U with the tile's own
    // statistics, read when it runs (the tile's buffer is not rewritten before the next group's
    // DMA: PAIR shapes, AHEAD = GRP).  On uniform rows the tile maxima vary by a few 1e-4 of the
    // band.  The two-buffer shapes keep the per-tile term (round 5).
    constexpr bool TFG = PAIR;
    float tk[QG], tfc[QG];  // (TFG) the tile term and the fast-test threshold, per query group
    [[maybe_unused]] int tic[QG];  // (I8) the integer fast-test threshold of tfc
    if constexpr (TFG) {
        const float4 smax = *a.tsmax;
#pragma unroll
        for (int g = 0; g < QG; g++) {
            tk[g] = fmaf(coef + 0x1p-18f, smax.x, fmaf(qe2[g], smax.y, eq2[g] * smax.z));
            if constexpr (I8) tk[g] += smax.w * (1.0f + 0x1p-20f);  // nu: the integer norm terms' residual
        }
    }
    float tfb[QG];     // tf without the tile term
    auto make_tfb = [&](int g) __attribute__((always_inline)) {
        tfb[g] = qvalid[g] ? ((thr[g] - qn[g]) + fmaf(coef, qn[g], eta)) + 0x1p-18f * (fabsf(thr[g]) + qn[g]) : -INF;
        if constexpr (TFG) tfc[g] = tfb[g] + tk[g];
        if constexpr (I8) tic[g] = knn_i8_fast_thr(tfc[g], s2);
    };
#pragma unroll
    for (int g = 0; g < QG; g++) make_tfb(g);
    // tile term: tq = {the tile's maximum norm tmax, the operand-rounding bound of this query
    // against the tile's rows, 2 (|q| max|t - rt| + |q - rq| max|rt|) (1 + 2^-17)}
    auto tf_of = [&](int g, float2 tq) __attribute__((always_inline)) {
        return fmaf(coef + 0x1p-18f, tq.x, tfb[g]) + tq.y;
    };
    // the tile's statistics, from its LDS image (the header's last slot, fp32): one broadcast
    // read, in order with the fragment reads -- no scalar memory load in the loop
    struct TQ { float2 v[QG]; };
    auto tile_q = [&](int buf) __attribute__((always_inline)) -> TQ {
        const float4 w = *reinterpret_cast<const float4*>(tiles + buf * TILE + HDR + 4 * BN);
        TQ r;
#pragma unroll
        for (int g = 0; g < QG; g++) r.v[g] = make_float2(w.x, fmaf(qe2[g], w.y, eq2[g] * w.z));
        if constexpr (I8) {  // the tile's nu joins the band
            const float nu = *reinterpret_cast<const float*>(tiles + buf * TILE + HDR + 4 * BN + 12) * (1.0f + 0x1p-20f);
#pragma unroll
            for (int g = 0; g < QG; g++) r.v[g].y += nu;
        }
        return r;
    };

    // tiles of the piece, rounded up to an even count: the scan loop below runs tiles in twos
    // with no exit between them, so only accB is live out of it (with an odd tail the compiler
    // copies both accumulator sets -- 32 v_mov -- at every back edge).  The extra tile reads the
    // next BN rows (another piece's, or the padding the train tile blocks carry past the
    // 64-row grid, run_gemm), which the row_end test rejects.
    // (quads / octets: a multiple of four / eight -- the loop runs whole groups, so every tile's
    // place in its group is a compile-time constant; up to 7 extra 32-row tiles, within the 256
    // pad rows past the train grid, run_gemm)
    constexpr int TSTEP = GRP > 2 ? GRP : 2;
    const int ntiles = fused_piece_tiles(row_end - row_begin, BN, GRP);
    static_assert(TSTEP == (GRP > 2 ? GRP : 2), "fused_piece_tiles");
    // Scan order (a.cursor set: the host does so for the multi-segment schedule): the piece's
    // tiles rotated to start where this XCD's other blocks are (per XCD: the 64-row unit the last
    // block to publish was at, if inside this piece) -- so the blocks one XCD runs at once
    // stream the same rows through its L2 instead of drifting apart (blocks are dispatched to
    // the XCDs round-robin).  Correctness does not depend on the order: every tile is scanned
    // once and the threshold logic is order-free.
    // All waves of the block must use the same order (they DMA pieces of the same tiles): thread
    // 0 reads the cursor and hands the rotation to the others through LDS (blk_rot, written
    // before the block barrier below, read after it).
    const int xcd = blockIdx.x & 7;
    int* blk_rot = reinterpret_cast<int*>(smem + NBUF * TILE + (RL ? 0 : BM * hs * (int)sizeof(float)));
    if (threadIdx.x == 0) {
        // (the schedule's rotation, knn_fused_range_piece: whole barrier groups, so a tile keeps
        // its place in its group)
        int r0 = fused_rot_tiles(rot_units, BN, GRP, ntiles);
        if (a.cursor && ntiles > 0) {
            const int64_t cu =
                (int64_t)__hip_atomic_load(&a.cursor[xcd], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) * 64;
            if (cu > row_begin && cu < row_end) r0 = (int)((cu - row_begin) / BN);
        }
        *blk_rot = r0;
    }
    int rot = 0;  // (set after the barrier)
    // (PARK) this thread's slots: quarter v of slot s at park_v + (4 s + v) 16 NT, the word at
    // park_w + s 4 NT; pcnt: the records it holds, in slots 0 .. pcnt - 1 (a flush takes them all)
    constexpr int PR = FUSED_PARK_SLOTS;
    [[maybe_unused]] unsigned char* park_v = smem + fused_park_off(NBUF * TILE, 64 * NW, (int)threadIdx.x, 0, 0);
    [[maybe_unused]] unsigned char* park_w = smem + fused_park_off(NBUF * TILE, 64 * NW, (int)threadIdx.x, 0, 4);
    [[maybe_unused]] int pcnt = 0;
    // the first row of logical tile t (t < ntiles): physical tile (t + rot) mod ntiles
    auto tile_row = [&](int t) __attribute__((always_inline)) -> int64_t {
        int pt = t + rot;
        pt = pt >= ntiles ? pt - ntiles : pt;
        return row_begin + (int64_t)pt * BN;
    };

    // ---- LDS-DMA of tiles (same image as k_gemm_filter: slot P -> row P / SLOTS, slot P % SLOTS,
    // the pad slot duplicates slot 0; rows past row_end are read (padding or the next piece's
    // rows) and rejected by index).  Every tile is whole: the train tile blocks are padded to
    // the 64-row grid (run_gemm), so a piece is always the scalar tile base + this lane's fixed
    // offset -- no per-tile address arithmetic in VGPRs.
    // (piece ins = wave + NW i: fused_dma_piece.  Rotating the DMA_INS % NW remainder pieces
    // between the waves measured no faster -- between the two waves of a pair on the round-3
    // kernel, r03r; with the tile's index over all eight waves on this one)
    constexpr int DMA_FULL = DMA_INS / NW;
    uint32_t doff[DMA_PER_WAVE];
#pragma unroll
    for (int i = 0; i < DMA_PER_WAVE; i++) {
        doff[i] = fused_dma_src_off(fused_dma_piece(NW, wave, i) * 64 + lane, BN, RB, HS, ldb);
    }
    const uint32_t lds_tiles = __builtin_amdgcn_readfirstlane(lds_addr(tiles));
    struct DmaTile { const unsigned char* src; uint32_t lds; };
    // the source of a tile: its block in the train operand (the piece's first row is a multiple
    // of 64, BN divides 64)
    const unsigned char* piece_src = trainb + (row_begin / BN) * TB;
    auto dma_desc = [&](int buf, int t) -> DmaTile {  // logical tile t of the piece
        int pt = t + rot;
        pt = pt >= ntiles ? pt - ntiles : pt;
        return DmaTile{piece_src + (int64_t)pt * TB, lds_tiles + (uint32_t)(buf * TILE)};
    };
    // The last piece of a tile is issued whole: its lanes past the header re-read the header's
    // last slot into the buffer's slack (TILE = DMA_INS KiB), so no piece needs an exec mask.
    auto dma_piece = [&](int i, const DmaTile& d) __attribute__((always_inline)) {
        const int ins = fused_dma_piece(NW, wave, i);
        if (i < DMA_FULL || ins < DMA_INS) dma16s(doff[i], d.src, d.lds + (uint32_t)ins * 1024u);
    };
    // piece i goes out in k-step (i NS) / DMA_PER_WAVE of the step
    auto dma_at = [&](int s, bool on, const DmaTile& d) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < DMA_PER_WAVE; i++)
            if (on && (i * NS) / DMA_PER_WAVE == s) dma_piece(i, d);
    };

    // ---- one tile's MFMAs into X; in between, the fast test of the previous tile (Y): a v_min3
    // chain per accumulator; returns bit 16c (x 0xffff) when some lane of accumulator c holds a
    // passing value (the slow path builds the value set, pass_set)
    constexpr int PF = FUSED_PF / NACC;  // k-steps of A fragments read ahead
    uint4 pa[PF], pb[PF];                // PAIR: the odd step's first fragments, read early
    auto prefetch = [&](int buf) __attribute__((always_inline)) {
        const unsigned char* tile = tiles + buf * TILE;
        const unsigned char* a0p = tile + fused_frag_off(j, h, 0, STRIDE);
        const unsigned char* a1p = tile + fused_frag_off((RG == 2 ? 32 : 0) + j, h, 0, STRIDE);
#pragma unroll
        for (int s = 0; s < PF && s < NS; s++) {
            pa[s] = *reinterpret_cast<const uint4*>(a0p + fused_frag_off(0, 0, s, STRIDE));
            if (RG == 2) pb[s] = *reinterpret_cast<const uint4*>(a1p + fused_frag_off(0, 0, s, STRIDE));
        }
    };
    auto step = [&](accx16 (&X)[NACC], accx16 (&Y)[NACC], int buf, bool dma_on, const DmaTile& dd,
                    const AccT (&tf)[QG], bool pre, AccT (&mn_out)[NACC]) -> uint32_t {
        const unsigned char* tile = tiles + buf * TILE;
        const unsigned char* a0p = tile + fused_frag_off(j, h, 0, STRIDE);
        const unsigned char* a1p = tile + fused_frag_off((RG == 2 ? 32 : 0) + j, h, 0, STRIDE);
        // each accumulator's chain starts from its rows' norms: register r of row group rg is row
        // 32 rg + (r & 3) + 8 (r >> 2) + 4h (four broadcast ds_read_b128 per row group; the QG
        // accumulators of a row group share them as the first MFMA's C operand)
        // (the norms land in row group rg's query-group-0 accumulator X[rg]; at k-step 0 the other
        // query groups' MFMAs take them as their C operand first, then X[rg]'s own -- no copy)
#pragma unroll
        for (int rg = 0; rg < RG; rg++) {
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++) {
                const accx4 v = *reinterpret_cast<const accx4*>(tile + fused_norm_off(HDR, h, rg, g4));
                X[rg][4 * g4] = v.x;
                X[rg][4 * g4 + 1] = v.y;
                X[rg][4 * g4 + 2] = v.z;
                X[rg][4 * g4 + 3] = v.w;
            }
        }
        // (I8: the running maximum -- the test is max_r a_r >= ti)
        AccT mn[NACC];
#pragma unroll
        for (int c = 0; c < NACC; c++) {
            if constexpr (I8) mn[c] = (int)0x80000000u;
            else mn[c] = INF;
        }
        uint4 xa[NS], xb[NS];
#pragma unroll
        for (int s = 0; s < PF && s < NS; s++) {
            if (pre) {
                xa[s] = pa[s];
                if (RG == 2) xb[s] = pb[s];
            } else {
                xa[s] = *reinterpret_cast<const uint4*>(a0p + fused_frag_off(0, 0, s, STRIDE));
                if (RG == 2) xb[s] = *reinterpret_cast<const uint4*>(a1p + fused_frag_off(0, 0, s, STRIDE));
            }
        }
#pragma unroll
        for (int s = 0; s < NS; s++) {
            dma_at(s, dma_on, dd);
            if (s + PF < NS) {
                xa[s + PF] = *reinterpret_cast<const uint4*>(a0p + fused_frag_off(0, 0, s + PF, STRIDE));
                if (RG == 2) xb[s + PF] = *reinterpret_cast<const uint4*>(a1p + fused_frag_off(0, 0, s + PF, STRIDE));
            }
#pragma unroll
            for (int cc = 0; cc < NACC; cc++) {
                const int c = s == 0 ? NACC - 1 - cc : cc;  // (k-step 0: query group 0 last)
                const int rg = c % RG, g = c / RG;
                if constexpr (I8) {
                    const intx4 A = __builtin_bit_cast(intx4, (RG == 2 && rg) ? xb[s] : xa[s]);
                    X[c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A, __builtin_bit_cast(intx4, qf[g][s]),
                                                                 s == 0 ? X[rg] : X[c], 0, 0, 0);
                } else {
                    const bf16x8 A = __builtin_bit_cast(bf16x8, (RG == 2 && rg) ? xb[s] : xa[s]);
                    X[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, __builtin_bit_cast(bf16x8, qf[g][s]),
                                                                   s == 0 ? X[rg] : X[c], 0, 0, 0);
                }
#pragma unroll
                for (int v = s * VPS; v < (s + 1) * VPS && v < 16; v++) {
                    if constexpr (I8) mn[c] = max(mn[c], Y[c][v]);
                    else mn[c] = fminf(mn[c], Y[c][v]);
                }
                // computed here, beside this k-step's MFMAs: without the opaque use the
                // compiler sinks the whole v_min3 chain into the last k-step, where it
                // runs exposed after the final MFMA
                if (s * VPS < 16) asm volatile("" : "+v"(mn[c]));
            }
        }
        // which accumulators hold a passing value; the slow path builds their value sets
        // (pass_set) -- usually one of the two
        uint32_t u = 0u;
#pragma unroll
        for (int c = 0; c < NACC; c++)
            u |= __ballot(I8 ? mn[c] >= tf[c / RG] : mn[c] <= tf[c / RG]) != 0ull ? (0xffffu << (16 * c)) : 0u;
#pragma unroll
        for (int c = 0; c < NACC; c++) mn_out[c] = mn[c];
        return u;
    };

    // append candidate (L, U) of global row t to query group g's sub-slice of this lane half
    // (past its capacity: counted only, the rescore then sends the query to the exact scan)
    auto store_cand32 = [&](int g, float L, float U, int32_t t) __attribute__((always_inline)) {
        if (ccnt[g] < cap_sub) {
            const int64_t o = q[g] * (int64_t)a.cap + (int64_t)(2 * seg + h) * cap_sub + ccnt[g];
            a.cand[o] = CandRec{t, L, U};
        }
        ccnt[g]++;
    };
    auto store_cand = [&](int g, float L, float U, int64_t t) __attribute__((always_inline)) {
        store_cand32(g, L, U, (int32_t)t);
    };
    // (heap shapes, QG = 1) keep candidate (L, U) of global row t: the exact test against the
    // current threshold, the candidate store into this lane half's sub-slice, and, if U beats
    // the heap root, a sift-down of the query's 4-ary max-heap (node n >= 1 in H[n-1], the root
    // in H[hs-1]: the four children of node i are one aligned 16-byte read at H[4i]).  Only one
    // lane of a query runs it at a time.
    auto accept = [&](float L, float U, int64_t t) __attribute__((always_inline)) {
        if (!(L <= thr[0])) return;
        store_cand(0, L, U, t);
        if (U < root) {
            float* H = topU + jl[0] * hs;
            int i = 0;
            float newroot = U;
            for (;;) {
                if (4 * i + 1 > k - 1) break;
                const float4 cc = *reinterpret_cast<const float4*>(H + 4 * i);
                const float cm = fmaxf(fmaxf(cc.x, cc.y), fmaxf(cc.z, cc.w));
                if (cm <= U) break;
                const int ci = cm == cc.x ? 0 : cm == cc.y ? 1 : cm == cc.z ? 2 : 3;
                H[i == 0 ? hs - 1 : i - 1] = cm;
                if (i == 0) newroot = cm;
                i = 4 * i + 1 + ci;
            }
            H[i == 0 ? hs - 1 : i - 1] = U;
            root = newroot;
            thr[0] = fminf(thr[0], root);
        }
    };
    auto sync_roots = [&](int hh) __attribute__((always_inline)) {
        const float other = __shfl_xor(root, 32);
        if (h != hh) root = other;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    auto publish = [&]() __attribute__((always_inline)) {  // (heap shapes)
        if (qvalid[0]) {
            thr[0] = fminf(thr[0], root);
            if (a.nseg > 1 && h == 0 && thr[0] < published[0]) {
                atomicMin(&a.gthr[q[0]], f2o(thr[0]));
                published[0] = thr[0];
            }
            make_tfb(0);
        }
    };
    // certified bounds L <= D <= U of value y of query group g against tile stats tq: Delta =
    // coef (qn + tmax) + eta + rho -- the tile's maximum norm tmax >= the row's norm, a slightly
    // wider band (still L <= D <= U) for no per-value norm read
    // (I8: y is the integer a, G = qn - s2 float(a); the conversion, the fma's rounding and s2's own
    // are inside coef, and the tile's nu is in tq.y)
    auto bounds = [&](int g, auto y, float2 tq, float& L, float& U) __attribute__((always_inline)) {
        float G;
        if constexpr (I8) G = fmaf(-s2, (float)y, qn[g]);
        else G = qn[g] + y;
        const float dl = fmaf(coef, qn[g] + tq.x, eta) + tq.y;
        L = G - dl;
        U = G + dl;
    };

    // value v (wave-uniform) of accumulators Y: a scalar-indexed register read (v_movrels),
    // so the walk below is a runtime loop with one copy of its body -- a static walk over
    // the 16 NACC values replicates accept() per value, and the code no longer fits the
    // instruction cache (measured 10x slower on B)
    auto yval = [&](accx16 (&Y)[NACC], int v) __attribute__((always_inline)) -> float {
        if constexpr (NACC == 1) return Y[0][v & 15];
        else return (v >> 4) ? Y[1][v & 15] : Y[0][v & 15];
    };
    // (heap shapes) the values of Y some lane passes (bit 16c + r), for the accumulators set in
    // acc: per group of 4 values (rows 8g .. 8g+3 of the lane half) one ballot of their minimum,
    // then one v_cmp + ballot per value of the passing groups only
    auto pass_set = [&](accx16 (&Y)[NACC], float tf, uint32_t acc) __attribute__((always_inline)) -> uint32_t {
        uint32_t u = 0u;
#pragma unroll
        for (int c = 0; c < NACC; c++)
            if ((acc >> (16 * c)) & 1u) {  // (wave-uniform) only the accumulators that pass
#pragma unroll
                for (int g4 = 0; g4 < 4; g4++) {
                    const float gm = fminf(fminf(Y[c][4 * g4], Y[c][4 * g4 + 1]), fminf(Y[c][4 * g4 + 2], Y[c][4 * g4 + 3]));
                    if (__ballot(gm <= tf)) {
#pragma unroll
                        for (int r = 4 * g4; r < 4 * g4 + 4; r++)
                            u |= (__ballot(Y[c][r] <= tf) != 0ull ? 1u : 0u) << (16 * c + r);
                    }
                }
            }
        return u;
    };
    // immediate slow path (4-wave heap shapes): the passing values of tile tp, visited by
    // index; the two lanes of a query take turns (one heap writer at a time)
    auto slow = [&](accx16 (&Y)[NACC], int tp, float tf, float2 tq, uint32_t u) {
        const int64_t tbase = tile_row(tp);
        u = pass_set(Y, tf, u);
        while (u) {
            const int v = __builtin_ctz(u);
            u &= u - 1u;
            const float y = yval(Y, v);
            const bool p = y <= tf;
            const int r = v & 15;
            const int row = 32 * (v >> 4) + (r & 3) + 8 * (r >> 2) + 4 * h;
            const int64_t t = tbase + row;
#pragma unroll 1
            for (int hh = 0; hh < 2; hh++) {
                if (!__ballot(p && h == hh)) continue;
                if (p && h == hh && t < row_end) {
                    float L, U;
                    bounds(0, y, tq, L, U);
                    accept(L, U, t);
                }
                sync_roots(hh);
            }
        }
        publish();
    };

    // register-list slow path (KR > 0): the two lanes of a query (its two row halves) each keep
    // an ascending list lst[] of their own half's ceil(k/2) smallest U (k <= 16: KR = 8, LL = 8;
    // k <= 32: KR = 32, LL = 16; 32 < k <= 104: KR = 104, LL = 52; the first LL - ceil(k/2)
    // entries are -inf pads) and insert only their own values (LL v_med3); the bound is the
    // larger of the two halves' ceil(k/2)-th smallest -- at least 2 ceil(k/2) >= k kept rows
    // have U <= it.  A little looser than the exact k-th smallest, with no LDS heap and no lane
    // taking turns, for all queries of the wave at once.  (Until round 5, k <= 16 kept one exact
    // 16-entry list in both lanes, each inserting both lanes' values: 32 v_med3 and a lane swap
    // per insert; the halves keep ~20 % more candidates and measured A 20.05 -> 19.84 ms, its
    // 8-GPU share 3.05 -> 2.97 ms, same box, r05v.)  (QG = 2: one list per query group.)
    float lst[QG][RL ? LL : 1];
    if constexpr (RL) {
        const int pads = LL - (k + 1) / 2;
#pragma unroll
        for (int g = 0; g < QG; g++)
#pragma unroll
            for (int i = 0; i < LL; i++) lst[g][i] = i < pads ? -INF : INF;
    }
    // min as v_med3 against a -inf the compiler cannot see: with a literal -inf it folds the
    // med3 back into v_min_f32 and canonicalises both inputs (two more v_max per min)
    float ninf_op;
    asm("s_mov_b32 %0, 0xff800000" : "=s"(ninf_op));
    auto fmin_op = [&](float a, float b) __attribute__((always_inline)) {
        return __builtin_amdgcn_fmed3f(a, b, ninf_op);
    };
    auto list_insert = [&](int g, float w) __attribute__((always_inline)) {
#pragma unroll
        for (int i = LL - 1; i >= 1; i--) lst[g][i] = __builtin_amdgcn_fmed3f(lst[g][i - 1], w, lst[g][i]);
        lst[g][0] = fmin_op(lst[g][0], w);
    };
    // the other lane half's copy of a word (v_permlane32_swap: one of the swap's two results
    // is this lane's own word, the other its partner's)
    auto partner = [&](float x) __attribute__((always_inline)) -> float {
        return __uint_as_float(lane_xor(__float_as_uint(x), 32));
    };
    // Lane-parallel slow path.  Passes are sparse (A: a wave-tile has one in about 8 tiles,
    // usually one query, one value), so instead of visiting the passing positions one
    // wave-wide step at a time, every lane takes ITS OWN passing values, one per round, all
    // lanes at once: one scan of the lane's 16 values of a passing accumulator yields its
    // passing set (a 16-bit mask) and the value of the lowest passing index; later rounds take
    // the next set bit; fn(c, idx, y) then handles every lane's candidate together
    // (idx < 0: none).  Rounds = the most passing values of one lane in the accumulator (1
    // unless the threshold is still loose).  Any processing order keeps every true neighbour:
    // a row is kept iff L <= the threshold at its turn, and the threshold is always the k-th
    // smallest U of kept rows.
    auto lane_rounds = [&](accx16 (&Y)[NACC], const AccT (&tf)[QG], const AccT (&mnY)[NACC], uint32_t u,
                           auto&& fn) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < NACC; c++) {
            if (!((u >> (16 * c)) & 1u)) continue;  // (wave-uniform) no lane passes in c
            const AccT tfc = tf[c / RG];
            // round 1, one scan of the lane's 16 values from r = 15 down to 0: the passing set as
            // a 16-bit mask m = 2m + (y_r <= tf) (v_addc_co_u32 with the compare's VCC as
            // carry-in) and the value of the LOWEST passing index (v_cndmask on the same VCC) --
            // three VALU per value in one asm block (no hazard padding between values), no SGPR
            // mask pairs held.  The lowest passing index is ffs(m) - 1 and "passes twice" is
            // m & (m - 1); later rounds take the next lowest set bit.  Same box (r05n) against the
            // compiler's scan (compare + index, value and count selects: ~4.5 VALU per value):
            // A filter 19.94 -> 19.55 ms, B 465.3 -> 456.7, C1 1683.6 -> 1643.6.
            // (Scanning the highest passing group of four, found by the group minima, measured
            // 4-8 % slower: r03q; the count from the compares' wave masks by scalar ops, 2.7 %
            // slower on B: r03s.)
            uint32_t m = 0u;
            AccT yv = I8 ? (AccT)0 : (AccT)INF;
            int idx;
            auto pick = [](uint32_t mm) __attribute__((always_inline)) { return __ffs((int)mm) - 1; };  // lowest set bit
            if constexpr (KR <= 32) {
                // k <= 32 (lists of 16): the value is the fast test's minimum -- a lane with ONE
                // passing value passes with its minimum, so the scan only builds the passing mask
                // (compare + add-with-carry, 2 VALU per value); only when some lane passes twice, a
                // second mask of the positions equal to the minimum picks its index.  Same box (r05p):
                // A filter 20.07 -> 19.85 ms, B 466.7 -> 463.3; C1 (k = 100: more lanes pass twice,
                // each paying the second mask) 1677 -> 1687, so KR = 104 keeps the value scan
                if constexpr (I8) asm volatile(KNN_FUSED_SCAN16("v_cmp_ge_i32_e32") : "+v"(m) : "v"(tfc), KNN_FUSED_SCAN16_Y(Y[c]) : "vcc");
                else asm volatile(KNN_FUSED_SCAN16("v_cmp_le_f32_e32") : "+v"(m) : "v"(tfc), KNN_FUSED_SCAN16_Y(Y[c]) : "vcc");
                yv = mnY[c];
                if (__ballot((m & (m - 1u)) != 0u)) {
                    uint32_t e = 0u;
                    if constexpr (I8) asm volatile(KNN_FUSED_SCAN16("v_cmp_eq_i32_e32") : "+v"(e) : "v"(yv), KNN_FUSED_SCAN16_Y(Y[c]) : "vcc");
                    else asm volatile(KNN_FUSED_SCAN16("v_cmp_eq_f32_e32") : "+v"(e) : "v"(yv), KNN_FUSED_SCAN16_Y(Y[c]) : "vcc");
                    idx = pick(m & e);
                } else {
                    idx = pick(m);
                }
            } else {
                asm volatile("v_cmp_le_f32_e32 vcc, %18, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %18, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             "v_cmp_le_f32_e32 vcc, %17, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %17, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             "v_cmp_le_f32_e32 vcc, %16, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %16, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             "v_cmp_le_f32_e32 vcc, %15, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %15, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             "v_cmp_le_f32_e32 vcc, %14, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %14, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             "v_cmp_le_f32_e32 vcc, %13, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %13, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             "v_cmp_le_f32_e32 vcc, %12, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %12, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             "v_cmp_le_f32_e32 vcc, %11, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %11, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             "v_cmp_le_f32_e32 vcc, %10, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %10, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             "v_cmp_le_f32_e32 vcc, %9, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %9, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             "v_cmp_le_f32_e32 vcc, %8, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %8, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             "v_cmp_le_f32_e32 vcc, %7, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %7, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             "v_cmp_le_f32_e32 vcc, %6, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %6, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             "v_cmp_le_f32_e32 vcc, %5, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %5, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             "v_cmp_le_f32_e32 vcc, %4, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %4, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             "v_cmp_le_f32_e32 vcc, %3, %2\n\t"
                             "v_cndmask_b32_e32 %1, %1, %3, vcc\n\t"
                             "v_addc_co_u32_e32 %0, vcc, %0, %0, vcc\n\t"
                             : "+v"(m), "+v"(yv)
                             : "v"(tfc), "v"(Y[c][0]), "v"(Y[c][1]), "v"(Y[c][2]), "v"(Y[c][3]), "v"(Y[c][4]), "v"(Y[c][5]), "v"(Y[c][6]), "v"(Y[c][7]), "v"(Y[c][8]), "v"(Y[c][9]), "v"(Y[c][10]), "v"(Y[c][11]), "v"(Y[c][12]), "v"(Y[c][13]), "v"(Y[c][14]), "v"(Y[c][15])
                             : "vcc");
                idx = pick(m);  // -1 when nothing passes
            }
            fn(c, idx, yv);
            if (__ballot((m & (m - 1u)) != 0u)) {
                m = idx >= 0 ? m ^ (1u << idx) : 0u;
#pragma unroll 1
                for (int round = 1; round < 16; round++) {
                    if (!__ballot(m != 0u)) break;
                    idx = pick(m);
                    yv = I8 ? (AccT)0 : (AccT)INF;
                    // the value at idx: compare + select per value in one asm block (the
                    // compiler's form pads each pair with a hazard s_nop)
                    asm volatile("v_cmp_eq_u32_e32 vcc, 0, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %2, vcc\n\t"
                                 "v_cmp_eq_u32_e32 vcc, 1, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %3, vcc\n\t"
                                 "v_cmp_eq_u32_e32 vcc, 2, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %4, vcc\n\t"
                                 "v_cmp_eq_u32_e32 vcc, 3, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %5, vcc\n\t"
                                 "v_cmp_eq_u32_e32 vcc, 4, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %6, vcc\n\t"
                                 "v_cmp_eq_u32_e32 vcc, 5, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %7, vcc\n\t"
                                 "v_cmp_eq_u32_e32 vcc, 6, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %8, vcc\n\t"
                                 "v_cmp_eq_u32_e32 vcc, 7, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %9, vcc\n\t"
                                 "v_cmp_eq_u32_e32 vcc, 8, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %10, vcc\n\t"
                                 "v_cmp_eq_u32_e32 vcc, 9, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %11, vcc\n\t"
                                 "v_cmp_eq_u32_e32 vcc, 10, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %12, vcc\n\t"
                                 "v_cmp_eq_u32_e32 vcc, 11, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %13, vcc\n\t"
                                 "v_cmp_eq_u32_e32 vcc, 12, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %14, vcc\n\t"
                                 "v_cmp_eq_u32_e32 vcc, 13, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %15, vcc\n\t"
                                 "v_cmp_eq_u32_e32 vcc, 14, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %16, vcc\n\t"
                                 "v_cmp_eq_u32_e32 vcc, 15, %1\n\t"
                                 "v_cndmask_b32_e32 %0, %0, %17, vcc\n\t"
                                 : "+v"(yv)
                                 : "v"(idx), "v"(Y[c][0]), "v"(Y[c][1]), "v"(Y[c][2]), "v"(Y[c][3]), "v"(Y[c][4]), "v"(Y[c][5]), "v"(Y[c][6]), "v"(Y[c][7]), "v"(Y[c][8]), "v"(Y[c][9]), "v"(Y[c][10]), "v"(Y[c][11]), "v"(Y[c][12]), "v"(Y[c][13]), "v"(Y[c][14]), "v"(Y[c][15])
                                 : "vcc");
                    fn(c, idx, yv);
                    m = idx >= 0 ? m ^ (1u << idx) : 0u;
                }
            }
        }
    };
    // a kept row into this lane's list and candidate sub-slice (register lists).  (Round 6: these
    // inserts deferred -- kept rows queued two per lane, flushed for all lanes together every
    // 16 / 64 tiles or when a queue filled -- measured A 19.59 -> 19.98 / 19.65 ms, B 469.8 ->
    // 471.2, A's 8-GPU share equal, same box, r06l: the sparse late visits' cost is the lane
    // scan and its latency, not the insert)
    auto keep_row = [&](int g, bool keep, float L, float U, int64_t t) __attribute__((always_inline)) {
        if constexpr (RL) {
            if (keep) store_cand(g, L, U, t);
            const float w = (keep && U < lst[g][LL - 1]) ? U : INF;
            if (__ballot(w < INF)) {
                list_insert(g, w);
                thr[g] = fmin_op(thr[g], __builtin_amdgcn_fmed3f(lst[g][LL - 1], partner(lst[g][LL - 1]), INF));
            }
        }
    };
    auto slow_rl = [&](accx16 (&Y)[NACC], int tp, const AccT (&tf)[QG], const TQ& tq, const AccT (&mnY)[NACC],
                       uint32_t u) {
        if constexpr (RL) {
            const int64_t tbase = tile_row(tp);
            // (the band's half-width hoisted per tile and 32-bit row compares measured no faster:
            // r05q)
            auto visit = [&](int c, int idx, AccT yv) __attribute__((always_inline)) {
                const int g = c / RG;
                const int row = 32 * (c % RG) + (idx & 3) + 8 * (idx >> 2) + 4 * h;
                const int64_t t = tbase + row;
                float L, U;
                bounds(g, yv, tq.v[g], L, U);
                keep_row(g, idx >= 0 && t < row_end && L <= thr[g], L, U, t);
            };
            lane_rounds(Y, tf, mnY, u, visit);
#pragma unroll
            for (int g = 0; g < QG; g++) make_tfb(g);
        }
    };

    // ---- parked passes (PARK).  park(): after a fast test with passing lanes.  When every
    // passing lane has a free slot for each of its passing accumulators, those lanes write their
    // records -- the accumulator's 16 values and the word 2 (logical tile) + accumulator -- under
    // their exec mask and the tile is done for now (returns true); else nothing is written and
    // the caller takes the immediate path.  A slot index is pcnt masked to the ring, and pcnt < PR
    // holds wherever a record is written, so no store leaves the thread's own slots.
    auto park = [&](accx16 (&Y)[NACC], int tp, const AccT (&tf)[QG], const AccT (&mnY)[NACC]) __attribute__((always_inline)) -> bool {
        if constexpr (PARK) {
            bool ps[NACC];
            int need = 0;
#pragma unroll
            for (int c = 0; c < NACC; c++) {
                ps[c] = mnY[c] >= tf[c / RG];
                need += ps[c] ? 1 : 0;
            }
            if (__ballot(pcnt + need > PR)) return false;
#pragma unroll
            for (int c = 0; c < NACC; c++) {
                if (ps[c]) {
                    const int s = pcnt & (PR - 1);
                    unsigned char* pv = park_v + s * (4 * 16 * NT);
#pragma unroll
                    for (int v = 0; v < 4; v++)
                        *reinterpret_cast<int4*>(pv + v * (16 * NT)) =
                            make_int4(Y[c][4 * v], Y[c][4 * v + 1], Y[c][4 * v + 2], Y[c][4 * v + 3]);
                    *reinterpret_cast<int*>(park_w + s * (4 * NT)) = 2 * tp + c;
                    pcnt++;
                }
            }
            return true;
        }
        return false;
    };
    // flush_ring(): every lane's records, oldest first, one slot per round for all lanes at once.
    // The 16 values are scanned again against the CURRENT fast-test threshold (it only tightens;
    // any processing order keeps every true neighbour, lane_rounds), then bounds, row_end test,
    // candidate store and list insert as slow_rl's visit.  The tile's statistics for the bounds
    // come from its header in the train operand (its LDS buffer may be overwritten by now): the
    // words tile_q reads, so L and U are the immediate path's bits.  make_tfb once per query group
    // at the end.  Called at two places only (the share tile's place and the end of the piece),
    // so the code of the other tile places holds no copy.
    auto flush_ring = [&](const unsigned char* piece_base) __attribute__((always_inline)) {
        if constexpr (PARK) {
            if (!__ballot(pcnt > 0)) return;
            uint32_t nrec = 0;
#pragma unroll 1
            for (int s = 0; s < PR; s++) {
                const bool have = pcnt > s;
                const uint64_t hm = __ballot(have);
                if (!hm) break;
                nrec += (uint32_t)__popcll(hm);
                accx16 V = accx16{};
                int w = 0;
                float4 st = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (have) {
                    w = *reinterpret_cast<const int*>(park_w + s * (4 * NT));
                    int pt = (w >> 1) + rot;
                    pt = pt >= ntiles ? pt - ntiles : pt;
                    st = *reinterpret_cast<const float4*>(piece_base + (int64_t)pt * TB + BN * RB + 4 * BN);
                    const unsigned char* pv = park_v + s * (4 * 16 * NT);
#pragma unroll
                    for (int v = 0; v < 4; v++) {
                        const int4 x = *reinterpret_cast<const int4*>(pv + v * (16 * NT));
                        V[4 * v] = x.x; V[4 * v + 1] = x.y; V[4 * v + 2] = x.z; V[4 * v + 3] = x.w;
                    }
                }
                const int cl = w & 1;
                int ptl = (w >> 1) + rot;
                ptl = ptl >= ntiles ? ptl - ntiles : ptl;
                const int64_t tbase = row_begin + (int64_t)ptl * BN;
                AccT mx = V[0];
#pragma unroll
                for (int v = 1; v < 16; v++) mx = max(mx, V[v]);
                const float nu = st.w * (1.0f + 0x1p-20f);
#pragma unroll
                for (int g = 0; g < QG; g++) {
                    const bool act = have && cl / RG == g;
                    if (!__ballot(act)) continue;
                    const float2 tq = make_float2(st.x, fmaf(qe2[g], st.y, eq2[g] * st.z) + nu);  // (tile_q)
                    uint32_t m = 0u;
                    asm volatile(KNN_FUSED_SCAN16("v_cmp_ge_i32_e32") : "+v"(m) : "v"(tic[g]), KNN_FUSED_SCAN16_Y(V) : "vcc");
                    m = act ? m : 0u;
                    // (as lane_rounds, k <= 32: a lane with one passing value passes with its maximum)
                    AccT yv = mx;
                    int idx;
                    if (__ballot((m & (m - 1u)) != 0u)) {
                        uint32_t e = 0u;
                        asm volatile(KNN_FUSED_SCAN16("v_cmp_eq_i32_e32") : "+v"(e) : "v"(yv), KNN_FUSED_SCAN16_Y(V) : "vcc");
                        idx = __ffs((int)(m & e)) - 1;
                    } else {
                        idx = __ffs((int)m) - 1;
                    }
#pragma unroll 1
                    for (int round = 0; round < 16; round++) {
                        const int row = 32 * (cl % RG) + (idx & 3) + 8 * (idx >> 2) + 4 * h;
                        const int64_t t = tbase + row;
                        float L, U;
                        bounds(g, yv, tq, L, U);
                        keep_row(g, idx >= 0 && t < row_end && L <= thr[g], L, U, t);
                        m = idx >= 0 ? m & ~(1u << idx) : 0u;
                        if (!__ballot(m != 0u)) break;
                        idx = __ffs((int)m) - 1;
                        yv = 0;
#pragma unroll
                        for (int v = 0; v < 16; v++) yv = idx == v ? V[v] : yv;
                    }
                }
            }
            pcnt = 0;
#pragma unroll
            for (int g = 0; g < QG; g++) make_tfb(g);
            if (a.park_cnt && lane == 0) atomicAdd(a.park_cnt, (unsigned long long)nrec);
        }
    };

    // deferred slow path (8-wave heap shapes): passing values with L <= thr are queued -- (L,
    // U, row) in registers -- and flushed through accept() every FUSED_DEFER_EVERY tiles by all
    // waves together, or when some lane's queue is full.  A threshold waiting for the flush is
    // stale but still valid (it only ever tightens).  The queue is three register vectors read
    // with a wave-uniform index (v_movrels), so the flush is a runtime loop with one copy of
    // accept()
    constexpr int RQ = FUSED_RQ;
    typedef float qvecf __attribute__((ext_vector_type(RQ)));
    typedef int qveci __attribute__((ext_vector_type(RQ)));
    qvecf qL = qvecf{}, qU = qvecf{};
    qveci qT = qveci{};
    int qcnt = 0;
    auto flush = [&]() __attribute__((always_inline)) {
#pragma unroll 1
        for (int hh = 0; hh < 2; hh++) {
#pragma unroll 1
            for (int i = 0; i < RQ; i++) {
                const bool mine = h == hh && i < qcnt;
                if (!__ballot(mine)) break;
                if (mine) accept(qL[i], qU[i], (int64_t)qT[i]);
            }
            sync_roots(hh);
        }
        qcnt = 0;
        publish();
    };
    // (the heap shapes visit the passing positions wave-wide: per value only a queue append,
    // so the lane-parallel scan would cost more than it saves -- C1 259.8 vs 273.3 ms, r03p)
    auto record = [&](accx16 (&Y)[NACC], int tp, float tf, float2 tq, uint32_t u) {
        const int64_t tbase = tile_row(tp);
        u = pass_set(Y, tf, u);
        while (u) {
            const int v = __builtin_ctz(u);
            u &= u - 1u;
            const float y = yval(Y, v);
            const bool p = y <= tf;
            if (__ballot(p && qcnt >= RQ)) flush();
            const int r = v & 15;
            const int row = 32 * (v >> 4) + (r & 3) + 8 * (r >> 2) + 4 * h;
            const int64_t t = tbase + row;
            if (p && t < row_end) {
                float L, U;
                bounds(0, y, tq, L, U);
                if (L <= thr[0]) {
#pragma unroll
                    for (int i = 0; i < RQ; i++) {
                        qL[i] = i == qcnt ? L : qL[i];
                        qU[i] = i == qcnt ? U : qU[i];
                        qT[i] = i == qcnt ? (int)t : qT[i];
                    }
                    qcnt++;
                }
            }
        }
    };

    accx16 accA[NACC], accB[NACC];
#pragma unroll
    for (int c = 0; c < NACC; c++) accA[c] = accB[c] = accx16{};
    __syncthreads();  // LDS init is complete before any DMA lands; blk_rot is written
    rot = __builtin_amdgcn_readfirstlane(*blk_rot);
#pragma unroll
    for (int p = 0; p < AHEAD; p++)
        if (p < ntiles) {
            const DmaTile d0 = dma_desc(p, p);
#pragma unroll
            for (int i = 0; i < DMA_PER_WAVE; i++) dma_piece(i, d0);
        }
    constexpr bool DEFER = NW == 8 && !RL;
    // tile terms (max norm, rounding bound) of the tile in the pipeline (it) and of tile it-1
    TQ tm_prev;
#pragma unroll
    for (int g = 0; g < QG; g++) tm_prev.v[g] = make_float2(0.0f, 0.0f);
    // threshold exchanges between the pieces of a query (gthr): every FUSED_SHARE_EVERY tiles
    // (also after tiles 2, 4, ..., 32 measured no fewer kept rows and B 3 % slower: r04d)
    auto share_now = [&](int it) __attribute__((always_inline)) {
        return (it & (FUSED_SHARE_EVERY - 1)) == FUSED_SHARE_EVERY - 1;
    };
    // List exchange between the pieces of a query (register-list shapes, a.lshare): a piece's
    // own list holds the k smallest U of ITS rows only, so the k-th value other pieces publish
    // through gthr is the k-th best of 1/P of the rows -- with P pieces the threshold trails a
    // single scan's by a factor P in rank (A's 8-GPU share, P ~ 5: 599 kept rows per query
    // against 172).  At tiles 32, 64, 128, ... each piece publishes its list (pads as +inf) and
    // takes the k-th smallest U of the union of every piece's list: a valid bound, as the
    // pieces' rows are disjoint and every published value is the U of a kept row.  Any value
    // read may be stale or from a list being rewritten: a list only ever lowers its entries
    // position by position, so a stale mix counts no more rows below a bound than the current
    // list holds (a looser bound, never a wrong one).  Per lane half (its rows), the
    // bound the larger of the two halves' union values.
    auto list_share_now = [&](int it) __attribute__((always_inline)) {
        return (it >= FUSED_LIST_FIRST && ((it + 1) & it) == 0) || (it & (FUSED_LIST_EVERY - 1)) == FUSED_LIST_EVERY - 1;
    };
    auto exchange_lists = [&]() __attribute__((always_inline)) {
        if constexpr (RL) {
            const int W = a.lshare_w;
#pragma unroll
            for (int g = 0; g < QG; g++) {
                float* base = a.lshare + ((qvalid[g] ? q[g] : 0) * (int64_t)a.nseg) * W + LL * h;
                if (qvalid[g]) {
                    uint32_t* dst = reinterpret_cast<uint32_t*>(base + (int64_t)seg * W);
#pragma unroll
                    for (int i = 0; i < LL; i++)
                        __hip_atomic_store(dst + i, __float_as_uint(lst[g][i] == -INF ? INF : lst[g][i]), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                }
                float tmp[LL];
#pragma unroll
                for (int i = 0; i < LL; i++) tmp[i] = lst[g][i];
                // a published list: +inf at the pad positions [0, pads), then its real values
                // ascending (+inf where not filled yet) -- reading starts at the chunk holding the
                // first real value, and a chunk whose smallest value no lane can take ends it
                const int pads = LL - (k + 1) / 2;
                for (int p = 0; p < a.nseg; p++) {
                    if (p == seg) continue;
                    const uint32_t* src = reinterpret_cast<const uint32_t*>(base + (int64_t)p * W);
#pragma unroll 1
                    for (int i0 = pads & ~3; i0 < LL; i0 += 4) {
                        float w[4];
#pragma unroll
                        for (int i = 0; i < 4; i++)
                            w[i] = qvalid[g] ? __uint_as_float(__hip_atomic_load(src + i0 + i, __ATOMIC_RELAXED,
                                                                                 __HIP_MEMORY_SCOPE_AGENT))
                                             : INF;
                        const float wmin = fmin_fast(fmin_fast(w[0], w[1]), fmin_fast(w[2], w[3]));
                        if (!__ballot(wmin < tmp[LL - 1])) break;
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const float wi = w[i] < tmp[LL - 1] ? w[i] : INF;
#pragma unroll
                            for (int e = LL - 1; e >= 1; e--) tmp[e] = __builtin_amdgcn_fmed3f(tmp[e - 1], wi, tmp[e]);
                            tmp[0] = fmin_fast(tmp[0], wi);
                        }
                    }
                }
                const float ub = __builtin_amdgcn_fmed3f(tmp[LL - 1], partner(tmp[LL - 1]), INF);
                if (qvalid[g] && ub < thr[g]) {
                    thr[g] = ub;
                    make_tfb(g);
                }
            }
        }
    };
    // one tile of the scan; posc: the tile's place in its barrier group (it % GRP), static
    auto iter = [&](auto posc, accx16 (&X)[NACC], accx16 (&Y)[NACC], int it) {
        constexpr int POS = decltype(posc)::value;
        // (PARK) the parked records go through the slow path before the thresholds are exchanged:
        // share tiles and list exchanges all fall on a group's last place (tiles 31, 63, 127, ...)
        if constexpr (PARK && POS == GRP - 1) {
            if (share_now(it) || (QG == 1 && a.lshare && list_share_now(it))) flush_ring(piece_src);
        }
        if constexpr (RL && QG == 1 && KR <= 32) {
            if (a.lshare && list_share_now(it)) exchange_lists();
        }
        if (share_now(it)) {
            if (QG == 2 && a.pace) {  // (the host paces the 64-query shapes only)
                steps++;
                if (threadIdx.x == 0) fused_pace(a.pace + 2 * xcd, steps);
            }
            if (a.cursor && threadIdx.x == 0)
                __hip_atomic_store(&a.cursor[xcd], (uint32_t)(tile_row(it) >> 6), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            if (a.nseg > 1) {
#pragma unroll
                for (int g = 0; g < QG; g++) {
                    if (!qvalid[g]) continue;
                    if constexpr (RL) {  // publish this query's bound (the heap path does it per accept)
                        if (h == 0 && thr[g] < published[g]) {
                            atomicMin(&a.gthr[q[g]], f2o(thr[g]));
                            published[g] = thr[g];
                        }
                    }
                    // thresholds published by other segments of this query
                    const float gv = o2f(__hip_atomic_load(&a.gthr[q[g]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                    if (gv < thr[g]) { thr[g] = gv; make_tfb(g); }
                }
            }
        }
        // the tiles of this step (both of a pair) have landed -- every wave's pieces: each wave
        // waits for all of its own vector-memory ops, then the barrier -- and every wave is done
        // with the buffers the next DMAs overwrite
        if (POS == 0) wait_dma_barrier();
        // this tile's terms, for its fast test in the next iteration (the tile is resident:
        // landed before this step's barrier, not overwritten before the next one)
        TQ tm_cur;
        if constexpr (!TFG) tm_cur = tile_q(it % NBUF);
        // Tile DMAs: step it issues tile it + AHEAD's pieces between its MFMAs.  (Every tile of the
        // next group issued at once right after a group's barrier measured slower everywhere, r05d:
        // the barrier wait is the waves' slow-path skew, not the last DMA's latency.  DESIGN.md)
        const bool dma_on = it + AHEAD < ntiles;
        const DmaTile dd = dma_desc((it + AHEAD) % NBUF, it + AHEAD);
        AccT tf[QG];
#pragma unroll
        for (int g = 0; g < QG; g++) {
            if constexpr (I8) tf[g] = it > 0 ? tic[g] : 0x7fffffff;
            else tf[g] = it > 0 ? (TFG ? tfc[g] : tf_of(g, tm_prev.v[g])) : -INF;
        }
        AccT mnY[NACC];
        const uint32_t uY = step(X, Y, it % NBUF, dma_on, dd, tf, POS != 0, mnY);
        // PAIR: the pair's next tile is resident since its barrier -- its first fragments are
        // read now, so their latency hides under the slow path below
        if (POS != GRP - 1 && it + 1 < ntiles) prefetch((it + 1) % NBUF);
        if (uY && !park(Y, it - 1, tf, mnY)) {
            // (TFG: the previous tile's own statistics, for the bounds, from its buffer now)
            const TQ tq = TFG ? tile_q((it - 1) % NBUF) : tm_prev;
            if constexpr (RL) slow_rl(Y, it - 1, tf, tq, mnY, uY);
            else if constexpr (DEFER) record(Y, it - 1, tf[0], tq.v[0], uY);
            else slow(Y, it - 1, tf[0], tq.v[0], uY);
        }
        if constexpr (DEFER) {
            if ((it & (FUSED_DEFER_EVERY - 1)) == FUSED_DEFER_EVERY - 1 && __ballot(qcnt > 0)) flush();
        }
        if constexpr (!TFG) tm_prev = tm_cur;
    };
    typedef std::integral_constant<int, 0> P0;
    typedef std::integral_constant<int, 1 % GRP> P1;
    if (!wave_live) {
        // (no valid query) the same barriers, and this wave's pieces of every tile's DMA
        for (int it = 0; it < ntiles; it++) {
            if (it % GRP == 0) wait_dma_barrier();
            if (it + AHEAD < ntiles) {
                const DmaTile dd = dma_desc((it + AHEAD) % NBUF, it + AHEAD);
#pragma unroll
                for (int i = 0; i < DMA_PER_WAVE; i++) dma_piece(i, dd);
            }
        }
    } else if constexpr (GRP == 8) {  // octets (the 64-query shape's default)
        for (int it = 0; it < ntiles; it += 8) {
            iter(P0{}, accA, accB, it);
            iter(P1{}, accB, accA, it + 1);
            iter(std::integral_constant<int, 2>{}, accA, accB, it + 2);
            iter(std::integral_constant<int, 3>{}, accB, accA, it + 3);
            iter(std::integral_constant<int, 4>{}, accA, accB, it + 4);
            iter(std::integral_constant<int, 5>{}, accB, accA, it + 5);
            iter(std::integral_constant<int, 6>{}, accA, accB, it + 6);
            iter(std::integral_constant<int, 7>{}, accB, accA, it + 7);
        }
    } else if constexpr (GRP == 4) {
        for (int it = 0; it < ntiles; it += 4) {
            iter(P0{}, accA, accB, it);
            iter(P1{}, accB, accA, it + 1);
            iter(std::integral_constant<int, 2>{}, accA, accB, it + 2);
            iter(std::integral_constant<int, 3>{}, accB, accA, it + 3);
        }
    } else {
        for (int it = 0; it < ntiles; it += 2) {
            iter(P0{}, accA, accB, it);
            iter(P1{}, accB, accA, it + 1);
        }
    }
    if (ntiles > 0 && wave_live) {
        // drain: the last tile's accumulators (ntiles is even: accB)
        const int last = ntiles - 1;
        if constexpr (TFG) tm_prev = tile_q(last % NBUF);  // (no DMA since: the buffer holds it)
        AccT tf[QG];
#pragma unroll
        for (int g = 0; g < QG; g++) {
            if constexpr (I8) tf[g] = tic[g];
            else tf[g] = TFG ? tfc[g] : tf_of(g, tm_prev.v[g]);
        }
        if constexpr (RL) {
            AccT mnB[NACC];
#pragma unroll
            for (int c = 0; c < NACC; c++) {
                if constexpr (I8) mnB[c] = (int)0x80000000u;
                else mnB[c] = INF;
#pragma unroll
                for (int v = 0; v < 16; v++) {
                    if constexpr (I8) mnB[c] = max(mnB[c], accB[c][v]);
                    else mnB[c] = fminf(mnB[c], accB[c][v]);
                }
            }
            slow_rl(accB, last, tf, tm_prev, mnB, 0xffffffffu);
        } else {
            if (pass_set(accB, tf[0], 0xffffffffu)) {
                if constexpr (DEFER) record(accB, last, tf[0], tm_prev.v[0], 0xffffffffu);
                else slow(accB, last, tf[0], tm_prev.v[0], 0xffffffffu);
            }
        }
    }
    if constexpr (DEFER) {
        if (__ballot(qcnt > 0)) flush();
    }
    // (PARK) the records still parked: the ring is empty at every return
    if constexpr (PARK) flush_ring(piece_src);
    // the final bound of this piece, any segment count: k_rescore stages only the candidates
    // with L <= gthr (every value there is a k-th smallest U of kept rows, so >= the k-th
    // smallest U of all of them)
    if constexpr (!RL) {
        if (qvalid[0]) thr[0] = fminf(thr[0], root);
    }
#pragma unroll
    for (int g = 0; g < QG; g++)
        if (qvalid[g] && h == 0 && thr[g] < published[g]) atomicMin(&a.gthr[q[g]], f2o(thr[g]));
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int g = 0; g < QG; g++)
        if (qvalid[g]) a.cnt[(int64_t)(2 * seg + h) * a.nq + q[g]] = ccnt[g];
}

// One piece of a block's range [x, x1) of the balanced schedule's (query tile, 64-row unit)
// space, T units per query tile: units [t0, t1) of query tile ql, scanned from unit t0 + rot.
// A range runs from its END: the head of its later query tile first (from train row 0), then
// the tail of the earlier one.  At time tau every two-piece block is then at unit tau, and after
// its switch at tau + g, g = T - (x1 - x) the same for every block: two sweeps that stream the
// train rows together through the L2s and the Infinity Cache (in range order each block would
// start from its own row, all 260 MB of A's train operand in use at once, cycling through a
// 256 MiB cache).  A range inside ONE query
// tile (about 23 % of A's blocks) has t0 <= g: started at t0 it would be a private stream
// somewhere between the two sweeps, so it starts at unit g instead, beside the second sweep,
// and wraps to its first g - t0 units at the end (rot; the scan order is free, fused_piece).
struct FusedRangePiece { int64_t ql, t0, t1, rot; };
__host__ __device__ inline FusedRangePiece knn_fused_range_piece(int64_t x, int64_t x1, int64_t T, bool first) {
    FusedRangePiece p;
    p.ql = (x1 - 1) / T;
    p.t0 = (x > p.ql * T ? x : p.ql * T) - p.ql * T;
    p.t1 = x1 - p.ql * T;
    const int64_t g = T - (x1 - x);
    p.rot = first && x / T == (x1 - 1) / T && g > p.t0 && g < p.t1 ? g - p.t0 : 0;
    return p;
}

// The grid (knn_fused_schedule): blocks [0, p1) take one whole query tile each (qt = block,
// every train row) -- whole rounds of the resident blocks, all sweeping the train rows from
// row 0 together (one L2 stream per XCD); the remaining query tiles' (qtile, 64-row tile)
// work is one linear space of w2 units cut into g2 equal ranges, one per block [p1, p1+g2):
// a range covers the tail of one query tile and the head of the next (a piece each), so the
// last round of blocks ends together instead of a partial wave of whole query tiles.
// Pieces of one query tile share thresholds through gthr like segments (piece id = block -
// the first block of that query tile).  One call site of fused_piece (instruction cache).
template <int RB, int MINW, int NBUF, int NW, int QG, int RG, int KR, bool I8 = false, bool PARK = false>
__global__ __launch_bounds__(64 * NW, MINW) void k_gemm_fused(GemmFilterArgs a) {
    if ((a.gate && *a.gate == 0) || (*a.status & KNN_STATUS_GEMM_UNSAFE)) return;  // not taken / exact path
    const int64_t T = a.tiles64;  // 64-row units per query tile
    const int b = blockIdx.x;
    // g2 < 0: segment mode -- block = (segment b / n_qtiles, query tile b % n_qtiles), one piece
    const bool segmode = a.g2 < 0;
    const bool p1 = !segmode && b < a.p1_blocks;
    const int64_t b2 = b - a.p1_blocks;
    auto lo = [&](int64_t bb) { return bb * a.w2 / a.g2; };
    int64_t x = 0, x1 = 1;
    if (!segmode) {
        x = p1 ? (int64_t)b * T : lo(b2);
        x1 = p1 ? x + T : lo(b2 + 1);
    }
    const int qbase = p1 ? 0 : a.p1_blocks;
    // (a.pace) pacing steps of this block, over its pieces (thread 0's copy is the one used).  A
    // block joins at its XCD's current average: one that starts when others are far into
    // their ranges (a later round of blocks) must not hold them back.
    int steps = 0;
    // (b & 7: the XCD under round-robin dispatch over eight of them, as the scan cursor assumes;
    // the two words are read one after the other, not as a pair.  A wrong guess or a torn read
    // only costs the gain: the waits stay bounded and no result depends on them.)
    if (QG == 2 && a.pace && threadIdx.x == 0) {
        int32_t* p = a.pace + 2 * (b & 7);
        const int sum = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int n = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        steps = n > 0 && sum > 0 ? sum / n : 0;
        __hip_atomic_fetch_add(p, steps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(p + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // (the pieces of a range and their order: knn_fused_range_piece)
    for (bool first = true; x < x1; first = false) {
        int qt, seg;
        int64_t rb, re, adv, rot = 0;
        if (segmode) {
            qt = b % a.n_qtiles;
            seg = b / a.n_qtiles;
            rb = (int64_t)seg * a.seg_len;
            re = min(a.nt, rb + a.seg_len);
            adv = 1;
        } else {
            const FusedRangePiece p = knn_fused_range_piece(x, x1, T, first);
            const int64_t ql = p.ql, t0 = p.t0, t1 = p.t1;
            rot = p.rot;
            qt = qbase + (int)ql;
            // the block whose range holds the query tile's first unit: largest bb with lo(bb) <= ql T
            seg = p1 ? 0 : (int)(b2 - ((ql * T + 1) * a.g2 - 1) / a.w2);
            rb = t0 * 64;
            re = min(a.nt, t1 * 64);
            adv = t1 - t0;
        }
        if (!first) __syncthreads();  // every wave is done with the previous piece's LDS
        fused_piece<RB, NBUF, NW, QG, RG, KR, I8, PARK>(a, qt, seg, rb, re, rot, steps);
        if (segmode) x += adv;
        else x1 -= adv;
    }
    if (QG == 2 && a.pace && threadIdx.x == 0) {
        __hip_atomic_fetch_add(a.pace + 2 * (b & 7), -steps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(a.pace + 2 * (b & 7) + 1, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Balanced schedule (see k_gemm_fused): whole rounds of query tiles, the rest cut into g2 equal
// ranges of 64-row units (at least min(T, 256) units each).  Returns the grid and sets *nseg
// to the most pieces one query tile gets (its candidate sub-slices).
int knn_fused_schedule(GemmFilterArgs& a, int slots, int* nseg) {
    const int64_t T = (a.nt + 63) / 64;
    const int64_t nqt = a.n_qtiles;
    a.tiles64 = T;
    const int64_t R = nqt / slots, r = nqt - R * slots;
    a.p1_blocks = (int)(R * slots);
    *nseg = 1;
    if (r == 0) {
        a.g2 = 0;  // whole rounds only
        a.w2 = 0;
        return a.p1_blocks;
    }
    const int64_t W = r * T;
    const int64_t minp = std::min<int64_t>(T, 256);
    const int64_t g2 = std::max<int64_t>(1, std::min<int64_t>(slots, W / minp));
    a.g2 = (int)g2;
    a.w2 = W;
    auto blk = [&](int64_t xx) { return ((xx + 1) * g2 - 1) / W; };
    for (int64_t ql = 0; ql < r; ql++) *nseg = std::max<int>(*nseg, (int)(blk((ql + 1) * T - 1) - blk(ql * T) + 1));
    return a.p1_blocks + (int)g2;
}

// ---------------------------------------------------------------------------------
// plan and launch
// ---------------------------------------------------------------------------------
// (the int8 operand class's header has the bf16 form's slots: bn int32 words + the statistics)
static size_t fused_lds_of(int row_bytes, int k, int nw, int rg, int nbuf, bool heaps, int qg = 1, bool park = false) {
    const int bn = 32 * rg, bm = 32 * qg * nw;
    const int hs = bn / 4 + 1;  // (fused_piece: header slots)
    const int ins = (bn * (row_bytes / 16 + 1) + hs + 63) / 64;
    // (+ 16 bytes: the block's scan rotation, k_gemm_fused)
    // (+ the parked passes' ring, fused_park_off: past the rotation word)
    return (size_t)nbuf * ins * 1024 + (heaps ? (size_t)bm * heap_stride(k) * sizeof(float) : 0) + 16 +
           (park ? (size_t)fused_park_bytes(64 * nw) : 0);
}

int knn_fused_list_share_width(const FilterPlan& f) {
    if (!f.ls || !(f.kr == 8 || f.kr == 32)) return 0;
    return f.kr == 32 ? 32 : 16;  // (two lane halves' lists)
}

bool knn_fused_supported(int d) { return d == 64 || d == 128 || d == 256; }

// Shapes (d = features; rows of 2d bytes -- the accumulators start from the norms in the tile
// header: B, d = 64, 614 -> 586 ms against a norm k-step, r03q; int8 rows: d bytes).
// Block = NW waves x 32 QG queries; NBUF tile buffers, one barrier per NBUF / 2 tiles (NBUF = 2: per tile):
//  * k <= 32 (register lists, KR = 8 / 32), 8 waves:
//      d <= 128, many queries (below): 64 queries per wave on 32-row tiles, NBUF = 16 (octets)
//      d <= 128 otherwise:             32 per wave on 64-row tiles, NBUF = 8 (quads), list exchange
//      d = 256:                        32 per wave on 64-row tiles, NBUF = 4 (pairs: eight buffers
//                                      do not fit), list exchange
//    (pairs against two buffers: A 33.4 -> 31.3 ms, round 2; 8-wave blocks: B 765 -> 743 ms)
//  * d = 256, 32 < k <= 104 (KR = 104): 8 waves, 32 per wave on 32-row tiles, NBUF = 8 (quads).
//  * k > 32 otherwise (LDS heaps, KR = 0): d = 64 in 4-wave blocks on 64-row tiles, NBUF = 2, two
//    blocks per CU (the other block hides the per-tile barrier and fast test of 5-step tiles) while
//    two blocks' heaps fit; else 8-wave blocks: 64-row tiles with NBUF = 4 when they fit beside
//    the heaps, else NBUF = 2, else 32-row tiles with NBUF = 2, else no plan (nw = 0).
// Register lists, one per lane half: k <= 16 8 entries (KR = 8), k <= 32 16 (KR = 32: exact
// 32-entry lists cost a block per CU of occupancy and 9 % of time on B).
// The register-list tile groups above always fit: they hold no heaps, so their LDS does not
// depend on k (d = 128: 16 x 9 KiB and 8 x 18 KiB = 144 KiB; d = 256: 4 x 34 KiB = 136 KiB and
// 8 x 17 KiB).  k_gemm_fused is instantiated for exactly these (fused_fn_k).
FilterPlan knn_fused_plan(int d, int k, int64_t nq, int num_cus, const FusedForce& force, int max_pieces, bool i8) {
    // int8 operand rows (d bytes): d = 128, the register-list shapes
    if (i8 && (d != 128 || k > 32)) return FilterPlan{0, 0, 0, 0, 0, 0, 0};
    const int rb = i8 ? d : 2 * d;
    const size_t cap = 160 * 1024 - 256;  // room for the kernel's static LDS
    // d = 256, 32 < k <= 104 (C): per-half 52-entry register lists instead of LDS heaps, so
    // the tile buffers get the LDS the heaps held -- 32-row tiles in quads (one barrier per 128
    // rows) instead of one barrier per 32-row tile (force.heaps: the heap shape).  (64-row
    // tiles in pairs, the other way to the same barrier count, spill: two more accumulators.)
    const int kr = k <= 16 ? 8 : k <= 32 ? 32 : (k <= 104 && d == 256 && !force.heaps) ? 104 : 0;
    auto make = [&](int nw, int rg, int minw, int nbuf, int qg = 1) {
        // parked passes: the int8 register-list shapes (their half-size tiles leave the ring's
        // 68 KiB free); force.park = 0 keeps the immediate path (a test hook, as force.qg)
        const bool park = i8 && kr > 0 && kr <= 32 && (force.park < 0 ? FUSED_PARK_DEFAULT : force.park != 0);
        FilterPlan f{nw, qg, rg, minw, nbuf, 32 * qg * nw, fused_lds_of(rb, k, nw, rg, nbuf, kr == 0, qg, park)};
        f.kr = kr;
        f.i8 = i8 ? 1 : 0;
        f.park = park ? 1 : 0;
        return f;
    };
    // Register-list shapes: 64 queries per wave on 32-row tiles (QG = 2: each A fragment read
    // from LDS feeds two MFMAs, the two accumulators share one norm read, and each tile copy
    // serves 512 queries -- half the LDS reads and DMA per MFMA) when the 512-query blocks fill
    // a round of CUs: at least 384 queries per CU, or (round 6) when the query tiles times the
    // most pieces a query's candidate list allows (max_pieces, the caller's capacity rule)
    // reach 80 % of the CUs (one such block per CU: 8 waves at ~240 VGPRs).  Fewer queries
    // would leave CUs idle (pieces beyond max_pieces overflow the lists) or cut each query
    // tile into many pieces (each piece starts its thresholds from +inf), so they keep 32 per
    // wave on 64-row tiles (with the list exchange).  Same box (profiles/r04c): A 24.08 -> 23.19
    // ms, B 575.9 -> 550.9 ms; A's 8-GPU share (12,500 queries) 3.40 -> 6.33 ms with QG = 2.
    // The fill rule (profiles/r06_studies/r06qg, r06qh; filter ms, QG = 1 -> 2, A's rows, d and
    // k): 18,750 queries (37 tiles x 5 pieces = 71 % of the CUs) 4.57 -> 4.83, 21,875 (84 %)
    // 5.21 -> 5.02, 25,000 5.73 -> 5.19, 50,000 11.02 -> 10.10, 75,000 16.49 -> 14.50, 90,000
    // 18.27 -> 16.83; B's rows (2 pieces): 31,250 (48 %) 17.2 -> 29.1, 62,500 (96 %) 31.9 -> 30.7.
    // force.qg = 1|2 forces the choice (a test hook, snapshot at knn_create).
    // (d = 256 keeps 32 queries per wave: two query groups' operands alone are 128 VGPRs)
    const bool fills = (nq + 511) / 512 * (int64_t)std::max(max_pieces, 1) * 5 >= (int64_t)4 * num_cus;
    const bool qg2 = d <= 128 && (force.qg == 2 || (force.qg != 1 && (nq >= (int64_t)384 * num_cus || fills)));
    // tiles in octets: 16 buffers, one barrier per eight 32-row tiles, the loop running whole
    // groups so each tile's place is static (pairs -> quads: B 557.2 -> 501.1 ms, A 22.61 ->
    // 21.67 ms, r04i; quads -> octets: A 21.49 -> 20.80 ms, B 504.6 -> 483.8 ms, r04y).
    if (kr > 0 && qg2) return make(8, 1, 2, 16, 2);
    if (kr == 104) return make(8, 1, 2, 8);
    // list exchange between a query's pieces (a.lshare, knn_capi.cpp): the QG = 1 shapes only
    // (QG = 2 with it: A 21.81 -> 22.84 ms; on A's 8-GPU share, 10 pieces, 3.55 ms against
    // QG = 1's 3.38 -- more pieces, more kept rows: r04l, r04p)
    if (kr > 0) {
        // 64-row tiles in quads where eight buffers fit (d <= 128): A's 8-GPU share 3.08 -> 2.96 ms,
        // A at QG = 1 23.05 -> 22.31 (r04u)
        FilterPlan f = make(8, 2, 2, d <= 128 ? 8 : 4);
        f.ls = 1;
        return f;
    }
    if (kr == 0 && d == 64 && fused_lds_of(rb, k, 4, 2, 2, true) <= cap / 2) return make(4, 2, 2, 2);
    if (fused_lds_of(rb, k, 8, 2, 4, kr == 0) <= cap) return make(8, 2, 2, 4);
    if (fused_lds_of(rb, k, 8, 2, 2, kr == 0) <= cap) return make(8, 2, 2, 2);
    if (fused_lds_of(rb, k, 8, 1, 2, kr == 0) <= cap) return make(8, 1, 2, 2);
    return FilterPlan{0, 0, 0, 0, 0, 0, 0};  // k too large for the LDS heaps: not supported
}

// the kernel of plan f's shape; nullptr: a shape knn_fused_plan never makes
template <int RB, int KR, bool I8 = false, bool PARK = false>
static const void* fused_fn_k(const FilterPlan& f) {
#define KNN_FUSED_FN(NB, NW, QG, RG) reinterpret_cast<const void*>(&k_gemm_fused<RB, 2, NB, NW, QG, RG, KR, I8, PARK>)
    static_assert(!I8 || ((KR == 8 || KR == 32) && RB == 128), "int8 operands: register lists, k <= 32, d = 128");
    static_assert(!PARK || I8, "parked passes: the int8 shapes");
    if constexpr (KR == 104) {
        return KNN_FUSED_FN(8, 8, 1, 1);
    } else if constexpr (KR > 0 && RB <= 256) {  // d <= 128: 64 queries per wave in octets, or quads of 64-row tiles
        if (f.qg == 2) return f.nbuf == 16 ? KNN_FUSED_FN(16, 8, 2, 1) : nullptr;
        return f.nbuf == 8 ? KNN_FUSED_FN(8, 8, 1, 2) : nullptr;
    } else if constexpr (KR > 0) {  // d = 256: pairs
        return f.qg == 1 && f.nbuf == 4 ? KNN_FUSED_FN(4, 8, 1, 2) : nullptr;
    } else {
        if (f.nw == 4) return KNN_FUSED_FN(2, 4, 1, 2);
        if (f.rg == 2) return f.nbuf == 4 ? KNN_FUSED_FN(4, 8, 1, 2) : KNN_FUSED_FN(2, 8, 1, 2);
        return KNN_FUSED_FN(2, 8, 1, 1);
    }
#undef KNN_FUSED_FN
}
template <int RB>
static const void* fused_fn(const FilterPlan& f) {
    if constexpr (RB == 512)
        if (f.kr == 104) return fused_fn_k<RB, 104>(f);
    return f.kr == 8 ? fused_fn_k<RB, 8>(f) : f.kr == 32 ? fused_fn_k<RB, 32>(f) : fused_fn_k<RB, 0>(f);
}

static const void* fused_ptr(int d, const FilterPlan& f) {
    if (f.i8) {
        if (d != 128) return nullptr;
        if (f.park) return f.kr == 8 ? fused_fn_k<128, 8, true, true>(f) : f.kr == 32 ? fused_fn_k<128, 32, true, true>(f) : nullptr;
        return f.kr == 8 ? fused_fn_k<128, 8, true>(f) : f.kr == 32 ? fused_fn_k<128, 32, true>(f) : nullptr;
    }
    return d == 64 ? fused_fn<128>(f) : d == 128 ? fused_fn<256>(f) : fused_fn<512>(f);
}

bool knn_fused_has_kernel(int d, const FilterPlan& f) { return knn_fused_supported(d) && f.nw > 0 && fused_ptr(d, f) != nullptr; }

hipError_t knn_fused_occupancy(int d, const FilterPlan& f, int* blocks_per_cu) {
    if (!knn_fused_supported(d) || f.nw == 0 || !fused_ptr(d, f)) return hipErrorInvalidValue;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, fused_ptr(d, f), 64 * f.nw, f.lds);
}

hipError_t knn_launch_fused(const GemmFilterArgs& a, const FilterPlan& f, hipStream_t st) {
    // (operand rows are packed: a pitch of d elements, bf16 or int8)
    if (!knn_fused_has_kernel(a.d, f) || a.ld_t != a.d || a.ld_q != a.d || !a.qstat) return hipErrorInvalidValue;
    if (f.i8 ? !(a.i8_s2 > 0.0f) : a.i8_s2 != 0.0f) return hipErrorInvalidValue;
    if (f.park && !f.i8) return hipErrorInvalidValue;
    if (f.kr > 0 && !(f.nw == 8 && ((f.nbuf == (a.d == 256 ? 4 : 8) && f.qg == 1 && f.rg == 2 && f.kr <= 32) ||
                                     (f.nbuf == 16 && f.qg == 2 && f.rg == 1 && f.kr <= 32) ||
                                     (f.nbuf == 8 && f.qg == 1 && f.rg == 1 && f.kr == 104 && a.d == 256))))
        return hipErrorInvalidValue;  // (fused_fn_k)
    void* args[] = {const_cast<GemmFilterArgs*>(&a)};
    const dim3 grid((unsigned)(a.g2 < 0 ? (int64_t)a.n_qtiles * a.nseg : (int64_t)a.p1_blocks + a.g2));
    hipError_t e = hipLaunchKernel(fused_ptr(a.d, f), grid, dim3(64 * f.nw), args, f.lds, st);
    if (e != hipSuccess) return e;
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}

// ---------------------------------------------------------------------------------
// Host views of the tile copy's piece map and of the balanced schedule (the same functions the
// kernel runs), for tests/test_fused_tile_image.py.  No GPU call.
// ---------------------------------------------------------------------------------
// The tile image of the 8-wave shapes, from the kernel's own FilterTile: out[8] = {row bytes, rows
// per tile, LDS row stride, slots per row, header offset, header slots, DMA pieces, buffer bytes}
template <int RB, int RG>
static void fused_image_of(int* out) {
    constexpr int HS = 32 * RG / 4 + 1;  // (as fused_piece)
    typedef FilterTile<RB, 8, 1, RG, HS> FT;
    const int v[8] = {RB, FT::BN, FT::STRIDE, FT::SLOTS, FT::HDR, HS, FT::DMA_INS, FT::TILE};
    for (int i = 0; i < 8; i++) out[i] = v[i];
}
extern "C" int knn_fused_debug_image(int d, int rg, int* out) {
    if (!knn_fused_supported(d) || (rg != 1 && rg != 2)) return -1;
    if (d == 64) rg == 1 ? fused_image_of<128, 1>(out) : fused_image_of<128, 2>(out);
    else if (d == 128) rg == 1 ? fused_image_of<256, 1>(out) : fused_image_of<256, 2>(out);
    else rg == 1 ? fused_image_of<512, 1>(out) : fused_image_of<512, 2>(out);
    return 0;
}
// the LDS offsets lane (j, h) reads: the A fragment of row 32 g + j at k-step s, and the norm
// read of register group g4 (the kernel's fused_frag_off / fused_norm_off on that image)
extern "C" int knn_fused_debug_read_off(int d, int rg, int g, int j, int h, int s, int g4, int* frag, int* norm) {
    int im[8];
    if (knn_fused_debug_image(d, rg, im) != 0) return -1;
    *frag = fused_frag_off(32 * g + j, h, s, im[2]);
    *norm = fused_norm_off(im[4], h, g, g4);
    return 0;
}

// d features, nw waves, rg 32-row groups per tile.  src_off[64 ins]: the source offset of each
// 16-byte slot of the LDS image; issued[tiles][ins]: how many waves issue piece ins of tile t;
// per_wave[nw]: pieces a wave issues over the tiles.  Returns ins, the pieces per tile.
extern "C" int knn_fused_debug_piece_map(int d, int nw, int rg, int tiles, uint32_t* src_off, int* issued,
                                         int* per_wave) {
    int g[8];
    if (nw != 8 || tiles < 0 || knn_fused_debug_image(d, rg, g) != 0) return -1;
    const int rb = g[0], bn = g[1], hs = g[5], ins = g[6];
    for (int P = 0; P < 64 * ins; P++) src_off[P] = fused_dma_src_off(P, bn, rb, hs, rb);
    for (int i = 0; i < tiles * ins; i++) issued[i] = 0;
    for (int w = 0; w < nw; w++) {
        per_wave[w] = 0;
        for (int t = 0; t < tiles; t++) {
            for (int i = 0; i < (ins + nw - 1) / nw; i++)
                if (fused_dma_piece(nw, w, i) < ins) issued[t * ins + fused_dma_piece(nw, w, i)]++, per_wave[w]++;
        }
    }
    return ins;
}

// The plan knn_fused_plan makes (qg 0|1|2 and heaps as FusedForce): out[11] = {nw, qg, rg, minw,
// nbuf, bm, lds, kr, ls, i8, whether the library holds the plan's kernel}
extern "C" int knn_fused_debug_plan(int d, int k, long long nq, int num_cus, int qg, int heaps, int max_pieces, int i8,
                                    long long* out) {
    if (!knn_fused_supported(d) || k < 1) return -1;
    FusedForce force;
    force.qg = qg;
    force.heaps = heaps != 0;
    const FilterPlan f = knn_fused_plan(d, k, nq, num_cus, force, max_pieces, i8 != 0);
    const long long v[11] = {f.nw, f.qg, f.rg, f.minw, f.nbuf, f.bm, (long long)f.lds, f.kr, f.ls, f.i8,
                             knn_fused_has_kernel(d, f) ? 1 : 0};
    for (int i = 0; i < 11; i++) out[i] = v[i];
    return 0;
}

// The parked passes' ring of the int8 plan with qg 1|2 query groups per wave (d = 128):
// out[5] = {slots per thread, threads, bytes of the tile buffers, first byte of the ring, one
// past its last}
extern "C" int knn_fused_debug_park(int qg, long long* out) {
    if (qg != 1 && qg != 2) return -1;
    int im[8];
    if (knn_fused_debug_image(64, qg == 2 ? 1 : 2, im) != 0) return -1;  // (rows of 128 bytes: d = 64 bf16, d = 128 int8)
    const int tiles = (qg == 2 ? 16 : 8) * im[7], nt = 512;
    const long long v[5] = {FUSED_PARK_SLOTS, nt, tiles, fused_park_base(tiles), fused_park_base(tiles) + fused_park_bytes(nt)};
    for (int i = 0; i < 5; i++) out[i] = v[i];
    return 0;
}
// the LDS byte offset of thread t's slot s, quarter v (0..3: 16 bytes of values; 4: the word) --
// the kernel's fused_park_off on that plan; -1: no such slot
extern "C" long long knn_fused_debug_park_off(int qg, int t, int s, int v) {
    long long g[5];
    if (knn_fused_debug_park(qg, g) != 0 || t < 0 || t >= g[1] || s < 0 || s >= g[0] || v < 0 || v > 4) return -1;
    return fused_park_off((int)g[2], (int)g[1], t, s, v);
}

// The pieces of the balanced schedule of n_qtiles query tiles against nt train rows on `slots`
// resident blocks, in the order the blocks run them: out[6 i] = {block, query tile, t0, t1,
// rot, the piece's place in its block} (64-row units); with bn > 0 also out[6 i + 4] in tiles as
// the kernel scans it (fused_rot_tiles for bn-row tiles in groups of grp) and out[6 i + 5] the
// piece's tiles (fused_piece_tiles).  Returns the piece count (-1: more than
// cap); *grid and *nseg as knn_fused_schedule.
extern "C" int knn_fused_debug_schedule(long long nt, int n_qtiles, int slots, int bn, int grp, long long* out,
                                        int cap, int* grid, int* nseg) {
    if (nt < 1 || n_qtiles < 1 || slots < 1) return -1;
    GemmFilterArgs a{};
    a.nt = nt;
    a.n_qtiles = n_qtiles;
    *grid = knn_fused_schedule(a, slots, nseg);
    const int64_t T = a.tiles64;
    int n = 0;
    for (int b = 0; b < *grid; b++) {
        const bool p1 = b < a.p1_blocks;
        const int64_t b2 = b - a.p1_blocks;
        int64_t x = p1 ? (int64_t)b * T : b2 * a.w2 / a.g2;
        int64_t x1 = p1 ? x + T : (b2 + 1) * a.w2 / a.g2;
        int place = 0;
        for (bool first = true; x < x1; first = false) {
            const FusedRangePiece p = knn_fused_range_piece(x, x1, T, first);
            if (n >= cap) return -1;
            long long* o = out + 6 * (int64_t)n++;
            o[0] = b; o[1] = (p1 ? 0 : a.p1_blocks) + p.ql; o[2] = p.t0; o[3] = p.t1; o[4] = p.rot; o[5] = place++;
            if (bn > 0) {  // (rows as the kernel's piece: [64 t0, min(nt, 64 t1)))
                const int nt_p = fused_piece_tiles(std::min<int64_t>(nt, p.t1 * 64) - p.t0 * 64, bn, grp);
                o[4] = fused_rot_tiles(p.rot, bn, grp, nt_p);
                o[5] = nt_p;
            }
            x1 -= p.t1 - p.t0;
        }
    }
    return n;
}
