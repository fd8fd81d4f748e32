// knn_device.h -- device helpers shared by the kernel translation units of libknn_amd
// (knn_kernels.hip, knn_metric.hip, knn_radius.hip, knn_radius_gemm.hip, knn_fused.hip, knn_seed.hip, knn_vote_weighted.hip, knn_regress.hip, knn_lof.hip): keys and
// wave bitonic networks, the vote and outputs of a finished wave list, the lane-shift insert, bf16 helpers, ordered-float bits, LDS-DMA issue and the GEMM filter tile
// geometry.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <float.h>
#include <stdint.h>

#include "knn_kernels.h"

typedef unsigned long long u64;

// Grid of a grid-stride elementwise kernel over `total` items (256 threads per block): at most
// 2^20 blocks.  A dispatch's size is a 32-bit count of work-items, so one thread per item
// would wrap for more than 2^32 items (a 32M x 256 generator fill has 8.2e9) and leave the
// tail untouched.
static inline unsigned elementwise_grid(int64_t total) {
    return (unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)1 << 20);
}
// a gated stage (AUTO's re-run, rarely taken) launches at most 2048 blocks of a grid-stride
// kernel: a re-run not taken then costs a few thousand empty waves, not one per 256 elements
static inline unsigned gated_grid(unsigned grid, const void* gate) {
    return gate ? std::min(grid, 2048u) : grid;
}
#define KNN_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return e_; } while (0)
static constexpr u64 KEY_NONE = ~0ull;
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx2 __attribute__((ext_vector_type(2)));
#ifndef KNN_FILTER_PK
#define KNN_FILTER_PK 0
#endif

// ---------------------------------------------------------------------------------
// Keys and wave-level bitonic networks (64 lanes, one element per lane per register)
// ---------------------------------------------------------------------------------
__device__ __forceinline__ u64 make_key(float dist, uint32_t idx) {
    if (!(dist < FLT_MAX)) return KEY_NONE;  // main.cpp:47 against the FLT_MAX sentinel
    return ((u64)__float_as_uint(dist) << 32) | (u64)idx;
}

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

__device__ __forceinline__ u64 umin64(u64 a, u64 b) { return a < b ? a : b; }
__device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a < b ? b : a; }

// The word of lane ^ j (j a power of two <= 32, a constant once the networks below are
// unrolled), without ds_bpermute: j = 1, 2 by a DPP quad permutation, j = 4, 8 by two DPP
// row shifts (row_shl / row_shr: the partner sits j lanes up or down inside its row of 16)
// and a select, j = 16 by ds_swizzle's xor mode (no address operand), j = 32 by
// v_permlane32_swap (one of its two results is the other half's word).  All but j = 16 are
// VALU instructions, so a compare-exchange stage waits on no LDS round trip.
__device__ __forceinline__ uint32_t lane_xor(uint32_t v, int j) {
    const int lane = lane_id();
    switch (j) {
        case 1: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
        case 2: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);  // quad_perm [2,3,0,1]
        case 4: {
            const uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x104, 0xF, 0xF, false);  // row_shl:4
            const uint32_t dn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);  // row_shr:4
            return (lane & 4) ? dn : up;
        }
        case 8: {
            const uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x108, 0xF, 0xF, false);  // row_shl:8
            const uint32_t dn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);  // row_shr:8
            return (lane & 8) ? dn : up;
        }
        case 16: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (16 << 10) | 0x1F);  // xor_mask 16, and_mask 31
        default: {
            const auto sw = __builtin_amdgcn_permlane32_swap(v, v, false, false);
            return (lane & 32) ? sw[0] : sw[1];
        }
    }
}
__device__ __forceinline__ u64 lane_xor64(u64 v, int j) {
    return ((u64)lane_xor((uint32_t)(v >> 32), j) << 32) | (u64)lane_xor((uint32_t)v, j);
}

// compare-exchange with lane ^ j; keep the smaller key if keep_min
__device__ __forceinline__ u64 cx(u64 v, int j, bool keep_min) {
    const u64 o = lane_xor64(v, j);
    return keep_min ? umin64(v, o) : umax64(v, o);
}

// full bitonic sort of 64 keys across the wave
__device__ __forceinline__ u64 sort64(u64 v, bool descending) {
    const int lane = lane_id();
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int j = size >> 1; j > 0; j >>= 1) {
            bool up = ((lane & size) == 0) != descending;
            bool lower = (lane & j) == 0;
            v = cx(v, j, lower == up);
        }
    }
    return v;
}

// bitonic merge of a bitonic 64-sequence
__device__ __forceinline__ u64 merge64(u64 v, bool ascending) {
    const int lane = lane_id();
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) v = cx(v, j, ((lane & j) == 0) == ascending);
    return v;
}

// Wave-resident sorted list of the 64*R smallest keys: element e = 64*r + lane lives in
// T[r] of lane (e & 63).  Merge one batch of 64 new keys (one per lane).
template <int R>
__device__ __forceinline__ void topk_merge(u64 (&T)[R], u64 x) {
    x = sort64(x, /*descending=*/true);
    u64 y = umin64(T[R - 1], x);  // half-cleaner: the 64 smallest of T[R-1] u x, bitonic
    if constexpr (R == 1) {
        T[0] = merge64(y, true);
    } else {
        // [T0..T(R-2) ascending, T(R-1) descending] is bitonic over 64R elements
        T[R - 1] = merge64(y, false);
#pragma unroll
        for (int s = R / 2; s >= 1; s >>= 1) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                if ((r & s) == 0) {
                    u64 a = T[r], b = T[r + s];
                    T[r] = umin64(a, b);
                    T[r + s] = umax64(a, b);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) T[r] = merge64(T[r], true);
    }
}

// topk_merge for a batch that is already ascending across the lanes (a prefix of a sorted
// list, KEY_NONE padding at the end): reversed by one lane permutation instead of sorted
template <int R>
__device__ __forceinline__ void topk_merge_sorted(u64 (&T)[R], u64 x) {
    const int src = 4 * (63 - lane_id());
    const u64 rev = ((u64)(uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)(x >> 32)) << 32) |
                    (u64)(uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)x);
    u64 y = umin64(T[R - 1], rev);  // half-cleaner: the 64 smallest of T[R-1] u x, bitonic
    if constexpr (R == 1) {
        T[0] = merge64(y, true);
    } else {
        T[R - 1] = merge64(y, false);
#pragma unroll
        for (int s = R / 2; s >= 1; s >>= 1) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                if ((r & s) == 0) {
                    u64 a = T[r], b = T[r + s];
                    T[r] = umin64(a, b);
                    T[r + s] = umax64(a, b);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) T[r] = merge64(T[r], true);
    }
}

// element e of the wave list, broadcast to every lane
template <int R>
__device__ __forceinline__ u64 list_at(const u64 (&T)[R], int e) {
    u64 v = T[0];
#pragma unroll
    for (int r = 1; r < R; r++)
        if (r == (e >> 6)) v = T[r];
    return __shfl(v, e & 63);
}

// ---------------------------------------------------------------------------------
// Feature elements: fp32, or bf16 bits widened exactly (bf16 -> fp32 is a 16-bit shift)
// ---------------------------------------------------------------------------------
typedef uint16_t bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
// filter operand tag for ELEM_SPLIT rows (bf16 bits [hi(d) | lo(d)] of fp32 data)
struct split_t { uint16_t v; };

// fp32 -> bf16 bits, round to nearest even (finite inputs)
__device__ __forceinline__ uint32_t bf16_rne(float x) {
    const uint32_t b = __float_as_uint(x);
    return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(bf16_t v) { return __uint_as_float((uint32_t)v << 16); }

// four consecutive elements as fp32 (p aligned to 4 elements)
__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 load4(const bf16_t* p) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u),
                       __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u));
}

// One quad of a bf16 filter operand row (k_tn_rows, k_round_rows, and their host view
// knn_debug_operand_rows): columns c .. c+3 of the operand, rn(scale * x) of the caller's row of
// d elements and zero bits from column d on.  A quad inside the row is one load; the row's last
// partial quad is read by element, so nothing at column d or beyond is touched.
__host__ __device__ __forceinline__ uint32_t operand_rne(float x) {
    const uint32_t b = __builtin_bit_cast(uint32_t, x);
    return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
}
__host__ __device__ __forceinline__ float operand_widen(float v) { return v; }
__host__ __device__ __forceinline__ float operand_widen(bf16_t v) { return __builtin_bit_cast(float, (uint32_t)v << 16); }
template <typename E>
__host__ __device__ __forceinline__ uint2 operand_quad(const E* row, int c, int d, float scale) {
    if (c >= d) return make_uint2(0u, 0u);
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#if defined(__HIP_DEVICE_COMPILE__)
    if (c + 4 <= d) {
        const float4 q = load4(row + c);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else
#endif
    {
        for (int t = 0; t < 4; t++)
            if (c + t < d) v[t] = operand_widen(row[c + t]);
    }
    uint32_t o[4];
    for (int t = 0; t < 4; t++) o[t] = c + t < d ? operand_rne(scale * v[t]) : 0u;  // (zero bits whatever scale's sign)
    return make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
}

// ---------------------------------------------------------------------------------
// The int8 filter operand class (fp32 data, KNN_ALGO_GEMM_I8; DESIGN.md "int8 filter operands").
// One symmetric scale per train set, s = max|t| / 127; a row element x becomes the integer
//   n = clamp(rne(x / s), -127, 127)      (-128 is never produced; NaN -> -127)
// and stands for the real number s n in the certificate.  Queries use the train set's s (a
// query outside the train range saturates; its residual is measured like any other).  With
// s2 = fl(2 s s) the filter's value is y* = tn - s2 (nq . nt), an exact integer sum times s2.
// Every kernel that quantises, and the host tests, go through these functions.
// ---------------------------------------------------------------------------------
__host__ __device__ inline int knn_i8_quant(float x, float s) {
    float r = rintf(x / s);
    if (!(r >= -127.0f)) r = -127.0f;
    if (r > 127.0f) r = 127.0f;
    return (int)r;
}
__host__ __device__ inline float knn_i8_s2(float s) { return 2.0f * s * s; }
// the integer the accumulator of a row starts from (negated): about tn / s2, in [0, 2^30]
__host__ __device__ inline int32_t knn_i8_norm_q(float tn, float s2) {
    float r = floorf(tn / s2);
    if (!(r >= 0.0f)) r = 0.0f;
    if (r > 0x1p30f) r = 0x1p30f;
    return (int32_t)r;
}
// an upper bound of |tn - s2 n| (binary64: the product errs by <= 2^-53 s2 n, covered by the
// tn term; the conversion and the factor round up)
__host__ __device__ inline float knn_i8_norm_res(float tn, float s2, int32_t n) {
    double e = (double)tn - (double)s2 * (double)n;
    e = e < 0.0 ? -e : e;
    return (float)e * (1.0f + 0x1p-20f) + (tn < 0.0f ? -tn : tn) * 0x1p-40f + 0x1p-126f;
}
// The integer fast test.  ti = knn_i8_fast_thr(tf, s2) is an integer <= -tf / s2 (real
// arithmetic, s2 > 0), so for every integer a: -s2 a <= tf  =>  a >= -tf / s2 >= ti -- the
// test a >= ti passes a superset of the float test.  The division rounds once (relative
// 2^-24); 2^-20 |x| + 1 below x covers it and the floor.  tf = -inf (no valid query): INT32_MAX,
// which no accumulator reaches; tf = +inf or NaN: INT32_MIN, everything passes.
__host__ __device__ inline int32_t knn_i8_fast_thr(float tf, float s2) {
    float x = -tf / s2;
    if (x >= 0x1p31f) return 0x7fffffff;
    if (!(x > -0x1p31f)) return (int32_t)0x80000000u;
    x = floorf(fmaf(x < 0.0f ? x : -x, 0x1p-20f, x) - 1.0f);
    if (!(x > -0x1p31f)) return (int32_t)0x80000000u;
    return (int32_t)x;
}
// The seed pass's bound (k_seed_thr, DESIGN.md "Seeded thresholds"): U of accumulator value a for a
// query with norm qn and statistics qs = {|q|, |q - rq|}, by the slow path's formula (fused_piece's
// bounds and tile_q) with the train set's maxima smax (a.tsmax) in place of the tile's own
// statistics.  Every term is monotone in the statistic it takes, so U >= the slow path's U of the
// same row >= its direct-form distance D; and U is non-increasing in a (-s2 < 0, float(a) is
// monotone).  A NaN or infinite qn gives a non-finite U, which the caller must not publish.
__host__ __device__ inline float knn_i8_seed_bound(int32_t a, float qn, float2 qs, float s2, float coef, float eta,
                                                   float4 smax) {
    const float qe2 = 2.0f * qs.x * (1.0f + 0x1p-17f);
    const float eq2 = 2.0f * qs.y * (1.0f + 0x1p-17f);
    const float G = fmaf(-s2, (float)a, qn);
    const float dl = fmaf(coef, qn + smax.x, eta) + (fmaf(qe2, smax.y, eq2 * smax.z) + smax.w * (1.0f + 0x1p-20f));
    return G + dl;
}
// The k-th largest (with multiplicity) of a multiset of int32, given count_ge(t) = how many of its
// values are >= t: the largest t with count_ge(t) >= k, built bit by bit from the top of the
// values' order-preserving unsigned keys (32 counts).  Fewer than k values: INT32_MIN.
template <typename CountGE>
__host__ __device__ inline int32_t knn_kth_largest_i32(int k, CountGE count_ge) {
    uint32_t key = 0u;
    for (int b = 31; b >= 0; b--) {
        const uint32_t c = key | (1u << b);
        if (count_ge((int32_t)(c ^ 0x80000000u)) >= k) key = c;
    }
    return (int32_t)(key ^ 0x80000000u);
}
// a group maximum at or below this is an empty group: pad rows start their accumulators from
// -2^30 (k_i8_rows), and a valid row's a = nq . nt - n_r is above -2^22 at d = 128
static constexpr int32_t KNN_SEED_EMPTY = -(1 << 29);

// ordered uint <-> float (monotone for all non-NaN floats)
__device__ __forceinline__ uint32_t f2o(float f) {
    uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float o2f(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// min / max of two non-NaN floats as one v_med3 (fminf/fmaxf add two canonicalising v_max in
// IEEE mode): the middle of {a, b, -inf} is min(a, b), of {a, b, +inf} max(a, b)
__device__ __forceinline__ float fmin_fast(float a, float b) {
    return __builtin_amdgcn_fmed3f(a, b, __uint_as_float(0xff800000u));
}
__device__ __forceinline__ float fmax_fast(float a, float b) {
    return __builtin_amdgcn_fmed3f(a, b, __uint_as_float(0x7f800000u));
}

__device__ __forceinline__ float f4get(const float4& v, int i) {
    return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}
__device__ __forceinline__ float u4getf(const uint4& v, int i) {
    return __uint_as_float(i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w);
}

// LDS-DMA issued by inline asm: the compiler does not see these as LDS writes, so it
// does not put a vmcnt(0) in front of the next LDS read (which would serialise every
// tile's compute behind the DMA of the tile after it); the kernel orders them itself
// with waits + s_barrier (wait_dma_barrier).  M0 = the LDS destination (wave-uniform),
// written in the same statement that reads it (the compiler reserves M0 and does not
// preserve it around the statement: the statement saves and restores it).  Wait states
// inside the string, which the compiler does not pad: the SALU write of M0 needs 1 before
// the load reads it (s_nop 0); the scalar base may come straight from v_readfirstlane (a
// VALU write of an SGPR), which needs 5 before a vector-memory instruction reads it as its
// base -- s_nop 2 (3) and the two M0 moves (2) open the string.  Every
// operand is a value fixed before the statement (scalar tile base, the lane's constant
// offset VGPR): no per-tile address arithmetic feeds a DMA.
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}
// a wave-uniform value the compiler may have kept in VGPRs, as SGPRs
__device__ __forceinline__ const void* sgpr_ptr(const void* p) {
    const uint64_t v = (uint64_t)(uintptr_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (const void*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}
// scalar base + 32-bit per-lane offset (no per-lane 64-bit address math in the loop)
__device__ __forceinline__ void dma16s(uint32_t voff, const void* sbase, uint32_t lds) {
    sbase = sgpr_ptr(sbase);
    lds = __builtin_amdgcn_readfirstlane(lds);
    uint32_t keep;
    asm volatile("s_nop 2\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds)
                 : "memory");
}
__device__ __forceinline__ void dma4s(uint32_t voff, const void* sbase, uint32_t lds) {
    sbase = sgpr_ptr(sbase);
    lds = __builtin_amdgcn_readfirstlane(lds);
    uint32_t keep;
    asm volatile("s_nop 2\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds)
                 : "memory");
}
// The tile barrier of the LDS-DMA filters: this wave's tile DMAs have landed (vmcnt(0): its
// pieces of the tiles about to be read) AND every LDS read it issued has returned its data
// (lgkmcnt(0)), then s_barrier.  Both halves are needed:
//  * RAW -- after the barrier every wave's pieces of the next tiles are in LDS;
//  * WAR -- a ds_read is asynchronous, and s_barrier does not wait for it.  The DMAs issued
//    after this barrier overwrite the buffers the previous tiles used; a read of such a buffer
//    still in flight at the barrier (its MFMA scheduled after it) would return the NEW bytes.
//    With lgkmcnt(0) here no read of any earlier tile outlives the barrier, whatever order
//    the compiler gives the k-steps (without it the filter was correct only while a
//    per-k-step sched_barrier kept each tile's reads and MFMAs ahead of the barrier).
__device__ __forceinline__ void wait_dma_barrier() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// per-query 4-ary heap stride in floats: node n >= 1 in slot n-1, the root in the last slot;
// slots of nodes >= k hold -inf up to the last child group a parent < k reads (slot k+1)
__host__ __device__ __forceinline__ int heap_stride(int k) { return (k + 3 + 3) & ~3; }

// tile geometry shared by the kernel and the host's LDS sizing: NW waves per block,
// QG 32-query groups per wave, RG 32-row groups per tile; NACC = QG * RG accumulators;
// HS header slots of 16 B after the rows (the fused filter's per-tile norms and statistics)
template <int RB, int NW, int QG, int RG, int HS = 0>
struct FilterTile {
    static constexpr int NACC = QG * RG;             // 32x32 accumulators per wave per tile
    static constexpr int BN = 32 * RG;               // train rows per tile
    static constexpr int BM = 32 * QG * NW;          // queries per block
    static constexpr int STRIDE = RB + 16;           // LDS bytes per tile row
    static constexpr int SLOTS = RB / 16 + 1;        // 16-B slots per padded row
    static constexpr int DMA_INS = (BN * SLOTS + HS + 63) / 64;     // 1 KiB DMA instructions per tile
    static constexpr int LAST_LANES = BN * SLOTS + HS - 64 * (DMA_INS - 1);  // active lanes of the last
    static constexpr int TILE = DMA_INS * 1024;      // LDS bytes per buffer (>= BN * STRIDE + 16 HS)
    static constexpr int HDR = BN * STRIDE;          // LDS offset of the header
};

// LDS byte offset, inside a tile's image of rows of `stride` bytes, of the 16 bytes lane (j, h)
// reads of row `row` at k-step s (the A fragment of k_gemm_fused: ds_read_b128)
__host__ __device__ constexpr int fused_frag_off(int row, int h, int s, int stride) {
    return row * stride + 16 * h + 32 * s;
}
// LDS byte offset of the header's norm read of lane half h, row group rg, register group g4
__host__ __device__ constexpr int fused_norm_off(int hdr, int h, int rg, int g4) {
    return hdr + 4 * (4 * h) + 4 * (32 * rg + 8 * g4);
}
// Parked passes (k_gemm_fused<..., PARK>, DESIGN.md "Parked passes"): every thread of the block
// owns FUSED_PARK_SLOTS record slots in LDS past the tile buffers (and the 16 bytes of the scan
// rotation).  A record is one accumulator's 16 values of that lane, as four 16-byte quarters,
// and one word.  Quarters lie [slot][quarter][thread] in 16-byte units, so the 64 lanes of a
// wave reading one (slot, quarter) read 1 KiB of consecutive bytes (every b128 lane group
// touches each bank once); the words follow, [slot][thread].  v < 4: quarter v; v == 4: the word.
// (the slot count is a power of two: a slot index is masked with it - 1, never compared)
static constexpr int FUSED_PARK_SLOTS = 2;
static_assert((FUSED_PARK_SLOTS & (FUSED_PARK_SLOTS - 1)) == 0, "parked passes: slot index by mask");
__host__ __device__ constexpr int fused_park_base(int tile_bytes) { return tile_bytes + 16; }
__host__ __device__ constexpr int fused_park_off(int tile_bytes, int nt, int t, int s, int v) {
    return fused_park_base(tile_bytes) +
           (v < 4 ? ((s * 4 + v) * nt + t) * 16 : FUSED_PARK_SLOTS * 4 * nt * 16 + (s * nt + t) * 4);
}
__host__ __device__ constexpr int fused_park_bytes(int nt) { return FUSED_PARK_SLOTS * nt * (64 + 4); }

// Tiles a fused-filter piece of `rows` rows scans: whole barrier groups (at least pairs) of bn-row
// tiles, the extra ones past the piece's end (rejected by index)
__host__ __device__ constexpr int fused_piece_tiles(int64_t rows, int bn, int grp) {
    const int ts = grp > 2 ? grp : 2;
    return rows > 0 ? ((int)((rows + bn - 1) / bn) + ts - 1) / ts * ts : 0;
}
// The schedule's rotation of a piece (64-row units, knn_fused_range_piece) in tiles: whole
// barrier groups, so a tile keeps its place in its group; inside the piece
__host__ __device__ constexpr int fused_rot_tiles(int64_t rot_units, int bn, int grp, int ntiles) {
    const int r0 = (int)(rot_units * (64 / bn)) / grp * grp;
    return r0 < ntiles ? r0 : 0;
}
// The 1 KiB DMA pieces of a fused-filter tile (k_gemm_fused): the i-th piece wave w of nw issues
// (when it is below the tile's piece count)
__host__ __device__ constexpr int fused_dma_piece(int nw, int w, int i) { return w + nw * i; }
// byte offset in a tile's source (rows of pitch ldb, then the header) of the 16 bytes that land
// in slot P of the padded LDS image (slot P -> row P / slots, slot P % slots; the pad slot
// re-copies slot 0; slots past the header re-read its last slot)
__host__ __device__ constexpr uint32_t fused_dma_src_off(int P, int bn, int rb, int hs, int64_t ldb) {
    const int slots = rb / 16 + 1;
    if (hs > 0 && P >= bn * slots) return (uint32_t)(bn * rb + 16 * (P - bn * slots < hs - 1 ? P - bn * slots : hs - 1));
    const int row = P / slots < bn - 1 ? P / slots : bn - 1, sl = P % slots;
    return (uint32_t)(row * ldb + 16 * (sl == slots - 1 ? 0 : sl));
}

// ---------------------------------------------------------------------------------
// The vote of main.cpp:64-78 without a C-sized table (any class count): the argmax of
// the label counts over the list entries, ties to the smallest label.  lab[r] is the
// label of list element 64r + lane (-1: none / outside the list).  k rounds of one
// broadcast + R ballots.  Returns (count << 32) | (0xffffffff - label), 0 if empty.
// ---------------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ u64 vote_ballot(const int (&lab)[R], int k) {
    u64 best = 0;
    for (int e = 0; e < k; e++) {
        int le = lab[0];
#pragma unroll
        for (int r = 1; r < R; r++)
            if (r == (e >> 6)) le = lab[r];
        le = __shfl(le, e & 63);
        if (le < 0) continue;
        int cnt = 0;
#pragma unroll
        for (int r = 0; r < R; r++) cnt += __popcll(__ballot(lab[r] == le));
        best = umax64(best, ((u64)(uint32_t)cnt << 32) | (u64)(0xffffffffu - (uint32_t)le));
    }
    return best;
}

// ---------------------------------------------------------------------------------
// Outputs for one query from a finished wave list: the neighbour list (dist, idx_base +
// idx, label) and, when o.pred is set, the vote of main.cpp:64-78.
// counts: wave-private LDS array of C ints, or NULL for the table-free vote_ballot
// (class counts above KNN_VOTE_LDS_MAX_C).  Runs on one wave.
// lab0 (optional): the label of element `lane` of T[0], already loaded by the caller.
// ---------------------------------------------------------------------------------
template <int R>
__device__ void finish_query(const u64 (&T)[R], int k, int C, const int32_t* __restrict__ labels,
                             int* counts, int64_t q, const QueryOut& o, int32_t* __restrict__ status,
                             const int* lab0 = nullptr) {
    const int lane = lane_id();
    const bool vote = o.pred != nullptr;
    const bool lds_vote = vote && counts != nullptr;
    if (lds_vote) {
        for (int c = lane; c < C; c += 64) counts[c] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    u64 kth = list_at(T, k - 1);
    bool bad = (kth == KEY_NONE);
    int labr[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        labr[r] = -1;
        int e = 64 * r + lane;
        if (e < k) {
            const u64 key = T[r];
            const int64_t off = q * o.stride + e;
            if (key != KEY_NONE) {
                int32_t idx = (int32_t)(uint32_t)(key & 0xffffffffull);
                const int lab = (r == 0 && lab0) ? *lab0 : labels[idx];
                if (o.dist) o.dist[off] = __uint_as_float((uint32_t)(key >> 32));
                if (o.idx) o.idx[off] = (int32_t)(o.idx_base + idx);
                if (o.label) o.label[off] = lab;
                if (lab >= 0 && lab < C) {
                    labr[r] = lab;
                    if (lds_vote) atomicAdd(&counts[lab], 1);
                } else {
                    atomicOr(status, KNN_STATUS_BAD_LABEL);
                }
            } else {
                if (o.dist) o.dist[off] = FLT_MAX;
                if (o.idx) o.idx[off] = -1;
                if (o.label) o.label[off] = -1;
            }
        }
    }
    if (!vote) return;
    u64 best = 0;
    if (lds_vote) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // argmax, strict '>' scanning 0..C-1 == max count, smallest label on ties
        for (int c = lane; c < C; c += 64) {
            u64 v = ((u64)(uint32_t)counts[c] << 32) | (u64)(0xffffffffu - (uint32_t)c);
            best = umax64(best, v);
        }
#pragma unroll
        for (int j = 32; j > 0; j >>= 1) best = umax64(best, __shfl_xor(best, j));
    } else {
        best = vote_ballot<R>(labr, k);
    }
    if (lane == 0) {
        o.pred[q] = bad ? 0 : (int32_t)(0xffffffffu - (uint32_t)(best & 0xffffffffull));
        if (bad) atomicOr(status, KNN_STATUS_TOO_FEW);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------------------------
// The k <= 16 list of the direct-form tile kernels (k_direct_tile, k_direct_rows, k_metric_tile)
// ---------------------------------------------------------------------------------
// Insert key y into the ascending list held in lanes 0..15 of T (lanes >= k hold KEY_NONE and
// are left alone: in_list = lane < k).  y's train index is above every listed one (rows are
// visited in ascending order), so `T > y` on the 64-bit keys is main.cpp:47's strict `<` on the
// distance.  Lane e takes lane e-1's key (row_shr:1; lane 0 of a row reads 0 <= y) when both
// are above y, y itself when only its own is: the first key above y moves up one lane and the
// k-th falls off.  Needs k <= 16 (one DPP row).
__device__ __forceinline__ void shift_insert(u64& T, u64 y, bool in_list) {
    const uint32_t phi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(T >> 32), 0x111, 0xF, 0xF, true);
    const uint32_t plo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)T, 0x111, 0xF, 0xF, true);
    const u64 prev = ((u64)phi << 32) | (u64)plo;
    const bool gt = in_list && T > y;
    T = gt ? (prev > y ? prev : y) : T;
}
// distance of list element k-1 (wave-uniform): the insertion threshold, FLT_MAX while the list
// has fewer than k keys (main.cpp:33's sentinel)
__device__ __forceinline__ float kth_dist(u64 T, int k) {
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(T >> 32), k - 1);
    return hi == 0xffffffffu ? FLT_MAX : __uint_as_float(hi);
}
#ifndef DT_SHIFT_MAX
#define DT_SHIFT_MAX 8  // passing rows per tile and query up to which the lane shift beats the sort
#endif

// the binary32 weight of a neighbour at distance d (knn_amd.h "Weighted vote"; k_vote_weighted
// and k_regress_sweep): 1, 1 / sqrtf(d) or 1 / d, correctly rounded (no fast-math flag on the
// files that use it); under the zero rule 1 for d == 0 and 0 otherwise
__device__ __forceinline__ float vote_weight(int kind, bool zero_mode, float d) {
    if (kind == KNN_VOTE_W_UNIFORM) return 1.0f;
    if (zero_mode) return d == 0.0f ? 1.0f : 0.0f;
    return kind == KNN_VOTE_W_INV_DIST ? 1.0f / sqrtf(d) : 1.0f / d;
}

// What the list kernels k_vote_weighted and k_regress_sweep share; no arithmetic.  (k_vote_sweep
// keeps its own copy of the self-removal: through list_skip its 1024-entry form allocated one
// more spilled scalar register.)
// Self-removal: the place of the entry left out of query q's list row[0 .. kin) -- the first
// equal to self_base + q, the last when none is, kin (none) without self_base.  Elements at or
// behind it read one place further on.  One wave per list, element e = 64 r + lane.
template <int R>
__device__ __forceinline__ int list_skip(const int32_t* __restrict__ row, int kin, int64_t self_base, int64_t q,
                                         int lane) {
    int skip = kin;
    if (self_base >= 0) {
        const int64_t self = self_base + q;
        skip = kin - 1;
#pragma unroll
        for (int r = R - 1; r >= 0; r--) {
            const int e = 64 * r + lane;
            const u64 m = __ballot(e < kin && (int64_t)row[e] == self);
            if (m) skip = 64 * r + __ffsll(m) - 1;
        }
    }
    return skip;
}
// the zero rule of the weighted kinds looks at the first entry that is left: present, at d == 0
__device__ __forceinline__ bool list_zero_mode(int weights, const int32_t* __restrict__ row,
                                               const float* __restrict__ drow, int skip) {
    if (weights == KNN_VOTE_W_UNIFORM) return false;
    const int first = skip == 0 ? 1 : 0;
    return row[first] >= 0 && drow[first] == 0.0f;
}
