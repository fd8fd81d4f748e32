// knn_radius_dev.h -- what the radius distance passes share: one feature of a metric and the scalar
// query loads (knn_radius.hip's k_radius_tile, knn_radius_sweep.hip's k_radius_sweep_tile); the LDS
// tile image and the exact distance of a pair (knn_radius_gemm.hip's k_radius_gemm,
// knn_radius_sweep.hip's k_radius_sweep_gemm).
// Include it with contraction off (the files that do are built with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knn_kernels.h"

#include "knn_device.h"

// one feature of metric M: the accumulator after (q_i, t_i)
template <int M>
__device__ __forceinline__ float radius_step(float acc, float q, float t) {
    const float df = q - t;
    if constexpr (M == METRIC_SQEUCLIDEAN)
        return acc + df * df;
    else if constexpr (M == METRIC_MANHATTAN)
        return acc + __builtin_fabsf(df);
    else
        return __builtin_fmaxf(acc, __builtin_fabsf(df));
}

// Four consecutive query elements as fp32 through the constant address space.  The query rows are
// wave-uniform operands and are only read, but this kernel stores to global memory inside its tile
// loop (the lists, the class-count atomics), so the compiler can no longer prove that a plain load
// of them is not clobbered and emits a vector global_load per query and group (measured: the count
// pass at 30.6 ms against k_direct_tile's 27.1 on 262,144 x 64 x 16,384).  A constant-address-space
// load of a uniform address is the s_load_dwordx4 that k_metric_tile gets by itself.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 load4q(const float* p) {
    const f32x4 v = *(const __attribute__((address_space(4))) f32x4*)(uintptr_t)p;
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float4 load4q(const bf16_t* p) {
    const u32x2 v = *(const __attribute__((address_space(4))) u32x2*)(uintptr_t)p;
    return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u),
                       __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u));
}

// tile image in LDS: the fused filter's (rows padded to RB + 16 bytes, then the header: 64 norms and
// the tile's statistics), two buffers
template <int RB>
struct RadiusGemmTile {
    static constexpr int STRIDE = RB + 16;           // LDS bytes per tile row
    static constexpr int SPR = RB / 16;              // 16-byte slots per operand row
    static constexpr int HDR = 64 * STRIDE;          // LDS offset of the header
    static constexpr int HS = 64 / 4 + 1;            // header slots: 64 fp32 norms + the statistics
    static constexpr int NSL = 64 * SPR + HS;        // 16-byte slots of one tile block
    static constexpr int TILE = HDR + 16 * HS;       // LDS bytes per buffer
    static constexpr int64_t TB = 64 * (int64_t)RB + 16 * HS;  // bytes of one tile block in the train operand
};

// D of k_direct_tile / k_radius_tile for one pair, from the caller's rows: acc = acc + (q_i - t_i)
// (q_i - t_i), i ascending, one rounding per operation (radius_step<SQEUCLIDEAN>, knn_radius.hip)
template <typename E>
__device__ __forceinline__ float radius_exact(const E* __restrict__ q, const E* __restrict__ t, int d) {
    float acc = 0.0f;
    for (int i = 0; i < d; i += 4) {
        const float4 a = load4(q + i), b = load4(t + i);
        float df = a.x - b.x;
        acc = acc + df * df;
        df = a.y - b.y;
        acc = acc + df * df;
        df = a.z - b.z;
        acc = acc + df * df;
        df = a.w - b.w;
        acc = acc + df * df;
    }
    return acc;
}
