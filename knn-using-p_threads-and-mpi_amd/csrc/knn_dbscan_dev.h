// knn_dbscan_dev.h -- the lock-free union-find of DBSCAN's link step (include/knn_amd.h "DBSCAN";
// DESIGN.md "DBSCAN", "Union-find"), shared by k_radius_tile, k_radius_gemm (their RADIUS_LINK
// mode) and the kernels of knn_dbscan.hip.
//
// parent [n] int32 starts as parent[i] = i.  Every write lowers an entry: a root is hooked under a
// SMALLER root with a compare-and-swap, and a path is shortened with atomicMin towards an ancestor.
// So parent[x] <= x always, a value read earlier is still an ancestor of x however stale it is,
// and when every union is done the root of a component is its smallest row, whatever the order
// the unions ran in.  All reads are relaxed atomic loads at agent scope and all writes are atomics
// (the blocks of one pass sit on eight XCDs with an L2 each: plain loads and stores are not
// reliably seen between them inside one kernel).
//
// A walk only ever moves to a smaller index, on either side of a union and across its retries, so
// one union takes at most 3 n + 8 steps in all; the cap below is that bound.  Reaching it means the
// forest is corrupt: the loop sets KNN_STATUS_UF_LIMIT and leaves instead of spinning.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ int32_t uf_load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x (path halving on the way), or -1 when the step budget ran out
__device__ __forceinline__ int32_t uf_find(int32_t* parent, int32_t x, int64_t& budget) {
    int32_t p = uf_load(parent + x);
    while (p != x) {
        if (--budget < 0) return -1;
        const int32_t g = uf_load(parent + p);
        if (g != p) atomicMin(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

// joins the sets of rows a and b of the n; true when this call hooked a root (a successful union)
__device__ __forceinline__ bool uf_union(int32_t* parent, int32_t a, int32_t b, int64_t n, int32_t* status) {
    int64_t budget = 3 * n + 8;
    for (;;) {
        a = uf_find(parent, a, budget);
        if (a >= 0) b = uf_find(parent, b, budget);
        if (a < 0 || b < 0 || --budget < 0) {
            atomicOr(status, KNN_STATUS_UF_LIMIT);
            return false;
        }
        if (a == b) return false;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return true;
        // someone else hooked hi first: go on from where it points now
        a = old;
        b = lo;
    }
}
