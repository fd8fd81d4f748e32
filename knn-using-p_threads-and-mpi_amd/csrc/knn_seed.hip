// knn_seed.hip -- seeded thresholds of the int8 fused filter (gfx950).  DESIGN.md "Seeded
// thresholds".
//
// k_gemm_fused starts every piece from thr = gthr[q], which run_gemm fills with +inf: until a
// piece's own lists have converged nearly every tile takes the slow path.  k_seed_thr runs before
// the filter, over a strided sample of the train tile blocks the filter reads, and lowers gthr[q]
// to an upper bound B >= D_(k)(q), the query's exact k-th distance.  Any such B is a valid start:
// every row of the exact top-k has L <= D <= D_(k) <= B, so the filter keeps it, and k_rescore's
// L <= gthr staging sees a value that only the filter lowers further.
//
// The bound needs no lists.  In the accumulator layout of v_mfma_i32_32x32x32_i8 register v of
// lane half h always holds tile row (v & 3) + 8 (v >> 2) + 4h, so the elementwise maximum of the
// accumulators over the sampled 32-row tiles is the maximum of a = nq . nt - n_r over one of 32
// disjoint groups of sampled rows (16 registers x 2 lane halves) per query.  Each non-empty
// group's maximum belongs to a row of its own, so k distinct rows have a >= the k-th largest group
// maximum a_k, and U (knn_i8_seed_bound) is non-increasing in a and >= D for every row:
// D_(k) <= U(a_k).  For 16 < k <= 32 odd and even sampled tiles keep separate maxima, 64 groups
// (the k-th of 32 groups degenerates towards k = 32).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "knn_device.h"
#include "knn_kernels.h"

// Sample size and slicing (DESIGN.md "Seeded thresholds", the S study)
static constexpr int SEED_ROWS = 32768;       // train rows sampled, at most (and at most an eighth of the rows)
static constexpr int SEED_MIN_ROWS = 64;      // fewer sampled rows than this: no seed
static constexpr int SEED_SLICE_ROWS = 4096;  // a slice of the sample (few query tiles) has at least these rows

static constexpr int SEED_D = 128;                            // int8 operand rows: d = 128 bytes
static constexpr int SEED_STRIDE = SEED_D + 16;               // LDS bytes per row (conflict-free ds_read_b128, FilterTile)
static constexpr int SEED_HDR = 32 * SEED_STRIDE;             // a 32-row tile's header in its LDS image
static constexpr int SEED_SLOTS = 32 * 9 + 8;                 // 16-byte slots of a tile's LDS image: padded rows, header
static constexpr int SEED_DMA = (SEED_SLOTS + 63) / 64;       // 1 KiB LDS-DMA instructions per tile
static constexpr int SEED_TILE = SEED_DMA * 1024;             // LDS bytes per tile
static constexpr int SEED_CH = 8;                             // 32-row tiles per chunk: one per wave to copy, one barrier per chunk
static constexpr int SEED_NT = 512;                           // 8 waves x 64 queries

SeedSample knn_seed_sample(int64_t nt, int bn, int64_t nq, int num_cus) {
    SeedSample s;
    if (nt <= 0 || nq <= 0 || (bn != 32 && bn != 64)) return s;
    const int64_t tiles = (nt + bn - 1) / bn;  // tile blocks that hold a train row
    const int64_t ns = std::min<int64_t>(SEED_ROWS / bn, tiles / 8);
    if (ns * bn < SEED_MIN_ROWS) return s;
    s.ns = (int)ns;
    s.stride = tiles / ns;
    // few query tiles: several blocks per query tile, each over every slices-th sampled tile block
    const int64_t qblocks = (nq + SEED_NT - 1) / SEED_NT;
    const int64_t by_rows = std::max<int64_t>(1, ns * bn / SEED_SLICE_ROWS);
    s.slices = (int)std::max<int64_t>(1, std::min<int64_t>(std::max(num_cus, 1) / qblocks, by_rows));
    return s;
}

// The sampled tile blocks of knn_seed_sample (no GPU call; tests/test_gpu_seed.py plants rows by
// them): out[0..min(ns, cap)) = their tile-block numbers, info = {ns, stride, slices}.  Returns ns.
extern "C" int knn_debug_seed_tiles(long long nt, int bn, long long nq, int num_cus, long long* out, int cap,
                                    long long* info) {
    const SeedSample s = knn_seed_sample(nt, bn, nq, num_cus);
    if (info) { info[0] = s.ns; info[1] = s.stride; info[2] = s.slices; }
    for (int i = 0; out && i < s.ns && i < cap; i++) out[i] = (long long)i * s.stride;
    return s.ns;
}
// host views of knn_i8_seed_bound and of the group selection (tests/test_seed_cpu.py).  No GPU call.
// par = {qn, |q|, |q - rq|, s2, coef, eta, smax.x, smax.y, smax.z, smax.w}
extern "C" int knn_debug_seed_bound(const int32_t* a, long long n, const float* par, float* out) {
    if (!a || !par || !out || n < 0) return -1;
    for (long long i = 0; i < n; i++)
        out[i] = knn_i8_seed_bound(a[i], par[0], make_float2(par[1], par[2]), par[3], par[4], par[5],
                                   make_float4(par[6], par[7], par[8], par[9]));
    return 0;
}
// *out = the k-th largest of the g group maxima m (knn_kth_largest_i32, the kernel's selection);
// returns whether it is a seed: 1 when at least k groups are not empty
extern "C" int knn_debug_seed_select(const int32_t* m, int g, int k, int32_t* out) {
    if (!m || !out || g < 0 || k < 1) return -1;
    *out = knn_kth_largest_i32(k, [&](int32_t t) {
        int c = 0;
        for (int i = 0; i < g; i++) c += m[i] >= t ? 1 : 0;
        return c;
    });
    return *out > KNN_SEED_EMPTY ? 1 : 0;
}

// ---------------------------------------------------------------------------------
// k_seed_thr<GS>: block = 8 waves x 64 queries (two 32-query groups, two accumulators per wave)
// against its slice of the sampled tile blocks, taken as 32-row tiles: the same operand bytes per
// lane and k-step as fused_piece (bytes [32 s + 16 h, +16) of a row, the accumulator started from
// the header's -n_r words).  Chunks of SEED_CH tiles are staged in LDS once per block (LDS-DMA a
// chunk ahead, two buffers, one barrier per chunk) and read by every wave.  Per tile and
// accumulator: four MFMAs, and 16 max into the running group maxima beside the next tile's MFMAs --
// no lists, ballots, stores or branches in the loop.  GS: sets of group maxima (1: k <= 16, 32
// groups; 2: k <= 32, 64 groups, even / odd tiles of the slice).  A chunk's tiles past the slice's
// end are copies of the operand's last tile block: pad rows (zero features, -2^30), which win no
// group.
// ---------------------------------------------------------------------------------
template <int GS>
__global__ __launch_bounds__(SEED_NT) void k_seed_thr(SeedArgs a) {
    if ((a.gate && *a.gate == 0) || (*a.status & KNN_STATUS_GEMM_UNSAFE)) return;  // as k_gemm_fused
    typedef int intx4 __attribute__((ext_vector_type(4)));
    typedef int intx16 __attribute__((ext_vector_type(16)));
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * SEED_CH * SEED_TILE];

    const int tid = threadIdx.x;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int qblocks = (int)((a.nq + SEED_NT - 1) / SEED_NT);
    const int qb = blockIdx.x % qblocks, sl = blockIdx.x / qblocks;
    const int slices = a.sample.slices;
    const int sub = a.bn >> 5;                                      // 32-row tiles per tile block
    const int64_t tb = (int64_t)a.bn * SEED_D + 4 * a.bn + 16;      // bytes of a tile block (k_i8_rows)
    const int nblk = (a.sample.ns - sl + slices - 1) / slices;      // sampled tile blocks of this slice
    const int ntile = nblk * sub;                                   // ... as 32-row tiles
    const int nchunk = (ntile + SEED_CH - 1) / SEED_CH;
    const unsigned char* tblk = reinterpret_cast<const unsigned char*>(a.tblk);

    // this lane's queries, one per 32-query group (both lane halves: the same queries, the other
    // 16 bytes of each k-step)
    int64_t q[2];
    uint4 qf[2][4];
#pragma unroll
    for (int g = 0; g < 2; g++) {
        q[g] = (int64_t)qb * SEED_NT + (wave * 2 + g) * 32 + j;
        const bool valid = q[g] < a.nq;
        const unsigned char* qrow = reinterpret_cast<const unsigned char*>(a.qop) + (valid ? q[g] : 0) * SEED_D;
#pragma unroll
        for (int s = 0; s < 4; s++)
            qf[g][s] = valid ? *reinterpret_cast<const uint4*>(qrow + 32 * s + 16 * h) : make_uint4(0u, 0u, 0u, 0u);
    }
    // the query rows have arrived before the scan starts: the compiler does not count the DMA
    // loads below or see their waits, and would otherwise wait for these loads -- and with them for
    // every copy in flight -- at the head of the MFMA loop
#define KNN_SEED_Q4(Q) "+v"(Q.x), "+v"(Q.y), "+v"(Q.z), "+v"(Q.w)
#pragma unroll
    for (int g = 0; g < 2; g++)
        asm volatile("" : KNN_SEED_Q4(qf[g][0]), KNN_SEED_Q4(qf[g][1]), KNN_SEED_Q4(qf[g][2]), KNN_SEED_Q4(qf[g][3]));
#undef KNN_SEED_Q4

    // Staging by LDS-DMA (dma16s, as k_gemm_fused): wave w copies tile w of every chunk, SEED_DMA
    // instructions of 64 x 16 bytes.  Slot P = 64 i + lane of the tile's image <- row P / 9, slot
    // P % 9 of the row (the pad slot re-copies slot 0), then the 32 header words; slots past the
    // image repeat its last.  The lane's source offsets are relative to the tile block and fixed
    // for the whole scan (a 64-row block's second half: tile parity = wave parity, SEED_CH is
    // even); the block's address is scalar.  The copy of chunk c + 1 is in flight under the MFMAs
    // of chunk c; wait_dma_barrier closes every chunk.  A tile past the slice's end copies the
    // operand's last tile block, which holds pad rows only (a.pad_blk).
    const int su = sub == 2 ? (wave & 1) : 0;
    uint32_t doff[SEED_DMA];
#pragma unroll
    for (int i = 0; i < SEED_DMA; i++) {
        const int P = min(64 * i + lane, SEED_SLOTS - 1);
        const int row = P / 9, slot = P - 9 * row;
        doff[i] = P < 32 * 9 ? (uint32_t)(su * 32 * SEED_D + row * SEED_D + 16 * (slot == 8 ? 0 : slot))
                             : (uint32_t)(a.bn * SEED_D + 128 * su + 16 * (P - 32 * 9));
    }
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane(lds_addr(smem));
    auto copy_chunk = [&](int c) __attribute__((always_inline)) {
        const int u = c * SEED_CH + wave;  // this wave's 32-row tile of the slice
        const int64_t tblock = u < ntile ? (sl + (int64_t)(u / sub) * slices) * a.sample.stride : a.pad_blk;
        const unsigned char* src = tblk + tblock * tb;
        const uint32_t dst = lds0 + (uint32_t)(((c & 1) * SEED_CH + wave) * SEED_TILE);
#pragma unroll
        for (int i = 0; i < SEED_DMA; i++) dma16s(doff[i], src, dst + 1024u * i);
    };

    intx16 mx[GS][2];
#pragma unroll
    for (int s = 0; s < GS; s++)
#pragma unroll
        for (int g = 0; g < 2; g++)
#pragma unroll
            for (int v = 0; v < 16; v++) mx[s][g][v] = (int)0x80000000u;

    // One tile: its eight MFMAs into X and, issued between them, the 32 max of the tile before it
    // (Y, into maxima set `set`) -- software pipelining as in fused_piece: the matrix pipe runs an
    // MFMA for 8 passes while the wave's VALU takes the four max beside it, so one wave keeps the
    // pipe busy on its own.  (Left to the compiler the max all follow the MFMAs they wait for,
    // and the barrier keeps the two waves of a SIMD in the same phase: measured 0.46 ms for the
    // 32,768-row sample of A against 0.22 ms of MFMA time.)
    auto tile_step = [&](const unsigned char* tile, intx16 (&X)[2], const intx16 (&Y)[2], int set) __attribute__((always_inline)) {
#pragma unroll
        for (int g4 = 0; g4 < 4; g4++) {
            const int4 v = *reinterpret_cast<const int4*>(tile + fused_norm_off(SEED_HDR, h, 0, g4));
            X[0][4 * g4] = v.x; X[0][4 * g4 + 1] = v.y; X[0][4 * g4 + 2] = v.z; X[0][4 * g4 + 3] = v.w;
        }
        intx4 A[4];
#pragma unroll
        for (int s = 0; s < 4; s++)
            A[s] = __builtin_bit_cast(intx4, *reinterpret_cast<const uint4*>(tile + fused_frag_off(j, h, s, SEED_STRIDE)));
#pragma unroll
        for (int s = 0; s < 4; s++) {
#pragma unroll
            for (int gg = 0; gg < 2; gg++) {
                const int g = s == 0 ? 1 - gg : gg;  // (k-step 0: group 1 first, both from X[0]'s header words)
                X[g] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[s], __builtin_bit_cast(intx4, qf[g][s]), s == 0 ? X[0] : X[g], 0, 0, 0);
                const int m = 2 * s + gg;        // this MFMA's share of Y: four values
#pragma unroll
                for (int v = 4 * (m & 3); v < 4 * (m & 3) + 4; v++) mx[set][m >> 2][v] = max(mx[set][m >> 2][v], Y[m >> 2][v]);
            }
        }
#pragma unroll
        for (int m = 0; m < 8; m++) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA,
            __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);  // four VALU
        }
    };
    intx16 accA[2], accB[2];
#pragma unroll
    for (int g = 0; g < 2; g++)
#pragma unroll
        for (int v = 0; v < 16; v++) accB[g][v] = (int)0x80000000u;  // (no tile before the first)

    if (nchunk > 0) copy_chunk(0);
    wait_dma_barrier();
    for (int c = 0; c < nchunk; c++) {
        if (c + 1 < nchunk) copy_chunk(c + 1);
        const unsigned char* buf = smem + (c & 1) * SEED_CH * SEED_TILE;
        // tiles in twos (SEED_CH is even and a chunk starts at an even tile of the slice): the even
        // tile into accA beside the max of the odd tile before it, then the odd one into accB
#pragma unroll 1
        for (int tp = 0; tp < SEED_CH; tp += 2) {
            tile_step(buf + tp * SEED_TILE, accA, accB, GS - 1);
            tile_step(buf + (tp + 1) * SEED_TILE, accB, accA, 0);
        }
        wait_dma_barrier();
    }
    // the last tile (an odd one)
#pragma unroll
    for (int g = 0; g < 2; g++)
#pragma unroll
        for (int v = 0; v < 16; v++) mx[GS - 1][g][v] = max(mx[GS - 1][g][v], accB[g][v]);

    // per query: the k-th largest of its 32 GS group maxima (this lane's and its partner's, the
    // other lane half), then the bound; lane half 0 publishes
    const float4 smax = *a.tsmax;
#pragma unroll
    for (int g = 0; g < 2; g++) {
        const int32_t ak = knn_kth_largest_i32(a.k, [&](int32_t t) __attribute__((always_inline)) {
            int cnt = 0;
#pragma unroll
            for (int s = 0; s < GS; s++)
#pragma unroll
                for (int v = 0; v < 16; v++) cnt += mx[s][g][v] >= t ? 1 : 0;
            return cnt + __shfl_xor(cnt, 32);
        });
        if (q[g] < a.nq && h == 0 && ak > KNN_SEED_EMPTY) {  // (at least k groups are not empty)
            const float U = knn_i8_seed_bound(ak, a.qnorm[q[g]], a.qstat[q[g]], a.i8_s2, a.coef, a.eta, smax);
            if (fabsf(U) < __uint_as_float(0x7f800000u)) {  // finite (false for NaN): a NaN never reaches gthr
                atomicMin(&a.gthr[q[g]], f2o(U));
                if (a.seed_out) atomicMin(&a.seed_out[q[g]], f2o(U));
            }
        }
    }
}

hipError_t knn_launch_seed_thr(const SeedArgs& a, hipStream_t st) {
    const SeedSample& s = a.sample;
    if (s.ns <= 0 || a.nq <= 0) return hipSuccess;
    if ((a.bn != 32 && a.bn != 64) || a.k < 1 || a.k > 32 || !(a.i8_s2 > 0.0f) || s.stride < 1 || s.slices < 1 ||
        a.pad_blk < 0 || !a.tblk || !a.qop || !a.qnorm || !a.qstat || !a.tsmax || !a.gthr || !a.status)
        return hipErrorInvalidValue;
    const int64_t grid = (a.nq + SEED_NT - 1) / SEED_NT * s.slices;
    if (a.k <= 16) hipLaunchKernelGGL(k_seed_thr<1>, dim3((unsigned)grid), dim3(SEED_NT), 0, st, a);
    else hipLaunchKernelGGL(k_seed_thr<2>, dim3((unsigned)grid), dim3(SEED_NT), 0, st, a);
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}
