// knn_wide.hip -- the GEMM-form candidate filter for wide rows, 256 < d <= 4096 (gfx950).
// DESIGN.md "Any row width".
//
// k_gemm_filter and k_gemm_fused keep a query's whole operand row in VGPRs for the scan (64 VGPRs
// per 32 queries at d = 256): a wider row does not fit.  k_gemm_wide cuts the features into chunks
// of 128 and turns the loop around: a wave keeps the ACCUMULATORS of a group of G = 8 train tiles
// (32 rows each) across the chunks, and for every chunk reloads its queries' B fragments of that
// chunk (the bf16 query operand, L2-resident) while the block copies the chunk's tile images
// global -> LDS.  After the last chunk the G accumulators hold q.t over the whole row and the
// group is tested tile by tile, exactly as k_gemm_filter tests a tile.
//
// It speaks k_gemm_filter's protocol (knn_kernels.hip): the same GemmFilterArgs, bf16 operand rows
// [rows][dp] (rounded fp32 data or bf16 data; dp = d rounded up to a multiple of 128, the columns
// past d zero bits), the same fast test and the same L, U, Delta, the same LDS 4-ary heaps of the k
// smallest U, CandRec{idx, L, U} into sub-slice 2 seg + h, cnt, thresholds tightened through gthr
// across segments.  k_rescore's general path runs behind it unchanged.
//
// Block = 8 waves x 32 queries (BM = 256), two waves per SIMD: <= 256 registers per lane.
//   8 accumulators (128 registers) + one chunk's B fragments (8 k-steps x 4 = 32 registers).
// One (tile, chunk) image is k_gemm_filter's 256-byte tile image (FilterTile<256, 8, 1, 1>: 32 rows
// padded to 272 bytes, conflict-free ds_read_b128, 9 KiB), copied by LDS-DMA into two buffers with
// one barrier per image; images run in the order (group, chunk, tile).  The group's norm terms
// ((1-c) tn and tn of its 256 rows) are copied once per group into a ring of one slot.
// The B fragments of the next chunk are loaded k-step by k-step behind the last tile's MFMA that
// read the registers they replace; the loads land under the same wait as that step's tile copy.
//
// Bytes per MFMA from L2: a B fragment (1 KiB per wave) feeds G = 8 MFMAs, an image k-step (1 KiB)
// feeds the block's 8 waves: 1024 (1/8 + 1/8) = 256 bytes per MFMA, against 1024 (1 + 1/8) with
// G = 1.  Train rows past nt are the operand's zero pad rows (the grid of 256-row groups) with +inf
// norm terms: they never pass.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "knn_device.h"
#include "knn_kernels.h"

static constexpr int WIDE_NW = 8;     // waves per block, 32 queries each
static constexpr int WIDE_G = 8;      // train tiles per group = accumulators per wave (even: buffer = tile & 1)
static constexpr int WIDE_CB = 256;   // bytes of one chunk of an operand row: 128 bf16 features
static constexpr int WIDE_NBUF = 2;   // image buffers
typedef FilterTile<WIDE_CB, WIDE_NW, 1, 1> WideTile;
static constexpr int WIDE_GR = WIDE_G * WideTile::BN;  // train rows per group

__global__ __launch_bounds__(64 * WIDE_NW, 2) void k_gemm_wide(GemmFilterArgs a) {
    if ((a.gate && *a.gate == 0) || (*a.status & KNN_STATUS_GEMM_UNSAFE)) return;  // not taken / exact path
    typedef WideTile FT;
    constexpr int NW = WIDE_NW, G = WIDE_G, GR = WIDE_GR, CB = WIDE_CB;
    constexpr int BN = FT::BN, BM = FT::BM, STRIDE = FT::STRIDE, SLOTS = FT::SLOTS;
    constexpr int DMA_INS = FT::DMA_INS, TILE = FT::TILE;
    constexpr int NT = 64 * NW;
    constexpr int DMA_PER_WAVE = (DMA_INS + NW - 1) / NW;
    constexpr int NS = CB / 32;  // k-steps per chunk: 16 B per lane half per step
    static_assert(G % WIDE_NBUF == 0 && WIDE_NBUF == 2, "an image's buffer is its tile's parity");
    static_assert(GR == 4 * 64 && NW == 8, "the norm copy: four waves per term, 64 rows each");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* tiles = smem;                                        // [2][TILE]
    float* ring = reinterpret_cast<float*>(smem + WIDE_NBUF * TILE);    // [2][GR]: (1-c) tn, tn
    const int hs = heap_stride(a.k);
    float* topU = ring + 2 * GR;                                        // [BM][hs] max-heaps of U
    const int cap_sub = a.cap_seg / 2;  // candidate sub-slice of one lane half (h) of a query

    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // scalar: uniform DMA branches
    const int j = lane & 31;
    const int h = lane >> 5;
    const int qt = blockIdx.x % a.n_qtiles;
    const int seg = blockIdx.x / a.n_qtiles;
    const int64_t row_begin = (int64_t)seg * a.seg_len;  // (a multiple of GR: the launcher checks)
    const int64_t row_end = min(a.nt, row_begin + a.seg_len);
    const int k = a.k;
    const int nc = a.d / (CB / 2);  // chunks per row (a.d: the operand width, a multiple of 128)
    const float INF = __uint_as_float(0x7f800000u);
    const float coef = a.coef, eta = a.eta, c1 = 1.0f - a.coef;
    const float tnmax = o2f(*a.tnmax);
    const int64_t ldb = (int64_t)a.ld_t * 2;  // train operand row pitch, bytes
    const unsigned char* trainb = reinterpret_cast<const unsigned char*>(a.train);

    for (int i = threadIdx.x; i < BM * hs; i += NT) {
        const int e = i % hs;
        topU[i] = (e == hs - 1 || e <= k - 2) ? INF : -INF;  // root, nodes 1..k-1: +inf
    }
    for (int i = threadIdx.x; i < 2 * GR; i += NT) ring[i] = INF;

    // this lane's query (local jl, global q) and its state
    const int jl = wave * 32 + j;
    const int64_t q = (int64_t)qt * BM + jl;
    const bool qvalid = q < a.nq;
    const float qn = qvalid ? a.qnorm[q] : 0.0f;
    float thr = qvalid ? o2f(a.gthr[q]) : -INF;
    float published = thr;
    float root = INF;  // the heap root (k-th smallest U kept so far), mirrored in both lanes
    int ccnt = 0;      // candidates this lane half kept (its sub-slice fill)
    auto make_tf = [&](float th) -> float {
        if (!qvalid) return -INF;
        const float m = 0x1p-16f * (fabsf(th) + qn + tnmax);
        return ((th - c1 * qn) + eta) + m;
    };
    float tf = make_tf(thr);
    // B fragments of one chunk: 16 bytes of the query row per k-step s, bytes [CB c + 32 s + 16 h, + 16)
    const unsigned char* qrow = reinterpret_cast<const unsigned char*>(a.test) + (qvalid ? q : 0) * (int64_t)a.ld_q * 2 + 16 * h;
    auto load_frag = [&](int c, int s) -> uint4 {
        return qvalid ? *reinterpret_cast<const uint4*>(qrow + (int64_t)c * CB + 32 * s) : make_uint4(0u, 0u, 0u, 0u);
    };
    uint4 qf[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) qf[s] = load_frag(0, s);

    // LDS-DMA of one image: slot P (16 B) of the padded image -> row P / SLOTS, slot P % SLOTS; the
    // pad slot (SLOTS-1) gets a duplicate of slot 0.  The last instruction is partial (LAST_LANES
    // active; each buffer has room for a whole one).
    uint32_t doff[DMA_PER_WAVE];  // per-lane byte offsets of this wave's DMA slots in an image
#pragma unroll
    for (int i = 0; i < DMA_PER_WAVE; i++) {
        const int P = (wave + NW * i) * 64 + lane;
        const int row = min(P / SLOTS, BN - 1), sl = P % SLOTS;
        doff[i] = (uint32_t)(row * ldb + 16 * (sl == SLOTS - 1 ? 0 : sl));
    }
    const uint32_t lds_tiles = __builtin_amdgcn_readfirstlane(lds_addr(tiles));
    const uint32_t lds_ring = __builtin_amdgcn_readfirstlane(lds_addr(ring));
    // the image of tile rows [r0, r0 + BN), chunk c, into buffer buf: every image is whole (the
    // operand rows cover the grid of GR-row groups, its width is whole chunks)
    auto dma_image = [&](int buf, int64_t r0, int c) __attribute__((always_inline)) {
        const unsigned char* src = trainb + r0 * ldb + (int64_t)c * CB;
        const uint32_t lds = lds_tiles + (uint32_t)(buf * TILE);
#pragma unroll
        for (int i = 0; i < DMA_PER_WAVE; i++) {
            const int ins = wave + NW * i;
            if (ins < DMA_INS) {
                if (ins == DMA_INS - 1 && lane >= FT::LAST_LANES) continue;
                dma16s(doff[i], src, lds + (uint32_t)ins * 1024u);
            }
        }
    };
    // the norm terms of the group at row g0: waves 0-3 the fast test's (1-c) tn, waves 4-7 tn
    auto dma_norms = [&](int64_t g0) __attribute__((always_inline)) {
        if (wave < 4) dma4s(4u * lane, a.tnp + g0 + 64 * wave, lds_ring + (uint32_t)(256 * wave));
        else dma4s(4u * lane, a.tnorm + g0 + 64 * (wave - 4), lds_ring + (uint32_t)(4 * GR + 256 * (wave - 4)));
    };

    // keep candidate (L, U) of global row t: the exact test against the current threshold, the
    // candidate store into this lane half's sub-slice, and, if U beats the heap root, a sift-down
    // of the 4-ary max-heap (node n >= 1 in H[n-1], the root in H[hs-1]: the four children
    // 4i+1..4i+4 of node i are one aligned 16-byte read at H[4i]).  Only one lane of a query may
    // run it at a time.
    auto accept = [&](float L, float U, int64_t t) __attribute__((always_inline)) {
        if (!(L <= thr)) return;
        if (ccnt < cap_sub) {
            const int64_t o = q * (int64_t)a.cap + (int64_t)(2 * seg + h) * cap_sub + ccnt;
            a.cand[o] = CandRec{(int32_t)t, L, U};
        }
        ccnt++;
        if (U < root) {
            float* H = topU + jl * hs;
            int i = 0;
            float newroot = U;
            for (;;) {
                if (4 * i + 1 > k - 1) break;
                const float4 cc = *reinterpret_cast<const float4*>(H + 4 * i);
                const float m01 = fmaxf(cc.x, cc.y), m23 = fmaxf(cc.z, cc.w);
                const float cm = fmaxf(m01, m23);
                if (cm <= U) break;
                const int ci = cm == cc.x ? 0 : cm == cc.y ? 1 : cm == cc.z ? 2 : 3;
                H[i == 0 ? hs - 1 : i - 1] = cm;
                if (i == 0) newroot = cm;
                i = 4 * i + 1 + ci;
            }
            H[i == 0 ? hs - 1 : i - 1] = U;
            root = newroot;
            thr = fminf(thr, root);
        }
    };
    // after a round of accepts: the partner lane takes the root
    auto sync_roots = [&](int hh) __attribute__((always_inline)) {
        const float other = __shfl_xor(root, 32);
        if (h != hh) root = other;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    auto publish = [&]() __attribute__((always_inline)) {
        if (qvalid) {
            thr = fminf(thr, root);
            // publish for the other segments of this query (single segment: nobody reads it)
            if (a.nseg > 1 && h == 0 && thr < published) {
                atomicMin(&a.gthr[q], f2o(thr));
                published = thr;
            }
            tf = make_tf(thr);
        }
    };
    // the fast test and the slow path of tile t of the group at row g0 (accumulator Y), as
    // k_gemm_filter's: y = fma(-2, q.t, (1-c) tn) <= tf is a superset of L <= thr; a wave re-checks
    // exactly only when some lane passes
    auto test_tile = [&](const floatx16& Y, int t, int64_t g0) __attribute__((always_inline)) {
        const float* tnpY = ring + BN * t;
        float4 t4[4];
#pragma unroll
        for (int rq = 0; rq < 4; rq++) t4[rq] = *reinterpret_cast<const float4*>(tnpY + 8 * rq + 4 * h);
        uint32_t m = 0;  // bit v = value v passes (built high to low)
#pragma unroll
        for (int v = 15; v >= 0; v--) m = (m << 1) | (uint32_t)(fmaf(-2.0f, Y[v], f4get(t4[v >> 2], v & 3)) <= tf);
        if (!__ballot(m != 0u)) return;
        // the two lanes of a query take turns, so each heap has one writer at a time
        for (int hh = 0; hh < 2; hh++) {
            uint32_t mm = (h == hh) ? m : 0u;
            while (__ballot(mm != 0u)) {
                if (mm != 0u) {
                    const int b = __builtin_ctz(mm);
                    mm &= mm - 1u;
                    // the value by a select tree on the bits of b (no dynamic register index)
                    float lv[16];
#pragma unroll
                    for (int v = 0; v < 16; v++) lv[v] = Y[v];
#pragma unroll
                    for (int lvl = 0; lvl < 4; lvl++) {
                        const bool hi = (b >> lvl) & 1;
#pragma unroll
                        for (int v = 0; v < (16 >> (lvl + 1)); v++) lv[v] = hi ? lv[2 * v + 1] : lv[2 * v];
                    }
                    const int row = BN * t + (b & 3) + 8 * (b >> 2) + 4 * h;
                    const float s = qn + ring[GR + row];
                    const float Gv = fmaf(-2.0f, lv[0], s);
                    const float dl = fmaf(coef, s, eta);
                    const int64_t tt = g0 + row;
                    if (tt < row_end) accept(Gv - dl, Gv + dl, tt);
                }
            }
            sync_roots(hh);
        }
        publish();
    };

    const int ngroups = row_end > row_begin ? (int)((row_end - row_begin + GR - 1) / GR) : 0;
    floatx16 acc[G];
    __syncthreads();  // LDS init above is complete before any DMA lands
    if (ngroups > 0) dma_image(0, row_begin, 0);
    for (int grp = 0; grp < ngroups; grp++) {
        const int64_t g0 = row_begin + (int64_t)grp * GR;
        if (a.nseg > 1 && qvalid) {
            // pick up thresholds published by other segments
            const float gv = o2f(__hip_atomic_load(&a.gthr[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            if (gv < thr) { thr = gv; tf = make_tf(thr); }
        }
#pragma unroll
        for (int t = 0; t < G; t++) acc[t] = floatx16{};
        for (int c = 0; c < nc; c++) {
            const bool more = c + 1 < nc;
#pragma unroll
            for (int t = 0; t < G; t++) {
                // image (grp, c, t) landed; every wave is done with the buffer the next DMA
                // overwrites (the previous image's) and, at a group's first image, with the ring
                wait_dma_barrier();
                if (t + 1 < G) dma_image((t + 1) & 1, g0 + (t + 1) * BN, c);
                else if (more) dma_image(0, g0, c + 1);
                else if (grp + 1 < ngroups) dma_image(0, g0 + GR, 0);
                if (t == 0 && c == 0) dma_norms(g0);
                const unsigned char* ap = tiles + (t & 1) * TILE + j * STRIDE + 16 * h;
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    const bf16x8 A = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(ap + 32 * s));
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A, __builtin_bit_cast(bf16x8, qf[s]), acc[t], 0, 0, 0);
                    // the group's last use of this chunk's fragment s: the next chunk's (the next
                    // group's first) replaces it
                    if (t == G - 1) qf[s] = load_frag(more ? c + 1 : 0, s);
                }
            }
        }
        // (the group's norm terms landed before the second image's barrier: nc G >= 8 images)
#pragma unroll
        for (int t = 0; t < G; t++) test_tile(acc[t], t, g0);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (qvalid) a.cnt[(int64_t)(2 * seg + h) * a.nq + q] = ccnt;
}

// ---------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------
int knn_wide_width(int d) { return d > 256 && d <= 4096 ? (d + 127) / 128 * 128 : 0; }

int knn_wide_group_rows() { return WIDE_GR; }

FilterPlan knn_wide_plan(int k) {
    const size_t lds = (size_t)WIDE_NBUF * WideTile::TILE + ((size_t)2 * WIDE_GR + (size_t)WideTile::BM * heap_stride(k)) * sizeof(float);
    return FilterPlan{WIDE_NW, 1, 1, 2, WIDE_NBUF, WideTile::BM, lds};
}

// The plan knn_wide_plan makes: out[8] = {nw, qg, rg, minw, nbuf, bm, lds, train rows per group}.  A
// test hook like knn_fused_debug_plan (tests/test_plan_lattice_cpu.py).  No GPU call.
extern "C" int knn_debug_wide_plan(int k, long long* out) {
    if (!out || k < 1) return -1;
    const FilterPlan f = knn_wide_plan(k);
    const long long v[8] = {f.nw, f.qg, f.rg, f.minw, f.nbuf, f.bm, (long long)f.lds, knn_wide_group_rows()};
    for (int i = 0; i < 8; i++) out[i] = v[i];
    return 0;
}

hipError_t knn_wide_occupancy(int k, int* blocks_per_cu) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, reinterpret_cast<const void*>(&k_gemm_wide),
                                                        64 * WIDE_NW, knn_wide_plan(k).lds);
}

hipError_t knn_launch_wide(const GemmFilterArgs& a, hipStream_t st) {
    // packed bf16 operand rows of whole chunks; segments of whole groups (the last one may end
    // inside the operand's pad rows); the LDS of k <= 128
    if (knn_wide_width(a.d) != a.d || a.ld_t != a.d || a.ld_q != a.d || a.k < 1 || a.k > 128 || a.nseg < 1 ||
        a.seg_len % WIDE_GR || a.n_qtiles < 1)
        return hipErrorInvalidValue;
    const FilterPlan f = knn_wide_plan(a.k);
    if (f.lds > 160 * 1024) return hipErrorInvalidValue;
    void* args[] = {const_cast<GemmFilterArgs*>(&a)};
    const dim3 grid((unsigned)((int64_t)a.n_qtiles * a.nseg));
    hipError_t e = hipLaunchKernel(reinterpret_cast<const void*>(&k_gemm_wide), grid, dim3(64 * f.nw), args, f.lds, st);
    if (e != hipSuccess) return e;
    KNN_LAUNCH_CHECK();
    return hipSuccess;
}
