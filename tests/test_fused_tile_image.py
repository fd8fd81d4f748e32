"""CPU-side checks of the fused filter's tile copy, schedule and plan (k_gemm_fused), through the
host views the library exports of the functions and tile geometry its kernel runs
(knn_fused_debug_image, knn_fused_debug_read_off, knn_fused_debug_piece_map,
knn_fused_debug_schedule, knn_fused_debug_plan): the bank model of the LDS image's fragment reads,
the piece map of the LDS-DMA (which wave issues which 1 KiB piece, and from which source bytes),
the balanced schedule's cover and rotations, and the plan rule's shapes (each has a kernel and
fits the LDS).  No GPU call."""
import ctypes
import itertools
import math

import numpy as np
import pytest

NW = 8
# (d, rg, tiles per barrier group) of the product's 8-wave shapes: 64-query waves on 32-row
# tiles in octets (A, B), 32-query waves on 64-row tiles in quads (A's 8-GPU share) or pairs
# (d = 256), C1's 32-row tiles in quads
SHAPES = [(128, 1, 8), (64, 1, 8), (128, 2, 4), (64, 2, 4), (256, 2, 2), (256, 1, 4)]


@pytest.fixture(scope="module")
def lib(knn):
    lib = knn.load_library()
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.knn_fused_debug_piece_map.argtypes = [I, I, I, I, P, P, P]
    lib.knn_fused_debug_piece_map.restype = I
    lib.knn_fused_debug_schedule.argtypes = [ctypes.c_longlong, I, I, I, I, P, I, P, P]
    lib.knn_fused_debug_image.argtypes = [I, I, P]
    lib.knn_fused_debug_image.restype = I
    lib.knn_fused_debug_read_off.argtypes = [I, I, I, I, I, I, I, P, P]
    lib.knn_fused_debug_read_off.restype = I
    lib.knn_fused_debug_schedule.restype = I
    lib.knn_fused_debug_plan.argtypes = [I, I, ctypes.c_longlong, I, I, I, I, I, P]
    lib.knn_fused_debug_plan.restype = I
    return lib


def image(lib, d, rg):
    """The kernel's tile geometry (FilterTile): a dict of its constants."""
    out = np.zeros(8, np.int32)
    assert lib.knn_fused_debug_image(d, rg, out.ctypes.data) == 0
    return dict(zip(("rb", "bn", "stride", "slots", "hdr", "hs", "ins", "tile"), out.tolist()))


def piece_map(lib, d, rg, tiles):
    ins_max = image(lib, d, rg)["ins"]
    src = np.zeros(64 * ins_max, np.uint32)
    issued = np.full(tiles * ins_max, -1, np.int32)
    per_wave = np.zeros(NW, np.int32)
    ins = lib.knn_fused_debug_piece_map(d, NW, rg, tiles, src.ctypes.data, issued.ctypes.data, per_wave.ctypes.data)
    assert ins == ins_max
    return ins, src, issued[:tiles * ins].reshape(tiles, ins), per_wave


# ds_read_b128 serves a wave in four passes of 16 lanes: these two sets and their +32 twins
B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
               [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
B128_GROUPS += [[l + 32 for l in g] for g in B128_GROUPS[:2]]


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("rg", [1, 2])
def test_bank_model_of_fragment_and_norm_reads(lib, d, rg):
    """The addresses are the kernel's own (fused_frag_off / fused_norm_off on FilterTile's
    stride and header offset): every 16-lane pass of every k-step's ds_read_b128 touches 64
    distinct 4-byte banks inside the tile's rows, each read is the 16 bytes of its row the MFMA
    operand wants (the piece map below says which source bytes lie there), and the norm reads
    are broadcasts inside the header (one address per lane half)."""
    im = image(lib, d, rg)
    assert im["rb"] == 2 * d and im["bn"] == 32 * rg and im["hdr"] >= im["bn"] * im["rb"]
    assert im["hdr"] + 16 * im["hs"] <= im["tile"] == 1024 * im["ins"]
    frag, norm = ctypes.c_int(), ctypes.c_int()

    def off(g, lane, s, g4=0):
        assert lib.knn_fused_debug_read_off(d, rg, g, lane & 31, lane >> 5, s, g4, ctypes.byref(frag),
                                            ctypes.byref(norm)) == 0
        return frag.value, norm.value

    for g in range(rg):
        for s in range(im["rb"] // 32):
            for lanes in B128_GROUPS:
                banks = set()
                for lane in lanes:
                    a, _ = off(g, lane, s)
                    row = 32 * g + (lane & 31)
                    assert a % 16 == 0 and row * im["stride"] <= a and a + 16 <= row * im["stride"] + im["rb"]
                    assert a - row * im["stride"] == 16 * (lane >> 5) + 32 * s     # (no swizzle: slot 2s + h)
                    banks |= {(a // 4 + w) % 64 for w in range(4)}
                assert len(banks) == 64, (d, g, s, lanes)
        for g4 in range(4):
            for lanes in B128_GROUPS:
                ns = {off(g, lane, 0, g4)[1] for lane in lanes}
                assert len(ns) == 1
                n = ns.pop()
                # four fp32 norms of rows 32 g + 8 g4 + 4 h ..: inside the header's norm slots
                assert n == im["hdr"] + 4 * (32 * g + 8 * g4 + 4 * (lanes[0] >> 5)) and n + 16 <= im["hdr"] + 4 * im["bn"]


@pytest.mark.parametrize("d,rg,grp", SHAPES)
def test_piece_map_writes_every_slot_once(lib, d, rg, grp):
    """Piece ins lands lane-linear at LDS byte 1024 ins + 16 lane.  Every (row, slot) the
    fragment reads use, and every header slot, is written exactly once per tile, from the bytes
    of the tile block (rows of 2d bytes, then bn fp32 norms and the statistics) that belong
    there; the pad slot of a row and the slack past the header are the only other writes."""
    im = image(lib, d, rg)
    rb, bn, slots, hs, stride, hdr = im["rb"], im["bn"], im["slots"], im["hs"], im["stride"], im["hdr"]
    assert hs == bn // 4 + 1                      # bn fp32 norms + one slot of statistics
    ins, src, issued, per_wave = piece_map(lib, d, rg, 2 * NW)
    assert 64 * (ins - 1) < bn * slots + hs <= 64 * ins
    # every piece of every tile from exactly one wave (the remainder pieces always from the first
    # waves: rotating them measured no faster, so the per-wave counts are not equal)
    assert (issued == 1).all() and per_wave.sum() == 2 * NW * ins
    want = {}
    for row in range(bn):
        for sl in range(rb // 16):
            want[row * stride + 16 * sl] = row * rb + 16 * sl
    for i in range(hs):
        want[hdr + 16 * i] = bn * rb + 16 * i
    seen = set()
    for P in range(64 * ins):
        lds = 16 * P
        assert src[P] % 16 == 0 and src[P] + 16 <= bn * rb + 16 * hs   # inside the tile block
        if lds in want:
            assert src[P] == want[lds], (P, src[P])
            seen.add(lds)
    assert seen == set(want)


def max_splits(nt, k, cap=64 * 32, smax=8):  # knn_capi.cpp max_splits
    best = 1
    for s in range(2, smax + 1):
        e = k * (1.0 + math.log(max(nt / s / k, 1.0))) + 64.0
        if 1.5 * (0.5 * e + 32.0) > cap // s // 2:
            break
        best = s
    return best


# knn_capi.cpp: the host takes the balanced schedule when its pieces per query tile fit the
# candidate list (max_splits) -- of these (query tiles, CUs), at k = 10: A's 196 and 391 tiles at
# every size; 25 tiles (A's 8-GPU share) and 1 tile only where a query tile is one piece
@pytest.mark.parametrize("nqt,cus", [(196, 256), (25, 256), (391, 256), (1, 256)])
@pytest.mark.parametrize("nt", [1_000_000, 40_000, 16_384 + 64 * 3 + 17])
@pytest.mark.parametrize("bn,grp", [(32, 8), (32, 4), (64, 4), (64, 2)])
def test_balanced_schedule_covers_and_rotates(lib, nqt, cus, nt, bn, grp):
    """Every (query tile, 64-row unit) is in exactly one piece.  Where the pieces per query tile
    fit max_splits (the cases the host accepts; asserted for the ones it must) no query tile has
    more pieces than reported.  The rotation the kernel scans with (fused_rot_tiles on the
    schedule's, for bn-row tiles in groups of grp) is a multiple of the group length, inside the
    piece's tiles (fused_piece_tiles), at most a group short of the schedule's, and given only
    to a block whose range lies inside one query tile, which then starts beside the second
    sweep."""
    T = (nt + 63) // 64
    cap = 4 * (nqt + cus) + 16
    grid, nseg = ctypes.c_int(), ctypes.c_int()
    units = np.zeros((cap, 6), np.int64)
    n = lib.knn_fused_debug_schedule(nt, nqt, cus, 0, 0, units.ctypes.data, cap, ctypes.byref(grid), ctypes.byref(nseg))
    tiles = np.zeros((cap, 6), np.int64)
    assert lib.knn_fused_debug_schedule(nt, nqt, cus, bn, grp, tiles.ctypes.data, cap, ctypes.byref(grid),
                                        ctypes.byref(nseg)) == n
    assert 0 < n <= cap and grid.value <= nqt // cus * cus + cus
    units, tiles = units[:n], tiles[:n]
    cover = np.zeros((nqt, T), np.int32)
    pieces = np.zeros(nqt, np.int32)
    per_block = np.bincount(units[:, 0], minlength=grid.value)
    assert per_block.min() >= 1 and per_block.max() <= 2
    tpu = 64 // bn
    for (b, qt, t0, t1, rot, place), (_, _, _, _, r0, ntiles) in zip(units, tiles):
        assert 0 <= qt < nqt and 0 <= t0 < t1 <= T
        cover[qt, t0:t1] += 1
        pieces[qt] += 1
        assert 0 <= rot < t1 - t0
        if rot:
            assert per_block[b] == 1 and place == 0
            # the second sweep: every two-piece block is at unit tau + T - (its range) at time tau
            assert t0 + rot == T - (t1 - t0)
        rows = min(nt, 64 * t1) - 64 * t0
        assert ntiles % max(grp, 2) == 0 and 0 <= ntiles * bn - rows < max(grp, 2) * bn
        assert r0 % grp == 0 and 0 <= r0 < ntiles and rot * tpu - grp < r0 <= rot * tpu
    assert (cover == 1).all()
    assert pieces.max() == nseg.value
    accepted = nseg.value <= max_splits(nt, 10)
    if nqt in (196, 391):
        assert accepted, (nqt, nt, nseg.value)
    if accepted:
        assert pieces.max() <= max_splits(nt, 10)
    if (nqt, nt) == (196, 1_000_000):
        assert (units[:, 4] > 0).sum() >= 0.2 * grid.value   # A: about 23 % of the blocks


PLAN_FIELDS = ("nw", "qg", "rg", "minw", "nbuf", "bm", "lds", "kr", "ls", "i8", "has_kernel")
PLAN_GRID = dict(d=[64, 128, 256], k=[1, 8, 16, 17, 32, 33, 64, 100, 104, 105, 128],
                 nq=[1, 255, 256, 512, 3125, 12500, 25000, 100000, 1000000], num_cus=[64, 256],
                 max_pieces=[1, 2, 5, 8, 16, 32], qg=[0, 1, 2], heaps=[0, 1], i8=[0, 1])


def plan_grid(lib):
    """Every point of PLAN_GRID with the plan knn_fused_plan makes for it."""
    out = np.zeros(len(PLAN_FIELDS), np.int64)
    ptr = out.ctypes.data
    for d, k, nq, cus, mp, qg, heaps, i8 in itertools.product(*PLAN_GRID.values()):
        assert lib.knn_fused_debug_plan(d, k, nq, cus, qg, heaps, mp, i8, ptr) == 0
        yield (d, k, nq, cus, mp, qg, heaps, i8), dict(zip(PLAN_FIELDS, out.tolist()))


def test_every_plan_has_a_kernel_and_fits_the_lds(lib):
    """Over PLAN_GRID (every k at which the rule changes shape, query counts on both sides of the
    fill rule, both forced queries per wave, the forced heap shape, both operand classes): a
    plan has a kernel in the library and fits 160 KiB of LDS less the 256 bytes the plan leaves
    for the kernel's static LDS; 64-query waves only at d <= 128; int8 plans only at d = 128,
    k <= 32; and each shape has the tile buffers the comment block above knn_fused_plan states --
    for the heap shapes, whose buffers depend on k, the largest group that fits."""
    cap = 160 * 1024 - 256
    tile = {(d, rg): image(lib, d, rg)["tile"] for d in (64, 128, 256) for rg in (1, 2)}
    n_plans = 0
    for (d, k, nq, cus, mp, qg, heaps, i8), f in plan_grid(lib):
        at = (d, k, nq, cus, mp, qg, heaps, i8)
        kr = 8 if k <= 16 else 32 if k <= 32 else 104 if (k <= 104 and d == 256 and not heaps) else 0
        if i8 and not (d == 128 and k <= 32):
            assert f["nw"] == 0, at
            continue
        if f["nw"] == 0:
            assert kr == 0 and not f["has_kernel"], at   # only the LDS heaps can be too large
            continue
        n_plans += 1
        assert f["has_kernel"] == 1 and 0 < f["lds"] <= cap, (at, f)
        assert f["kr"] == kr and f["i8"] == i8 and f["bm"] == 32 * f["qg"] * f["nw"] and f["minw"] == 2, (at, f)
        assert f["qg"] == 1 or (f["qg"] == 2 and d <= 128 and kr in (8, 32)), (at, f)
        if qg == 1 or (qg == 2 and d <= 128 and kr in (8, 32)):
            assert f["qg"] == qg, (at, f)
        shape = (f["nw"], f["qg"], f["rg"], f["nbuf"], f["ls"])
        if kr in (8, 32):
            want = (8, 2, 1, 16, 0) if f["qg"] == 2 else (8, 1, 2, 8 if d <= 128 else 4, 1)
            assert shape == want, (at, f)
        elif kr == 104:
            assert shape == (8, 1, 1, 8, 0), (at, f)
        else:
            # LDS heaps: lds = nbuf tiles + the block's heaps (4 hs bytes per query) + 16
            heap8 = (f["lds"] - 16 - f["nbuf"] * tile[d, f["rg"]]) * 256 // f["bm"]
            small = 2 * tile[d, 2] + heap8 // 2 + 16          # the 4-wave shape's LDS
            if d == 64 and small <= cap // 2:
                assert shape == (4, 1, 2, 2, 0), (at, f)
                continue
            fits = [(rg, nb) for rg, nb in ((2, 4), (2, 2), (1, 2)) if nb * tile[d, rg] + heap8 + 16 <= cap]
            assert fits and shape == (8, 1, fits[0][0], fits[0][1], 0), (at, f, fits)
    assert n_plans >= 12960   # (at least the register-list points: 5 of 11 k, and int8 at d = 128)
