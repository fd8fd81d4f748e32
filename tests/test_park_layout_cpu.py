"""CPU-side checks of the parked passes' ring (k_gemm_fused<..., PARK>, DESIGN.md "Parked
passes"), through the host views of the kernel's own offset function (knn_fused_debug_park,
knn_fused_debug_park_off): every thread's record slots are aligned, disjoint, past the tile
buffers and inside the plan's LDS, and a wave's ds_read_b128 of one (slot, quarter) is
conflict-free under the b128 lane groups.  No GPU call."""
import ctypes
import itertools

import numpy as np
import pytest

from test_fused_tile_image import B128_GROUPS, PLAN_FIELDS, PLAN_GRID

CAP = 160 * 1024 - 256


@pytest.fixture(scope="module")
def lib(knn):
    lib = knn.load_library()
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.knn_fused_debug_park.argtypes = [I, P]
    lib.knn_fused_debug_park.restype = I
    lib.knn_fused_debug_park_off.argtypes = [I, I, I, I]
    lib.knn_fused_debug_park_off.restype = ctypes.c_longlong
    lib.knn_fused_debug_plan.argtypes = [I, I, ctypes.c_longlong, I, I, I, I, I, P]
    lib.knn_fused_debug_plan.restype = I
    lib.knn_fused_debug_image.argtypes = [I, I, P]
    lib.knn_fused_debug_image.restype = I
    return lib


def ring(lib, qg):
    out = np.zeros(5, np.int64)
    assert lib.knn_fused_debug_park(qg, out.ctypes.data) == 0
    return dict(zip(("slots", "threads", "tiles", "begin", "end"), out.tolist()))


def plan(lib, k, nq, qg):
    out = np.zeros(len(PLAN_FIELDS), np.int64)
    assert lib.knn_fused_debug_plan(128, k, nq, 256, qg, 0, 5, 1, out.ctypes.data) == 0
    return dict(zip(PLAN_FIELDS, out.tolist()))


def offsets(lib, qg):
    """off[t, s, v]: v < 4 the 16-byte quarters, v == 4 the word."""
    r = ring(lib, qg)
    off = np.array([[[lib.knn_fused_debug_park_off(qg, t, s, v) for v in range(5)]
                     for s in range(r["slots"])] for t in range(r["threads"])], np.int64)
    return r, off


@pytest.mark.parametrize("qg", [1, 2])
def test_ring_geometry(lib, qg):
    r = ring(lib, qg)
    im = np.zeros(8, np.int32)
    assert lib.knn_fused_debug_image(64, 1 if qg == 2 else 2, im.ctypes.data) == 0  # rows of 128 bytes
    assert r["threads"] == 512 and r["slots"] >= 2
    assert r["slots"] & (r["slots"] - 1) == 0            # the kernel masks a slot index
    assert r["tiles"] == (16 if qg == 2 else 8) * int(im[7]) == 80 * 1024
    assert r["begin"] >= r["tiles"] + 16                  # (the scan rotation's word lies between)
    assert r["end"] - r["begin"] == r["slots"] * r["threads"] * (64 + 4)
    # out-of-range arguments have no slot
    for t, s, v in [(-1, 0, 0), (512, 0, 0), (0, r["slots"], 0), (0, -1, 0), (0, 0, 5), (0, 0, -1)]:
        assert lib.knn_fused_debug_park_off(qg, t, s, v) == -1
    assert lib.knn_fused_debug_park_off(3, 0, 0, 0) == -1


@pytest.mark.parametrize("qg", [1, 2])
def test_offsets_aligned_disjoint_and_inside(lib, qg):
    r, off = offsets(lib, qg)
    assert (off >= 0).all()
    assert (off[:, :, :4] % 16 == 0).all() and (off[:, :, 4] % 4 == 0).all()
    # every byte of every record: pairwise disjoint, past the tile buffers, inside the ring
    used = np.zeros(r["end"], np.int32)
    for v in range(5):
        for b in range(16 if v < 4 else 4):
            np.add.at(used, (off[:, :, v] + b).ravel(), 1)
    assert used.max() == 1
    assert used[:r["begin"]].sum() == 0
    assert used[r["begin"]:].sum() == r["slots"] * r["threads"] * 68 == r["end"] - r["begin"]
    # ... and inside the LDS of both int8 plans (k <= 16 and k <= 32 lists)
    for k in (10, 32):
        f = plan(lib, k, 100000 if qg == 2 else 3125, qg)
        assert f["i8"] == 1 and f["qg"] == qg and f["has_kernel"] == 1, f
        assert r["end"] <= f["lds"] <= CAP, (f, r)


@pytest.mark.parametrize("qg", [1, 2])
def test_flush_reads_are_conflict_free(lib, qg):
    """ds_read_b128 of one (slot, quarter) by the 64 lanes of each of the eight waves: inside each
    of the four 16-lane groups every one of the 64 banks is touched once; the word reads
    (ds_read_b32, two groups of 32 lanes, 32 banks) likewise."""
    r, off = offsets(lib, qg)
    for w, s, v in itertools.product(range(8), range(r["slots"]), range(4)):
        a = off[64 * w:64 * w + 64, s, v]
        for g in B128_GROUPS:
            banks = np.concatenate([(a[g] // 4 + i) % 64 for i in range(4)])
            assert len(set(banks.tolist())) == 64, (w, s, v)
    for w, s in itertools.product(range(8), range(r["slots"])):
        a = off[64 * w:64 * w + 64, s, 4]
        for half in (a[:32], a[32:]):
            assert len(set(((half // 4) % 32).tolist())) == 32, (w, s)


def test_int8_plans_of_the_grid_fit(lib):
    """The int8 points of the plan grid (ring included in lds) stay under 160 KiB - 256."""
    out = np.zeros(len(PLAN_FIELDS), np.int64)
    n = 0
    g = dict(PLAN_GRID, i8=[1])
    for d, k, nq, cus, mp, qg, heaps, i8 in itertools.product(*g.values()):
        assert lib.knn_fused_debug_plan(d, k, nq, cus, qg, heaps, mp, i8, out.ctypes.data) == 0
        f = dict(zip(PLAN_FIELDS, out.tolist()))
        if f["nw"] == 0:
            continue
        n += 1
        assert 0 < f["lds"] <= CAP and f["has_kernel"] == 1, ((d, k, nq, cus, mp, qg, heaps), f)
        assert f["lds"] >= ring(lib, f["qg"])["tiles"] + 16
    assert n > 0
