"""The local outlier factor on the GPU (knn_lof_fit_device / knn_lof_score_device /
knn_lof_lists_device; k_lof_compact, k_lof_lrd, k_lof_score).

Bar: exact equality.  kd, lrd and lof are compared bit for bit with test_lof_cpu's numpy
restatement fed the lists the same context exports; the lists themselves are compared with a
brute force on the CPU where that is cheap; the MFMA-filtered and the multi-pass contexts return the
bits of the direct one.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_sweep import _dev
from test_lof_cpu import (CHEBYSHEV, EUCLIDEAN, MANHATTAN, brute_lists, lof_novelty_reference, lof_reference,
                          mixed_rows)
from test_regress_cpu import fbits

pytestmark = pytest.mark.gpu

METRICS = {EUCLIDEAN: "euclidean", MANHATTAN: "manhattan", CHEBYSHEV: "chebyshev"}
NT_FILTER = 16_447          # the filter tests' small set (test_filter_width_cpu.NT): tails, nt % 64 != 0


def dbits(x):
    """float64 array -> uint64 bit patterns, every NaN mapped to one pattern."""
    x = np.ascontiguousarray(x, np.float64)
    return np.where(np.isnan(x), np.uint64(0x7FF8000000000000), x.view(np.uint64))


def _rows_dev(x):
    """Device rows of the narrowest 16-byte-aligned pitch, as a column view of the true width."""
    import torch
    n, d = x.shape
    t = torch.zeros((n, (d + 3) // 4 * 4), dtype=torch.float32)
    t[:, :d] = torch.from_numpy(np.ascontiguousarray(x))
    return t.to("cuda:0")[:, :d]


def _fit(knn, ctx, xd, k_lo, k_hi, expect=None):
    """lof_fit_device with every output: (kd, lrd, lof, dist, idx) as host arrays; expect: the
    status a KnnError must carry (the outputs are written before it is raised)."""
    import torch
    n, Kr, dev = xd.shape[0], k_hi - k_lo + 1, xd.device
    kd = torch.empty((n, Kr), dtype=torch.float32, device=dev)
    lrd = torch.empty((n, Kr), dtype=torch.float64, device=dev)
    lof = torch.empty((Kr, n), dtype=torch.float32, device=dev)
    dist = torch.empty((n, k_hi + 1), dtype=torch.float32, device=dev)
    idx = torch.empty((n, k_hi + 1), dtype=torch.int32, device=dev)
    if expect is None:
        model = ctx.lof_fit_device(xd, k_lo, k_hi, lof=lof, dist=dist, idx=idx, kd=kd, lrd=lrd)
        assert model.kd is kd and model.lrd is lrd and model.lof is lof and (model.k_lo, model.k_hi) == (k_lo, k_hi)
    else:
        with pytest.raises(knn.KnnError) as e:
            ctx.lof_fit_device(xd, k_lo, k_hi, lof=lof, dist=dist, idx=idx, kd=kd, lrd=lrd)
        assert e.value.status == expect, e.value
    return tuple(t.cpu().numpy() for t in (kd, lrd, lof, dist, idx))


def _same_as_reference(got, k_lo, k_hi, metric, too_few=False):
    kd, lrd, lof, dist, idx = got
    rkd, rlrd, rlof, few = lof_reference(idx, dist, 0, k_lo, k_hi, metric)
    assert few == too_few
    assert np.array_equal(fbits(kd), fbits(rkd)), "kd"
    assert np.array_equal(dbits(lrd), dbits(rlrd)), "lrd"
    assert np.array_equal(fbits(lof), fbits(rlof)), "lof"
    return rkd, rlrd, rlof


@pytest.fixture(scope="module")
def mixed(knn):
    """The small mixed case per metric: the rows on the device, a direct context's fit over 1..7
    and the brute-force lists."""
    x = mixed_rows()
    xd = _rows_dev(x)
    out = {}
    for metric, name in METRICS.items():
        c = knn.Context(0, algo="direct", metric=name)
        try:
            out[metric] = _fit(knn, c, xd, 1, 7)
        finally:
            c.close()
    return x, xd, out


@pytest.mark.parametrize("metric", sorted(METRICS))
def test_small_mixed(knn, mixed, metric):
    """n = 193, d = 5, range 1..7: 9 copies of one row (a row absent from its own list, the 1e-10
    path), 3 copies of another (zero distances in a finite sum), one far row."""
    x, xd, out = mixed
    got = out[metric]
    kd, lrd, lof, dist, idx = got
    bidx, bdist = brute_lists(x, x, 8, metric)
    assert np.array_equal(idx, bidx) and np.array_equal(fbits(dist), fbits(bdist))
    assert 192 not in idx[192]
    _same_as_reference(got, 1, 7, metric)
    assert np.isfinite(lof).all() and (lrd[3] > 1e9).all() and lof[6, 57] > 5
    # the helpers, on the device tensor and on the host array
    import torch
    m = knn.lof_max(torch.from_numpy(lof).to("cuda:0"))
    assert np.array_equal(m.cpu().numpy(), lof.max(axis=0)) and np.array_equal(knn.lof_max(lof), lof.max(axis=0))
    want = np.flatnonzero(lof.max(axis=0) > 1.5)
    assert 57 in want and len(want) < 60
    assert np.array_equal(knn.lof_outliers(m).cpu().numpy(), want) and np.array_equal(knn.lof_outliers(lof.max(axis=0)), want)
    assert np.array_equal(knn.lof_outliers(lof[6], 3.0), np.flatnonzero(lof[6] > 3.0))


def test_lof_device_is_the_fit_scores(knn, mixed):
    """lof_device (scores alone, lists in workspace) returns the fit's lof; a single k is its row."""
    x, xd, out = mixed
    c = knn.Context(0, algo="direct")
    try:
        assert np.array_equal(fbits(c.lof_device(xd, 1, 7).cpu().numpy()), fbits(out[EUCLIDEAN][2]))
        one = c.lof_device(xd, 5).cpu().numpy()
        assert one.shape == (1, 193) and np.array_equal(fbits(one[0]), fbits(out[EUCLIDEAN][2][4]))
        sub = c.lof_device(xd, 3, 5).cpu().numpy()
        assert np.array_equal(fbits(sub), fbits(out[EUCLIDEAN][2][2:5]))
    finally:
        c.close()


@pytest.mark.parametrize("k_lo,k_hi", [(60, 70), (64, 64)])
def test_range_across_the_lane_boundary(knn, k_lo, k_hi):
    """n = 300: lists of 71 entries and k = 60..70 (two registers per lane), and the single k = 64."""
    x = np.random.default_rng(5).standard_normal((300, 6)).astype(np.float32)
    x[100:104] = x[7]
    c = knn.Context(0, algo="direct")
    try:
        got = _fit(knn, c, _rows_dev(x), k_lo, k_hi)
    finally:
        c.close()
    bidx, bdist = brute_lists(x, x, k_hi + 1, EUCLIDEAN)
    assert np.array_equal(got[4], bidx) and np.array_equal(fbits(got[3]), fbits(bdist))
    _same_as_reference(got, k_lo, k_hi, EUCLIDEAN)
    assert np.isfinite(got[2]).all()


def test_too_few_rows(knn):
    """n = 5, range 1..7: KNN_ERANGE; k <= 4 finite and the restatement's, k >= 5 NaN."""
    x = np.random.default_rng(2).standard_normal((5, 3)).astype(np.float32)
    c = knn.Context(0, algo="direct")
    try:
        got = _fit(knn, c, _rows_dev(x), 1, 7, expect=knn.KNN_ERANGE)
    finally:
        c.close()
    assert (got[4][:, 5:] == -1).all()
    _same_as_reference(got, 1, 7, EUCLIDEAN, too_few=True)
    assert np.isfinite(got[2][:4]).all() and np.isnan(got[2][4:]).all() and np.isnan(got[1][:, 4:]).all()


@pytest.fixture(scope="module")
def filter_rows(oracle):
    return {d: oracle.gen(71 + d, 0, 0, NT_FILTER, d)[0] for d in (64, 96)}


@pytest.mark.parametrize("d", [64, 96])
def test_mfma_filter_gives_the_direct_bits(knn, filter_rows, d):
    """d = 64 and d = 96 (operands padded to 128), 16,447 rows, k = 20: the context that runs the
    bf16 MFMA filter returns the bits of the direct one, and both the restatement's."""
    xd = _rows_dev(filter_rows[d])
    out = {}
    for algo in ("gemm_bf16", "direct"):
        c = knn.Context(0, algo=algo)
        try:
            out[algo] = _fit(knn, c, xd, 20, 20)
            st = c.stats()
        finally:
            c.close()
        if algo == "gemm_bf16":
            assert st["filter_operands"] == "bf16 rounded" and st["filter_width"] == (64 if d == 64 else 128), st
        else:
            assert st["filter_operands"] is None, st
    for a, b in zip(out["gemm_bf16"], out["direct"]):
        assert np.array_equal(a.view(np.uint32 if a.dtype != np.float64 else np.uint64),
                              b.view(np.uint32 if b.dtype != np.float64 else np.uint64))
    _same_as_reference(out["gemm_bf16"], 20, 20, EUCLIDEAN)
    assert np.isfinite(out["direct"][2]).all()


def test_determinism_and_passes(knn, filter_rows, monkeypatch):
    """Two calls return the same bits, and a context whose GEMM pass loop is cut into four pieces
    (KNN_WS_QUERIES, the knob of test_gpu_list_passes) the bits of the one that runs one pass."""
    xd = _rows_dev(filter_rows[64])
    c = knn.Context(0, algo="gemm_bf16")
    try:
        a = _fit(knn, c, xd, 10, 12)
        b = _fit(knn, c, xd, 10, 12)
    finally:
        c.close()
    monkeypatch.setenv("KNN_WS_QUERIES", "5000")
    c = knn.Context(0, algo="gemm_bf16")
    try:
        p = _fit(knn, c, xd, 10, 12)
        assert c.stats()["filter_operands"] == "bf16 rounded"
    finally:
        c.close()
    for x, y, z in zip(a, b, p):
        v = np.uint64 if x.dtype == np.float64 else np.uint32
        assert np.array_equal(x.view(v), y.view(v)) and np.array_equal(x.view(v), z.view(v))
    assert np.isfinite(a[2]).all()


@pytest.mark.parametrize("metric", sorted(METRICS))
def test_novelty(knn, mixed, metric):
    """67 queries against the 193 rows through LofModel.score_device, one query equal to a train
    row (it keeps that row at distance 0)."""
    import torch
    x, xd, out = mixed
    q = np.random.default_rng(9).standard_normal((67, 5)).astype(np.float32) * np.float32(1.5)
    q[11] = x[30]
    qd = _rows_dev(q)
    c = knn.Context(0, algo="direct", metric=METRICS[metric])
    try:
        model = c.lof_fit_device(xd, 2, 7)
        got = model.score_device(qd).cpu().numpy()
        # the lists the same context reports for these queries
        pred = torch.empty(67, dtype=torch.int32, device="cuda:0")
        dist = torch.empty((67, 7), dtype=torch.float32, device="cuda:0")
        idx = torch.empty((67, 7), dtype=torch.int32, device="cuda:0")
        c.predict_device(xd, torch.zeros(193, dtype=torch.int32, device="cuda:0"), qd, 7, 1, pred, dist, idx)
        kd, lrd = model.kd.cpu().numpy(), model.lrd.cpu().numpy()
    finally:
        c.close()
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    bidx, bdist = brute_lists(x, q, 7, metric)
    assert np.array_equal(idx, bidx) and np.array_equal(fbits(dist), fbits(bdist))
    assert idx[11, 0] == 30 and dist[11, 0] == 0
    assert np.array_equal(fbits(kd), fbits(out[metric][0][:, 1:])) and np.array_equal(dbits(lrd), dbits(out[metric][1][:, 1:]))
    want, few = lof_novelty_reference(idx, dist, kd, lrd, 2, 7, metric)
    assert not few and got.shape == (6, 67)
    assert np.array_equal(fbits(got), fbits(want)) and np.isfinite(got).all()


def test_lists_already_held(knn, mixed):
    """lof_lists_device on the lists loo_device exports (self-removed, [n][7]) and on the fit's own
    export (before self-removal, self_base = 0) equals lof_device; validation of the caller's lists."""
    import torch
    x, xd, out = mixed
    kd0, lrd0, lof0, dist0, idx0 = out[EUCLIDEAN]
    c = knn.Context(0, algo="direct")
    try:
        dist = torch.empty((193, 7), dtype=torch.float32, device="cuda:0")
        idx = torch.empty((193, 7), dtype=torch.int32, device="cuda:0")
        c.loo_device(xd, torch.zeros(193, dtype=torch.int32, device="cuda:0"), 7, 1, dist=dist, idx=idx)
        lof, kd, lrd = c.lof_lists_device(idx, dist, 1, 7, kd=True, lrd=True)
        assert np.array_equal(fbits(lof.cpu().numpy()), fbits(lof0))
        assert np.array_equal(fbits(kd.cpu().numpy()), fbits(kd0)) and np.array_equal(dbits(lrd.cpu().numpy()), dbits(lrd0))
        lof, _, _ = c.lof_lists_device(_dev(idx0), _dev(dist0), 1, 7, self_base=0)
        assert np.array_equal(fbits(lof.cpu().numpy()), fbits(lof0))
        # a sub-range reads the first k_hi entries of wider rows
        lof, _, _ = c.lof_lists_device(idx, dist, 2, 4)
        assert np.array_equal(fbits(lof.cpu().numpy()), fbits(lof0[1:4]))
        # an index equal to n, a negative index that is not the missing marker, a negative and a
        # NaN distance: KNN_EINVAL from the validation kernel, and no gather read with them
        for what, at, val, text in (("idx", (17, 3), 193, "lof: a list index is outside [0, n)"),
                                    ("idx", (0, 0), -2, "lof: a list index is outside [0, n)"),
                                    ("dist", (50, 6), -1.0, "lof: a neighbour distance is NaN or negative"),
                                    ("dist", (192, 0), float("nan"), "lof: a neighbour distance is NaN or negative")):
            bi, bd = idx.clone(), dist.clone()
            (bi if what == "idx" else bd)[at] = val
            with pytest.raises(knn.KnnError) as e:
                c.lof_lists_device(bi, bd, 1, 7)
            assert e.value.status == knn.KNN_EINVAL and text in str(e.value), (what, e.value)
        # the context is usable afterwards
        lof, _, _ = c.lof_lists_device(idx, dist, 1, 7)
        assert np.array_equal(fbits(lof.cpu().numpy()), fbits(lof0))
    finally:
        c.close()


def test_strided_rows(knn, mixed):
    """The train tensor is a column view of a wider tensor whose other columns hold NaN."""
    import torch
    x, xd, out = mixed
    parent = torch.full((194, 12), float("nan"), dtype=torch.float32)
    parent[:193, 4:9] = torch.from_numpy(x)
    pd = parent.to("cuda:0")
    view = pd[:193, 4:9]
    assert view.stride(0) == 12 and view.data_ptr() % 16 == 0
    q = x[:40] + np.float32(0.25)
    qparent = torch.full((41, 8), float("nan"), dtype=torch.float32)
    qparent[:40, :5] = torch.from_numpy(q)
    qview = qparent.to("cuda:0")[:40, :5]
    c = knn.Context(0, algo="direct")
    try:
        got = _fit(knn, c, view, 1, 7)
        model = c.lof_fit_device(view, 1, 7)
        nov = model.score_device(qview).cpu().numpy()
        ref = c.lof_fit_device(xd, 1, 7).score_device(_rows_dev(q)).cpu().numpy()
    finally:
        c.close()
    for a, b in zip(got, out[EUCLIDEAN]):
        v = np.uint64 if a.dtype == np.float64 else np.uint32
        assert np.array_equal(a.view(v), b.view(v))
    assert np.array_equal(fbits(nov), fbits(ref)) and np.isfinite(nov).all()
    assert np.array_equal(fbits(pd.cpu().numpy()), fbits(parent.numpy()))


def test_profile_names_the_stages(knn, mixed):
    x, xd, out = mixed
    c = knn.Context(0, algo="direct", profile=1)
    try:
        lof = c.lof_device(xd, 1, 7).cpu().numpy()
        times = c.stage_times()
    finally:
        c.close()
    assert "lof" in times and times["lof"] > 0 and "direct_tile" in times, times
    assert np.array_equal(fbits(lof), fbits(out[EUCLIDEAN][2]))


def test_argument_checks(knn, mixed):
    """k_lo < 1, k_hi > 255, k_lo > k_hi and no output asked for: KNN_EINVAL and the library's text,
    through the three entry points of the C ABI."""
    import torch
    x, xd, out = mixed
    c = knn.Context(0, algo="direct")
    lib, ref = knn.load_library(), ctypes.byref
    try:
        tr = knn._device_dataset(xd)
        buf = torch.zeros(193 * 256, dtype=torch.float64, device="cuda:0").data_ptr()
        idx = torch.zeros((193, 256), dtype=torch.int32, device="cuda:0").data_ptr()

        def calls(k_lo, k_hi, o):
            yield lib.knn_lof_fit_device(c.h, ref(tr), k_lo, k_hi, o, None, None, None, None, None)
            yield lib.knn_lof_score_device(c.h, ref(tr), ref(tr), k_lo, k_hi, buf, buf, o, None)
            yield lib.knn_lof_lists_device(c.h, 193, k_hi, idx, buf, 256, -1, k_lo, k_hi, None, None, o, None)

        for k_lo, k_hi in ((0, 7), (1, 256), (5, 4), (-3, -3)):
            for st in calls(k_lo, k_hi, buf):
                assert st == knn.KNN_EINVAL
                assert lib.knn_last_error(c.h).decode() == f"lof: k_lo={k_lo}, k_hi={k_hi} outside 1 <= k_lo <= k_hi <= 255"
        for st in calls(1, 7, None):
            assert st == knn.KNN_EINVAL
            assert lib.knn_last_error(c.h).decode() == "lof: kd, lrd and lof are all NULL"
        # the lists' length must be the range's
        assert lib.knn_lof_lists_device(c.h, 193, 9, idx, buf, 256, -1, 1, 7, None, None, buf, None) == knn.KNN_EINVAL
        assert lib.knn_lof_lists_device(c.h, 193, 7, idx, buf, 256, 0, 1, 7, None, None, buf, None) == knn.KNN_EINVAL
        assert lib.knn_lof_lists_device(c.h, 193, 8, idx, buf, 256, 5, 1, 7, None, None, buf, None) == knn.KNN_EINVAL
        # an empty set is no error
        assert lib.knn_lof_lists_device(c.h, 0, 7, None, None, 7, -1, 1, 7, None, None, buf, None) == knn.KNN_OK
    finally:
        c.close()
