"""GPU checks of the radius-neighbour feature (k_radius_tile and the kernels behind it) through
every entry point: counts, class counts, the uniform vote, CSR lists, forced train segments, bf16
rows, special values, leave-one-out, the class-count paths, the weighted vote and regression,
bad arguments, strided rows, determinism, metric switching and the CLI.

Bar: exact equality everywhere, floats compared as uint32 bits.  The yardstick is the numpy
restatement in test_radius_cpu.py (pinned there to scalar definitions) on the float32 distance
matrix of test_metric_cpu.metric_distances; the thresholds are entries of that matrix, so every
non-zero one has a pair with D == thr.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA, PKG_DIR
from test_gpu_strided_rows import Strided, _layout, _packed
from test_metric_cpu import CHEBYSHEV, EUCLIDEAN, FLT_MAX, MANHATTAN, bits, metric_distances, metric_set
from test_radius_cpu import (INV_DIST, INV_SQDIST, METRIC_NAMES, METRICS, RADIUS_SHAPES, UNIFORM, WEIGHT_NAMES,
                             count_vote_reference, radius_reference, radius_regress_reference, radius_thresholds,
                             radius_vote_reference)

pytestmark = pytest.mark.gpu

C = 10
OUTLIER = -7


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def _pad4(x):
    """Device rows are 16-byte aligned: zero columns up to a multiple of 4 (the call passes the
    true d, so they are never read as features)."""
    return np.pad(x, ((0, 0), (0, -x.shape[1] % 4)))


def _np(t):
    return None if t is None else t.cpu().numpy()


@pytest.fixture(scope="module")
def ctxs(knn):
    cs = {m: knn.Context(0, algo="auto", profile=1, metric=METRIC_NAMES[m]) for m in METRICS}
    yield cs
    for c in cs.values():
        c.close()


def _qlabels(nq, C=C):
    return np.random.default_rng(nq).integers(0, C, size=nq).astype(np.int32)


def _run(ctx, d_tr, d_tl, d_te, thr, d, C=C, ql=None, self_base=None, lists=True):
    """count pass with every output, then the fill: numpy arrays."""
    count, pred, correct, cc, off = ctx.radius_count_device(
        d_tr, d_tl, d_te, threshold=thr, num_classes=C, query_labels=None if ql is None else _dev(ql),
        self_base=self_base, outlier_label=OUTLIER, class_counts=True, offsets=True, d=d)
    st = ctx.stage_times()
    assert "radius_count" in st and "direct_tile" not in st and "metric_tile" not in st, st
    idx = dist = None
    if lists:
        idx, dist = ctx.radius_fill_device(d_tr, d_te, off, threshold=thr, self_base=self_base, d=d)
        assert "radius_fill" in ctx.stage_times()
    return _np(count), _np(pred), _np(correct), _np(cc), _np(off), _np(idx), _np(dist)


def _assert_matches(got, ref, tl, ql, what, C=C):
    count, pred, correct, cc, off, idx, dist = got
    rcount, roff, ridx, rdist, rcc = ref
    assert np.array_equal(count, rcount), f"{what}: count"
    assert np.array_equal(cc, rcc), f"{what}: class counts"
    rpred = count_vote_reference(rcc, OUTLIER)
    assert np.array_equal(pred, rpred), f"{what}: pred"
    if ql is not None:
        assert correct.dtype == np.int64 and correct[0] == (rpred == ql).sum(), f"{what}: correct"
    assert off.dtype == np.int64 and np.array_equal(off, roff), f"{what}: offsets"
    if idx is not None:
        assert idx.dtype == np.int32 and np.array_equal(idx, ridx), f"{what}: idx"
        assert np.array_equal(bits(dist), bits(rdist)), f"{what}: dist bits"


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,nt,nq,kind", RADIUS_SHAPES)
def test_radius_shapes(ctxs, oracle, d, nt, nq, kind, metric):
    tr, tl, te = metric_set(oracle, kind, nt, nq, d)
    ql = _qlabels(nq)
    D = metric_distances(tr, te, metric)
    d_tr, d_tl, d_te = _dev(_pad4(tr)), _dev(tl), _dev(_pad4(te))
    for thr in radius_thresholds(D):
        ref = radius_reference(tr, te, thr, metric, labels=tl, C=C, D=D)
        got = _run(ctxs[metric], d_tr, d_tl, d_te, float(thr), d, ql=ql)
        _assert_matches(got, ref, tl, ql, f"thr={thr!r}")


@pytest.mark.parametrize("d,nt,nq,kind", [s for s in RADIUS_SHAPES if s[1] == 65])
def test_radius_distance_bits(ctxs, oracle, d, nt, nq, kind):
    """Under Euclidean the distance a fill reports for a pair is predict_device's exported
    distance for it (k = nt) and the oracle's distance()."""
    import torch
    tr, tl, te = metric_set(oracle, kind, nt, nq, d)
    d_tr, d_tl, d_te = _dev(_pad4(tr)), _dev(tl), _dev(_pad4(te))
    ctx = ctxs[EUCLIDEAN]
    off, idx, dist = ctx.radius_neighbors_device(d_tr, d_te, threshold=3.0e38, d=d)
    off, idx, dist = _np(off), _np(idx), _np(dist)
    assert np.array_equal(off, np.arange(nq + 1) * nt) and np.array_equal(idx, np.tile(np.arange(nt), nq))
    got = dist.reshape(nq, nt)
    pred = torch.empty(nq, dtype=torch.int32, device=d_te.device)
    kd = torch.empty((nq, nt), dtype=torch.float32, device=d_te.device)
    ki = torch.empty((nq, nt), dtype=torch.int32, device=d_te.device)
    ctx.predict_device(d_tr, d_tl, d_te, nt, C, pred, kd, ki, d=d)
    kd, ki = kd.cpu().numpy(), ki.cpu().numpy()
    for q in range(nq):
        assert np.array_equal(bits(got[q, ki[q]]), bits(kd[q]))
    want = np.array([[oracle.lib.oracle_distance(oracle.p(te[q]), oracle.p(tr[t]), d) for t in range(nt)]
                     for q in range(nq)], np.float32)
    assert np.array_equal(bits(got), bits(want))


@pytest.fixture(scope="module")
def seg_set(oracle):
    tr, tl, te = metric_set(oracle, "float", 4096, 257, 11)
    refs = {}
    for m in METRICS:
        D = metric_distances(tr, te, m)
        for thr in radius_thresholds(D)[2:]:
            refs.setdefault(m, []).append((thr, radius_reference(tr, te, thr, m, labels=tl, C=C, D=D)))
    return tr, tl, te, refs


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("splits", [1, 3, 7, 32])
def test_radius_segments(knn, seg_set, splits, metric):
    """Forced train segments: a query's list is the segments' parts in ascending index order."""
    tr, tl, te, refs = seg_set
    ql = _qlabels(len(te))
    d_tr, d_tl, d_te = _dev(_pad4(tr)), _dev(tl), _dev(_pad4(te))
    ctx = knn.Context(0, profile=1, train_splits=splits, metric=METRIC_NAMES[metric])
    try:
        for thr, ref in refs[metric]:
            got = _run(ctx, d_tr, d_tl, d_te, float(thr), tr.shape[1], ql=ql)
            assert ctx.stats()["train_segments"] == splits
            _assert_matches(got, ref, tl, ql, f"splits={splits} thr={thr!r}")
            off, idx = got[4], got[5]
            inner = np.ones(len(idx), bool)
            inner[off[:-1][off[:-1] < len(idx)]] = False          # the first entry of each segment
            assert (np.diff(idx.astype(np.int64), prepend=-1)[inner] > 0).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("metric", METRICS)
def test_radius_bf16(ctxs, oracle, metric):
    import torch
    tr, tl = oracle.gen(23, 0, 0, 1000, 72, kind=1)
    te, _ = oracle.gen(23, 1, 0, 65, 72, kind=1)
    tr[500:600] = tr[:100]
    te[:16] = tr[:16]
    b_tr, b_te = _dev(tr).to(torch.bfloat16), _dev(te).to(torch.bfloat16)
    assert torch.equal(b_tr.to(torch.float32).cpu(), torch.from_numpy(tr))   # bf16-exact values
    D = metric_distances(tr, te, metric)
    ql = _qlabels(65)
    for thr in radius_thresholds(D):
        got = _run(ctxs[metric], b_tr, _dev(tl), b_te, float(thr), 72, ql=ql)
        _assert_matches(got, radius_reference(tr, te, thr, metric, labels=tl, C=C, D=D), tl, ql, f"bf16 thr={thr!r}")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", ["nan_inf", "subnormal", "huge_thr"])
def test_radius_special_values(ctxs, case, metric):
    rng = np.random.default_rng(31)
    nt, nq, d = 1000, 33, 24
    tr = rng.standard_normal((nt, d)).astype(np.float32)
    te = rng.standard_normal((nq, d)).astype(np.float32)
    te[:8] = tr[:8]
    if case == "nan_inf":
        tr[5, 3] = np.nan
        tr[70, 23] = np.inf
        tr[71, 0] = -np.inf
        tr[200] = np.nan
        te[2, 3] = np.nan
        te[9, 23] = np.inf
    elif case == "subnormal":
        tr = (tr * 2.0 ** -140).astype(np.float32)
        te = (te * 2.0 ** -140).astype(np.float32)
    else:
        tr[::7] *= np.float32(1.0e19)       # squares near FLT_MAX, L1 sums past it
        tr[3] = np.float32(3.0e38)
    tl = rng.integers(0, C, size=nt).astype(np.int32)
    D = metric_distances(tr, te, metric)
    fin = np.sort(D[np.isfinite(D)])
    if case == "huge_thr":
        thrs = [np.nextafter(np.float32(FLT_MAX), np.float32(0))]
    else:
        thrs = [np.float32(0.0), fin[len(fin) // 20], fin[len(fin) // 2]]
    if case == "subnormal" and metric != EUCLIDEAN:
        assert 0 < thrs[1] < np.finfo(np.float32).tiny              # a subnormal threshold
    d_tr, d_tl, d_te = _dev(tr), _dev(tl), _dev(te)
    for thr in thrs:
        ref = radius_reference(tr, te, thr, metric, labels=tl, C=C, D=D)
        _assert_matches(_run(ctxs[metric], d_tr, d_tl, d_te, float(thr), d), ref, tl, None, f"{case} thr={thr!r}")


@pytest.mark.parametrize("metric", METRICS)
def test_radius_leave_one_out(knn, ctxs, oracle, metric):
    tr, tl, _ = metric_set(oracle, "grid", 1000, 9, 3)              # duplicated rows, many equal distances
    ctx = ctxs[metric]
    d_tr, d_tl = _dev(_pad4(tr)), _dev(tl)
    D = metric_distances(tr, tr, metric)
    for thr in (np.float32(0.0), radius_thresholds(D)[2]):
        ref = radius_reference(tr, tr, thr, metric, self_base=0, labels=tl, C=C, D=D)
        got = _run(ctx, d_tr, d_tl, d_tr, float(thr), 3, ql=tl, self_base=0)
        _assert_matches(got, ref, tl, tl, f"loo thr={thr!r}")
        off, idx = got[4], got[5]
        for q in range(len(tr)):
            seg = idx[off[q]:off[q + 1]]
            assert q not in seg
            copies = np.nonzero((tr == tr[q]).all(axis=1))[0]
            assert set(copies) - {q} <= set(seg)                    # equal copies of the row stay
        pred, _, count, correct = ctx.radius_loo_device(d_tr, d_tl, threshold=float(thr), num_classes=C,
                                                        outlier_label=OUTLIER, d=3)
        assert np.array_equal(_np(pred), got[1]) and np.array_equal(_np(count), got[0])
        assert _np(correct)[0] == got[2][0]
    # a window of queries further up: self rows 100 + q
    ref = radius_reference(tr, tr[100:357], 0.0, metric, self_base=100, labels=tl, C=C)
    got = _run(ctx, d_tr, d_tl, d_tr[100:357], 0.0, 3, self_base=100)
    _assert_matches(got, ref, tl, None, "loo window")
    with pytest.raises(knn.KnnError) as e:
        ctx.radius_count_device(d_tr, d_tl, d_tr[:257], threshold=1.0, num_classes=C, self_base=1000 - 256, d=3)
    assert e.value.status == knn.KNN_EINVAL


@pytest.mark.parametrize("splits", [0, 3])
@pytest.mark.parametrize("nc", [10, 64, 65, 16384])
def test_radius_class_count_paths(knn, oracle, nc, splits):
    """C = 10 and 64: per-wave LDS counts; 65: no longer fits the LDS block (integer atomics on
    class_counts); 16384: the limit.  With train segments the LDS counts are added, not stored."""
    tr, _, te = metric_set(oracle, "float", 1000, 257, 11)
    rng = np.random.default_rng(nc)
    tl = rng.integers(0, nc, size=len(tr)).astype(np.int32)
    tl[:3] = nc - 1
    ql = _qlabels(len(te), nc)
    D = metric_distances(tr, te, EUCLIDEAN)
    thr = radius_thresholds(D)[2]
    d_tr, d_te = _dev(_pad4(tr)), _dev(_pad4(te))
    ctx = knn.Context(0, profile=1, train_splits=splits)
    try:
        ref = radius_reference(tr, te, thr, EUCLIDEAN, labels=tl, C=nc, D=D)
        _assert_matches(_run(ctx, d_tr, _dev(tl), d_te, float(thr), 11, C=nc, ql=ql, lists=False), ref, tl, ql,
                        f"C={nc}", C=nc)
        # pred alone (no class counts asked): the same votes
        _, pred, correct, _, _ = ctx.radius_count_device(d_tr, _dev(tl), d_te, threshold=float(thr), num_classes=nc,
                                                         query_labels=_dev(ql), outlier_label=OUTLIER, d=11)
        assert np.array_equal(_np(pred), count_vote_reference(ref[4], OUTLIER))
        assert _np(correct)[0] == (count_vote_reference(ref[4], OUTLIER) == ql).sum()
        bad = tl.copy()
        bad[999] = nc                                               # nobody's neighbour need it be
        with pytest.raises(knn.KnnError) as e:
            ctx.radius_count_device(d_tr, _dev(bad), d_te, threshold=float(thr), num_classes=nc, d=11)
        assert e.value.status == knn.KNN_EINVAL
        # ... and the context still works
        count = ctx.radius_count_device(d_tr, None, d_te, threshold=float(thr), d=11)[0]
        assert np.array_equal(_np(count), ref[0])
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def vote_set(oracle):
    tr, tl, te = metric_set(oracle, "float", 1000, 257, 11)
    targets = np.random.default_rng(77).standard_normal(len(tr)).astype(np.float32)
    return tr, tl, te, targets


VOTE_KINDS = [(EUCLIDEAN, UNIFORM), (EUCLIDEAN, INV_DIST), (EUCLIDEAN, INV_SQDIST), (MANHATTAN, INV_DIST),
              (CHEBYSHEV, INV_DIST)]


@pytest.mark.parametrize("metric,weights", VOTE_KINDS)
def test_radius_weighted_vote_and_regression(ctxs, vote_set, metric, weights):
    """q = 0.002: empty segments; q = 0.05: a zero distance among non-zero ones (the queries that
    are copies of train rows); q = 0.5: segments of several 64-entry batches."""
    tr, tl, te, targets = vote_set
    ctx = ctxs[metric]
    ql = _qlabels(len(te))
    D = metric_distances(tr, te, metric)
    d_tr, d_tl, d_te, d_y = _dev(_pad4(tr)), _dev(tl), _dev(_pad4(te)), _dev(targets)
    wname = WEIGHT_NAMES[weights]
    for thr in radius_thresholds(D):
        rcount, roff, ridx, rdist, rcc = radius_reference(tr, te, thr, metric, labels=tl, C=C, D=D)
        rpred, rscores = radius_vote_reference(roff, ridx, rdist, tl, C, weights, metric, OUTLIER)
        rreg = radius_regress_reference(roff, ridx, rdist, targets, weights, metric)
        pred, scores, count, correct = ctx.radius_predict_device(
            d_tr, d_tl, d_te, threshold=float(thr), num_classes=C, weights=wname, outlier_label=OUTLIER,
            query_labels=_dev(ql), d=11)
        assert np.array_equal(_np(count), rcount)
        assert np.array_equal(_np(pred), rpred), (thr, wname)
        assert np.array_equal(bits(_np(scores)), bits(rscores)), (thr, wname)
        assert _np(correct)[0] == (rpred == ql).sum()
        reg, count = ctx.radius_regress_device(d_tr, d_y, d_te, threshold=float(thr), weights=wname, d=11)
        reg = _np(reg)
        empty = rcount == 0
        assert np.isnan(reg[empty]).all() and np.array_equal(bits(reg[~empty]), bits(rreg[~empty])), (thr, wname)
        assert (rpred[empty] == OUTLIER).all() and not bits(_np(scores))[empty].any()
        if thr == radius_thresholds(D)[1]:
            assert empty.any()
        if weights != UNIFORM and thr == radius_thresholds(D)[2]:
            seg0 = [rdist[roff[q]:roff[q + 1]] for q in range(len(te))]
            assert any((s == 0).any() and (s != 0).any() for s in seg0)        # the zero rule is exercised
        if weights == UNIFORM:
            # the vote on the lists equals the count pass
            off, idx, dist = ctx.radius_neighbors_device(d_tr, d_te, threshold=float(thr), d=11)
            vp, vc, vs = ctx.radius_vote_device(off, idx, None, d_tl, C, "uniform", OUTLIER, _dev(ql))
            assert np.array_equal(_np(vp), count_vote_reference(rcc, OUTLIER))
            assert np.array_equal(_np(vs), rcc.astype(np.float32)) and _np(vc)[0] == _np(correct)[0]


def test_radius_vote_refusals(knn, ctxs, vote_set):
    import torch
    tr, tl, te, targets = vote_set
    d_tr, d_tl, d_te = _dev(_pad4(tr)), _dev(tl), _dev(_pad4(te))
    ctx = ctxs[MANHATTAN]
    D = metric_distances(tr, te, MANHATTAN)
    thr = float(radius_thresholds(D)[2])
    with pytest.raises(knn.KnnError) as e:
        ctx.radius_predict_device(d_tr, d_tl, d_te, threshold=thr, num_classes=C, weights="sqdist", d=11)
    assert e.value.status == knn.KNN_EINVAL and "KNN_W_INV_SQDIST" in str(e.value)
    off, idx, dist = ctx.radius_neighbors_device(d_tr, d_te, threshold=thr, d=11)
    for what in ("nan", "negative", "index", "offsets"):
        o2, i2, d2 = off.clone(), idx.clone(), dist.clone()
        if what == "nan":
            d2[5] = float("nan")
        elif what == "negative":
            d2[5] = -1.0
        elif what == "index":
            i2[7] = len(tr)                                          # must not be followed
        else:
            o2[3] = o2[4] + 1                                        # offsets that decrease
        with pytest.raises(knn.KnnError) as e:
            ctx.radius_vote_device(o2, i2, d2, d_tl, C, "distance", OUTLIER)
        assert e.value.status == knn.KNN_EINVAL, what
        with pytest.raises(knn.KnnError) as e:
            ctx.radius_regress_vote_device(o2, i2, d2, _dev(targets), "distance")
        assert e.value.status == knn.KNN_EINVAL, what
    pred, _, _ = ctx.radius_vote_device(off, idx, dist, d_tl, C, "distance", OUTLIER)     # still works
    assert pred.shape[0] == len(te)


def _raw_datasets(knn, d_tr, d_tl, d_te, d):
    return knn._device_dataset(d_tr, d_tl, d), knn._device_dataset(d_te, None, d)


def test_radius_bad_arguments(knn, ctxs, oracle):
    import torch
    tr, tl, te = metric_set(oracle, "float", 1000, 33, 11)
    d_tr, d_tl, d_te = _dev(_pad4(tr)), _dev(tl), _dev(_pad4(te))
    ctx = ctxs[EUCLIDEAN]
    for thr in (float("nan"), -1.0e-30, float(FLT_MAX), float("inf")):
        with pytest.raises(knn.KnnError) as e:
            ctx.radius_count_device(d_tr, d_tl, d_te, threshold=thr, num_classes=C, d=11)
        assert e.value.status == knn.KNN_EINVAL, thr
    trd, ted = _raw_datasets(knn, d_tr, d_tl, d_te, 11)
    st = ctx.lib.knn_radius_count_device(ctx.h, ctypes.byref(trd), ctypes.byref(ted), 1.0, C, -1, -1, None, None, None,
                                         None, None, None, None)
    assert st == knn.KNN_EINVAL                                      # every output NULL
    with pytest.raises(knn.KnnError):
        ctx.radius_count_device(d_tr, d_tl, d_te, radius=1.0, threshold=1.0, num_classes=C, d=11)


@pytest.mark.parametrize("splits", [0, 3])
def test_radius_fill_is_clamped(knn, oracle, splits):
    """A fill with offsets taken at a SMALLER threshold than the one passed: KNN_EINVAL, and no
    element outside the stated segments is written.  idx / dist hold nq * nt elements, so even a
    kernel without the bound would stay inside the allocation: the test checks the clamp."""
    import torch
    tr, tl, te = metric_set(oracle, "float", 1000, 257, 11)
    nt, nq = len(tr), len(te)
    D = metric_distances(tr, te, EUCLIDEAN)
    small, big = radius_thresholds(D)[2], radius_thresholds(D)[3]
    d_tr, d_te = _dev(_pad4(tr)), _dev(_pad4(te))
    ctx = knn.Context(0, train_splits=splits)
    try:
        off = ctx.radius_count_device(d_tr, None, d_te, threshold=float(small), offsets=True, d=11)[4]
        total = int(off[-1].item())
        idx = torch.full((nq * nt,), -5, dtype=torch.int32, device=d_te.device)
        dist = torch.full((nq * nt,), -5.0, dtype=torch.float32, device=d_te.device)
        trd, ted = _raw_datasets(knn, d_tr, None, d_te, 11)
        st = ctx.lib.knn_radius_fill_device(ctx.h, ctypes.byref(trd), ctypes.byref(ted), float(big), -1,
                                            off.data_ptr(), idx.data_ptr(), dist.data_ptr(), None)
        assert st == knn.KNN_EINVAL
        assert "offsets" in ctx.lib.knn_last_error(ctx.h).decode()
        assert (idx[total:] == -5).all() and (dist[total:] == -5.0).all()
        # inside a segment: rows of that query within the larger threshold, or untouched
        _, roff, ridx, _, _ = radius_reference(tr, te, big, EUCLIDEAN, D=D)
        h_off, h_idx = off.cpu().numpy(), idx.cpu().numpy()
        for q in range(nq):
            seg = h_idx[h_off[q]:h_off[q + 1]]
            assert set(seg[seg != -5]) <= set(ridx[roff[q]:roff[q + 1]])
        # the right threshold on the same buffers
        st = ctx.lib.knn_radius_fill_device(ctx.h, ctypes.byref(trd), ctypes.byref(ted), float(small), -1,
                                            off.data_ptr(), idx.data_ptr(), dist.data_ptr(), None)
        assert st == knn.KNN_OK
        _, roff, ridx, rdist, _ = radius_reference(tr, te, small, EUCLIDEAN, D=D)
        assert np.array_equal(idx[:total].cpu().numpy(), ridx)
        assert np.array_equal(bits(dist[:total].cpu().numpy()), bits(rdist))
        assert (idx[total:] == -5).all()
    finally:
        ctx.close()


def test_radius_fill_after_rows_changed(knn, oracle):
    """A segmented fill takes the per-segment counts its count call left in the context.  Rows
    rewritten in place between the two calls make those counts stale: the fill must notice
    (KNN_EINVAL) and still write nothing outside the stated segments; on the restored rows, and on
    a fresh count, it is right again."""
    import torch
    tr, tl, te = metric_set(oracle, "float", 1000, 257, 11)
    nt, nq = len(tr), len(te)
    D = metric_distances(tr, te, EUCLIDEAN)
    thr = radius_thresholds(D)[2]
    ref = radius_reference(tr, te, thr, EUCLIDEAN, D=D)
    d_tr, d_te = _dev(_pad4(tr)), _dev(_pad4(te))
    keep = d_tr.clone()
    ctx = knn.Context(0, train_splits=3)
    try:
        off = ctx.radius_count_device(d_tr, None, d_te, threshold=float(thr), offsets=True, d=11)[4]
        total = int(off[-1].item())
        d_tr[:400] = d_tr[600:1000]                                  # neighbours move between the segments
        idx = torch.full((nq * nt,), -5, dtype=torch.int32, device=d_te.device)
        trd, ted = _raw_datasets(knn, d_tr, None, d_te, 11)
        st = ctx.lib.knn_radius_fill_device(ctx.h, ctypes.byref(trd), ctypes.byref(ted), float(thr), -1,
                                            off.data_ptr(), idx.data_ptr(), None, None)
        assert st == knn.KNN_EINVAL
        assert (idx[total:] == -5).all()
        d_tr.copy_(keep)
        for _ in range(2):                                           # counted again, then from the kept counts
            gi, gd = ctx.radius_fill_device(d_tr, d_te, off, threshold=float(thr), d=11)
            assert np.array_equal(_np(gi), ref[2]) and np.array_equal(bits(_np(gd)), bits(ref[3]))
    finally:
        ctx.close()


@pytest.mark.parametrize("metric", METRICS)
def test_radius_strided_rows(ctxs, oracle, metric):
    """Rows inside a wider, NaN-poisoned parent ("offset" layout: train and query strides differ,
    both column offsets non-zero): the same arrays as on contiguous copies, the parent unchanged."""
    d, nt, nq = 24, 1000, 65
    tr, tl = oracle.gen(53 + d, 0, 0, nt, d)
    te, _ = oracle.gen(53 + d, 1, 0, nq, d)
    te[:16] = tr[:16]
    (tld, tc0), (qld, qc0) = _layout("offset", d)
    T, Q = Strided(tr, tld, tc0, float("nan")), Strided(te, qld, qc0, float("nan"))
    D = metric_distances(tr, te, metric)
    ql = _qlabels(nq)
    d_tl = _dev(tl)
    for thr in radius_thresholds(D)[1:]:
        ref = radius_reference(tr, te, thr, metric, labels=tl, C=C, D=D)
        got = _run(ctxs[metric], T.view, d_tl, Q.view, float(thr), None, ql=ql)
        _assert_matches(got, ref, tl, ql, f"strided thr={thr!r}")
        packed = _run(ctxs[metric], _packed(T.view), d_tl, _packed(Q.view), float(thr), None, ql=ql)
        for a, b in zip(got, packed):
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                  b.view(np.uint32) if b.dtype == np.float32 else b)
    assert T.intact() and Q.intact()


def test_radius_determinism_and_empty(knn, ctxs, vote_set):
    import torch
    tr, tl, te, targets = vote_set
    ctx = ctxs[EUCLIDEAN]
    d_tr, d_tl, d_te = _dev(_pad4(tr)), _dev(tl), _dev(_pad4(te))
    D = metric_distances(tr, te, EUCLIDEAN)
    thr = float(radius_thresholds(D)[3])
    runs = []
    for _ in range(2):
        a = _run(ctx, d_tr, d_tl, d_te, thr, 11)
        p, s, c = ctx.radius_predict_device(d_tr, d_tl, d_te, threshold=thr, num_classes=C, weights="distance", d=11)
        r, _ = ctx.radius_regress_device(d_tr, _dev(targets), d_te, threshold=thr, weights="distance", d=11)
        runs.append([x for x in a if x is not None] + [_np(p), bits(_np(s)), _np(c), bits(_np(r))])
    for x, y in zip(*runs):
        assert np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)
    # nq = 0
    none = d_te[:0]
    count, pred, correct, cc, off = ctx.radius_count_device(d_tr, d_tl, none, threshold=thr, num_classes=C,
                                                            class_counts=True, offsets=True, d=11)
    assert count.numel() == 0 and pred.numel() == 0 and cc.shape == (0, C) and _np(off).tolist() == [0]
    off, idx, dist = ctx.radius_neighbors_device(d_tr, none, threshold=thr, d=11)
    assert idx.numel() == 0 and dist.numel() == 0
    pred, scores, count = ctx.radius_predict_device(d_tr, d_tl, none, threshold=thr, num_classes=C,
                                                    weights="distance", d=11)
    assert pred.numel() == 0 and count.numel() == 0


def test_radius_metric_switching(knn, oracle):
    tr, tl, te = metric_set(oracle, "float", 1000, 65, 11)
    d_tr, d_te = _dev(_pad4(tr)), _dev(_pad4(te))
    ctx = knn.Context(0)
    try:
        for name, metric in (("euclidean", EUCLIDEAN), ("manhattan", MANHATTAN), ("euclidean", EUCLIDEAN),
                             ("chebyshev", CHEBYSHEV)):
            ctx.set_metric(name)
            D = metric_distances(tr, te, metric)
            # radius=r: r * r in binary32 under the Euclidean metric, r itself under the others
            r = np.float32(1.1)
            thr = r * r if metric == EUCLIDEAN else r
            count = ctx.radius_count_device(d_tr, None, d_te, radius=float(r), d=11)[0]
            assert np.array_equal(_np(count), radius_reference(tr, te, thr, metric, D=D)[0])
            assert 0 < _np(count).sum() < D.size
    finally:
        ctx.close()


def _loo_reference(tf, r):
    """radius_reference(tf, tf, r * r, EUCLIDEAN, self_base=0) without the 30,803^2 matrix (15 s of
    CPU): per query only the rows whose feature f lies within 1.001 r are candidates, f the widest
    feature.  Nothing is lost: the float32 sum of non-negative terms never falls below one of them
    (a rounded add of a value >= 0 is monotone), so D >= fl(df_f * df_f), and a row outside the
    window has fl(df_f^2) > fl(r * r)."""
    thr = r * r
    f = int(np.argmax(tf.max(axis=0) - tf.min(axis=0)))
    order = np.argsort(tf[:, f], kind="stable")
    col = tf[order, f]
    lo = np.searchsorted(col, tf[:, f] - r * np.float32(1.001), "left")
    hi = np.searchsorted(col, tf[:, f] + r * np.float32(1.001), "right")
    idx, dist, count = [], [], np.zeros(len(tf), np.int32)
    for q in range(len(tf)):
        cand = np.sort(order[lo[q]:hi[q]])
        D = metric_distances(tf[cand], tf[q:q + 1], EUCLIDEAN)[0]
        m = (D <= thr) & (cand != q)
        idx.append(cand[m])
        dist.append(D[m])
        count[q] = m.sum()
    off = np.zeros(len(tf) + 1, np.int64)
    off[1:] = np.cumsum(count, dtype=np.int64)
    return count, off, np.concatenate(idx).astype(np.int32), np.concatenate(dist)


def _cli_reference(oracle, ds, loo, metric, weights, radius, outlier):
    tf, tl, _ = oracle.read_arff(f"{DATA}/{ds}-train.arff")
    qf, ql, _ = (tf, tl, 0) if loo else oracle.read_arff(f"{DATA}/{ds}-test.arff")
    Ctr = int(tl.max()) + 1
    r = np.float32(radius)
    thr = r * r if metric == EUCLIDEAN else r
    if loo:
        assert metric == EUCLIDEAN
        count, off, idx, dist = _loo_reference(tf, r)
        n = 300                                                     # ... pinned to the plain restatement on a window
        wc, wo, wi, wd, _ = radius_reference(tf, tf[1000:1000 + n], thr, metric, self_base=1000)
        assert np.array_equal(wc, count[1000:1000 + n]) and np.array_equal(wi, idx[off[1000]:off[1000 + n]])
        assert np.array_equal(bits(wd), bits(dist[off[1000]:off[1000 + n]]))
    else:
        count, off, idx, dist, _ = radius_reference(tf, qf, thr, metric, labels=tl, C=Ctr)
    pred, _ = radius_vote_reference(off, idx, dist, tl, Ctr, weights, metric, outlier)
    acc = np.float32((pred == ql).sum()) / np.float32(len(ql))
    return pred, acc, count, len(ql), len(tf)


# The `large` pair (every test row has exact copies among the train rows, so no radius leaves a row
# without neighbours there: its outlier count is 0, and its weighted runs go through the zero
# rule), and the `medium` pair at a radius that leaves most rows without a neighbour.
@pytest.mark.parametrize("ds,flags,radius,loo,metric,weights", [
    ("large", (), "1.5", False, EUCLIDEAN, UNIFORM),
    ("large", ("--metric=manhattan", "--weights=distance"), "2", False, MANHATTAN, INV_DIST),
    ("large", ("--sweep=loo",), "1.5", True, EUCLIDEAN, UNIFORM),
    ("medium", ("--weights=sqdist",), "2", False, EUCLIDEAN, INV_SQDIST),
])
def test_radius_cli(oracle, tmp_path, ds, flags, radius, loo, metric, weights):
    exe = os.path.join(PKG_DIR, "knn_cli")
    out = tmp_path / "pred.txt"
    r = subprocess.run([exe, f"{DATA}/{ds}-train.arff", f"{DATA}/{ds}-test.arff", "5", f"--radius={radius}",
                        "--outlier=-3", *flags], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, KNN_CLI_PRED_OUT=str(out)))
    assert r.returncode == 0, r.stderr
    pred, acc, count, nq, nt = _cli_reference(oracle, ds, loo, metric, weights, float(radius), -3)
    outliers = int((count == 0).sum())
    if ds == "medium":
        assert 0 < outliers < nq                                    # the radius makes both kinds of row
    else:
        assert 5 <= count.mean() <= 15
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 1, r.stdout
    assert lines[0].startswith(f"The radius-{float(radius):g} classifier for {nq} test instances on {nt} train "
                               "instances required "), lines[0]
    assert lines[0].endswith(f" ms CPU time. Accuracy was {acc:.4f}, {outliers} outliers"), lines[0]
    assert np.array_equal(np.array(out.read_text().split(), np.int32), pred)


def test_radius_cli_refusals():
    exe = os.path.join(PKG_DIR, "knn_cli")
    base = [exe, f"{DATA}/small-train.arff", f"{DATA}/small-test.arff", "5"]
    for flags in (["--radius=0.5", "--regress"], ["--radius=0.5", "--sweep"], ["--radius=abc"], ["--radius=-1"],
                  ["--radius=0.5x"], ["--radius="]):
        r = subprocess.run(base + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "radius" in r.stderr and r.stdout == "", (flags, r.returncode, r.stderr)
