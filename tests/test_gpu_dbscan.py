"""DBSCAN on the GPU (knn_dbscan_device / knn_dbscan_lists_device; k_radius_tile's and
k_radius_gemm's RADIUS_LINK / RADIUS_BORDER modes, knn_dbscan.hip).

Bar: exact equality of labels, count and summary with test_dbscan_cpu's restatement (itself pinned
to sklearn), through the direct and the MFMA form, one and several train segments, and the
lists-held entry.  The shapes are the smallest at which a piece can go wrong: one block and many,
ragged tails in rows and queries, thresholds that are matrix entries, border rows between two
clusters, a chain whose unions cross every tile in scrambled order.
"""
import numpy as np
import pytest

from test_dbscan_cpu import (CHEBYSHEV, EUCLIDEAN, MANHATTAN, METRICS, PAIRS, SETS, bridge_set, chain_set, dbscan_case,
                             dbscan_reference, dbscan_set, distances)
from test_metric_cpu import metric_distances

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STAGES = {"radius_count", "dbscan_link", "dbscan_border", "dbscan_labels"}
GUARD = -777


def _rows_dev(x, bf16=False):
    """Device rows of the narrowest 16-byte-aligned pitch, as a column view of the true width."""
    import torch
    n, d = x.shape
    unit = 8 if bf16 else 4
    t = torch.zeros((max(n, 1), (d + unit - 1) // unit * unit), dtype=torch.float32)
    t[:n, :d] = torch.from_numpy(np.ascontiguousarray(x))
    if bf16:
        t = t.to(torch.bfloat16)
    return t.to(DEV)[:n, :d]


@pytest.fixture(scope="module")
def ctxs(knn):
    """One direct context per metric (profile = 1: the stages are read)."""
    cs = {m: knn.Context(0, algo="direct", profile=1, metric=name) for m, name in METRICS.items()}
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def mfma(knn):
    c = knn.Context(0, algo="gemm_bf16", profile=2)
    yield c
    c.close()


def _run(ctx, xd, thr, m, **kw):
    labels, count, summary = ctx.dbscan_device(xd, threshold=float(thr), min_samples=m, count=True, **kw)
    return labels.cpu().numpy(), count.cpu().numpy(), summary.cpu().numpy()


def _same(got, ref, what=""):
    for g, r, name in zip(got, ref, ("labels", "count", "summary")):
        assert g.dtype == r.dtype and np.array_equal(g, r), f"{what}: {name}"


@pytest.mark.parametrize("metric", sorted(METRICS))
@pytest.mark.parametrize("n,d", SETS)
def test_dbscan_set(ctxs, n, d, metric):
    ctx = ctxs[metric]
    X = dbscan_set(n, d)
    xd = _rows_dev(X)
    for pair in range(len(PAIRS)):
        _, thr, m, ref = dbscan_case(n, d, metric, pair)
        got = _run(ctx, xd, thr, m)
        _same(got, ref, f"pair {pair}")
        assert STAGES <= set(ctx.stage_times()), ctx.stage_times()
        st = ctx.stats()
        assert st["radius_form"] == "direct"
        assert st["dbscan_border_queries"] == int(((ref[1] < m) & (ref[1] >= 2)).sum())
        count = ctx.radius_count_device(xd, None, xd, threshold=float(thr))[0].cpu().numpy()
        assert np.array_equal(count, got[1])


@pytest.mark.parametrize("metric", sorted(METRICS))
def test_bridge_set(ctxs, metric):
    X, D = distances("bridge", 0, 2, metric)
    ref = dbscan_reference(D, 1.0, 4)
    assert ref[2].tolist() == [58, 232, 29, 0]
    _same(_run(ctxs[metric], _rows_dev(X), 1.0, 4), ref)


@pytest.mark.parametrize("splits", [1, 3])
def test_chain_across_tiles(knn, splits):
    """4,099 rows: 65 tiles and 65 query blocks with a ragged tail in both; every union crosses
    tiles in scrambled order, and cluster 0's representative must be the chain's smallest row."""
    n = 4099
    X, D = distances("chain", n, 1, EUCLIDEAN)
    ref = dbscan_reference(D, 1.0, 3)
    assert ref[2].tolist() == [1, n - 2, 2, 0] and (ref[0] == 0).all()
    c = knn.Context(0, algo="direct", train_splits=splits, profile=2)
    try:
        _same(_run(c, _rows_dev(X), 1.0, 3), ref)
        st = c.stats()
        assert st["train_segments"] == splits
        assert st["dbscan_unions"] == n - 3  # one component of n - 2 core rows: that many hooks less one
    finally:
        c.close()


# ---------------------------------------------------------------------------------
# the MFMA form
# ---------------------------------------------------------------------------------
def _mfma_sets():
    yield "dbscan64", dbscan_set(4096, 64), [dbscan_case(4096, 64, EUCLIDEAN, p)[1:] for p in range(len(PAIRS))]
    X, D = distances("bridge", 0, 64, EUCLIDEAN)
    yield "bridge64", X, [(np.float32(1.0), 4, dbscan_reference(D, 1.0, 4))]
    X, D = distances("chain", 4099, 64, EUCLIDEAN)
    yield "chain64", X, [(np.float32(1.0), 3, dbscan_reference(D, 1.0, 3))]


@pytest.mark.parametrize("splits", [0, 3])
def test_mfma_form(knn, ctxs, splits):
    c = knn.Context(0, algo="gemm_bf16", train_splits=splits, profile=1)
    try:
        for name, X, cases in _mfma_sets():
            xd = _rows_dev(X)
            for thr, m, ref in cases:
                got = _run(c, xd, thr, m)
                assert c.stats()["radius_form"] == "mfma", name
                assert STAGES <= set(c.stage_times())
                if splits:
                    assert c.stats()["train_segments"] == splits
                _same(got, ref, f"{name} thr={thr!r}")
                _same(got, _run(ctxs[EUCLIDEAN], xd, thr, m), f"{name} direct")
    finally:
        c.close()


@pytest.mark.parametrize("d", [128, 256])
def test_mfma_form_wider_rows(mfma, ctxs, d):
    xd = _rows_dev(dbscan_set(4096, d))
    for pair in range(len(PAIRS)):
        _, thr, m, ref = dbscan_case(4096, d, EUCLIDEAN, pair)
        got = _run(mfma, xd, thr, m)
        assert mfma.stats()["radius_form"] == "mfma"
        _same(got, ref, f"pair {pair}")
        _same(got, _run(ctxs[EUCLIDEAN], xd, thr, m), "direct")


def test_mfma_unsafe_norm(mfma, ctxs):
    """One huge-norm row: the certificate does not hold, the direct form runs behind the gate."""
    X = dbscan_set(4096, 64).copy()
    X[7, 0] = 1.0e19
    _, thr, m, _ = dbscan_case(4096, 64, EUCLIDEAN, 1)
    ref = dbscan_reference(metric_distances(X, X, EUCLIDEAN), thr, m)
    assert ref[0][7] == -1 and ref[1][7] == 1
    xd = _rows_dev(X)
    got = _run(mfma, xd, thr, m)
    assert mfma.stats()["radius_form"] == "unsafe"
    _same(got, ref)
    _same(got, _run(ctxs[EUCLIDEAN], xd, thr, m), "direct")


# ---------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------
def test_edges(ctxs):
    ctx = ctxs[EUCLIDEAN]
    n, d = 1000, 3
    X, thr, _, _ = dbscan_case(n, d, EUCLIDEAN, 1)
    X = X.copy()
    X[300, 1] = np.nan
    D = metric_distances(X, X, EUCLIDEAN)
    xd = _rows_dev(X)
    # min_samples = 1: nothing but the NaN row is noise, and every duplicate group is one cluster
    ref = dbscan_reference(D, thr, 1)
    got = _run(ctx, xd, thr, 1)
    _same(got, ref, "min_samples=1")
    assert np.flatnonzero(got[0] == -1).tolist() == [300] and got[1][300] == 0
    assert np.array_equal(got[0][n // 2: n // 2 + n // 8], got[0][: n // 8])
    # min_samples = n + 1: all noise
    got = _run(ctx, xd, thr, n + 1)
    assert (got[0] == -1).all() and got[2].tolist() == [0, 0, 0, n]
    # thr = 0: the duplicate groups alone
    for m in (2, 3):
        ref = dbscan_reference(D, 0.0, m)
        assert m > 2 or ref[2][0] >= 50
        _same(_run(ctx, xd, 0.0, m), ref, f"thr=0 m={m}")
    # the NaN row at the usual pair
    _same(_run(ctx, xd, thr, 5), dbscan_reference(D, thr, 5), "NaN row")
    # n = 1 and n = 0
    got = _run(ctx, xd[:1], thr, 1)
    assert got[0].tolist() == [0] and got[1].tolist() == [1] and got[2].tolist() == [1, 1, 0, 0]
    got = _run(ctx, xd[:1], thr, 2)
    assert got[0].tolist() == [-1] and got[2].tolist() == [0, 0, 0, 1]
    got = _run(ctx, xd[:0], thr, 5)
    assert got[0].shape == (0,) and got[1].shape == (0,) and got[2].tolist() == [0, 0, 0, 0]


def _guarded(n):
    """An int32 output of n elements inside guard words: (whole tensor, the output's view)."""
    import torch
    whole = torch.full((n + 16,), GUARD, dtype=torch.int32, device=DEV)
    return whole, whole[8:8 + n]


def test_errors_leave_the_outputs_alone(knn, ctxs):
    ctx = ctxs[EUCLIDEAN]
    X, thr, m, _ = dbscan_case(1000, 3, EUCLIDEAN, 1)
    xd = _rows_dev(X)
    lw, lab = _guarded(len(X))
    cw, cnt = _guarded(len(X))
    for kw in (dict(threshold=float(thr), min_samples=0), dict(threshold=-1.0, min_samples=m),
               dict(threshold=float("nan"), min_samples=m), dict(threshold=float("inf"), min_samples=m),
               dict(threshold=float(np.finfo(np.float32).max), min_samples=m)):
        with pytest.raises(knn.KnnError) as e:
            ctx.dbscan_device(xd, labels=lab, count=cnt, **kw)
        assert e.value.status == knn.KNN_EINVAL, kw
        assert (lw == GUARD).all() and (cw == GUARD).all(), kw
    # and a good call writes the outputs and nothing around them
    ctx.dbscan_device(xd, threshold=float(thr), min_samples=m, labels=lab, count=cnt)
    ref = dbscan_case(1000, 3, EUCLIDEAN, 1)[3]
    assert np.array_equal(lab.cpu().numpy(), ref[0]) and np.array_equal(cnt.cpu().numpy(), ref[1])
    for w in (lw, cw):
        assert (w[:8] == GUARD).all() and (w[-8:] == GUARD).all()


# ---------------------------------------------------------------------------------
# the lists-held entry: a second, independent path on the GPU
# ---------------------------------------------------------------------------------
def _list_cases():
    X, D = distances("bridge", 0, 2, EUCLIDEAN)
    yield X, np.float32(1.0), 4, dbscan_reference(D, 1.0, 4)
    yield dbscan_case(1000, 11, EUCLIDEAN, 1)


def test_lists_entry(knn, ctxs):
    import torch
    ctx = ctxs[EUCLIDEAN]
    for X, thr, m, ref in _list_cases():
        n = len(X)
        xd = _rows_dev(X)
        off, idx, _ = ctx.radius_neighbors_device(xd, xd, threshold=float(thr), return_distance=False)
        lw, lab = _guarded(n)
        cw, cnt = _guarded(n)
        labels, count, summary = ctx.dbscan_lists_device(off, idx, min_samples=m, labels=lab, count=cnt)
        got = (labels.cpu().numpy(), count.cpu().numpy(), summary.cpu().numpy())
        _same(got, ref, "lists")
        _same(got, _run(ctx, xd, thr, m), "fused passes")
        assert STAGES - {"radius_count"} <= set(ctx.stage_times())
        for w in (lw, cw):
            assert (w[:8] == GUARD).all() and (w[-8:] == GUARD).all()
        # an index outside [0, n), in a core row's list and in a noise row's
        for row in (int(np.flatnonzero(ref[1] >= m)[0]), int(np.argmin(ref[1]))):
            for bad_value in (n, -1):
                bad = idx.clone()
                bad[int(off[row].item())] = bad_value
                with pytest.raises(knn.KnnError) as e:
                    ctx.dbscan_lists_device(off, bad, min_samples=m, labels=lab, count=cnt)
                assert e.value.status == knn.KNN_EINVAL
                for w in (lw, cw):
                    assert (w[:8] == GUARD).all() and (w[-8:] == GUARD).all()
        # offsets that decrease
        bad_off = off.clone()
        bad_off[3] = bad_off[4] + 1
        with pytest.raises(knn.KnnError) as e:
            ctx.dbscan_lists_device(bad_off, idx, min_samples=m)
        assert e.value.status == knn.KNN_EINVAL
        with pytest.raises(knn.KnnError) as e:
            ctx.dbscan_lists_device(off, idx, min_samples=0)
        assert e.value.status == knn.KNN_EINVAL
    # no rows
    labels, count, summary = ctx.dbscan_lists_device(torch.zeros(1, dtype=torch.int64, device=DEV),
                                                     torch.zeros(0, dtype=torch.int32, device=DEV), count=True)
    assert labels.numel() == 0 and summary.cpu().tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------
# layouts, element types, repeats, neighbours on the same context
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["pad", "offset", "half"])
def test_strided_rows_with_nan_pad_columns(ctxs, layout):
    from test_gpu_strided_rows import Strided, _layout
    X, thr, m, ref = dbscan_case(1000, 11, EUCLIDEAN, 1)
    (ld, c0), _ = _layout(layout, 12)
    s = Strided(np.pad(X, ((0, 0), (0, 1)), constant_values=np.nan), ld, c0, float("nan"))
    got = _run(ctxs[EUCLIDEAN], s.view[:, :11], thr, m)
    _same(got, ref, layout)
    # (d= on the wider view: the same rows)
    _same(_run(ctxs[EUCLIDEAN], s.view, thr, m, d=11), ref, layout + " d=")
    assert s.intact()


@pytest.mark.parametrize("algo,n,d", [("direct", 1000, 11), ("gemm_bf16", 4096, 64)])
def test_bf16_rows(knn, algo, n, d):
    import torch
    X, thr, m, ref = dbscan_case(n, d, EUCLIDEAN, 1)
    xd = _rows_dev(X, bf16=True)
    assert xd.dtype == torch.bfloat16 and np.array_equal(xd.float().cpu().numpy(), X)  # the rows are bf16-exact
    c = knn.Context(0, algo=algo)
    try:
        _same(_run(c, xd, thr, m), ref)
        assert c.stats()["radius_form"] == ("mfma" if algo == "gemm_bf16" else "direct")
    finally:
        c.close()


@pytest.mark.parametrize("which", ["direct", "mfma"])
def test_repeated_calls_give_the_same_bits(ctxs, mfma, which):
    ctx = mfma if which == "mfma" else ctxs[EUCLIDEAN]
    X, thr, m, ref = dbscan_case(4096, 64, EUCLIDEAN, 2)
    xd = _rows_dev(X)
    for call in range(5):
        _same(_run(ctx, xd, thr, m), ref, f"call {call}")


@pytest.mark.parametrize("algo", ["direct", "gemm_bf16"])
def test_other_calls_in_between(knn, algo):
    """A top-k call and a radius count call between two DBSCAN calls on a caching context."""
    import torch
    X, thr, m, ref = dbscan_case(4096, 64, EUCLIDEAN, 1)
    xd = _rows_dev(X)
    lab = torch.zeros(len(X), dtype=torch.int32, device=DEV)
    c = knn.Context(0, algo=algo, cache_train=True)
    try:
        _same(_run(c, xd, thr, m), ref, "first")
        pred = torch.empty(64, dtype=torch.int32, device=DEV)
        c.predict_device(xd, lab, xd[:64], 5, 1, pred)
        want = c.radius_count_device(xd, None, xd[:100], threshold=float(thr))[0].cpu().numpy()
        assert np.array_equal(want, ref[1][:100])
        _same(_run(c, xd, thr, m), ref, "second")
        other = dbscan_case(4096, 64, EUCLIDEAN, 0)
        _same(_run(c, xd, other[1], other[2]), other[3], "another threshold")
    finally:
        c.close()
