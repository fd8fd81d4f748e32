"""The mutual-reachability spanning tree on the GPU (knn_mst_device, knn_mst_cut_device; knn_mst.hip).

Bar: (w, a, b, core, summary[:2]) equal test_mst_cpu's restatement exactly, dtype included -- the
restatement is pinned to Kruskal, scipy and sklearn there.  The forest under the strict order is
unique, so the list shortcut, the train segments and the form of the list pass may change the rounds
and the rows sent through passes, never an output bit.
"""
import numpy as np
import pytest

from test_dbscan_cpu import CHEBYSHEV, EUCLIDEAN, MANHATTAN, METRICS, SETS, dbscan_set, distances
from test_dbscan_sweep_cpu import Q8, thresholds_of
from test_gpu_dbscan import DEV, GUARD, _rows_dev
from test_metric_cpu import bits, metric_distances
from test_mst_cpu import LIST_L, copies_set, gaussian_set, mst_case, mst_cut, mst_reference

pytestmark = pytest.mark.gpu

STAGES = {"mst_lists", "mst_resolve", "mst_pass", "mst_pick", "mst_sort"}


@pytest.fixture(scope="module")
def ctxs(knn):
    """One direct context per metric (profile = 1: the stages are read)."""
    cs = {m: knn.Context(0, algo="direct", profile=1, metric=name) for m, name in METRICS.items()}
    yield cs
    for c in cs.values():
        c.close()


def _run(ctx, xd, m, **kw):
    w, a, b, core, summary = ctx.mst_device(xd, min_samples=m, core=True, **kw)
    return w.cpu().numpy(), a.cpu().numpy(), b.cpu().numpy(), core.cpu().numpy(), summary.cpu().numpy()


def _same(got, ref, what=""):
    for g, r, name in zip(got[:4], ref[:4], ("w", "a", "b", "core")):
        assert g.dtype == r.dtype and g.shape == r.shape, f"{what}: {name} {g.dtype} {g.shape}"
        same = np.array_equal(bits(g), bits(r)) if g.dtype == np.float32 else np.array_equal(g, r)
        assert same, f"{what}: {name}"
    assert got[4].dtype == np.int64 and got[4][:2].tolist() == ref[4].tolist(), f"{what}: summary {got[4]}"


def _bound(n):
    return int(np.ceil(np.log2(max(n, 2)))) + 1


@pytest.mark.parametrize("metric", sorted(METRICS))
@pytest.mark.parametrize("n,d", SETS)
def test_dbscan_sets(ctxs, n, d, metric):
    ctx = ctxs[metric]
    xd = _rows_dev(dbscan_set(n, d))
    for m in (1, 4, 17, LIST_L + 1):  # (above the library's list length: the list is as long as min_samples)
        _, _, ref = mst_case("dbscan", n, d, metric, m)
        got = _run(ctx, xd, m)
        _same(got, ref, f"min_samples {m}")
        st = ctx.stats()
        assert 1 <= st["mst_rounds"] <= _bound(n) and st["mst_rounds"] == got[4][2]
        assert st["mst_pass_rows"] == got[4][3] <= n * st["mst_rounds"]
        assert STAGES <= set(ctx.stage_times()), ctx.stage_times()
        if m > LIST_L:
            # w >= c(q) = dlast: the list alone never decides a row
            assert st["mst_pass_rows"] == n * st["mst_rounds"]
        elif n >= 1000 and m <= 4:
            assert st["mst_pass_rows"] < n * st["mst_rounds"]


def test_gemm_list_pass(knn):
    """The lists through the MFMA-filtered top-k pass: the same distances, so the same tree."""
    _, _, ref = mst_case("dbscan", 4096, 64, EUCLIDEAN, 4)
    c = knn.Context(0, algo="gemm_bf16")
    try:
        _same(_run(c, _rows_dev(dbscan_set(4096, 64)), 4), ref)
        assert c.stats()["filter_operands"] is not None
    finally:
        c.close()


def test_chain_across_tiles(knn, monkeypatch):
    """4,099 rows, every weight equal: 65 tiles and query blocks with ragged tails.  One and three
    train segments, the list shortcut on and off, fresh contexts: four identical results."""
    n = 4099
    _, _, ref = mst_case("chain", n, 1, EUCLIDEAN, 1)
    assert ref[4].tolist() == [n - 1, 1] and (ref[0] == 1.0).all()
    xd = _rows_dev(distances("chain", n, 1, EUCLIDEAN)[0])
    for lists in ("1", "0"):
        monkeypatch.setenv("KNN_MST_LISTS", lists)
        for splits in (1, 3):
            c = knn.Context(0, algo="direct", train_splits=splits)
            try:
                got = _run(c, xd, 1)
                _same(got, ref, f"lists {lists} splits {splits}")
                st = c.stats()
                assert st["train_segments"] == splits
                assert 1 <= st["mst_rounds"] <= 13
                if lists == "0":
                    assert st["mst_pass_rows"] == n * st["mst_rounds"]
                else:
                    assert st["mst_pass_rows"] < n * st["mst_rounds"]
            finally:
                c.close()


@pytest.mark.parametrize("L", ["0", "16"])
def test_list_length_hook(knn, monkeypatch, L):
    """KNN_MST_LIST_L: lists of max(min_samples, L) entries change the rows sent through passes, no bit."""
    _, _, ref = mst_case("dbscan", 1000, 3, EUCLIDEAN, 4)
    monkeypatch.setenv("KNN_MST_LIST_L", L)
    c = knn.Context(0, algo="direct")
    try:
        _same(_run(c, _rows_dev(dbscan_set(1000, 3)), 4), ref, f"L {L}")
        st = c.stats()
        if L == "0":
            assert st["mst_pass_rows"] == 1000 * st["mst_rounds"]
        else:
            assert st["mst_pass_rows"] < 1000 * st["mst_rounds"]
    finally:
        c.close()


@pytest.mark.parametrize("metric", sorted(METRICS))
def test_copies(ctxs, metric):
    """70 exact copies of one row: c = 0 ties, more copies than a list holds."""
    X = copies_set(200, 70)
    assert (X == X[3]).all(axis=1).sum() >= 70
    for m in (1, 4):
        _, _, ref = mst_case("copies", 200, 3, metric, m)
        _same(_run(ctxs[metric], _rows_dev(X), m), ref, f"min_samples {m}")
        assert (ref[0] == 0).sum() >= 69


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_small_sets(ctxs, n):
    X = gaussian_set(n, 3)
    for m in (1, min(n, 3)):
        ref = mst_reference(metric_distances(X, X, EUCLIDEAN), m)
        got = _run(ctxs[EUCLIDEAN], _rows_dev(X), m)
        _same(got, ref, f"n {n} min_samples {m}")
        assert got[4][0] == n - 1


def test_no_rows(ctxs):
    import torch
    w, a, b, core, summary = ctxs[EUCLIDEAN].mst_device(torch.zeros((0, 4), device=DEV), min_samples=1, core=True)
    assert w.numel() == a.numel() == b.numel() == core.numel() == 0 and summary.tolist() == [0, 0, 0, 0]
    labels, cs = ctxs[EUCLIDEAN].mst_cut_device(w, a, b, core, thresholds=[1.0, 2.0])
    assert tuple(labels.shape) == (2, 0) and cs.tolist() == [[0, 0, 0], [0, 0, 0]]


def test_bf16_rows(ctxs):
    X = dbscan_set(1000, 3)
    xd = _rows_dev(X, bf16=True)
    assert np.array_equal(xd.float().cpu().numpy(), X)  # the rows are bf16-exact: the same numbers
    for metric in (EUCLIDEAN, MANHATTAN):
        _, _, ref = mst_case("dbscan", 1000, 3, metric, 4)
        _same(_run(ctxs[metric], xd, 4), ref, f"metric {metric}")


@pytest.mark.parametrize("poison", [float("nan"), 1.0e3])
def test_strided_rows(ctxs, poison):
    """Rows as column views of a wider tensor whose other columns are poisoned."""
    import torch
    X = dbscan_set(1000, 11)
    n, d = X.shape
    ld, c0 = d + 9, 4
    parent = torch.full((n + 1, ld), poison, dtype=torch.float32)
    parent[:n, c0:c0 + d] = torch.from_numpy(X)
    dev = parent.to(DEV)
    view = dev[:n, c0:c0 + d]
    assert view.data_ptr() % 16 == 0 and (ld * 4) % 16 == 0
    for metric in sorted(METRICS):
        _, _, ref = mst_case("dbscan", n, d, metric, 4)
        _same(_run(ctxs[metric], view, 4), ref, f"metric {metric}")
    assert torch.equal(dev.cpu().view(torch.int32), parent.view(torch.int32))


def test_nan_row(ctxs):
    """A NaN feature under the Euclidean metric: the row has no edge and c = +inf."""
    X = gaussian_set(300, 5).copy()
    X[7, 1] = np.nan
    n = len(X)
    ref = mst_reference(metric_distances(X, X, EUCLIDEAN), 4)
    assert ref[4].tolist() == [n - 2, 2] and ref[3][7] == np.inf
    import torch
    w = torch.full((n + 7,), float(GUARD), dtype=torch.float32, device=DEV)
    a = torch.full((n + 7,), GUARD, dtype=torch.int32, device=DEV)
    b = torch.full((n + 7,), GUARD, dtype=torch.int32, device=DEV)
    got = ctxs[EUCLIDEAN].mst_device(_rows_dev(X), min_samples=4, core=True, w=w, a=a, b=b)
    _same(tuple(t.cpu().numpy() for t in got), ref)
    # the entries past E are the caller's
    assert (w[n - 2:] == GUARD).all() and (a[n - 2:] == GUARD).all() and (b[n - 2:] == GUARD).all()
    # the Chebyshev maximum skips the NaN difference: one tree
    ref = mst_reference(metric_distances(X, X, CHEBYSHEV), 4)
    assert ref[4].tolist() == [n - 1, 1]
    _same(_run(ctxs[CHEBYSHEV], _rows_dev(X), 4), ref)


def test_refusals(knn, ctxs):
    import torch
    ctx = ctxs[EUCLIDEAN]
    xd = _rows_dev(gaussian_set(40, 3))
    w = torch.full((48,), float(GUARD), dtype=torch.float32, device=DEV)
    a = torch.full((48,), GUARD, dtype=torch.int32, device=DEV)
    b = torch.full((48,), GUARD, dtype=torch.int32, device=DEV)
    for m in (41, 0, 257, -1):
        with pytest.raises(knn.KnnError) as e:
            ctx.mst_device(xd, min_samples=m, w=w, a=a, b=b)
        assert e.value.status == knn.KNN_EINVAL, m
        assert (w == GUARD).all() and (a == GUARD).all() and (b == GUARD).all(), m
    got = ctx.mst_device(xd, min_samples=40, core=True, w=w, a=a, b=b)
    _same(tuple(t.cpu().numpy() for t in got), mst_reference(metric_distances(*[gaussian_set(40, 3)] * 2, EUCLIDEAN), 40))
    assert (w[39:] == GUARD).all() and (a[39:] == GUARD).all() and (b[39:] == GUARD).all()


# ---------------------------------------------------------------------------------
# the cut
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,d,metric,m", [("set1000x3", 1000, 3, EUCLIDEAN, 5), ("set1000x11", 1000, 11, MANHATTAN, 5),
                                               ("set1000x3c", 1000, 3, CHEBYSHEV, 3)])
def test_cut_is_the_sweep_on_core_rows(ctxs, name, n, d, metric, m):
    """mst_cut_device at the 8 radii of a dbscan_sweep_device call on the same tensor: equal labels
    where the sweep's count >= min_samples, -1 elsewhere; equal clusters and core rows."""
    ctx = ctxs[metric]
    X, D = distances("dbscan", n, d, metric)
    thr = thresholds_of(D, Q8)
    xd = _rows_dev(X)
    sl, sc, ss = (t.cpu().numpy() for t in ctx.dbscan_sweep_device(xd, thresholds=thr, min_samples=m, count=True))
    w, a, b, core, summary = ctx.mst_device(xd, min_samples=m, core=True)
    labels, cs = ctx.mst_cut_device(w, a, b, core, thresholds=thr)
    assert "mst_cut" in ctx.stage_times()
    labels, cs = labels.cpu().numpy(), cs.cpu().numpy()
    assert labels.dtype == np.int32 and cs.dtype == np.int64 and labels.shape == (8, n) and cs.shape == (8, 3)
    assert np.array_equal(labels, np.where(sc >= m, sl, -1))
    assert np.array_equal(cs[:, :2], ss[:, :2]) and (cs[:, 1] + cs[:, 2] == n).all()
    if metric != CHEBYSHEV:
        assert cs[:, 0].max() >= 3 and (sl != labels).any()  # (the sweep assigned border rows; the cut does not)
    # and the restatement's cut of the restatement's tree
    _, _, ref = mst_case("dbscan", n, d, metric, m)
    rl, rs = mst_cut(ref[0], ref[1], ref[2], ref[3], thr, n)
    assert np.array_equal(labels, rl) and np.array_equal(cs, rs)
    # the edges need not be sorted, and a pitch wider than n leaves the columns past n alone
    import torch
    perm = torch.randperm(w.numel(), generator=torch.Generator().manual_seed(1)).to(DEV)
    out = torch.full((8, n + 5), GUARD, dtype=torch.int32, device=DEV)
    ctx.mst_cut_device(w[perm].contiguous(), a[perm].contiguous(), b[perm].contiguous(), core, thresholds=thr, labels=out)
    out = out.cpu().numpy()
    assert np.array_equal(out[:, :n], rl) and (out[:, n:] == GUARD).all()


def test_cut_refusals(knn, ctxs):
    import torch
    ctx = ctxs[EUCLIDEAN]
    X = gaussian_set(64, 3)
    w, a, b, core, _ = ctx.mst_device(_rows_dev(X), min_samples=1, core=True)
    for bad in (64, -1, 1 << 30):
        for which in (0, 1):
            ab = [a.clone(), b.clone()]
            ab[which][17] = bad
            with pytest.raises(knn.KnnError) as e:
                ctx.mst_cut_device(w, ab[0], ab[1], core, thresholds=[0.5, 1.0])
            assert e.value.status == knn.KNN_EINVAL, (bad, which)
    out = torch.full((2, 64), GUARD, dtype=torch.int32, device=DEV)
    for thr in ([1.0, 0.5], [-1.0], [float("nan")], [float("inf")], list(range(33)), []):
        with pytest.raises(knn.KnnError) as e:
            ctx.mst_cut_device(w, a, b, core, thresholds=thr, labels=out)
        assert e.value.status == knn.KNN_EINVAL, thr
        assert (out == GUARD).all(), thr
    # and a good call after the refused ones
    labels, cs = ctx.mst_cut_device(w, a, b, core, radii=[0.0, 10.0])
    assert cs.cpu().tolist() == [[64, 64, 0], [1, 64, 0]]
    assert labels[0].cpu().tolist() == list(range(64))
