"""The DBSCAN eps sweep on the GPU (knn_dbscan_sweep_device; knn_dbscan_sweep.hip).

Bar: row r of labels, count and summary equals, bit for bit, test_dbscan_sweep_cpu's restatement
(pinned to the single-radius restatement and through it to sklearn) AND what dbscan_device returns
at thr[r] on a direct context -- through the direct and the MFMA form, one and several train
segments.  The sets are those of the CPU file: they hold rows that are border rows at one level and
core rows at the next, clusters that merge between levels and border rows between two clusters, so
a wrong level chain, [lo, hi) range or min-root rule changes an output.
"""
import ctypes
import functools

import numpy as np
import pytest

from test_dbscan_cpu import EUCLIDEAN, METRICS, dbscan_set, distances
from test_dbscan_sweep_cpu import BRIDGE_THR, CASES, Q8, dbscan_sweep_reference, same_rows, sweep_case, thresholds_of
from test_gpu_dbscan import DEV, GUARD, _rows_dev
from test_metric_cpu import metric_distances

pytestmark = pytest.mark.gpu

STAGES = {"radius_sweep", "radius_sweep_finish", "dbscan_sweep_link", "dbscan_sweep_border", "dbscan_labels"}
CHAIN_THR = np.array([0.5, 1.0, 1.0, 2.0], np.float32)


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
    labels, count, summary = ctx.dbscan_sweep_device(xd, thresholds=thr, min_samples=m, count=True, **kw)
    return labels.cpu().numpy(), count.cpu().numpy(), summary.cpu().numpy()


def _singles(ctx, xd, thr, m):
    """R dbscan_device calls, stacked like the sweep's outputs."""
    rows = [ctx.dbscan_device(xd, threshold=float(t), min_samples=m, count=True) for t in thr]
    return tuple(np.stack([row[i].cpu().numpy() for row in rows]) for i in range(3))


def _check(ctx, direct, xd, thr, m, ref, what="", **kw):
    got = _run(ctx, xd, thr, m, **kw)
    same_rows(got, ref, what + " restatement")
    same_rows(got, _singles(direct, xd, thr, m), what + " single calls")
    return got


@functools.lru_cache(maxsize=None)
def chain_case(d):
    X, D = distances("chain", 4099, d, EUCLIDEAN)
    return X, CHAIN_THR, 3, dbscan_sweep_reference(D, CHAIN_THR, 3)


@functools.lru_cache(maxsize=None)
def wide_case(kind, n, d, spec, m):
    """A case outside the CPU file's table (the MFMA form's widths), Euclidean."""
    X, D = distances(kind, n, d, EUCLIDEAN)
    thr = thresholds_of(D, spec)
    return X, thr, m, dbscan_sweep_reference(D, thr, m)


# ---------------------------------------------------------------------------------
# the direct form, three metrics
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["set65x1", "set1000x3", "set1000x11", "bridge"])
def test_direct_form(ctxs, name):
    metric = CASES[name][3]
    X, _, thr, m, ref = sweep_case(name)
    ctx = ctxs[metric]
    _check(ctx, ctx, _rows_dev(X), thr, m, ref, name)
    ctx.dbscan_sweep_device(_rows_dev(X), thresholds=thr, min_samples=m)
    assert STAGES <= set(ctx.stage_times()), ctx.stage_times()
    st = ctx.stats()
    assert st["radius_form"] == "direct"
    assert st["dbscan_border_queries"] == ref[3]["candidates"]


@pytest.mark.parametrize("metric", sorted(METRICS))
def test_direct_form_wide_rows(ctxs, metric):
    """129 features: more than one chunk of a row, a ragged last group."""
    X, D = distances("dbscan", 1000, 129, metric)
    thr = thresholds_of(D, Q8)
    ref = dbscan_sweep_reference(D, thr, 5)
    _check(ctxs[metric], ctxs[metric], _rows_dev(X), thr, 5, ref, f"metric {metric}")
    assert ctxs[metric].stats()["radius_form"] == "direct"


@pytest.mark.parametrize("splits", [1, 3])
def test_chain_across_tiles(knn, ctxs, splits):
    """4,099 rows: 65 tiles and query blocks with a ragged tail in both; every union crosses tiles
    in scrambled order and every level's representative must be the chain's smallest row."""
    X, thr, m, ref = chain_case(1)
    n = len(X)
    assert (ref[0][0] == -1).all() and ref[2][0].tolist() == [0, 0, 0, n]
    for r in (1, 2, 3):
        assert (ref[0][r] == 0).all() and ref[2][r, 0] == 1
    c = knn.Context(0, algo="direct", train_splits=splits, profile=2)
    try:
        _check(c, ctxs[EUCLIDEAN], _rows_dev(X), thr, m, ref, f"splits {splits}")
        c.dbscan_sweep_device(_rows_dev(X), thresholds=thr, min_samples=m)
        st = c.stats()
        assert st["train_segments"] == splits
        assert st["dbscan_unions"] == ref[3]["unions"]
    finally:
        c.close()


# ---------------------------------------------------------------------------------
# the MFMA form
# ---------------------------------------------------------------------------------
def _mfma_cases():
    X, _, thr, m, ref = sweep_case("set4096x64")
    yield "set4096x64", X, thr, m, ref
    yield ("bridge64",) + wide_case("bridge", 0, 64, BRIDGE_THR, 4)
    yield ("chain64",) + chain_case(64)


@pytest.mark.parametrize("splits", [0, 3])
def test_mfma_form(knn, ctxs, splits):
    c = knn.Context(0, algo="gemm_bf16", train_splits=splits, profile=2)
    try:
        for name, X, thr, m, ref in _mfma_cases():
            xd = _rows_dev(X)
            _check(c, ctxs[EUCLIDEAN], xd, thr, m, ref, name)
            c.dbscan_sweep_device(xd, thresholds=thr, min_samples=m)
            st = c.stats()
            assert st["radius_form"] == "mfma", name
            assert STAGES <= set(c.stage_times())
            if splits:
                assert st["train_segments"] == splits
            if name != "chain64":  # (the chain's distances are integers far from every threshold's band)
                assert st["radius_exact_pairs"] > 0, name
    finally:
        c.close()


@pytest.mark.parametrize("d", [128, 256])
def test_mfma_form_wider_rows(mfma, ctxs, d):
    X, thr, m, ref = wide_case("dbscan", 4096, d, Q8, 5)
    _check(mfma, ctxs[EUCLIDEAN], _rows_dev(X), thr, m, ref, f"d={d}")
    mfma.dbscan_sweep_device(_rows_dev(X), thresholds=thr, min_samples=m)
    st = mfma.stats()
    assert st["radius_form"] == "mfma" and st["radius_exact_pairs"] > 0


def test_mfma_unsafe_norm(mfma, ctxs):
    """One huge-norm row: the certificate does not hold, the direct form runs behind the gate."""
    X = dbscan_set(4096, 64).copy()
    X[7, 0] = 1.0e19
    D = metric_distances(X, X, EUCLIDEAN)
    thr = thresholds_of(D, Q8)
    ref = dbscan_sweep_reference(D, thr, 5)
    assert (ref[0][:, 7] == -1).all() and (ref[1][:, 7] == 1).all()
    xd = _rows_dev(X)
    got = _run(mfma, xd, thr, 5)
    assert mfma.stats()["radius_form"] == "unsafe"
    same_rows(got, ref, "unsafe")
    same_rows(got, _singles(ctxs[EUCLIDEAN], xd, thr, 5), "unsafe single calls")


# ---------------------------------------------------------------------------------
# threshold lists
# ---------------------------------------------------------------------------------
def test_threshold_lists(ctxs):
    ctx = ctxs[EUCLIDEAN]
    X, D, thr8, m, _ = sweep_case("set1000x3")
    n = len(X)
    xd = _rows_dev(X)
    lists = {"R=1": thr8[3:4], "R=32 with duplicates": np.repeat(thr8, 4), "all equal": np.repeat(thr8[4:5], 5),
             "[0]": np.zeros(1, np.float32), "ending at 3e38": np.append(thr8[:3], np.float32(3e38))}
    for what, thr in lists.items():
        thr = np.asarray(thr, np.float32)
        got = _check(ctx, ctx, xd, thr, m, dbscan_sweep_reference(D, thr, m), what)
        for r in range(1, len(thr)):
            if thr[r] == thr[r - 1]:
                assert all(np.array_equal(g[r], g[r - 1]) for g in got), what
    got = _run(ctx, xd, lists["ending at 3e38"], m)
    assert got[2][-1].tolist() == [1, n, 0, 0]  # every row within 3e38 of every row: one cluster
    # min_samples = 1: every row is a core row at every level
    got = _check(ctx, ctx, xd, thr8, 1, dbscan_sweep_reference(D, thr8, 1), "min_samples=1")
    assert (got[2][:, 1] == n).all() and (got[0] >= 0).all()
    assert ctx.stats()["dbscan_border_queries"] == 0
    # min_samples = n + 1: all noise
    got = _run(ctx, xd, thr8, n + 1)
    assert (got[0] == -1).all() and (got[2] == np.array([0, 0, 0, n])).all()
    # radii= squares in binary32 under the Euclidean metric
    radii = np.sqrt(thr8.astype(np.float64)).astype(np.float32)
    labels, _, summary = ctx.dbscan_sweep_device(xd, radii=radii, min_samples=m)
    ref = dbscan_sweep_reference(D, radii * radii, m)
    assert np.array_equal(labels.cpu().numpy(), ref[0]) and np.array_equal(summary.cpu().numpy(), ref[2])


# ---------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_sets(ctxs, n):
    ctx = ctxs[EUCLIDEAN]
    X = dbscan_set(65, 3)[:n]
    D = metric_distances(X, X, EUCLIDEAN)
    thr = np.array([0.0, 1.0, 4.0, 64.0], np.float32) if n == 1 else thresholds_of(D, (0.01, 0.05, 0.2, 0.6))
    for m in (1, 3):
        _check(ctx, ctx, _rows_dev(X), thr, m, dbscan_sweep_reference(D, thr, m), f"n={n} m={m}")


def test_no_rows(ctxs):
    xd = _rows_dev(dbscan_set(65, 3))[:0]
    labels, count, summary = ctxs[EUCLIDEAN].dbscan_sweep_device(xd, thresholds=[1.0, 2.0], min_samples=3, count=True)
    assert labels.shape == (2, 0) and count.shape == (2, 0) and summary.cpu().tolist() == [[0, 0, 0, 0]] * 2


@pytest.mark.parametrize("name,algo", [("set1000x11", "direct"), ("set4096x64", "gemm_bf16")])
def test_bf16_rows(knn, ctxs, name, algo):
    import torch
    kind, n, d, _, _, m = CASES[name]
    X, D = distances(kind, n, d, EUCLIDEAN)  # (the case's rows under the Euclidean metric, 8 quantiles)
    thr = thresholds_of(D, Q8)
    xd = _rows_dev(X, bf16=True)
    assert xd.dtype == torch.bfloat16 and np.array_equal(xd.float().cpu().numpy(), X)  # the rows are bf16-exact
    c = knn.Context(0, algo=algo)
    try:
        _check(c, ctxs[EUCLIDEAN], xd, thr, m, dbscan_sweep_reference(D, thr, m), name)
        assert c.stats()["radius_form"] == ("mfma" if algo == "gemm_bf16" else "direct")
    finally:
        c.close()


@pytest.mark.parametrize("layout", ["pad", "offset", "half"])
def test_strided_rows_with_nan_pad_columns(ctxs, layout):
    from test_gpu_strided_rows import Strided, _layout
    X, D = distances("dbscan", 1000, 11, EUCLIDEAN)
    thr = thresholds_of(D, Q8)
    ref = dbscan_sweep_reference(D, thr, 5)
    (ld, c0), _ = _layout(layout, 12)
    s = Strided(np.pad(X, ((0, 0), (0, 1)), constant_values=np.nan), ld, c0, float("nan"))
    same_rows(_run(ctxs[EUCLIDEAN], s.view[:, :11], thr, 5), ref, layout)
    same_rows(_run(ctxs[EUCLIDEAN], s.view, thr, 5, d=11), ref, layout + " d=")
    assert s.intact()


def test_pitched_outputs_keep_their_guard_columns(knn, ctxs):
    import torch
    ctx = ctxs[EUCLIDEAN]
    X, _, thr, m, ref = sweep_case("set1000x3")
    n, R, ld = len(X), len(thr), len(X) + 24
    xd = _rows_dev(X)
    lab = torch.full((R, ld), GUARD, dtype=torch.int32, device=DEV)
    cnt = torch.full((R, ld), GUARD, dtype=torch.int32, device=DEV)
    summary = torch.zeros((R, 4), dtype=torch.int64, device=DEV)
    tr = knn._device_dataset(xd, None, None)
    st = ctx.lib.knn_dbscan_sweep_device(ctx.h, ctypes.byref(tr), thr.ctypes.data, R, m, ld, lab.data_ptr(), cnt.data_ptr(),
                                         summary.data_ptr(), None)
    assert st == knn.KNN_OK
    assert (lab[:, n:] == GUARD).all() and (cnt[:, n:] == GUARD).all()
    same_rows((lab[:, :n].cpu().numpy(), cnt[:, :n].cpu().numpy(), summary.cpu().numpy()), ref, "ld_out")
    # the Python method with the caller's pitched labels
    lab.fill_(GUARD)
    labels, count, _ = ctx.dbscan_sweep_device(xd, thresholds=thr, min_samples=m, labels=lab, count=True)
    assert (lab[:, n:] == GUARD).all()
    assert np.array_equal(lab[:, :n].cpu().numpy(), ref[0]) and np.array_equal(count.cpu().numpy(), ref[1])


def test_count_pass_in_query_blocks(knn, ctxs, monkeypatch):
    """A workspace budget that takes the histograms of fewer rows than the set has: the entry walks
    the rows in query blocks by itself, in both forms, and returns the same bits."""
    monkeypatch.setenv("KNN_WS_QUERIES", "1")  # read at knn_create: 24,640 bytes of budget
    for name, algo in (("set1000x3", "direct"), ("set4096x64", "gemm_bf16")):
        X, _, thr, m, ref = sweep_case(name)
        c = knn.Context(0, algo=algo, profile=1)
        try:
            fit = c.lib.knn_radius_sweep_max_queries(c.h, len(thr), 0)
            assert 1 <= fit < len(X)
            same_rows(_run(c, _rows_dev(X), thr, m), ref, name)
            names = (ctypes.c_char_p * 256)()
            ms = (ctypes.c_float * 256)()
            k = c.lib.knn_stage_times(c.h, names, ms, 256)
            assert [names[i] for i in range(k)].count(b"radius_sweep") == -(-len(X) // fit)  # one per query block
        finally:
            c.close()


# ---------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------
def test_errors_leave_the_outputs_alone(knn, ctxs):
    import torch
    ctx = ctxs[EUCLIDEAN]
    X, _, thr, m, ref = sweep_case("set1000x3")
    n, R = len(X), len(thr)
    xd = _rows_dev(X)
    lab = torch.full((32, n + 8), GUARD, dtype=torch.int32, device=DEV)
    cnt = torch.full((32, n + 8), GUARD, dtype=torch.int32, device=DEV)
    summary = torch.full((32, 4), GUARD, dtype=torch.int64, device=DEV)
    tr = knn._device_dataset(xd, None, None)
    big = np.float32(np.finfo(np.float32).max)

    def call(t, m_=m, ld=n + 8, labels=lab, R_=None):
        t = np.asarray(t, np.float32)
        return ctx.lib.knn_dbscan_sweep_device(ctx.h, ctypes.byref(tr), t.ctypes.data if t.size else None,
                                               len(t) if R_ is None else R_, m_, ld,
                                               None if labels is None else labels.data_ptr(), cnt.data_ptr(),
                                               summary.data_ptr(), None)

    bad = [call(thr, m_=0), call(thr, m_=-3), call([]), call(np.ones(33)), call(thr, R_=0), call([-1.0]), call([np.nan]),
           call([np.inf]), call([big]), call([2.0, 1.0]), call([1.0, np.nan, 2.0]), call(thr, ld=n - 1),
           call(thr, labels=None), call(thr, R_=33)]
    assert bad == [knn.KNN_EINVAL] * len(bad), bad
    assert (lab == GUARD).all() and (cnt == GUARD).all() and (summary == GUARD).all()
    # the Python method: one of radii= / thresholds=, whole min_samples, radii >= 0
    for kw in (dict(), dict(radii=[1.0], thresholds=[1.0]), dict(radii=[-1.0]), dict(thresholds=[1.0], min_samples=2.5)):
        with pytest.raises(knn.KnnError) as e:
            ctx.dbscan_sweep_device(xd, **kw)
        assert e.value.status == knn.KNN_EINVAL, kw
    # and a good call writes the outputs and nothing around them
    assert call(thr) == knn.KNN_OK
    assert (lab[R:] == GUARD).all() and (lab[:, n:] == GUARD).all() and (summary[R:] == GUARD).all()
    same_rows((lab[:R, :n].cpu().numpy(), cnt[:R, :n].cpu().numpy(), summary[:R].cpu().numpy()), ref, "after the errors")


# ---------------------------------------------------------------------------------
# repeats, neighbours on the same context
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["direct", "mfma"])
def test_repeated_calls_give_the_same_bits(ctxs, mfma, which):
    ctx = mfma if which == "mfma" else ctxs[EUCLIDEAN]
    X, _, thr, m, ref = sweep_case("set4096x64")
    xd = _rows_dev(X)
    for call in range(4):
        same_rows(_run(ctx, xd, thr, m), ref, f"call {call}")


@pytest.mark.parametrize("algo", ["direct", "gemm_bf16"])
def test_other_calls_in_between(knn, algo):
    """A radius sweep and a single-radius DBSCAN between two sweeps on a caching context."""
    X, D, thr, m, ref = sweep_case("set4096x64")
    xd = _rows_dev(X)
    c = knn.Context(0, algo=algo, cache_train=True)
    try:
        same_rows(_run(c, xd, thr, m), ref, "first")
        count = c.radius_sweep_device(xd, None, xd[:100], thresholds=thr[:8])[0].cpu().numpy()
        assert np.array_equal(count, ref[1][:8, :100])
        labels, _, summary = c.dbscan_device(xd, threshold=float(thr[9]), min_samples=m)
        assert np.array_equal(labels.cpu().numpy(), ref[0][9]) and np.array_equal(summary.cpu().numpy(), ref[2][9])
        same_rows(_run(c, xd, thr, m), ref, "second")
        same_rows(_run(c, xd, thr[::3], m), tuple(a[::3] for a in ref[:3]), "another list")
    finally:
        c.close()
