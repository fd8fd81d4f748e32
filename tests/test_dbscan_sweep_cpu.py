"""The DBSCAN eps sweep (include/knn_amd.h "DBSCAN sweep"): the yardstick of the GPU tests.

dbscan_sweep_reference restates the sweep THE WAY THE GPU WORKS -- the bucket matrix, the
histogram prefix, the levels, one union per pair into the forest of the pair's level, the level
chain, the min-root border offers over [lo, hi) -- and is pinned to R calls of
test_dbscan_cpu.dbscan_reference (itself pinned to sklearn there) on every set, and to the scalar
definition on tiny hand cases.  Every comparison is exact equality.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, REPO
from test_dbscan_cpu import (CHEBYSHEV, EUCLIDEAN, MANHATTAN, dbscan_definition, dbscan_reference, distances,
                             quantile_thr, two_cluster_borders)
from test_metric_cpu import metric_distances

Q8 = (0.001, 0.002, 0.004, 0.007, 0.01, 0.015, 0.02, 0.03)
Q4 = (0.002, 0.01, 0.03, 0.1)
Q32 = tuple(np.linspace(0.0005, 0.03, 32).tolist())
BRIDGE_THR = (0.25, 1.0, 1.0, 2.0, 4.0, 300.0)
# name -> (builder kind, n, d, metric, quantiles or thresholds, min_samples)
CASES = {
    "set1000x3": ("dbscan", 1000, 3, EUCLIDEAN, Q8, 5),
    "set1000x11": ("dbscan", 1000, 11, MANHATTAN, Q8, 5),
    "set65x1": ("dbscan", 65, 1, CHEBYSHEV, Q4, 3),
    "set4096x64": ("dbscan", 4096, 64, EUCLIDEAN, Q32, 5),
    "bridge": ("bridge", 0, 2, EUCLIDEAN, BRIDGE_THR, 4),
}


class _Forest:
    """A union-find whose larger root is hooked under the smaller: a root is its set's smallest row."""

    def __init__(self, n):
        self.p = list(range(n))

    def find(self, x):
        p = self.p
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.p[max(a, b)] = min(a, b)
        return a != b


def dbscan_sweep_reference(D, thr, m):
    """(labels int32 [R][n], count int32 [R][n], summary int64 [R][4], info) of the float32 matrix D
    at the non-decreasing thresholds thr.  info: level [n], candidates (the rows of the border pass),
    unions (the hooks of the link pass and the level chain)."""
    D = np.asarray(D, np.float32)
    thr = np.asarray(thr, np.float32)
    n, R = len(D), len(thr)
    # a pair's bucket: the smallest r with D <= thr[r], R when there is none (a NaN is in none)
    bucket = np.searchsorted(thr, D, side="left") if n else np.zeros((0, 0), np.int64)
    bucket[np.isnan(D)] = R
    hist = np.zeros((n, R + 1), np.int64)
    for r in range(R + 1):
        hist[:, r] = (bucket == r).sum(axis=1)
    count = np.cumsum(hist[:, :R], axis=1).T.astype(np.int32).reshape(R, n)
    level = (count < m).sum(axis=0).astype(np.int64)  # c(i); the counts are nested
    # link: one union per pair t < q, into the forest of the level the pair first acts at
    forests = [_Forest(n) for _ in range(R)]
    unions = 0
    low = np.tril(bucket < R, -1) & (level < R)[:, None] & (level < R)[None, :]
    qq, tt = np.nonzero(low)
    at = np.maximum(bucket[qq, tt], np.maximum(level[qq], level[tt]))
    for q, t, a in zip(qq.tolist(), tt.tolist(), at.tolist()):
        if a < R:
            unions += forests[a].union(q, t)
    # the level chain: level r's components go into forest r + 1
    root = np.full((n, R), -1, np.int64)
    for r in range(R):
        for i in np.flatnonzero(level <= r).tolist():
            rt = forests[r].find(i)
            root[i, r] = rt
            if r + 1 < R and rt != i:
                unions += forests[r + 1].union(i, rt)
    # border: candidate q takes, at every level below c(q), the smallest root among its core neighbours
    big = np.iinfo(np.int64).max
    best = np.full((R, n), big, np.int64)
    cand = np.flatnonzero((level >= 1) & (count[np.maximum(level, 1) - 1, np.arange(n)] >= 2)) if n else np.zeros(0, int)
    for q in cand.tolist():
        hi = int(level[q])
        for t in np.flatnonzero((bucket[q] < hi) & (level < hi)).tolist():
            for r in range(max(int(bucket[q, t]), int(level[t])), hi):
                best[r, q] = min(best[r, q], root[t, r])
    labels = np.full((R, n), -1, np.int32)
    summary = np.zeros((R, 4), np.int64)
    for r in range(R):
        core = level <= r
        isroot = np.zeros(n + 1, np.int64)
        isroot[:n] = root[:, r] == np.arange(n)
        number = np.cumsum(isroot) - isroot  # the exclusive scan: the roots below
        labels[r, core] = number[root[core, r]]
        border = ~core & (best[r] < big)
        labels[r, border] = number[best[r, border]]
        summary[r] = [isroot.sum(), core.sum(), border.sum(), n - core.sum() - border.sum()]
    return labels, count, summary, dict(level=level, candidates=len(cand), unions=unions)


def thresholds_of(D, spec):
    """quantile_thr of every quantile below 1, a threshold list as it is (the bridge set's)."""
    if max(spec) < 1.0:
        return np.array([quantile_thr(D, q) for q in spec], np.float32)
    return np.array(spec, np.float32)


@functools.lru_cache(maxsize=None)
def sweep_case(name):
    """(X, D, thr float32 [R], min_samples, the restatement's result) of a named case, shared and read-only."""
    kind, n, d, metric, spec, m = CASES[name]
    X, D = distances(kind, n, d, metric)
    thr = thresholds_of(D, spec)
    ref = dbscan_sweep_reference(D, thr, m)
    for a in ref[:3]:
        a.setflags(write=False)
    return X, D, thr, m, ref


@functools.lru_cache(maxsize=None)
def single_calls(name):
    """R calls of the single-radius restatement, stacked like the sweep's outputs."""
    _, D, thr, m, _ = sweep_case(name)
    rows = [dbscan_reference(D, t, m) for t in thr]
    return tuple(np.stack([row[i] for row in rows]) for i in range(3))


def same_rows(got, ref, what=""):
    for g, r, name in zip(got[:3], ref[:3], ("labels", "count", "summary")):
        assert g.dtype == r.dtype and g.shape == r.shape and np.array_equal(g, r), f"{what}: {name}"


def exercise(name):
    """How much of the sweep a case exercises: (rows that are border at r and core at r + 1, summed
    over r; cluster merges between consecutive levels; border rows between two clusters, summed)."""
    _, D, thr, m, (labels, count, summary, info) = sweep_case(name)
    R = len(thr)
    core = count >= m
    grown = merges = two = 0
    for r in range(R):
        two += len(two_cluster_borders(D, thr[r], labels[r], count[r], m))
        if r + 1 < R:
            grown += int((~core[r] & (labels[r] >= 0) & core[r + 1]).sum())
            merges += int(summary[r, 0]) - len(set(labels[r + 1][core[r]].tolist()))
    return grown, merges, two


# ---------------------------------------------------------------------------------
# the restatement against the single-radius restatement and the scalar definition
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_sweep_restatement_equals_single_calls(name):
    _, D, thr, m, ref = sweep_case(name)
    assert (np.diff(thr) >= 0).all()
    same_rows(ref, single_calls(name), name)
    assert (ref[2][:, 1:].sum(axis=1) == len(D)).all()


@pytest.mark.parametrize("metric", [EUCLIDEAN, MANHATTAN, CHEBYSHEV])
def test_hand_cases(metric):
    col = lambda *v: np.array(v, np.float32).reshape(-1, 1)
    cases = [(col(0, 1, 2, 10), [0.5, 1.0, 1.0, 8.0, 100.0], 3),
             (col(5, 3, 5, 3, 7, 5), [0.0, 0.0, 2.0, 4.0], 2),
             (col(0, 4, 1, 9), [1.0, 3.0, 5.0], 1),
             (col(0, 1, 2), [0.0, 5.0], 4),
             (col(0, np.nan, 1, 2), [0.0, 1.0, 2.0], 2),
             (col(3), [0.0, 1.0], 1),
             (col(0, 1, 2, 3, 4, 5, 6, 20, 21), [0.0, 1.0, 2.0, 16.0, 25.0, 400.0], 3)]
    from test_dbscan_cpu import bridge_set
    cases.append((bridge_set(G=2), list(BRIDGE_THR), 4))
    for X, thr, m in cases:
        D = metric_distances(X, X, metric)
        labels, count, summary, _ = dbscan_sweep_reference(D, thr, m)
        Dl = [[float(v) for v in row] for row in D]
        for r, t in enumerate(np.asarray(thr, np.float32)):
            dl, dc, dcore = dbscan_definition(Dl, float(t), m)
            assert labels[r].tolist() == dl and count[r].tolist() == dc, (thr, r)
            assert summary[r, 1] == sum(dcore) and summary[r, 0] == len(set(dl) - {-1})


def test_the_sets_exercise_the_sweep():
    """A wrong level chain, a wrong [lo, hi) range or a wrong min-root rule must change an output:
    rows that are border rows at r and core rows at r + 1, clusters that merge between levels and
    border rows between two clusters all occur, in the numbers the restatement gives."""
    assert exercise("set1000x3") == (400, 55, 44)
    assert exercise("set4096x64") == (1384, 231, 25)
    assert exercise("bridge") == (29, 57, 87)
    assert min(exercise("set1000x11")) >= 1
    assert exercise("set65x1")[1] >= 1  # (65 rows: clusters merge, no more is asked of it)
    level = sweep_case("set4096x64")[4][3]["level"]
    assert sorted(set(level.tolist())) == list(range(33))
    assert sweep_case("bridge")[4][2][:, 0].tolist() == [0, 58, 58, 58, 29, 1]


# ---------------------------------------------------------------------------------
# the surfaces that need no GPU
# ---------------------------------------------------------------------------------
def test_symbols_exported(knn):
    lib = knn.load_library()
    assert hasattr(lib, "knn_dbscan_sweep_device")
    assert callable(knn.Context.dbscan_sweep_device) and callable(knn.best_eps)
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(PKG_DIR, "libknn_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    assert "KNN_dbscan_sweep(ArffData*, float const*, int, int, long*)" in out


def test_best_eps(knn):
    """The most clusters first, then the fewest noise rows, then the smallest index."""
    s = np.array([[2, 9, 0, 5], [3, 9, 0, 7], [3, 9, 1, 4], [3, 9, 2, 4], [1, 9, 0, 0]], np.int64)
    assert knn.best_eps(s) == 2          # rows 1..3 have the most clusters; 2 and 3 tie on noise
    assert knn.best_eps(s[::-1]) == 1    # (the same rows reversed: 3, 2, 1 -> indices 1, 2, 3)
    assert knn.best_eps(s[:2]) == 1      # more clusters beat fewer noise rows
    assert knn.best_eps(np.zeros((4, 4), np.int64)) == 0
    assert knn.best_eps(s[4:]) == 0
    assert knn.best_eps(sweep_case("bridge")[4][2]) == 1
    with pytest.raises(knn.KnnError):
        knn.best_eps(np.zeros((0, 4), np.int64))


# the CLI refuses a bad --dbscan-radii before it creates a context: no GPU is needed
CLI = os.path.join(PKG_DIR, "knn_cli")
SMALL = [os.path.join(REPO, "tests", "data", f"small-{s}.arff") for s in ("train", "test")]


@pytest.mark.parametrize("extra", [
    ["--dbscan-radii=abc"], ["--dbscan-radii=-1"], ["--dbscan-radii=nan"], ["--dbscan-radii="], ["--dbscan-radii=2,1"],
    ["--dbscan-radii=1,,2"], ["--dbscan-radii=1,2,"], ["--dbscan-radii=" + ",".join(["1"] * 33)],
    ["--dbscan-radii=1,2", "--dbscan=1"], ["--dbscan-radii=1,2", "--min-samples=0"],
    ["--dbscan-radii=1,2", "--min-samples=x"], ["--dbscan-radii=1,2", "--lof"], ["--dbscan-radii=1,2", "--sweep"],
    ["--dbscan-radii=1,2", "--sweep=loo"], ["--dbscan-radii=1,2", "--regress"], ["--dbscan-radii=1,2", "--radius=2"],
    ["--dbscan-radii=1,2", "--radii=1,2"], ["--dbscan-radii=1,2", "--weights=distance"],
    ["--dbscan-radii=1,2", "--outlier=3"], ["--dbscan-radii=1,2", "--lof-threshold=2"]])
def test_cli_refuses(extra):
    r = subprocess.run([CLI, *SMALL, "5", *extra], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    # (--lof-threshold= without --lof is refused by the LOF switch's own check, which comes first)
    assert ("usage: --lof" if "--lof-threshold=2" in extra else "usage: --dbscan-radii=") in r.stderr and r.stdout == ""
