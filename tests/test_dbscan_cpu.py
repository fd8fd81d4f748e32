"""DBSCAN (include/knn_amd.h "DBSCAN"): the yardstick and the builders of the GPU tests.

dbscan_reference restates the header's rules in numpy on a float32 distance matrix.  It is pinned
two ways: to a scalar, plain-Python definition (sklearn's own expansion order: cluster c is grown
completely before cluster c + 1 starts) on tiny hand cases, and to sklearn.cluster.DBSCAN with
metric="precomputed" on every builder set.  Every comparison is exact equality.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, REPO
from test_metric_cpu import CHEBYSHEV, EUCLIDEAN, MANHATTAN, metric_distances

METRICS = {EUCLIDEAN: "euclidean", MANHATTAN: "manhattan", CHEBYSHEV: "chebyshev"}
# (quantile of the positive distances, min_samples)
PAIRS = ((0.002, 3), (0.01, 5), (0.03, 8))
SETS = ((65, 1), (1000, 3), (1000, 11), (4096, 64), (1000, 129))


def dbscan_reference(D, thr, min_samples):
    """(labels int32 [n], count int32 [n], summary int64 [4]) of the rules in knn_amd.h from the
    float32 matrix D [n][n] (test_metric_cpu.metric_distances(tr, tr, metric))."""
    D = np.asarray(D, np.float32)
    n = len(D)
    with np.errstate(invalid="ignore"):
        M = D <= np.float32(thr)  # (a NaN distance is never a member)
    count = M.sum(axis=1).astype(np.int32)
    core = count >= min_samples
    # components of the core rows: union-find over the edges i > j, the smaller root wins
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    ii, jj = np.nonzero(np.tril(M & core[:, None] & core[None, :], -1))
    for i, j in zip(ii.tolist(), jj.tolist()):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    root = np.array([find(i) if core[i] else -1 for i in range(n)], np.int64)
    reps = np.unique(root[core])  # ascending: cluster c's representative is its smallest row
    labels = np.full(n, -1, np.int32)
    labels[core] = np.searchsorted(reps, root[core]).astype(np.int32)
    # border: the smallest cluster number among the core neighbours
    big = np.iinfo(np.int32).max
    near = np.where(M & core[None, :], labels[None, :], big).min(axis=1) if n else np.zeros(0, np.int32)
    border = ~core & (near < big)
    labels[border] = near[border]
    summary = np.array([len(reps), core.sum(), border.sum(), n - core.sum() - border.sum()], np.int64)
    return labels, count, summary


def dbscan_definition(D, thr, min_samples):
    """Scalar definition on lists of Python floats: sklearn's expansion, one cluster at a time."""
    n = len(D)
    nb = [[j for j in range(n) if D[i][j] <= thr] for i in range(n)]
    core = [len(nb[i]) >= min_samples for i in range(n)]
    labels = [-1] * n
    c = 0
    for i in range(n):
        if labels[i] != -1 or not core[i]:
            continue
        labels[i] = c
        stack = [i]
        while stack:
            v = stack.pop()
            if core[v]:
                for w in nb[v]:
                    if labels[w] == -1:
                        labels[w] = c
                        stack.append(w)
        c += 1
    return labels, [len(x) for x in nb], core


# ---------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------
def dbscan_set(n, d, seed=None):
    """Six blobs on a 1/8 grid in features 0 and 1 and a seventh of the rows spread wide; further
    features small; an eighth of the rows exact copies of the first eighth."""
    r = np.random.default_rng(7 + d if seed is None else seed)
    centres = r.integers(-40, 41, (6, 2))
    which = r.integers(0, 7, n)
    P = np.where(which[:, None] < 6, centres[np.minimum(which, 5)] + np.rint(r.normal(0, 3.0, (n, 2))),
                 r.integers(-60, 61, (n, 2)))
    X = np.zeros((n, d), np.float32)
    X[:, :min(2, d)] = (P / 8)[:, :min(2, d)]
    if d > 2:
        X[:, 2:] = r.integers(-2, 3, (n, d - 2)) / 1024
    X[n // 2: n // 2 + n // 8] = X[: n // 8]
    return X


def bridge_set(G=29, d=2, seed=3):
    """G gadgets of nine points, 16 apart: a middle point with three neighbours (itself and one
    core row of a cluster on either side, both at distance exactly 1) between two clusters of four."""
    pts = []
    for g in range(G):
        x = 16.0 * g
        pts.append((x, 0.0))
        for s in (-1.0, 1.0):
            pts += [(x + s, 0.0), (x + 1.5 * s, 0.5), (x + 1.5 * s, -0.5), (x + 2.0 * s, 0.0)]
    X = np.zeros((len(pts), d), np.float32)
    X[:, :2] = np.array(pts, np.float32)
    return X[np.random.default_rng(seed).permutation(len(X))]


def chain_set(n, d=1):
    """The integers 0 .. n - 1 in scrambled order along feature 0: with thr = 1, one chain."""
    X = np.zeros((n, d), np.float32)
    X[:, 0] = np.random.default_rng(1).permutation(n)
    return X


@functools.lru_cache(maxsize=None)
def distances(kind, n, d, metric):
    """The float32 self-distance matrix of a builder set (shared, read-only)."""
    X = {"dbscan": dbscan_set, "chain": chain_set}[kind](n, d) if kind != "bridge" else bridge_set(d=d)
    D = metric_distances(X, X, metric)
    D.setflags(write=False)
    return X, D


def quantile_thr(D, q):
    """A matrix entry: a kernel that tested `<` would count differently."""
    return np.float32(np.quantile(D[D > 0], q, method="lower"))


@functools.lru_cache(maxsize=None)
def dbscan_case(n, d, metric, pair):
    """(X, thr, min_samples, (labels, count, summary)) of dbscan_set(n, d) at PAIRS[pair]."""
    X, D = distances("dbscan", n, d, metric)
    q, m = PAIRS[pair]
    thr = quantile_thr(D, q)
    return X, thr, m, dbscan_reference(D, thr, m)


def two_cluster_borders(D, thr, labels, count, m):
    """Per border row adjacent to >= 2 clusters: (row, the clusters of its core neighbours)."""
    core = count >= m
    out = []
    for i in np.flatnonzero(~core & (labels >= 0)):
        nb = np.flatnonzero((D[i] <= thr) & core)
        if len(set(labels[nb].tolist())) >= 2:
            out.append((int(i), nb))
    return out


# ---------------------------------------------------------------------------------
# the restatement against the scalar definition
# ---------------------------------------------------------------------------------
def _same_as_definition(X, thr, m, metric=EUCLIDEAN):
    D = metric_distances(X, X, metric)
    labels, count, summary = dbscan_reference(D, thr, m)
    dl, dc, dcore = dbscan_definition([[float(v) for v in row] for row in D], float(np.float32(thr)), m)
    assert labels.tolist() == dl
    assert count.tolist() == dc
    assert summary[1] == sum(dcore) and summary[0] == len(set(dl) - {-1})
    assert summary.sum() - summary[0] == len(X)
    return labels, count, summary


@pytest.mark.parametrize("metric", sorted(METRICS))
def test_hand_cases(metric):
    col = lambda *v: np.array(v, np.float32).reshape(-1, 1)
    # D == thr: 0, 1, 2 are each other's neighbours at distance exactly 1
    labels, count, _ = _same_as_definition(col(0, 1, 2, 10), 1.0, 3, metric)
    assert labels.tolist() == [0, 0, 0, -1] and count.tolist() == [2, 3, 2, 1]
    # thr = 0 with duplicates: a duplicate group of min_samples rows is a cluster
    labels, _, summary = _same_as_definition(col(5, 3, 5, 3, 7, 5), 0.0, 2, metric)
    assert labels.tolist() == [0, 1, 0, 1, -1, 0] and summary.tolist() == [2, 5, 0, 1]
    # min_samples = 1: every row is a core row
    labels, _, summary = _same_as_definition(col(0, 4, 1, 9), 1.0, 1, metric)
    assert labels.tolist() == [0, 1, 0, 2] and summary.tolist() == [3, 4, 0, 0]
    # min_samples > n: nothing but noise
    labels, _, summary = _same_as_definition(col(0, 1, 2), 5.0, 4, metric)
    assert labels.tolist() == [-1, -1, -1] and summary.tolist() == [0, 0, 0, 3]
    # a NaN row has an empty neighbourhood, itself included (the Chebyshev maximum skips a NaN
    # difference -- knn_amd.h "Metrics" -- so there the row is at distance 0 of every row)
    labels, count, summary = _same_as_definition(col(0, np.nan, 1, 2), 1.0, 2, metric)
    if metric == CHEBYSHEV:
        assert labels.tolist() == [0, 0, 0, 0] and count.tolist() == [3, 4, 4, 3]
    else:
        assert labels.tolist() == [0, -1, 0, 0] and count.tolist() == [2, 0, 3, 2]
    # border rows between two clusters (the bridge gadgets, two of them)
    _same_as_definition(bridge_set(G=2), 1.0, 4, metric)


# ---------------------------------------------------------------------------------
# the restatement against sklearn, on every builder set
# ---------------------------------------------------------------------------------
def _same_as_sklearn(D, thr, m, ref):
    cluster = pytest.importorskip("sklearn.cluster")
    labels, count, summary = ref
    sk = cluster.DBSCAN(eps=float(thr), min_samples=m, metric="precomputed").fit(np.asarray(D).astype(np.float64))
    assert np.array_equal(sk.labels_.astype(np.int32), labels)
    assert np.array_equal(sk.core_sample_indices_, np.flatnonzero(count >= m))


def _metrics_of(n):
    # (the 4,096-row matrix is checked under the Euclidean metric alone: the others take as long again)
    return sorted(METRICS) if n <= 1000 else [EUCLIDEAN]


@pytest.mark.parametrize("n,d", SETS)
def test_dbscan_set_against_sklearn(n, d):
    for metric in _metrics_of(n):
        _, D = distances("dbscan", n, d, metric)
        for pair in range(len(PAIRS)):
            _, thr, m, ref = dbscan_case(n, d, metric, pair)
            _same_as_sklearn(D, thr, m, ref)
            labels, count, summary = ref
            assert (D == thr).sum() >= 4  # the threshold is a matrix entry, met more than once
            if metric == CHEBYSHEV:
                continue
            if n >= 1000:
                assert summary[0] >= 3 and summary[2] >= 30 and summary[3] >= 100 and summary[1] >= 500, summary
            else:
                assert summary[0] >= 1, summary


@pytest.mark.parametrize("d", [2, 64])
@pytest.mark.parametrize("metric", sorted(METRICS))
def test_bridge_set(metric, d):
    X, D = distances("bridge", 0, d, metric)
    thr, m = np.float32(1.0), 4
    ref = dbscan_reference(D, thr, m)
    _same_as_sklearn(D, thr, m, ref)
    labels, count, summary = ref
    assert len(X) == 261 and summary.tolist() == [58, 232, 29, 0]
    two = two_cluster_borders(D, thr, labels, count, m)
    assert len(two) >= 20
    # how many rows tell the rule from the two plausible wrong ones
    first = nearest = 0
    for i, nb in two:
        assert (D[i, nb] == thr).all()  # the border pairs sit exactly on the threshold
        first += labels[nb.min()] != labels[i]
        near = nb[D[i, nb] == D[i, nb].min()].min()
        nearest += labels[near] != labels[i]
    assert first >= 8 and nearest >= 8, (first, nearest)


@pytest.mark.parametrize("metric", sorted(METRICS))
def test_chain_set(metric):
    X, D = distances("chain", 1000, 1, metric)
    ref = dbscan_reference(D, 1.0, 3)
    _same_as_sklearn(D, 1.0, 3, ref)
    labels, count, summary = ref
    assert summary.tolist() == [1, 998, 2, 0] and (labels == 0).all()


def test_sizes_helper(knn):
    assert knn.dbscan_sizes(np.array([0, -1, 2, 0, 2, 2], np.int32)).tolist() == [2, 0, 3]
    assert knn.dbscan_sizes(np.full(4, -1, np.int32)).tolist() == []


# ---------------------------------------------------------------------------------
# the CLI refuses a bad --dbscan before it creates a context: no GPU is needed
# ---------------------------------------------------------------------------------
CLI = os.path.join(PKG_DIR, "knn_cli")
SMALL = [os.path.join(REPO, "tests", "data", f"small-{s}.arff") for s in ("train", "test")]


@pytest.mark.parametrize("extra", [
    ["--dbscan=abc"], ["--dbscan=-1"], ["--dbscan=nan"], ["--dbscan="], ["--dbscan=1", "--min-samples=0"],
    ["--dbscan=1", "--min-samples=x"], ["--min-samples=3"], ["--dbscan=1", "--lof"], ["--dbscan=1", "--sweep"],
    ["--dbscan=1", "--sweep=loo"], ["--dbscan=1", "--regress"], ["--dbscan=1", "--radius=2"],
    ["--dbscan=1", "--radii=1,2"], ["--dbscan=1", "--weights=distance"], ["--dbscan=1", "--outlier=3"],
    ["--dbscan=1", "--lof-threshold=2"]])
def test_cli_refuses(extra):
    r = subprocess.run([CLI, *SMALL, "5", *extra], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    # (--lof-threshold= without --lof is refused by the LOF switch's own check, which comes first)
    assert ("usage: --lof" if "--lof-threshold=2" in extra else "usage: --dbscan=R") in r.stderr and r.stdout == ""
