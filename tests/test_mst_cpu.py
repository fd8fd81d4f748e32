"""The mutual-reachability spanning tree (include/knn_amd.h "Spanning tree"): the yardstick of the
GPU tests, in numpy on a float32 distance matrix.

mst_reference is Prim's algorithm under the header's STRICT edge order (w, min(a, b), max(a, b)); the
minimum spanning forest under a strict order is unique, so any correct algorithm returns the same
edge set.  It is pinned three ways, all exact:
  * to Kruskal under the same order, and its sorted weights to scipy's minimum_spanning_tree (every
    minimum spanning tree has the same multiset of weights, ties or not);
  * its cut to sklearn.cluster.DBSCAN(metric="precomputed") on the core rows, -1 elsewhere;
  * knn.mst_linkage + scipy's fcluster(Z, t, "distance") to the cut with min_samples = 1.
boruvka restates the GPU driver's rounds with the list shortcut (resolved / unresolved rows, the
strict inequality) and must return the same edges with it and without.
"""
import functools

import numpy as np
import pytest

from test_dbscan_cpu import METRICS, PAIRS, SETS, dbscan_reference, distances, quantile_thr
from test_metric_cpu import CHEBYSHEV, EUCLIDEAN, FLT_MAX, MANHATTAN, bits, metric_distances

INF = np.float32(np.inf)
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
LIST_L = 32  # the library's list length beyond min_samples (knn_capi.cpp KNN_MST_LIST_L)


# ---------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------
def qualifying(D):
    """D where a pair qualifies (top-k's rule D < FLT_MAX; NaN never does), +inf elsewhere."""
    D = np.asarray(D, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(D < FLT_MAX, D, INF)


def core_distances(D, min_samples):
    """c float32 [n]: the min_samples-th smallest qualifying D(i, .), the row itself included; +inf
    when fewer rows qualify."""
    return np.sort(qualifying(D), axis=1)[:, min_samples - 1].astype(np.float32)


def reach_weights(D, c):
    """w float32 [n][n] = fmaxf(fmaxf(c(a), c(b)), D), +inf where the pair is no edge; the diagonal is none."""
    Dq = qualifying(D)
    W = np.fmax(np.fmax(c[:, None], c[None, :]), Dq).astype(np.float32)
    W[Dq == INF] = INF
    np.fill_diagonal(W, INF)
    return W, Dq < INF  # (an edge may weigh +inf: c = +inf with a finite D)


def _keys(w_row, edge_row, u, n):
    """uint64 keys bits(w) << 26 | lo << 13 | hi of row u's pairs (n <= 8192); NONE where no edge."""
    t = np.arange(n, dtype=np.uint64)
    lo, hi = np.minimum(t, np.uint64(u)), np.maximum(t, np.uint64(u))
    k = (bits(w_row).astype(np.uint64) << np.uint64(26)) | (lo << np.uint64(13)) | hi
    k[~edge_row] = NONE
    k[u] = NONE
    return k


def mst_reference(D, min_samples):
    """(w float32 [E], a int32 [E], b int32 [E], core float32 [n], summary int64 [2] = {E, n - E}):
    vectorised Prim under the strict order, one tree per component, the edges sorted by the order."""
    D = np.asarray(D, np.float32)
    n = len(D)
    assert n <= 8192
    c = core_distances(D, min_samples) if n else np.zeros(0, np.float32)
    W, edge = reach_weights(D, c) if n else (D, D)
    intree = np.zeros(n, bool)
    best = np.full(n, NONE, np.uint64)
    out = []
    for _ in range(n):
        cand = np.where(intree, NONE, best)
        v = int(np.argmin(cand)) if n else 0
        if cand[v] == NONE:  # a new tree: the smallest row outside
            v = int(np.flatnonzero(~intree)[0])
        else:
            out.append(int(cand[v]))
        intree[v] = True
        best = np.minimum(best, _keys(W[v], edge[v], v, n))
    out = np.sort(np.array(out, np.uint64))
    a = ((out >> np.uint64(13)) & np.uint64(8191)).astype(np.int32)
    b = (out & np.uint64(8191)).astype(np.int32)
    w = (out >> np.uint64(26)).astype(np.uint32).view(np.float32)
    return w, a, b, c, np.array([len(out), n - len(out)], np.int64)


def kruskal(D, min_samples):
    """The same forest by Kruskal: every edge in the strict order, a plain union-find."""
    n = len(D)
    c = core_distances(D, min_samples)
    W, edge = reach_weights(D, c)
    ii, jj = np.nonzero(np.triu(edge, 1))
    order = np.lexsort((jj, ii, bits(W[ii, jj])))
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    out = []
    for e in order.tolist():
        ra, rb = find(int(ii[e])), find(int(jj[e]))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            out.append(e)
            if len(out) == n - 1:
                break
    e = np.array(out, np.int64)
    return W[ii[e], jj[e]], ii[e].astype(np.int32), jj[e].astype(np.int32)


def mst_cut(w, a, b, core, thr, n):
    """(labels int32 [R][n], summary int64 [R][3] = {clusters, core rows, other rows}): per threshold
    the components of the edges with w <= thr over the rows with c <= thr, numbered by ascending
    smallest row; every other row -1."""
    thr = np.atleast_1d(np.asarray(thr, np.float32))
    labels = np.full((len(thr), n), -1, np.int32)
    summary = np.zeros((len(thr), 3), np.int64)
    for r, t in enumerate(thr):
        parent = list(range(n))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for e in np.flatnonzero(w <= t).tolist():
            ra, rb = find(int(a[e])), find(int(b[e]))
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        is_core = core <= t
        root = np.array([find(i) for i in range(n)], np.int64)
        reps = np.unique(root[is_core])
        labels[r, is_core] = np.searchsorted(reps, root[is_core]).astype(np.int32)
        summary[r] = (len(reps), is_core.sum(), n - is_core.sum())
    return labels, summary


# ---------------------------------------------------------------------------------
# the driver's rounds, with the list shortcut
# ---------------------------------------------------------------------------------
def top_lists(D, K):
    """(idx int32 [n][K], dist float32 [n][K], dlast float32 [n]): the K smallest (D, index) pairs
    of every row among the qualifying ones, -1 / +inf where missing; dlast = +inf for a list that
    holds every candidate of the row (K == n, or a missing entry)."""
    Dq = qualifying(D)
    n = len(Dq)
    idx = np.argsort(Dq, axis=1, kind="stable")[:, :K].astype(np.int32)
    dist = np.take_along_axis(Dq, idx, axis=1)
    idx[dist == INF] = -1
    complete = (dist == INF).any(axis=1) | (K >= n)
    return idx, dist, np.where(complete, INF, dist[:, -1]).astype(np.float32)


def row_key(w, t):
    return (np.uint64(np.float32(w).view(np.uint32)) << np.uint64(32)) | np.uint64(t)


def resolve(q, idx, dist, dlast, core, comp, strict=True):
    """(key, resolved) of row q from its list alone: the smallest bits(w) << 32 | t over the listed
    rows of another component; resolved iff the list is complete or that w < dlast STRICTLY."""
    best = NONE
    for t, dd in zip(idx[q].tolist(), dist[q].tolist()):
        if t < 0 or comp[t] == comp[q]:
            continue
        best = min(best, row_key(np.fmax(np.fmax(core[q], core[t]), np.float32(dd)), t))
    if dlast[q] == INF:
        return best, True
    if best == NONE:
        return best, False
    w = np.uint32(best >> np.uint64(32)).view(np.float32)
    return best, bool(w < dlast[q] if strict else w <= dlast[q])


def scan(q, W, edge, comp):
    """The pass: the smallest key of row q over ALL rows of another component."""
    ok = edge[q] & (comp != comp[q])
    if not ok.any():
        return NONE
    t = np.flatnonzero(ok)
    return ((bits(W[q, t]).astype(np.uint64) << np.uint64(32)) | t.astype(np.uint64)).min()


def boruvka(D, min_samples, K, use_lists=True):
    """(w, a, b, rounds, pass rows per round) by the driver's rounds: resolve or scan per row, the
    component minimum under (w, lo, hi), one union per component, flatten."""
    n = len(D)
    core = core_distances(D, min_samples)
    W, edge = reach_weights(D, core)
    idx, dist, dlast = top_lists(D, K)
    comp = np.arange(n)
    edges, rows = set(), []
    while len(edges) < n - 1:
        keys, sent = np.full(n, NONE, np.uint64), 0
        for q in range(n):
            key, done = resolve(q, idx, dist, dlast, core, comp) if use_lists else (NONE, False)
            if not done:
                sent += 1
                key = scan(q, W, edge, comp)
            keys[q] = key
        rows.append(sent)
        pick = {}
        for q in np.flatnonzero(keys != NONE).tolist():
            t = int(keys[q] & np.uint64(0xFFFFFFFF))
            e = (int(keys[q] >> np.uint64(32)), min(q, t), max(q, t))
            pick[comp[q]] = min(pick.get(comp[q], e), e)
        if not pick:
            break
        before = len(edges)
        edges |= set(pick.values())
        assert len(edges) > before
        parent = {int(r): int(r) for r in np.unique(comp)}

        def find(x):
            while parent[x] != x:
                x = parent[x]
            return x

        for _, lo, hi in pick.values():
            ra, rb = find(int(comp[lo])), find(int(comp[hi]))
            assert ra != rb or (_, lo, hi) in edges
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        comp = np.array([find(int(r)) for r in comp])
    e = sorted(edges)
    w = np.array([x[0] for x in e], np.uint32).view(np.float32)
    return w, np.array([x[1] for x in e], np.int32), np.array([x[2] for x in e], np.int32), len(rows), rows


# ---------------------------------------------------------------------------------
# builders shared with the GPU tests
# ---------------------------------------------------------------------------------
def gaussian_set(n=300, d=5, seed=11):
    return np.random.default_rng(seed).normal(0, 1, (n, d)).astype(np.float32)


def copies_set(n=200, copies=70, d=3, seed=5):
    """Lattice rows with `copies` exact copies of row 3 scattered among them: c = 0 ties, more copies
    than a list holds."""
    r = np.random.default_rng(seed)
    X = (r.integers(-20, 21, (n, d)) / 4).astype(np.float32)
    X[r.permutation(n)[:copies]] = X[3]
    return X


@functools.lru_cache(maxsize=None)
def mst_case(kind, n, d, metric, min_samples):
    """(X, D, mst_reference(D, min_samples)) of a builder set (shared, read-only)."""
    if kind == "gauss":
        X = gaussian_set(n, d)
        D = metric_distances(X, X, metric)
    elif kind == "copies":
        X = copies_set(n, d=d)
        D = metric_distances(X, X, metric)
    else:
        X, D = distances(kind, n, d, metric)
    return X, D, mst_reference(D, min_samples)


def partition(labels):
    """A labelling's partition, as a canonical tuple (first occurrence order)."""
    seen = {}
    return tuple(seen.setdefault(int(v), len(seen)) for v in labels)


# ---------------------------------------------------------------------------------
# pinned to Kruskal and scipy
# ---------------------------------------------------------------------------------
def _same_edges(got, want):
    for g, r, name in zip(got, want, "wab"):
        assert np.array_equal(bits(g) if name == "w" else g, bits(r) if name == "w" else r), name


@pytest.mark.parametrize("metric", sorted(METRICS))
@pytest.mark.parametrize("kind,n,d,m", [("gauss", 300, 5, 1), ("gauss", 300, 5, 4), ("dbscan", 1000, 3, 4),
                                        ("dbscan", 65, 1, 17), ("copies", 200, 3, 4), ("bridge", 0, 2, 4)])
def test_prim_is_kruskal(kind, n, d, m, metric):
    _, D, (w, a, b, c, summary) = mst_case(kind, n, d, metric, m)
    _same_edges((w, a, b), kruskal(D, m))
    assert summary.tolist() == [len(D) - 1, 1] and (a < b).all()
    key = (bits(w).astype(np.uint64) << np.uint64(32)) | a.astype(np.uint64)
    assert (np.diff(key.astype(np.float64)) >= 0).all()  # ascending by w, then a
    if kind != "gauss":
        assert (np.diff(bits(w).astype(np.int64)) == 0).sum() >= 10  # ties are the rule


@pytest.mark.parametrize("m", [1, 4])
def test_weights_against_scipy(m):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    _, D, (w, a, b, c, _) = mst_case("gauss", 300, 5, EUCLIDEAN, m)
    W, _ = reach_weights(D, c)
    assert (W[~np.eye(len(W), dtype=bool)] > 0).all()  # (scipy reads a zero as no edge)
    if m == 1:
        assert len(np.unique(w)) == len(w)  # no two tree edges tie
    T = csgraph.minimum_spanning_tree(W.astype(np.float64)).toarray()
    assert np.array_equal(np.sort(T[T > 0]).astype(np.float32), np.sort(w))


def test_core_distance_is_the_count_rule():
    """c(i) <= thr iff DBSCAN's count[i] >= min_samples at thr, thresholds on matrix entries."""
    _, D = distances("dbscan", 1000, 3, EUCLIDEAN)
    for q, m in PAIRS:
        thr = quantile_thr(D, q)
        _, count, _ = dbscan_reference(D, thr, m)
        assert np.array_equal(core_distances(D, m) <= thr, count >= m)


def test_nan_row():
    """A NaN feature: under the Euclidean and Manhattan metrics the row has no edge and c = +inf; the
    Chebyshev maximum skips the difference."""
    X = gaussian_set(40, 3)
    X[7, 1] = np.nan
    for metric in sorted(METRICS):
        w, a, b, c, summary = mst_reference(metric_distances(X, X, metric), 3)
        if metric == CHEBYSHEV:
            assert summary.tolist() == [39, 1] and np.isfinite(c).all()
        else:
            assert summary.tolist() == [38, 2] and c[7] == INF and 7 not in set(a) | set(b)
            assert np.isfinite(np.delete(c, 7)).all()


# ---------------------------------------------------------------------------------
# the cut against sklearn
# ---------------------------------------------------------------------------------
def _cut_is_dbscan_star(D, m, thrs):
    cluster = pytest.importorskip("sklearn.cluster")
    w, a, b, c, _ = mst_reference(D, m)
    n = len(D)
    labels, summary = mst_cut(w, a, b, c, thrs, n)
    D64 = np.asarray(D).astype(np.float64)
    for r, thr in enumerate(thrs):
        sk = cluster.DBSCAN(eps=float(thr), min_samples=m, metric="precomputed").fit(D64)
        core = np.zeros(n, bool)
        core[sk.core_sample_indices_] = True
        assert np.array_equal(labels[r], np.where(core, sk.labels_, -1).astype(np.int32)), (r, thr)
        assert summary[r].tolist() == [len(set(sk.labels_[core].tolist())), core.sum(), n - core.sum()]
        # and the project's own restatement, where it counts a row as core
        ref_labels, count, _ = dbscan_reference(D, thr, m)
        assert np.array_equal(labels[r], np.where(count >= m, ref_labels, -1))
    return labels, summary


@pytest.mark.parametrize("n,d", SETS)
def test_cut_dbscan_sets(n, d):
    for metric in (sorted(METRICS) if n <= 1000 else [EUCLIDEAN]):
        _, D = distances("dbscan", n, d, metric)
        for q, m in PAIRS:
            _cut_is_dbscan_star(D, m, [quantile_thr(D, q)])


@pytest.mark.parametrize("metric", sorted(METRICS))
def test_cut_bridge_and_chain(metric):
    _, D = distances("bridge", 0, 2, metric)
    labels, summary = _cut_is_dbscan_star(D, 4, np.array([0.5, 1.0, 2.0], np.float32))
    assert summary[1].tolist() == [58, 232, 29]  # the 29 middle points are border rows: not assigned
    _, D = distances("chain", 1000, 1, metric)
    labels, summary = _cut_is_dbscan_star(D, 3, np.array([0.5, 1.0, 1.0, 2.0], np.float32))
    assert summary[:, 0].tolist() == [0, 1, 1, 1] and summary[1, 1] == 998


# ---------------------------------------------------------------------------------
# the linkage helper against scipy
# ---------------------------------------------------------------------------------
def test_linkage_against_fcluster(knn):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    for kind, n, d in (("gauss", 300, 5), ("dbscan", 1000, 3)):
        _, D, (w, a, b, c, _) = mst_case(kind, n, d, EUCLIDEAN, 1)
        n = len(D)
        assert (c == 0).all()
        Z = knn.mst_linkage(w, a, b, n)
        assert Z.shape == (n - 1, 4) and Z.dtype == np.float64 and hierarchy.is_valid_linkage(Z)
        assert Z[-1, 3] == n and (Z[:, 0] < Z[:, 1]).all()
        for t in np.quantile(w, [0.0, 0.3, 0.7, 0.95, 1.0], method="lower"):
            labels, _ = mst_cut(w, a, b, c, [t], n)
            assert partition(hierarchy.fcluster(Z, float(t), "distance")) == partition(labels[0]), t


def test_linkage_refuses_a_forest(knn):
    with pytest.raises(ValueError):
        knn.mst_linkage(np.ones(2, np.float32), np.array([0, 2], np.int32), np.array([1, 3], np.int32), 4)
    with pytest.raises(ValueError):
        knn.mst_linkage(np.ones(3, np.float32), np.array([0, 1, 0], np.int32), np.array([1, 2, 2], np.int32), 4)
    assert knn.mst_linkage(np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32), 1).shape == (0, 4)


# ---------------------------------------------------------------------------------
# the list shortcut
# ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,d,m,K", [("gauss", 120, 3, 4, 16), ("copies", 200, 3, 4, 16), ("dbscan", 65, 1, 17, 17),
                                           ("dbscan", 65, 1, 1, 4), ("chain", 150, 1, 1, 3)])
def test_boruvka_with_and_without_lists(kind, n, d, m, K):
    _, D, (w, a, b, c, _) = mst_case(kind, n, d, EUCLIDEAN, m)
    n = len(D)
    on = boruvka(D, m, K, True)
    off = boruvka(D, m, K, False)
    _same_edges(on[:3], (w, a, b))
    _same_edges(off[:3], (w, a, b))
    bound = int(np.ceil(np.log2(n))) + 1
    assert on[3] <= bound and off[3] <= bound
    assert off[4] == [n] * off[3]       # without the shortcut every row goes through every pass
    if K == m:
        # w >= c(q) = dlast: no listed candidate is ever strictly below it -- why the lists are longer
        assert on[4] == off[4]
    else:
        assert sum(on[4]) < sum(off[4])  # with it some rows never go


def test_tie_at_dlast_is_unresolved():
    """w == dlast with an unlisted row of smaller index at the same w: the row must go through the
    pass.  Manhattan, min_samples = K = 3; row 2 (x = 0) lists itself, row 3 (x = 0.5) and row 0
    (x = 1, dlast = 1); row 1 (x = -1, D = 1) is unlisted.  With rows 0 and 2 in one component the
    listed candidate is row 3 at w = c(2) = 1 and the unlisted row 1 has w = 1 too."""
    X = np.array([[1.0], [-1.0], [0.0], [0.5], [-1.25]], np.float32)
    D = metric_distances(X, X, MANHATTAN)
    core = core_distances(D, 3)
    W, edge = reach_weights(D, core)
    idx, dist, dlast = top_lists(D, 3)
    assert idx[2].tolist() == [2, 3, 0] and dlast[2] == 1.0 and core[2] == 1.0
    assert W[2, 3] == 1.0 and W[2, 1] == 1.0
    comp = np.array([0, 1, 0, 3, 4])
    key, done = resolve(2, idx, dist, dlast, core, comp)
    assert key == row_key(1.0, 3) and not done
    assert resolve(2, idx, dist, dlast, core, comp, strict=False)[1]  # `<=` would have taken row 3
    assert scan(2, W, edge, comp) == row_key(1.0, 1)                 # the pass finds the smaller index
    w, a, b, _, _ = mst_reference(D, 3)
    for use in (True, False):
        _same_edges(boruvka(D, 3, 3, use)[:3], (w, a, b))
