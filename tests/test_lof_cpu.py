"""CPU-side checks of the local outlier factor: the numpy restatement that the GPU tests compare
bits against (lof_reference / lof_novelty_reference) is pinned to a second, definitional form and
cross-checked against sklearn's LocalOutlierFactor; the new entry points are declared, exported and
bound.  No GPU is needed here.

The rules (include/knn_amd.h, "Local outlier factor"): row i's list is its leave-one-out list;
delta is binary32 (sqrtf of the squared distance under the Euclidean metric); kd_k(i) = delta(i, o_k);
S_k(i) = sum_j (double)fmaxf(kd_k(o_j), delta(i, o_j)) in ascending j; lrd_k(i) = 1.0 / (S_k(i) / k +
1e-10); L_k(i) = sum_j lrd_k(o_j); LOF_k(i) = (float)(L_k(i) / (k * lrd_k(i))).  A prefix that reaches
a missing entry is NaN from there on.
"""
import os
import re

import numpy as np
import pytest

from conftest import REPO
from test_regress_cpu import fbits
from test_weighted_cpu import remove_self

EUCLIDEAN, MANHATTAN, CHEBYSHEV = 0, 1, 2


def lof_lists(idx, dist, self_base, k_hi, metric):
    """The self-removed lists of the restatement: (cidx int32 [n][k_hi], -1 = missing; delta float32
    [n][k_hi], NaN where missing).  idx / dist [n][kin >= k_hi (+ 1 with self_base)] as the library
    reports them (squared distances under the Euclidean metric)."""
    idx = np.asarray(idx, np.int32)
    dist = np.ascontiguousarray(dist, np.float32)
    if self_base is not None:
        idx, dist = remove_self(idx[:, :k_hi + 1], dist[:, :k_hi + 1], self_base)
    cidx = idx[:, :k_hi].copy()
    d = dist[:, :k_hi]
    with np.errstate(invalid="ignore"):
        delta = np.sqrt(d) if metric == EUCLIDEAN else d.copy()
    assert delta.dtype == np.float32
    delta[cidx < 0] = np.nan
    return cidx, delta


def _first_missing(cidx):
    miss = cidx < 0
    return np.where(miss.any(axis=1), miss.argmax(axis=1), cidx.shape[1])


def _lrd(cidx, delta, kd_table, k_lo, k_hi):
    """lrd float64 [rows][Kr] of rows with lists (cidx, delta) against kd_table float32 [n][Kr]: one
    step per list position, all rows at once, binary32 maximum and binary64 sum in list order."""
    assert kd_table.dtype == np.float32 and delta.dtype == np.float32
    n, Kr = len(cidx), k_hi - k_lo + 1
    fm = _first_missing(cidx)
    lrd = np.full((n, Kr), np.nan, np.float64)
    for e in range(Kr):
        k = k_lo + e
        S = np.zeros(n, np.float64)
        for j in range(k):
            kdv = kd_table[np.maximum(cidx[:, j], 0), e]
            reach = np.where(np.isnan(kdv), kdv, np.fmax(kdv, delta[:, j]))
            assert reach.dtype == np.float32
            S = S + reach.astype(np.float64)
        with np.errstate(invalid="ignore"):
            val = 1.0 / (S / np.float64(k) + 1e-10)
        lrd[:, e] = np.where(k <= fm, val, np.nan)
    return lrd


def _score(cidx, lrd_table, lrd_own, k_lo, k_hi):
    """lof float32 [Kr][rows]: binary64 sums of the neighbours' lrd in list order, one division,
    one rounding to binary32."""
    n, Kr = len(cidx), k_hi - k_lo + 1
    fm = _first_missing(cidx)
    lof = np.full((Kr, n), np.nan, np.float32)
    for e in range(Kr):
        k = k_lo + e
        L = np.zeros(n, np.float64)
        for j in range(k):
            L = L + lrd_table[np.maximum(cidx[:, j], 0), e]
        with np.errstate(invalid="ignore", divide="ignore"):
            val = (L / (np.float64(k) * lrd_own[:, e])).astype(np.float32)
        lof[e] = np.where(k <= fm, val, np.float32(np.nan))
    return lof


def lof_reference(idx, dist, self_base, k_lo, k_hi, metric):
    """Host restatement of k_lof_compact / k_lof_lrd / k_lof_score (test infrastructure) on the n
    rows' own lists: returns (kd float32 [n][Kr], lrd float64 [n][Kr], lof float32 [Kr][n],
    too_few)."""
    cidx, delta = lof_lists(idx, dist, self_base, k_hi, metric)
    kd = np.ascontiguousarray(delta[:, k_lo - 1:k_hi])
    lrd = _lrd(cidx, delta, kd, k_lo, k_hi)
    lof = _score(cidx, lrd, lrd, k_lo, k_hi)
    return kd, lrd, lof, bool((cidx < 0).any())


def lof_novelty_reference(qidx, qdist, kd, lrd, k_lo, k_hi, metric):
    """Novelty: the queries' plain top-k_hi lists against the fitted tables -> (lof float32 [Kr][nq],
    too_few)."""
    cidx, delta = lof_lists(qidx, qdist, None, k_hi, metric)
    own = _lrd(cidx, delta, np.ascontiguousarray(kd, np.float32), k_lo, k_hi)
    return _score(cidx, np.asarray(lrd, np.float64), own, k_lo, k_hi), bool((cidx < 0).any())


def lof_definition(idx, dist, self_base, k_lo, k_hi, metric):
    """The definition with nothing shared between the ks: per k and per row, Python floats
    (binary64) and numpy float32 scalars, from scratch."""
    cidx, delta = lof_lists(idx, dist, self_base, k_hi, metric)
    n, Kr = len(cidx), k_hi - k_lo + 1
    lof = np.full((Kr, n), np.nan, np.float32)

    def lrd_of(i, k):
        if (cidx[i, :k] < 0).any():
            return float("nan")
        S = 0.0
        for j in range(k):
            o = cidx[i, j]
            if (cidx[o, :k] < 0).any():
                return float("nan")
            kdo = np.float32(delta[o, k - 1])
            S = S + float(max(kdo, np.float32(delta[i, j])))
        return 1.0 / (S / float(k) + 1e-10)

    for e in range(Kr):
        k = k_lo + e
        lrd = [lrd_of(i, k) for i in range(n)]
        for i in range(n):
            if (cidx[i, :k] < 0).any():
                continue
            L = 0.0
            for j in range(k):
                L = L + lrd[cidx[i, j]]
            with np.errstate(invalid="ignore", divide="ignore"):
                lof[e, i] = np.float32(np.float64(L) / (np.float64(k) * np.float64(lrd[i])))
    return lof


def brute_lists(tr, te, k, metric):
    """Oracle-style brute force (test infrastructure): the k smallest (distance, index) pairs of
    every te row against tr, the distance accumulated one feature at a time in binary32 as the
    kernels do (squared differences, |differences| or their maximum); missing entries -1 / FLT_MAX."""
    tr = np.ascontiguousarray(tr, np.float32)
    te = np.ascontiguousarray(te, np.float32)
    acc = np.zeros((len(te), len(tr)), np.float32)
    for i in range(tr.shape[1]):
        df = te[:, i:i + 1] - tr[None, :, i]
        acc = acc + df * df if metric == EUCLIDEAN else acc + np.abs(df) if metric == MANHATTAN else np.maximum(acc, np.abs(df))
    assert acc.dtype == np.float32
    order = np.lexsort((np.broadcast_to(np.arange(len(tr)), acc.shape), acc), axis=1)[:, :k]
    idx = np.full((len(te), k), -1, np.int32)
    dist = np.full((len(te), k), np.finfo(np.float32).max, np.float32)
    idx[:, :order.shape[1]] = order
    dist[:, :order.shape[1]] = np.take_along_axis(acc, order, axis=1)
    return idx, dist


def mixed_rows(n=193, d=5, seed=11):
    """The small mixed case: random rows, one row repeated 9 times (more copies than k_hi + 1 = 8),
    one repeated 3 times, and one far row."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[[3, 20, 41, 60, 77, 100, 130, 150, 192]] = x[3]
    x[[8, 90, 171]] = x[8]
    x[57] = np.float32(25.0)
    return x


def ulp_diff(a, b):
    """|a - b| in units in the last place of binary32 (finite values of one sign)."""
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def test_lof_symbols_in_header_and_library(knn):
    with open(os.path.join(REPO, "include", "knn_amd.h")) as f:
        text = f.read()
    declared = set(re.findall(r"\b(knn_[a-z_0-9]+)\s*\(", text))
    assert "Local outlier factor" in text
    lib = knn.load_library()
    for s in ("knn_lof_fit_device", "knn_lof_score_device", "knn_lof_lists_device"):
        assert s in declared, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.knn_version() == 3
    for m in ("lof_device", "lof_fit_device", "lof_lists_device"):
        assert callable(getattr(knn.Context, m)), m
    assert callable(knn.LofModel.score_device) and callable(knn.lof_max) and callable(knn.lof_outliers)
    # NULL context: no crash, KNN_EINVAL (the argument checks behind a context run on the GPU:
    # test_gpu_lof.py::test_argument_checks -- no context exists without a device)
    assert lib.knn_lof_fit_device(None, None, 1, 7, None, None, None, None, None, None) == knn.KNN_EINVAL
    assert lib.knn_lof_score_device(None, None, None, 1, 7, None, None, None, None) == knn.KNN_EINVAL
    assert lib.knn_lof_lists_device(None, 0, 8, None, None, 8, 0, 1, 7, None, None, None, None) == knn.KNN_EINVAL


@pytest.mark.parametrize("metric", [EUCLIDEAN, MANHATTAN, CHEBYSHEV])
def test_restatement_matches_definition(metric):
    x = mixed_rows()
    idx, dist = brute_lists(x, x, 8, metric)
    kd, lrd, lof, too_few = lof_reference(idx, dist, 0, 1, 7, metric)
    assert not too_few and kd.shape == (193, 7) and lrd.dtype == np.float64 and lof.shape == (7, 193)
    want = lof_definition(idx, dist, 0, 1, 7, metric)
    assert np.array_equal(fbits(lof), fbits(want)) and np.isfinite(lof).all()
    # the case is the one the issue names: a row absent from its own list, the 1e-10 path, zero
    # distances inside a finite sum, and a large score
    assert 192 not in idx[192] and 3 in idx[3] and (dist[192] == 0).all()
    assert (lrd[3] > 1e9).all() and lof[6, 57] > 5 and kd[8, 1] == 0 and kd[8, 2] > 0
    # a sub-range is the same numbers
    sub = lof_reference(idx[:, :6], dist[:, :6], 0, 3, 5, metric)
    assert np.array_equal(fbits(sub[2]), fbits(lof[2:5])) and np.array_equal(sub[1], lrd[:, 2:5])


def test_missing_entries():
    """n = 5, range 1..7: k <= 4 finite, k >= 5 NaN."""
    x = np.random.default_rng(2).standard_normal((5, 3)).astype(np.float32)
    idx, dist = brute_lists(x, x, 8, EUCLIDEAN)
    assert (idx[:, 5:] == -1).all()
    kd, lrd, lof, too_few = lof_reference(idx, dist, 0, 1, 7, EUCLIDEAN)
    assert too_few and np.isfinite(lof[:4]).all() and np.isnan(lof[4:]).all() and np.isnan(lrd[:, 4:]).all()
    want = lof_definition(idx, dist, 0, 1, 7, EUCLIDEAN)
    assert np.array_equal(fbits(lof), fbits(want))


def test_helpers(knn):
    lof = np.array([[1.0, 2.5, np.nan, 0.9], [1.2, 1.6, np.nan, np.nan]], np.float32)
    m = knn.lof_max(lof)
    assert m.dtype == np.float32 and m[:2].tolist() == [np.float32(1.2), 2.5] and np.isnan(m[2]) and m[3] == np.float32(0.9)
    assert knn.lof_outliers(m).tolist() == [1] and knn.lof_outliers(m, 1.0).tolist() == [0, 1]
    assert knn.lof_outliers(m).dtype == np.int64


# the seed: confirmed on the CPU that sklearn's neighbour indices equal the restatement's lists at
# k = 5 and k = 20, for the fit and for the queries (seed 0, the first tried, holds); the test
# asserts it as its precondition
SK_SEED = 0
SK_N, SK_D, SK_NQ = 300, 4, 67


def _grid_rows(seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 20, size=(SK_N, SK_D)).astype(np.float64) * 2.0 ** -20
    q = rng.integers(0, 1 << 20, size=(SK_NQ, SK_D)).astype(np.float64) * 2.0 ** -20
    q[5] = x[17]                                   # a query equal to a train row
    return x, q


@pytest.mark.parametrize("k", [5, 20])
def test_rules_against_sklearn(k):
    """The rules, not the kernels, against sklearn.neighbors.LocalOutlierFactor under the Manhattan
    metric on features that are multiples of 2^-20 in [0, 1): every distance (a sum of 4 terms
    below 4) is exact in binary32 and binary64 alike.  Precondition, asserted: sklearn's neighbour
    indices equal the restatement's lists (no tie at a list's edge for this seed).  Then both sides
    are binary64 chains of at most 20 terms and one rounding to binary32: at most 1 ulp apart."""
    neighbors = pytest.importorskip("sklearn.neighbors")
    x, q = _grid_rows(SK_SEED)
    x32, q32 = x.astype(np.float32), q.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x)
    idx, dist = brute_lists(x32, x32, k + 1, MANHATTAN)
    m = neighbors.LocalOutlierFactor(n_neighbors=k, algorithm="brute", metric="manhattan").fit(x)
    sk_dist, sk_idx = m.kneighbors()
    cidx, delta = lof_lists(idx, dist, 0, k, MANHATTAN)
    assert np.array_equal(sk_idx, cidx) and np.array_equal(sk_dist, delta.astype(np.float64))
    kd, lrd, lof, too_few = lof_reference(idx, dist, 0, k, k, MANHATTAN)
    assert not too_few
    want = (-m.negative_outlier_factor_).astype(np.float32)
    ulps = ulp_diff(lof[0], want)
    print(f"k={k}: fit, largest difference {ulps.max()} ulp, {np.count_nonzero(ulps)} of {SK_N} rows differ")
    assert ulps.max() <= 1
    # novelty
    nov = neighbors.LocalOutlierFactor(n_neighbors=k, algorithm="brute", metric="manhattan", novelty=True).fit(x)
    qidx, qdist = brute_lists(x32, q32, k, MANHATTAN)
    sk_qd, sk_qi = nov.kneighbors(q)
    assert np.array_equal(sk_qi, qidx) and np.array_equal(sk_qd, qdist.astype(np.float64))
    assert qidx[5, 0] == 17 and qdist[5, 0] == 0
    got, too_few = lof_novelty_reference(qidx, qdist, kd, lrd, k, k, MANHATTAN)
    assert not too_few
    want = (-nov.score_samples(q)).astype(np.float32)
    ulps = ulp_diff(got[0], want)
    print(f"k={k}: novelty, largest difference {ulps.max()} ulp, {np.count_nonzero(ulps)} of {SK_NQ} queries differ")
    assert ulps.max() <= 1
