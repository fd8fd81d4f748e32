"""CPU-side checks of the radius-neighbour feature: the entry points are declared, exported and
bound, and the numpy restatements the GPU tests compare against (radius_reference,
radius_vote_reference, radius_regress_reference) are pinned to scalar definitions written with
float32 / float64 scalars and plain Python control flow.  The input sets and thresholds of
tests/test_gpu_radius.py are made here too, with assertions that they can tell a kernel that tests
'<' instead of '<=', loses empty neighbourhoods or caps a list at 1,024 from a right one.  No GPU
is needed here.

The rules (include/knn_amd.h, "Radius neighbours"): train row t is a neighbour of query q iff
D(q, t) <= thr, D the bits a top-k pass exports under the context's metric; with self_base the row
self_base + q is left out by index; lists are CSR in ascending train index; the weighted vote adds
binary32 weights in list order, with the zero rule on ANY zero distance of the segment; regression
adds in binary64 in list order; an empty segment votes outlier_label and predicts NaN.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, REPO
from test_metric_cpu import CHEBYSHEV, EUCLIDEAN, FLT_MAX, MANHATTAN, TINY_CASES, bits, metric_distances, metric_set

METRICS = (EUCLIDEAN, MANHATTAN, CHEBYSHEV)
METRIC_NAMES = {EUCLIDEAN: "euclidean", MANHATTAN: "manhattan", CHEBYSHEV: "chebyshev"}
UNIFORM, INV_DIST, INV_SQDIST = 0, 1, 2
WEIGHT_NAMES = {UNIFORM: "uniform", INV_DIST: "distance", INV_SQDIST: "sqdist"}

# (d, nt, nq, kind) of the GPU tests: one full tile plus one row; partial query blocks on both
# sides of 64; 1-3 trailing features; one chunk and more than DT_MAX_DC = 128; neighbourhoods
# above 1,024
RADIUS_SHAPES = [(1, 65, 1, "float"), (3, 1000, 257, "grid"), (11, 1000, 257, "float"), (11, 4096, 9, "grid"),
                 (64, 4096, 257, "float"), (64, 65, 9, "grid"), (129, 1000, 33, "float"), (260, 4096, 9, "float")]
QUANTILES = (0.002, 0.05, 0.5)


# ---------------------------------------------------------------------------------------
# restatements (numpy, vectorised) -- what the GPU tests compare against
# ---------------------------------------------------------------------------------------
def radius_members(D, thr, self_base=None):
    """bool [nq][nt]: D <= thr (a NaN or inf D never is), without the self row."""
    with np.errstate(invalid="ignore"):
        m = D <= np.float32(thr)
    if self_base is not None:
        q = np.arange(len(D))
        m[q, self_base + q] = False
    return m


def radius_reference(train, test, thr, metric, self_base=None, labels=None, C=None, D=None):
    """(count int32 [nq], offsets int64 [nq + 1], idx int32 [total], dist float32 [total],
    class_counts int32 [nq][C] or None): the lists in CSR form, ascending train index."""
    D = metric_distances(train, test, metric) if D is None else D
    m = radius_members(D, thr, self_base)
    count = m.sum(axis=1).astype(np.int32)
    offsets = np.zeros(len(D) + 1, np.int64)
    offsets[1:] = np.cumsum(count, dtype=np.int64)
    q, t = np.nonzero(m)                    # row-major: q ascending, t ascending within q
    cc = None
    if labels is not None:
        cc = np.zeros((len(D), C), np.int32)
        np.add.at(cc, (q, np.asarray(labels)[t]), 1)
    return count, offsets, t.astype(np.int32), D[q, t], cc


def count_vote_reference(cc, outlier):
    """The uniform vote of the count pass: argmax of the class counts, ties to the smallest
    label; outlier where there is no neighbour."""
    return np.where(cc.sum(axis=1) > 0, cc.argmax(axis=1), outlier).astype(np.int32)


def radius_weights(dist, weights, metric):
    """The binary32 weights of one segment (the zero rule included)."""
    dist = np.asarray(dist, np.float32)
    if weights == UNIFORM:
        return np.ones(len(dist), np.float32)
    if (dist == 0).any():
        return (dist == 0).astype(np.float32)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        if weights == INV_DIST and metric == EUCLIDEAN:
            w = np.float32(1.0) / np.sqrt(dist)
        else:
            assert weights == INV_DIST or metric == EUCLIDEAN   # no 1 / D^2 kind under the other metrics
            w = np.float32(1.0) / dist
    assert w.dtype == np.float32
    return w


def radius_vote_reference(offsets, idx, dist, labels, C, weights, metric, outlier):
    """(pred int32 [nq], scores float32 [nq][C]): S_c = fl(S_c + w_j) in float32 in ascending list
    position (numpy's accumulate adds one element at a time), argmax with ties to the smallest
    label, outlier and an all +0 row for an empty segment."""
    nq = len(offsets) - 1
    pred = np.full(nq, outlier, np.int32)
    scores = np.zeros((nq, C), np.float32)
    for q in range(nq):
        a, b = offsets[q], offsets[q + 1]
        if a == b:
            continue
        w = radius_weights(dist[a:b], weights, metric)
        lab = np.asarray(labels)[idx[a:b]]
        for c in np.unique(lab):
            scores[q, c] = np.add.accumulate(w[lab == c], dtype=np.float32)[-1]
        pred[q] = np.argmax(bits(scores[q]))        # S >= +0: the bits order like the values
    return pred, scores


def radius_regress_reference(offsets, idx, dist, targets, weights, metric):
    """float32 [nq]: (float)(N / Dn), both sums in float64 in list order; NaN for an empty segment."""
    nq = len(offsets) - 1
    pred = np.full(nq, np.nan, np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for q in range(nq):
            a, b = offsets[q], offsets[q + 1]
            if a == b:
                continue
            w = radius_weights(dist[a:b], weights, metric).astype(np.float64)
            y = np.asarray(targets, np.float32)[idx[a:b]].astype(np.float64)
            N = np.add.accumulate(w * y)[-1]
            Dn = np.add.accumulate(w)[-1]
            pred[q] = np.float32(N / Dn)
    return pred


def radius_thresholds(D):
    """The GPU tests' thresholds, taken from the reference distance matrix itself: +0.0 and the
    entries at sorted positions int(q * size).  A threshold that is a matrix entry has at least one
    pair with D == thr, so a kernel that tests '<' gets another count."""
    flat = np.sort(D, axis=None)
    return [np.float32(0.0)] + [flat[int(q * flat.size)] for q in QUANTILES]


# ---------------------------------------------------------------------------------------
# scalar definitions: float32 / float64 scalars, plain Python control flow
# ---------------------------------------------------------------------------------------
def distance_definition(qrow, trow, metric):
    zero = np.float32(0.0)
    acc = zero
    for i in range(len(trow)):
        df = np.float32(qrow[i]) - np.float32(trow[i])
        if metric == EUCLIDEAN:
            acc = np.float32(acc + np.float32(df * df))
            continue
        a = -df if df < zero else df               # |df|; NaN stays NaN
        if metric == MANHATTAN:
            acc = np.float32(acc + a)
        elif a > acc:                              # fmaxf: a NaN never compares greater
            acc = a
    return acc


def radius_definition(train, test, thr, metric, self_base=None):
    """Python lists: per query, [(train index, distance)] in ascending index."""
    out = []
    thr = np.float32(thr)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for q in range(len(test)):
            seg = []
            for t in range(len(train)):
                if self_base is not None and t == self_base + q:
                    continue
                D = distance_definition(test[q], train[t], metric)
                if D <= thr:                       # NaN fails; inf fails (thr < FLT_MAX)
                    seg.append((t, D))
            out.append(seg)
    return out


def weight_definition(seg_dist, j, weights, metric):
    one, zero = np.float32(1.0), np.float32(0.0)
    if weights == UNIFORM:
        return one
    any_zero = False
    for dd in seg_dist:
        if dd == zero:
            any_zero = True
    if any_zero:
        return one if seg_dist[j] == zero else zero
    if weights == INV_DIST and metric == EUCLIDEAN:
        return np.float32(one / np.float32(np.sqrt(np.float32(seg_dist[j]))))
    return np.float32(one / np.float32(seg_dist[j]))


def vote_definition(seg, labels, C, weights, metric, outlier):
    """(pred, [S_c]) of one segment [(t, D)]."""
    S = [np.float32(0.0)] * C
    if not seg:
        return outlier, S
    dist = [dd for _, dd in seg]
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        for j, (t, _) in enumerate(seg):
            S[labels[t]] = np.float32(S[labels[t]] + weight_definition(dist, j, weights, metric))
    best = 0
    for c in range(1, C):
        if S[c] > S[best]:
            best = c
    return best, S


def regress_definition(seg, targets, weights, metric):
    if not seg:
        return np.float32(np.nan)
    dist = [dd for _, dd in seg]
    N, Dn = np.float64(0.0), np.float64(0.0)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        for j, (t, _) in enumerate(seg):
            w = np.float64(weight_definition(dist, j, weights, metric))
            N = N + w * np.float64(np.float32(targets[t]))
            Dn = Dn + w
        return np.float32(N / Dn)


# ---------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------
RADIUS_SYMBOLS = ("knn_radius_count_device", "knn_radius_fill_device", "knn_radius_vote_device",
                  "knn_radius_regress_device")


def test_radius_symbols_and_bindings(knn):
    with open(os.path.join(REPO, "include", "knn_amd.h")) as f:
        src = f.read()
    declared = set(re.findall(r"\b(knn_[a-z_0-9]+)\s*\(", src))
    assert "Radius neighbours" in src
    assert re.search(r"ascending\s+train\s+index", src, re.I)      # the rules text fixes the list order
    assert "NOT distance-sorted" in src
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG_DIR, "libknn_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    lib = knn.load_library()
    for s in RADIUS_SYMBOLS:
        assert s in declared, s
        assert re.search(rf"\bT {s}$", out, re.M), s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.knn_version() == 3
    for m in ("radius_count_device", "radius_neighbors_device", "radius_predict_device", "radius_regress_device",
              "radius_loo_device", "radius_vote_device", "radius_regress_vote_device"):
        assert callable(getattr(knn.Context, m)), m
    # NULL context: no crash, KNN_EINVAL
    assert lib.knn_radius_count_device(None, None, None, 1.0, 1, -1, -1, None, None, None, None, None, None,
                                       None) == knn.KNN_EINVAL
    assert lib.knn_radius_fill_device(None, None, None, 1.0, -1, None, None, None, None) == knn.KNN_EINVAL
    assert lib.knn_radius_vote_device(None, 0, 0, None, None, None, None, 1, 0, -1, None, None, None, None,
                                      None) == knn.KNN_EINVAL
    assert lib.knn_radius_regress_device(None, 0, 0, None, None, None, None, 0, None, None) == knn.KNN_EINVAL


def test_radius_argument_means_squared_under_euclidean(knn):
    """radius= is squared in binary32 under the Euclidean metric and passed on under the others;
    exactly one of radius= / threshold= is given.  (Context._threshold reads only self.metric.)"""
    class Fake:
        metric = "euclidean"
    r = 0.1
    assert knn.Context._threshold(Fake, r, None) == float(np.float32(r) * np.float32(r))
    assert knn.Context._threshold(Fake, None, 0.25) == 0.25
    Fake.metric = "manhattan"
    assert knn.Context._threshold(Fake, r, None) == float(np.float32(r))
    for bad in ((None, None), (1.0, 1.0), (-1.0, None)):
        with pytest.raises(knn.KnnError) as e:
            knn.Context._threshold(Fake, *bad)
        assert e.value.status == knn.KNN_EINVAL


def _case_thresholds(tr, te, metric):
    """0, every finite distance of the case (D == thr exactly), the midpoints and values just
    outside, and a subnormal."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        vals = sorted({float(distance_definition(q, t, metric)) for q in te for t in tr
                       if distance_definition(q, t, metric) < FLT_MAX})
    thr = {0.0, float(np.float32(2.0 ** -140)), float(np.float32(3.0e38))}
    for v in vals:
        v32 = np.float32(v)
        thr.update({v, float(np.nextafter(v32, np.float32(0))) if v > 0 else 0.0,
                    float(np.nextafter(v32, np.float32(np.inf)))})
    return sorted(t for t in thr if 0 <= t < FLT_MAX)


def _b32(x):
    """One float32 scalar's bits."""
    return int(np.array(x, np.float32).reshape(1).view(np.uint32)[0])


def _compare(tr, te, thr, metric, self_base, labels, targets, C=3):
    count, off, idx, dist, cc = radius_reference(tr, te, thr, metric, self_base, labels, C)
    want = radius_definition(tr, te, thr, metric, self_base)
    assert list(count) == [len(s) for s in want]
    assert off[0] == 0 and list(np.diff(off)) == [len(s) for s in want]
    assert list(idx) == [t for s in want for t, _ in s]
    assert list(bits(dist)) == [_b32(dd) for s in want for _, dd in s]
    for q, s in enumerate(want):
        assert list(cc[q]) == [sum(1 for t, _ in s if labels[t] == c) for c in range(C)]
    assert list(count_vote_reference(cc, -7)) == [vote_definition(s, labels, C, UNIFORM, metric, -7)[0] for s in want]
    for w in (UNIFORM, INV_DIST, INV_SQDIST):
        if w == INV_SQDIST and metric != EUCLIDEAN:
            continue
        pred, sc = radius_vote_reference(off, idx, dist, labels, C, w, metric, -7)
        reg = radius_regress_reference(off, idx, dist, targets, w, metric)
        for q, s in enumerate(want):
            dp, dS = vote_definition(s, labels, C, w, metric, -7)
            assert pred[q] == dp, (thr, metric, w, q)
            assert list(bits(sc[q])) == [_b32(x) for x in dS], (thr, metric, w, q)
            dr = regress_definition(s, targets, w, metric)
            assert _b32(reg[q]) == _b32(dr) or (np.isnan(reg[q]) and np.isnan(dr)), (thr, metric, w, q)
    return count, off, idx, dist


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", sorted(TINY_CASES))
def test_restatements_equal_definitions(case, metric):
    tr, te = TINY_CASES[case]
    labels = np.arange(len(tr)) % 3
    targets = (np.arange(len(tr)) * 1.25 - 2).astype(np.float32)
    for thr in _case_thresholds(tr, te, metric):
        _compare(tr, te, thr, metric, None, labels, targets)
    for thr in _case_thresholds(tr, te, metric)[:6]:
        _compare(tr, te[:2], thr, metric, 1, labels, targets)


def test_restatement_special_values():
    """What the tiny cases are there to show, spelled out."""
    # D == thr exactly is a neighbour; the value below it is not
    tr, te = TINY_CASES["d1"]
    for metric, D in ((EUCLIDEAN, np.float32(1.75 * 1.75)), (MANHATTAN, np.float32(1.75)), (CHEBYSHEV, np.float32(1.75))):
        c_at = radius_reference(tr, te, D, metric)[0]
        c_below = radius_reference(tr, te, np.nextafter(D, np.float32(0)), metric)[0]
        assert c_at[0] == 3 and c_below[0] == 2, metric           # |0.5 - (-1.25)| = 1.75 is row 1
        # thr = 0: the two equal rows of query 0, nothing for query 1 (an empty neighbourhood)
        count, off, idx, dist, _ = radius_reference(tr, te, 0.0, metric)
        assert list(count) == [2, 0] and list(idx) == [0, 2] and not dist.any() and list(off) == [0, 2, 2]
    # a NaN feature: never a neighbour under Euclidean / Manhattan, skipped under Chebyshev
    tr, te = TINY_CASES["d5_nan"]
    big = np.float32(3.0e38)
    for metric in (EUCLIDEAN, MANHATTAN):
        idx = radius_reference(tr, te, big, metric)[2]
        count = radius_reference(tr, te, big, metric)[0]
        assert list(idx[:count[0]]) == [1, 3, 4] and count[1] == 0
    count, _, idx, dist, _ = radius_reference(tr, te, 0.0, CHEBYSHEV)
    assert list(idx[:count[0]]) == [0, 1, 2]                     # NaN differences ignored: distance 0
    assert count[1] == 1 and idx[count[0]] == 2                  # the NaN query feature meets the all-NaN row
    assert radius_reference(tr, te, big, CHEBYSHEV)[0][1] == 5
    # an overflowing L1 sum is inf: no neighbour at any threshold; its Chebyshev maximum is finite
    tr, te = TINY_CASES["d3_huge"]
    assert 0 not in radius_reference(tr, te, big, MANHATTAN)[2][:radius_reference(tr, te, big, MANHATTAN)[0][0]]
    assert 0 in radius_reference(tr, te, big, CHEBYSHEV)[2][:radius_reference(tr, te, big, CHEBYSHEV)[0][0]]
    assert radius_reference(tr, te, big, EUCLIDEAN)[0][0] == 2        # 9e76 overflows, 1 + 4 + 9 does not
    # a subnormal threshold separates subnormal distances
    tr, te = TINY_CASES["d3_subnormal"]
    sub = np.float32(2.0 ** -140)
    count, _, idx, dist, _ = radius_reference(tr, te, np.float32(6) * sub, MANHATTAN)
    assert list(idx[:count[0]]) == [1, 4] and (dist[:count[0]] > 0).all()      # L1 = 3 and 6 units
    assert (dist[:count[0]] < np.finfo(np.float32).tiny).all()
    assert radius_reference(tr, te, np.float32(5) * sub, MANHATTAN)[0][0] == 1
    # a zero distance among non-zero ones: only it weighs, under both weighted kinds, wherever it is
    off = np.array([0, 3], np.int64)
    idx = np.array([0, 1, 2], np.int32)
    dist = np.array([4.0, 0.0, 0.25], np.float32)
    labels = np.array([1, 2, 1], np.int32)
    targets = np.array([10.0, -3.0, 7.0], np.float32)
    for w in (INV_DIST, INV_SQDIST):
        pred, sc = radius_vote_reference(off, idx, dist, labels, 3, w, EUCLIDEAN, -1)
        assert pred[0] == 2 and list(sc[0]) == [0.0, 0.0, 1.0]
        assert radius_regress_reference(off, idx, dist, targets, w, EUCLIDEAN)[0] == -3.0
    pred, sc = radius_vote_reference(off, idx, dist, labels, 3, UNIFORM, EUCLIDEAN, -1)
    assert pred[0] == 1 and list(sc[0]) == [0.0, 2.0, 1.0]
    dist = np.array([4.0, 1.0, 0.25], np.float32)
    _, sc = radius_vote_reference(off, idx, dist, labels, 3, INV_DIST, EUCLIDEAN, -1)
    assert list(sc[0]) == [0.0, 2.5, 1.0]                                  # 1/2 + 1/0.5, 1/1
    _, sc = radius_vote_reference(off, idx, dist, labels, 3, INV_DIST, MANHATTAN, -1)
    assert list(sc[0]) == [0.0, 4.25, 1.0]                                 # 1/4 + 1/0.25
    # a self row with an equal copy: the copy stays, the self row goes
    tr = np.array([[1, 2], [5, 5], [1, 2], [9, 9]], np.float32)
    count, _, idx, _, _ = radius_reference(tr, tr, 0.0, EUCLIDEAN, self_base=0)
    assert list(count) == [1, 0, 1, 0] and list(idx) == [2, 0]
    # an empty segment: outlier, +0 scores, NaN
    off0 = np.array([0, 0], np.int64)
    e = np.zeros(0)
    pred, sc = radius_vote_reference(off0, e.astype(np.int32), e.astype(np.float32), labels, 3, INV_DIST, EUCLIDEAN, -7)
    assert pred[0] == -7 and not bits(sc).any()
    assert np.isnan(radius_regress_reference(off0, e.astype(np.int32), e.astype(np.float32), targets, UNIFORM, EUCLIDEAN)[0])


@pytest.fixture(scope="module")
def shape_stats(oracle):
    """Per GPU shape and metric: the thresholds and the neighbour counts at each."""
    out = {}
    for d, nt, nq, kind in RADIUS_SHAPES:
        tr, _, te = metric_set(oracle, kind, nt, nq, d)
        for metric in METRICS:
            D = metric_distances(tr, te, metric)
            thrs = radius_thresholds(D)
            out[d, nt, nq, kind, metric] = (D, thrs, [radius_members(D, t).sum(axis=1) for t in thrs])
    return out


def test_inputs_have_boundary_pairs(shape_stats):
    """(a) every non-zero threshold has at least one pair with D == thr: '<' instead of '<='
    changes a count."""
    for key, (D, thrs, _) in shape_stats.items():
        assert thrs[0] == 0 and bits(thrs[0]) == 0
        for t in thrs[1:]:
            assert np.isfinite(t) and t < FLT_MAX, (key, t)
            if t > 0:
                assert (D == t).any(), (key, t)
                with np.errstate(invalid="ignore"):
                    assert (D < t).sum() < (D <= t).sum(), (key, t)


def test_inputs_have_empty_neighbourhoods(shape_stats):
    """(b) on each "float" set with nq >= 33 at least 5 % of the queries have no neighbour at
    thr = 0, and on (11, 1000, 257) and (129, 1000, 33) at least 5 % have none at q = 0.002."""
    for (d, nt, nq, kind, metric), (_, thrs, counts) in shape_stats.items():
        if kind != "float" or nq < 33:
            continue
        empty0 = (counts[0] == 0).mean()
        empty1 = (counts[1] == 0).mean()
        print(f"d={d} nt={nt} nq={nq} {METRIC_NAMES[metric]}: empty at thr=0 {empty0:.3f}, at q=0.002 {empty1:.3f}")
        assert empty0 >= 0.05, (d, nt, nq, metric, empty0)
        if (d, nt, nq) in ((11, 1000, 257), (129, 1000, 33)):
            assert empty1 >= 0.05, (d, nt, nq, metric, empty1)


def test_inputs_have_long_lists(shape_stats):
    """(c) at nt = 4096 the q = 0.5 threshold gives some query more than 1,024 neighbours (no
    top-k list could hold them)."""
    for (d, nt, nq, kind, metric), (_, thrs, counts) in shape_stats.items():
        if nt != 4096:
            continue
        print(f"d={d} nq={nq} {kind} {METRIC_NAMES[metric]}: most neighbours at q=0.5 {counts[3].max()}")
        assert counts[3].max() > 1024, (d, nq, kind, metric, counts[3].max())
