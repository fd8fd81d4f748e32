"""CPU-side checks of the radius sweep (include/knn_amd.h "Radius sweep"): the entry points are
declared, exported and bound; the numpy restatements the GPU tests compare against
(radius_sweep_reference, radius_vote_sweep_reference) are pinned to the scalar definitions of
test_radius_cpu.py on tiny cases and to the single-threshold restatements; best_radius on ties; the
GPU tests' sets tell the rows of a sweep apart; and the share of pairs the MFMA form would have to
evaluate exactly for the whole threshold list (the band-model union).  No GPU is needed here.

The rules: thr[0 .. R - 1] is non-decreasing; train row t is in q's neighbourhood at index r iff
D(q, t) <= thr[r]; neighbourhoods are nested, so a pair has one bucket -- the smallest r with
D <= thr[r], or R -- and every output is a prefix sum over buckets.  Row r equals the
single-threshold call at thr[r] bit for bit.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, REPO
from test_metric_cpu import EUCLIDEAN, MANHATTAN, TINY_CASES, bits, metric_distances, metric_set
from test_radius_cpu import (INV_DIST, INV_SQDIST, METRICS, UNIFORM, _b32, count_vote_reference, radius_definition,
                             radius_reference, radius_thresholds, radius_vote_reference, vote_definition)
from test_radius_mfma_cpu import MFMA_SHAPES, band_model

# (d, nt, nq, kind) of the GPU tests' direct-form case: one tile plus one row with one query; 3
# trailing features and partial query blocks; more than one chunk with 1 trailing feature; more
# than DT_MAX_DC = 128 features, neighbourhoods above 1,024
SWEEP_SHAPES = [(1, 65, 1, "float"), (11, 1000, 257, "float"), (129, 1000, 33, "float"), (260, 4096, 9, "float")]
SWEEP_MFMA_SHAPES = MFMA_SHAPES + [(128, 4096, 257, "float")]
UNION_CAP = 0.10


# ---------------------------------------------------------------------------------------
# restatements (numpy) -- what the GPU tests compare against
# ---------------------------------------------------------------------------------------
def sweep_buckets(D, thr, self_base=None):
    """int [nq][nt]: the number of thresholds a pair is NOT within (R: in no neighbourhood; a NaN D
    is within none).  With a non-decreasing list that is the smallest r with D <= thr[r]."""
    thr = np.asarray(thr, np.float32)
    assert thr.ndim == 1 and (np.diff(thr) >= 0).all()
    with np.errstate(invalid="ignore"):
        b = (~(D[:, :, None] <= thr[None, None, :])).sum(axis=2)
    if self_base is not None:
        q = np.arange(len(D))
        b[q, self_base + q] = len(thr)
    return b


def radius_sweep_reference(D, thr, self_base=None, labels=None, C=None, outlier=-1, qlabels=None):
    """(count int32 [R][nq], class_counts int32 [R][nq][C] or None, pred int32 [R][nq] or None,
    correct int64 [R] or None, outliers int64 [R]) from the bucket histograms and their prefix
    sums -- not from R membership tests."""
    R, nq = len(thr), len(D)
    b = sweep_buckets(D, thr, self_base)
    hist = np.zeros((nq, R + 1), np.int64)
    q, t = np.nonzero(b < R + 1)                     # every pair
    np.add.at(hist, (q, b[q, t]), 1)
    count = np.cumsum(hist[:, :R], axis=1).T.astype(np.int32)
    outliers = (count == 0).sum(axis=1).astype(np.int64)
    if labels is None:
        return count, None, None, None, outliers
    chist = np.zeros((nq, R + 1, C), np.int64)
    np.add.at(chist, (q, b[q, t], np.asarray(labels)[t]), 1)
    cc = np.cumsum(chist[:, :R], axis=1).transpose(1, 0, 2).astype(np.int32)
    pred = np.where(count > 0, cc.argmax(axis=2), outlier).astype(np.int32)       # argmax: the first maximum
    correct = None if qlabels is None else (pred == np.asarray(qlabels)[None, :]).sum(axis=1).astype(np.int64)
    return count, cc, pred, correct, outliers


def filter_lists(offsets, idx, dist, thr):
    """The CSR sub-lists of the entries with dist <= thr, in list order."""
    with np.errstate(invalid="ignore"):
        keep = dist <= np.float32(thr)
    seg = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    off = np.zeros(len(offsets), np.int64)
    off[1:] = np.cumsum(np.bincount(seg[keep], minlength=len(offsets) - 1))
    return off, idx[keep], dist[keep]


def radius_vote_sweep_reference(offsets, idx, dist, labels, C, weights, metric, outlier, thr):
    """(pred int32 [R][nq], scores float32 [R][nq][C]): per r, radius_vote_reference on the sub-list
    of the entries with dist <= thr[r]."""
    out = [radius_vote_reference(*filter_lists(offsets, idx, dist, t), labels, C, weights, metric, outlier)
           for t in thr]
    return np.stack([p for p, _ in out]), np.stack([s for _, s in out])


# ---------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------
SWEEP_SYMBOLS = ("knn_radius_sweep_count_device", "knn_radius_vote_sweep_device", "knn_radius_sweep_max_queries")


def test_sweep_symbols_and_bindings(knn):
    with open(os.path.join(REPO, "include", "knn_amd.h")) as f:
        src = f.read()
    declared = set(re.findall(r"\b(knn_[a-z_0-9]+)\s*\(", src))
    assert "Radius sweep" in src
    assert re.search(r"ADDED\s+TO,\s+NOT\s+ZEROED", src)            # the header says who zeroes correct / outliers
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG_DIR, "libknn_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    lib = knn.load_library()
    for s in SWEEP_SYMBOLS:
        assert s in declared, s
        assert re.search(rf"\bT {s}$", out, re.M), s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.knn_version() == 3
    for m in ("radius_sweep_device", "radius_sweep_loo_device", "radius_vote_sweep_device",
              "radius_sweep_predict_device"):
        assert callable(getattr(knn.Context, m)), m
    assert callable(knn.best_radius)
    # NULL context: no crash, KNN_EINVAL
    assert lib.knn_radius_sweep_count_device(None, None, None, None, 1, 1, -1, -1, None, 0, None, None, None, None,
                                             None, None) == knn.KNN_EINVAL
    assert lib.knn_radius_vote_sweep_device(None, 0, 0, None, None, None, None, 1, 0, None, 1, -1, None, 0, None,
                                            None, None, None) == knn.KNN_EINVAL
    assert lib.knn_radius_sweep_max_queries(None, 4, 10) == 0


def test_radii_argument(knn):
    """radii= squares in binary32 under the Euclidean metric and passes on under the others;
    thresholds= is taken as it is; exactly one is given.  (Context._thresholds reads self.metric.)"""
    class Fake:
        metric = "euclidean"
    r = [0.1, 0.5, 0.5]
    got = knn.Context._thresholds(Fake, r, None)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(np.float32(r) * np.float32(r)))
    assert np.array_equal(knn.Context._thresholds(Fake, None, [0.25, 1.0]), np.float32([0.25, 1.0]))
    Fake.metric = "manhattan"
    assert np.array_equal(bits(knn.Context._thresholds(Fake, r, None)), bits(np.float32(r)))
    for bad in ((None, None), ([1.0], [1.0]), ([-1.0], None)):
        with pytest.raises(knn.KnnError) as e:
            knn.Context._thresholds(Fake, *bad)
        assert e.value.status == knn.KNN_EINVAL


def test_best_radius(knn):
    assert knn.best_radius([3, 7, 7, 2]) == 1                       # ties: the smallest index
    assert knn.best_radius(np.array([5, 5, 5], np.int64)) == 0
    assert knn.best_radius([0, 0, 1]) == 2
    assert knn.best_radius([4]) == 0
    for bad in ([], [[1, 2]]):
        with pytest.raises(knn.KnnError) as e:
            knn.best_radius(bad)
        assert e.value.status == knn.KNN_EINVAL


def _definition_rows(tr, te, thr, metric, self_base, labels, C, outlier):
    """Per r, from the scalar definitions: counts, class counts, the uniform vote."""
    rows = []
    for t in thr:
        segs = radius_definition(tr, te, t, metric, self_base)
        rows.append(([len(s) for s in segs],
                     [[sum(1 for j, _ in s if labels[j] == c) for c in range(C)] for s in segs],
                     [vote_definition(s, labels, C, UNIFORM, metric, outlier)[0] for s in segs]))
    return rows


def _tiny_lists(tr, te, metric):
    """A few threshold lists of a tiny case: every distinct finite distance (D == thr[r] exactly),
    equal adjacent thresholds, [0] alone, a list under which every neighbourhood is empty."""
    D = metric_distances(tr, te, metric)
    fin = np.unique(D[np.isfinite(D)])
    lists = [np.float32([0.0]), fin[:32].astype(np.float32), np.float32([3.0e38])]
    if len(fin) > 1:
        lists.append(np.float32([fin[0], fin[0], fin[1], fin[1], fin[-1]]))
        if fin[0] > 0:
            below = np.nextafter(fin[0], np.float32(0))
            lists.append(np.float32([0.0, below / 2, below]))       # empty at every r
    return D, lists


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", sorted(TINY_CASES))
def test_sweep_restatement_equals_definitions(case, metric):
    tr, te = TINY_CASES[case]
    C = 3
    labels = np.arange(len(tr)) % C
    ql = np.arange(len(te)) % C
    D, lists = _tiny_lists(tr, te, metric)
    for thr in lists:
        for self_base, q_te, q_D, q_ql in ((None, te, D, ql), (1, te[:2], D[:2], ql[:2])):
            count, cc, pred, correct, outliers = radius_sweep_reference(q_D, thr, self_base, labels, C, -7, q_ql)
            for r, (dc, dcc, dp) in enumerate(_definition_rows(tr, q_te, thr, metric, self_base, labels, C, -7)):
                assert list(count[r]) == dc, (case, metric, r)
                assert cc[r].tolist() == dcc, (case, metric, r)
                assert list(pred[r]) == dp, (case, metric, r)
                assert correct[r] == sum(int(p == l) for p, l in zip(dp, q_ql))
                assert outliers[r] == sum(1 for n in dc if n == 0)
                # row r is the single-threshold restatement at thr[r]
                rc, _, _, _, rcc = radius_reference(tr, q_te, thr[r], metric, self_base, labels, C, D=q_D)
                assert np.array_equal(count[r], rc) and np.array_equal(cc[r], rcc)
                assert np.array_equal(pred[r], count_vote_reference(rcc, -7))


def test_sweep_special_values():
    """What the tiny cases are there to show, spelled out."""
    tr, te = TINY_CASES["d1"]
    # D == thr[r] exactly is in bucket r; equal adjacent thresholds give equal rows; [0] alone
    for metric, Dv in ((EUCLIDEAN, np.float32(1.75 * 1.75)), (MANHATTAN, np.float32(1.75))):
        D = metric_distances(tr, te, metric)
        thr = np.float32([0.0, np.nextafter(Dv, np.float32(0)), Dv, Dv])
        count = radius_sweep_reference(D, thr)[0]
        assert list(count[:, 0]) == [2, 2, 3, 3], metric
        assert sweep_buckets(D, thr)[0, 1] == 2                     # |0.5 - (-1.25)| = 1.75 is row 1
        count, _, _, _, outliers = radius_sweep_reference(D, np.float32([0.0]))
        assert count.shape == (1, 2) and list(count[0]) == [2, 0] and list(outliers) == [1]
    # an empty neighbourhood at every r: the outlier label in every row
    D = metric_distances(tr, te, EUCLIDEAN)
    labels = np.arange(len(tr)) % 3
    count, cc, pred, correct, outliers = radius_sweep_reference(D[1:], np.float32([0.0, 1e-30, 1e-20]), None, labels,
                                                                3, -7, [0])
    assert not count.any() and not cc.any() and (pred == -7).all() and not correct.any() and list(outliers) == [1] * 3
    # a NaN feature is in no bucket under Euclidean: bucket R at every list
    tr, te = TINY_CASES["d5_nan"]
    D = metric_distances(tr, te, EUCLIDEAN)
    b = sweep_buckets(D, np.float32([0.0, 1.0, 3.0e38]))
    assert (b[np.isnan(D)] == 3).all() and np.isnan(D).any()
    # a zero distance among non-zero ones that enters at r = 0 while the rest enter later: the zero
    # rule holds in every sub-list that has the entry, which is all of them
    off = np.array([0, 3, 5], np.int64)
    idx = np.array([0, 1, 2, 0, 2], np.int32)
    dist = np.array([4.0, 0.0, 0.25, 1.0, 0.5], np.float32)
    labels = np.array([1, 2, 1], np.int32)
    thr = np.float32([0.0, 0.25, 0.5, 4.0])
    for w in (INV_DIST, INV_SQDIST):
        pred, sc = radius_vote_sweep_reference(off, idx, dist, labels, 3, w, EUCLIDEAN, -1, thr)
        assert list(pred[:, 0]) == [2, 2, 2, 2] and all(list(sc[r, 0]) == [0.0, 0.0, 1.0] for r in range(4))
    pred, sc = radius_vote_sweep_reference(off, idx, dist, labels, 3, UNIFORM, EUCLIDEAN, -1, thr)
    assert list(pred[:, 0]) == [2, 1, 1, 1] and list(sc[3, 0]) == [0.0, 2.0, 1.0] and list(sc[1, 0]) == [0.0, 1.0, 1.0]
    # query 1 has no zero distance and is empty at r = 0 and r = 1: outlier and a +0 row there
    pred, sc = radius_vote_sweep_reference(off, idx, dist, labels, 3, INV_DIST, MANHATTAN, -1, thr)
    assert list(pred[:, 1]) == [-1, -1, 1, 1] and not bits(sc[:2, 1]).any()
    assert list(sc[2, 1]) == [0.0, 2.0, 0.0] and list(sc[3, 1]) == [0.0, 3.0, 0.0]      # 1/0.5, then 1/1 + 1/0.5
    # a zero distance that is NOT in the sub-list does not switch the rule on: thr below it cannot
    # happen (0 is the least distance), so the rule of a sub-list is the rule of its own entries
    d2 = np.array([4.0, 1.0, 0.25], np.float32)
    _, sc = radius_vote_sweep_reference(off[:2], idx[:3], d2, labels, 3, INV_DIST, EUCLIDEAN, -1, np.float32([0.25, 4.0]))
    assert list(sc[0, 0]) == [0.0, 2.0, 0.0] and list(sc[1, 0]) == [0.0, 2.5, 1.0]


@pytest.mark.parametrize("metric", METRICS)
def test_vote_sweep_restatement_equals_definitions(metric):
    """Row r of the vote sweep is the scalar vote definition on the entries with D <= thr[r]."""
    tr, te = TINY_CASES["d1"]
    C = 3
    labels = np.arange(len(tr)) % C
    D, lists = _tiny_lists(tr, te, metric)
    top = np.float32(3.0e38)
    _, off, idx, dist, _ = radius_reference(tr, te, top, metric, D=D)
    for thr in lists:
        for w in (UNIFORM, INV_DIST, INV_SQDIST):
            if w == INV_SQDIST and metric != EUCLIDEAN:
                continue
            pred, sc = radius_vote_sweep_reference(off, idx, dist, labels, C, w, metric, -7, thr)
            for r, t in enumerate(thr):
                for q, seg in enumerate(radius_definition(tr, te, t, metric)):
                    dp, dS = vote_definition(seg, labels, C, w, metric, -7)
                    assert pred[r, q] == dp, (metric, w, r, q)
                    assert list(bits(sc[r, q])) == [_b32(x) for x in dS], (metric, w, r, q)


@pytest.fixture(scope="module")
def sweep_sets(oracle):
    out = {}
    for d, nt, nq, kind in SWEEP_SHAPES + SWEEP_MFMA_SHAPES:
        tr, tl, te = metric_set(oracle, kind, nt, nq, d)
        for metric in METRICS if (d, nt, nq, kind) in SWEEP_SHAPES else (EUCLIDEAN,):
            D = metric_distances(tr, te, metric)
            out[d, nt, nq, kind, metric] = (tl, D, np.float32(radius_thresholds(D)))
    return out


def test_inputs_discriminate(sweep_sets):
    """On the GPU tests' sets the rows of a sweep differ: consecutive rows of count differ for at
    least one query (a kernel that puts a pair into a neighbouring bucket changes a row), and pred
    differs between at least two rows (a kernel that votes every r from one row is caught).  On the
    "grid" sets, whose rows have copies, the 0.002 quantile of the distances is 0 like thr[0]: two
    equal thresholds, whose rows are equal by the rules -- there the equality is what is asserted,
    and every "float" set has four distinct thresholds."""
    for key, (tl, D, thr) in sweep_sets.items():
        assert len(thr) == 4 and thr[0] == 0 and (np.diff(thr) >= 0).all(), key
        assert (np.diff(thr) > 0).all() or key[3] == "grid", key
        assert (np.diff(thr) > 0).sum() >= 2, key
        count, _, pred, _, _ = radius_sweep_reference(D, thr, None, tl, 10, -7)
        for r in range(3):
            assert (count[r] != count[r + 1]).any() == (thr[r] < thr[r + 1]), (key, r)
        assert any((pred[r] != pred[r + 1]).any() for r in range(3)), key


@pytest.mark.parametrize("d,nt,nq,kind", [s for s in SWEEP_MFMA_SHAPES if s[3] == "float"])
def test_band_union(oracle, d, nt, nq, kind):
    """The pairs an MFMA-filtered sweep would have to evaluate exactly: those with ANY threshold
    inside [L, U).  The union bound from the single-threshold shares (3.9 % at the 0.5 quantile of
    d = 256, under 1 % at each of the other three) is at most 6.9 %; the cap is 10 %."""
    tr, _, te = metric_set(oracle, kind, nt, nq, d)
    D = metric_distances(tr, te, EUCLIDEAN)
    thr = radius_thresholds(D)
    L, U = band_model(tr, te)
    any_in = np.zeros(D.shape, bool)
    for t in thr:
        any_in |= (L <= float(t)) & ~(U <= float(t))
    share = any_in.mean()
    print(f"d={d} nt={nt} nq={nq} {kind}: union band {100 * share:.3f} % of the pairs")
    assert share <= UNION_CAP, (d, nt, nq, share)
