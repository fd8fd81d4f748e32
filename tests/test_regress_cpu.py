"""CPU-side checks of k-NN regression: the new entry points are exported, and the numpy float64
restatement that the GPU tests compare bits against (regress_reference) is pinned to a second,
definitional form, to sklearn's KNeighborsRegressor (a cross-check), and to hand-built cases of
the zero rule, missing entries and an infinite weight.  No GPU is needed here.

The rules (include/knn_amd.h, "Regression"): w_j is the weighted vote's binary32 weight;
N_k = N_{k-1} + (double)w_j (double)y_j and D_k = D_{k-1} + (double)w_j in binary64, in ascending
list position; the prediction for k is (float)(N_k / D_k); a prefix that reaches a missing entry
predicts NaN from there on.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, REPO
from test_weighted_cpu import INV_DIST, INV_SQDIST, KINDS, UNIFORM, list_weights, remove_self, small_set


def fbits(x):
    """float32 array -> its uint32 bit patterns with every NaN mapped to one pattern: the tests
    compare NaN positions, not NaN payloads."""
    x = np.ascontiguousarray(x, np.float32)
    return np.where(np.isnan(x), np.uint32(0x7FC00000), x.view(np.uint32))


def regress_reference(idx, dist, targets, weights, self_base=None):
    """Host restatement of k_regress_sweep (test infrastructure).  idx / dist [nq][kin]: each
    query's neighbour list, ascending by (distance, train index), -1 = none; targets float32 per
    train row.  Returns (pred_all float32 [kmax][nq], too_few).  One step per list position, all
    queries at once, in float64: N += w * y (the product of two float32 values is exact in
    float64), D += w, pred = float32(N / D).  A prefix that reaches a missing entry predicts NaN
    from there on and sets too_few."""
    idx = np.asarray(idx)
    targets = np.asarray(targets)
    assert targets.dtype == np.float32
    dist = np.zeros(idx.shape, np.float32) if dist is None else np.ascontiguousarray(dist, np.float32)
    if self_base is not None:
        idx, dist = remove_self(idx, dist, self_base)
    nq, kmax = idx.shape
    w = list_weights(idx, dist, weights).astype(np.float64)
    y = targets[np.maximum(idx, 0)].astype(np.float64)
    N = np.zeros(nq, np.float64)
    D = np.zeros(nq, np.float64)
    pred = np.full((kmax, nq), np.nan, np.float32)
    alive = np.ones(nq, bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(kmax):
            alive &= idx[:, j] >= 0
            N = N + w[:, j] * y[:, j]
            D = D + w[:, j]
            pred[j, alive] = (N[alive] / D[alive]).astype(np.float32)
    return pred, bool((~alive).any())


def regress_definition(idx, dist, targets, weights, self_base=None):
    """The definition, with nothing kept between prefixes: for every query and every k both sums
    are recomputed from scratch in list order with Python floats (binary64), then one division."""
    idx = np.asarray(idx)
    dist = np.ascontiguousarray(dist, np.float32)
    if self_base is not None:
        idx, dist = remove_self(idx, dist, self_base)
    nq, kmax = idx.shape
    pred = np.full((kmax, nq), np.nan, np.float32)
    too_few = False
    for q in range(nq):
        zero_mode = weights != UNIFORM and idx[q, 0] >= 0 and dist[q, 0] == 0
        for k in range(1, kmax + 1):
            if (idx[q, :k] < 0).any():
                too_few = True
                break
            N, D = 0.0, 0.0
            for j in range(k):
                d = np.float32(dist[q, j])
                if weights == UNIFORM:
                    wj = np.float32(1.0)
                elif zero_mode:
                    wj = np.float32(1.0 if d == 0 else 0.0)
                else:
                    with np.errstate(divide="ignore", over="ignore"):
                        wj = np.float32(1.0) / (np.sqrt(d) if weights == INV_DIST else d)
                assert wj.dtype == np.float32
                with np.errstate(invalid="ignore"):
                    N = N + float(wj) * float(targets[idx[q, j]])
                    D = D + float(wj)
            with np.errstate(invalid="ignore"):
                pred[k - 1, q] = np.float32(np.float64(N) / np.float64(D))
    return pred, too_few


def error_sums(pred_all, query_targets):
    """(sse, sae) float64 [kmax] of float32 predictions by math.fsum: the exactly rounded sums the
    kernel's fixed-order binary64 sums are bounded against (nq * 2^-52 relative)."""
    import math
    qt = np.asarray(query_targets, np.float32).astype(np.float64)
    sse, sae = [], []
    for row in np.asarray(pred_all, np.float32).astype(np.float64):
        e = row - qt
        if np.isnan(e).any():
            sse.append(np.nan)
            sae.append(np.nan)
        else:
            sse.append(math.fsum((e * e).tolist()))
            sae.append(math.fsum(np.abs(e).tolist()))
    return np.array(sse), np.array(sae)


def _targets(n, seed=31):
    return (np.random.default_rng(seed).standard_normal(n) * 100).astype(np.float32)


def test_regress_symbols_in_header_and_library(knn):
    with open(os.path.join(REPO, "include", "knn_amd.h")) as f:
        declared = set(re.findall(r"\b(knn_[a-z_0-9]+)\s*\(", f.read()))
    lib = knn.load_library()
    for s in ("knn_regress_vote_device", "knn_regress_sweep_device", "knn_regress_device", "knn_regress_sweep",
              "knn_arff_copy_targets"):
        assert s in declared, s
        assert hasattr(lib, s), s
    assert lib.knn_version() == 3
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(PKG_DIR, "libknn_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    for sig in ("KNN_regress_sweep(ArffData*, ArffData*, int, int, double*, double*)",
                "KNN_regress_sweep_loo(ArffData*, int, int, double*, double*)"):
        assert sig in out, sig
    for m in ("regress_sweep_device", "regress_loo_device", "regress_device", "regress_vote_device", "regress_sweep"):
        assert callable(getattr(knn.Context, m)), m
    assert callable(knn.best_k_error) and callable(knn.read_arff_targets)


@pytest.mark.parametrize("weights", KINDS)
def test_restatement_matches_definition(oracle, weights):
    tr, tl, C, te = small_set(oracle)
    y = _targets(len(tr))
    bad, _, dist, idx = oracle.knn(tr, tl, te, 8, C)
    assert bad == 0
    got = regress_reference(idx, dist, y, weights)
    want = regress_definition(idx, dist, y, weights)
    assert np.array_equal(fbits(got[0]), fbits(want[0])) and not np.isnan(got[0]).any()
    assert not got[1] and not want[1]
    # leave-one-out: kin = 9, the self row removed first
    bad, _, dist, idx = oracle.knn(tr, tl, tr, 9, C)
    assert bad == 0
    got = regress_reference(idx, dist, y, weights, self_base=0)
    want = regress_definition(idx, dist, y, weights, self_base=0)
    assert got[0].shape == (8, 300)
    assert np.array_equal(fbits(got[0]), fbits(want[0])) and not got[1] and not want[1]
    if weights != UNIFORM:
        # the case is no trivial one: zero rule rows, and rows the weights move
        _, d1 = remove_self(idx, dist, 0)
        assert (d1[:, 0] == 0).any() and (d1[:, 0] > 0).any()
        uni = regress_reference(idx, dist, y, UNIFORM, self_base=0)[0]
        assert (fbits(uni) != fbits(got[0])).any()


def test_uniform_is_the_mean():
    idx = np.array([[2, 0, 1]], np.int32)
    y = np.array([1.5, -4.0, 10.0], np.float32)
    pred, too_few = regress_reference(idx, None, y, UNIFORM)
    assert not too_few and pred[:, 0].tolist() == [10.0, 5.75, 2.5]


def test_against_sklearn():
    """A cross-check, not the yardstick.  Tolerances are derived, not tuned: uniform 2^-22 (both are
    float64 means of the same positive numbers, then one fp32 rounding); distance (d + 3) 2^-23 --
    the fp32 squared distance carries about (d + 1) 2^-24 relative error, half of it survives the
    square root, the weighted mean of positive targets moves by at most twice the weights'
    relative error, and one fp32 rounding is added.  Measured: 5.7e-8 (uniform), 7.1e-8."""
    neighbors = pytest.importorskip("sklearn.neighbors")
    rng = np.random.default_rng(3)
    d = 8
    tr = rng.standard_normal((2048, d)).astype(np.float32)
    te = rng.standard_normal((257, d)).astype(np.float32)
    y = rng.uniform(1, 101, 2048).astype(np.float32)
    acc = np.zeros((257, 2048), np.float32)
    for i in range(d):
        df = te[:, i:i + 1] - tr[None, :, i]
        acc = acc + df * df
    assert acc.dtype == np.float32
    order = np.lexsort((np.broadcast_to(np.arange(2048), acc.shape), acc), axis=1)[:, :64]
    idx = order.astype(np.int32)
    dist = np.take_along_axis(acc, order, axis=1)
    for weights, name, tol in ((UNIFORM, "uniform", 2.0 ** -22), (INV_DIST, "distance", (d + 3) * 2.0 ** -23)):
        pred, too_few = regress_reference(idx, dist, y, weights)
        assert not too_few
        for k in (1, 5, 64):
            m = neighbors.KNeighborsRegressor(n_neighbors=k, weights=name, algorithm="brute")
            m.fit(tr.astype(np.float64), y.astype(np.float64))
            want = m.predict(te.astype(np.float64))
            rel = np.abs(pred[k - 1].astype(np.float64) - want) / np.abs(want)
            print(f"{name} k={k}: largest relative difference {rel.max():.3g} (bound {tol:.3g})")
            assert rel.max() <= tol, (name, k, rel.max())


@pytest.mark.parametrize("weights", [INV_DIST, INV_SQDIST])
def test_zero_rule(weights):
    """Duplicates with different targets: the prediction freezes at the zero entries' mean."""
    y = np.array([10.0, 20.0, 60.0, -5.0, 7.25], np.float32)
    idx = np.array([[1, 2, 0, 3, 4], [4, 3, 2, 1, 0]], np.int32)
    dist = np.array([[0.0, 0.0, 0.0, 0.5, 2.0], [0.25, 0.5, 1.0, 2.0, 4.0]], np.float32)
    pred, too_few = regress_reference(idx, dist, y, weights)
    assert not too_few
    assert pred[:, 0].tolist() == [20.0, 40.0, 30.0, 30.0, 30.0]
    # no zero distance: ordinary weights, every entry moves the mean
    assert len(set(pred[:, 1].tolist())) == 5 and pred[0, 1] == 7.25
    want, _ = regress_definition(idx, dist, y, weights)
    assert np.array_equal(fbits(pred), fbits(want))


@pytest.mark.parametrize("weights", KINDS)
def test_missing_entries(weights):
    y = np.array([3.0, 1.0, -2.0], np.float32)
    idx = np.array([[0, 1, -1, -1], [2, 1, 0, 0]], np.int32)
    dist = np.array([[0.5, 2.0, 3e38, 3e38], [0.25, 0.25, 4.0, 5.0]], np.float32)
    pred, too_few = regress_reference(idx, dist, y, weights)
    assert too_few
    assert not np.isnan(pred[:2, 0]).any() and np.isnan(pred[2:, 0]).all()
    assert pred[0, 0] == 3.0 and not np.isnan(pred[:, 1]).any()
    want, few = regress_definition(idx, dist, y, weights)
    assert few and np.array_equal(fbits(pred), fbits(want))


def test_infinite_weight_gives_nan():
    y = np.array([1.0, 2.0, 3.0], np.float32)
    idx = np.array([[2, 1, 0]], np.int32)
    dist = np.array([[1e-40, 1.0, 2.0]], np.float32)
    assert dist[0, 0] > 0                      # a subnormal, kept: 1 / d overflows to +inf
    pred, too_few = regress_reference(idx, dist, y, INV_SQDIST)
    assert not too_few and np.isnan(pred).all()        # inf / inf
    want, _ = regress_definition(idx, dist, y, INV_SQDIST)
    assert np.array_equal(fbits(pred), fbits(want))
    # 1 / sqrt(1e-40) is finite: an ordinary, heavily weighted entry
    pred, _ = regress_reference(idx, dist, y, INV_DIST)
    assert np.isfinite(pred).all() and pred[0, 0] == 3.0


def test_best_k_error(knn):
    assert knn.best_k_error(np.array([4.0, 2.0, 2.0, 3.0])) == 2           # the tie goes to the smallest k
    assert knn.best_k_error(np.array([np.nan, 5.0, 1.0, np.nan])) == 3     # NaN is ignored
    assert knn.best_k_error(np.array([np.nan, np.inf])) == 2
    assert knn.best_k_error([7.0]) == 1
    with pytest.raises(knn.KnnError):
        knn.best_k_error(np.array([np.nan, np.nan]))


def test_arff_targets_keep_fractions_and_signs(knn, tmp_path):
    p = tmp_path / "t.arff"
    p.write_text("@RELATION t\n@ATTRIBUTE a NUMERIC\n@ATTRIBUTE b NUMERIC\n@ATTRIBUTE y NUMERIC\n@DATA\n"
                 "1,2,-3.75\n0.5,-1,0.125\n4,4,7\n")
    feat, y = knn.read_arff_targets(str(p))
    assert y.dtype == np.float32 and y.tolist() == [-3.75, 0.125, 7.0]
    assert feat.tolist() == [[1.0, 2.0], [0.5, -1.0], [4.0, 4.0]]
    f2, lab, _ = knn.read_arff(str(p))                   # read_arff is untouched: the truncated int
    assert np.array_equal(f2, feat) and lab.tolist() == [-3, 0, 7]
