"""CPU-side checks of the weighted vote: the new entry points are exported, and the numpy
float32 restatement that the GPU tests compare bits against (weighted_reference) is pinned to a
second, definitional form, to the uniform sweep's restatement, to the reference's golden
fixtures, and to hand-built cases of the zero rule, the inf tie and missing entries.  No GPU is
needed here.

The rules (include/knn_amd.h, "Weighted vote"): w_j = 1, 1.0f / sqrtf(d_j) or 1.0f / d_j in IEEE
binary32; when the first entry left after self-removal has d == 0 the weighted kinds give 1 to
every d == 0 entry and 0 to the rest; S_c(k) = the fp32 sum of w_j over j < k with label_j == c
in ascending list position; the prediction for k is the argmax of S_c(k), ties to the smallest
label.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA, KS, PKG_DIR, REPO, golden_pred
from test_sweep_cpu import loo_set_300, sweep_reference

UNIFORM, INV_DIST, INV_SQDIST = 0, 1, 2
KINDS = (UNIFORM, INV_DIST, INV_SQDIST)


def bits(x):
    """float32 array -> its uint32 bit patterns (what the tests compare)."""
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def remove_self(idx, dist, self_base):
    """The lists after self-removal: the entry equal to self_base + q is deleted from row q, and
    when none equals it the last entry is (k_vote_sweep's rule)."""
    nq, kin = idx.shape
    oi = np.empty((nq, kin - 1), idx.dtype)
    od = np.empty((nq, kin - 1), np.float32)
    for q in range(nq):
        hit = np.nonzero(idx[q] == self_base + q)[0]
        at = hit[0] if len(hit) else kin - 1
        oi[q] = np.delete(idx[q], at)
        od[q] = np.delete(dist[q], at)
    return oi, od


def list_weights(idx, dist, weights):
    """float32 [nq][kmax] weights of lists after self-removal (missing entries: 0)."""
    d = np.ascontiguousarray(dist, np.float32)
    one = np.float32(1.0)
    if weights == UNIFORM:
        w = np.ones(d.shape, np.float32)
    else:
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            w = one / np.sqrt(d) if weights == INV_DIST else one / d
        zero_mode = (idx[:, 0] >= 0) & (d[:, 0] == 0)
        w = np.where(zero_mode[:, None], (d == 0).astype(np.float32), w)
    w = np.where(idx >= 0, w, np.float32(0.0)).astype(np.float32)
    assert w.dtype == np.float32
    return w


def weighted_reference(idx, dist, labels, C, weights, self_base=None):
    """Host restatement of k_vote_weighted (test infrastructure).  idx / dist [nq][kin]: each
    query's neighbour list, ascending by (distance, train index), -1 = none.  Returns (pred_all
    int32 [kmax][nq], scores float32 [nq][C], too_few).  One step per list position, all queries
    at once: S[q][label] = fl(S[q][label] + w) in float32, and the argmax is kept incrementally
    -- only the label just added can become the new best, or tie it with a smaller label.  A
    prefix that reaches a missing entry predicts 0 from there on and sets too_few; that query's
    score row is all zero."""
    idx = np.asarray(idx)
    dist = np.ascontiguousarray(dist, np.float32)
    labels = np.asarray(labels)
    if self_base is not None:
        idx, dist = remove_self(idx, dist, self_base)
    nq, kmax = idx.shape
    w = list_weights(idx, dist, weights)
    S = np.zeros((nq, C), np.float32)
    pred = np.zeros((kmax, nq), np.int32)
    best_s = np.zeros(nq, np.float32)
    best_l = np.zeros(nq, np.int64)
    alive = np.ones(nq, bool)
    ar = np.arange(nq)
    for j in range(kmax):
        alive &= idx[:, j] >= 0
        qs = ar[alive]
        lab = labels[idx[qs, j]].astype(np.int64)
        s = S[qs, lab] + w[qs, j]          # float32 + float32 -> float32, round to nearest
        assert s.dtype == np.float32
        S[qs, lab] = s
        better = (s > best_s[qs]) | ((s == best_s[qs]) & (lab < best_l[qs]))
        best_s[qs[better]] = s[better]
        best_l[qs[better]] = lab[better]
        pred[j, qs] = best_l[qs]
    S[~alive] = 0
    return pred, S, bool((~alive).any())


def weighted_definition(idx, dist, labels, C, weights, self_base=None):
    """The definition, with nothing kept between prefixes: for every query and every k, every
    class's sum is recomputed from scratch in list order with float32 scalars, then argmax (the
    first maximum: the smallest label)."""
    idx = np.asarray(idx)
    dist = np.ascontiguousarray(dist, np.float32)
    if self_base is not None:
        idx, dist = remove_self(idx, dist, self_base)
    nq, kmax = idx.shape
    pred = np.zeros((kmax, nq), np.int32)
    scores = np.zeros((nq, C), np.float32)
    too_few = False
    for q in range(nq):
        zero_mode = weights != UNIFORM and idx[q, 0] >= 0 and dist[q, 0] == 0
        for k in range(1, kmax + 1):
            if (idx[q, :k] < 0).any():
                too_few = True
                scores[q] = 0
                break
            S = [np.float32(0.0)] * C
            for j in range(k):
                d = np.float32(dist[q, j])
                if weights == UNIFORM:
                    wj = np.float32(1.0)
                elif zero_mode:
                    wj = np.float32(1.0 if d == 0 else 0.0)
                else:
                    with np.errstate(divide="ignore", over="ignore"):
                        wj = np.float32(1.0) / (np.sqrt(d) if weights == INV_DIST else d)
                c = int(labels[idx[q, j]])
                S[c] = np.float32(S[c] + wj)
            pred[k - 1, q] = int(np.argmax(np.array(S, np.float32)))
            if k == kmax:
                scores[q] = S
    return pred, scores, too_few


def test_weighted_symbols_in_header_and_library(knn):
    with open(os.path.join(REPO, "include", "knn_amd.h")) as f:
        declared = set(re.findall(r"\b(knn_[a-z_0-9]+)\s*\(", f.read()))
    lib = knn.load_library()
    for s in ("knn_vote_weighted_device", "knn_sweep_weighted_device", "knn_predict_weighted_device",
              "knn_sweep_weighted"):
        assert s in declared, s
        assert hasattr(lib, s), s
    assert lib.knn_version() == 3
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(PKG_DIR, "libknn_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    for sig in ("KNN_sweep_weighted(ArffData*, ArffData*, int, int)", "KNN_sweep_loo_weighted(ArffData*, int, int)"):
        assert sig in out, sig
    for m in ("vote_weighted_device", "sweep_weighted_device", "loo_weighted_device", "predict_weighted_device",
              "sweep_weighted"):
        assert callable(getattr(knn.Context, m)), m
    assert knn.WEIGHTS == {"uniform": 0, "distance": 1, "sqdist": 2}
    p = knn.proba(np.array([[1.0, 3.0], [0.5, 0.5]], np.float32))
    assert np.array_equal(p, np.array([[0.25, 0.75], [0.5, 0.5]], np.float32))


def small_set(oracle):
    """loo_set_300 (300 rows, d = 6, integer grid: zero distances, duplicates, ties) with a few
    rows moved off the grid so that weights are no round numbers, and 40 queries: 20 copies of
    train rows, 20 off-grid points."""
    tr, tl, C = loo_set_300()
    rng = np.random.default_rng(21)
    tr = tr.copy()
    tr[::3] += rng.random((100, 6)).astype(np.float32) * np.float32(0.5)
    te = np.concatenate([tr[rng.integers(0, 300, 20)], rng.random((20, 6)).astype(np.float32) * 4 - 2])
    return tr, tl, C, te.astype(np.float32)


@pytest.mark.parametrize("weights", KINDS)
def test_restatement_matches_definition(oracle, weights):
    tr, tl, C, te = small_set(oracle)
    bad, _, dist, idx = oracle.knn(tr, tl, te, 8, C)
    assert bad == 0
    got = weighted_reference(idx, dist, tl, C, weights)
    want = weighted_definition(idx, dist, tl, C, weights)
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    assert not got[2] and not want[2]
    # leave-one-out: kin = 9, the self row removed first
    bad, _, dist, idx = oracle.knn(tr, tl, tr, 9, C)
    assert bad == 0
    got = weighted_reference(idx, dist, tl, C, weights, self_base=0)
    want = weighted_definition(idx, dist, tl, C, weights, self_base=0)
    assert got[0].shape == (8, 300)
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    if weights != UNIFORM:
        # the case is no trivial one: zero rule rows, and rows the weights decide differently
        _, d1 = remove_self(idx, dist, 0)
        assert (d1[:, 0] == 0).any() and (d1[:, 0] > 0).any()
        uni = weighted_reference(idx, dist, tl, C, UNIFORM, self_base=0)[0]
        assert (uni != got[0]).any()


def test_uniform_is_the_sweep_restatement(oracle):
    tr, tl, C = loo_set_300()
    bad, _, dist, idx = oracle.knn(tr, tl, tr, 8, C)
    assert bad == 0
    pred, scores, too_few = weighted_reference(idx, dist, tl, C, UNIFORM, self_base=0)
    ref, ref_few = sweep_reference(idx, tl, C, self_base=0)
    assert np.array_equal(pred, ref) and too_few == ref_few is False
    i1, _ = remove_self(idx, dist, 0)
    want = np.stack([np.bincount(tl[r], minlength=C) for r in i1]).astype(np.float32)
    assert np.array_equal(bits(scores), bits(want))


@pytest.mark.parametrize("ds", ["small", "medium"])
def test_uniform_matches_golden(oracle, ds):
    tf, tl, d = oracle.read_arff(f"{DATA}/{ds}-train.arff")
    qf, _, _ = oracle.read_arff(f"{DATA}/{ds}-test.arff")
    C = int(tl.max()) + 1
    bad, _, dist, idx = oracle.knn(tf, tl, qf, 100, C)
    assert bad == 0
    pred_all, scores, too_few = weighted_reference(idx, dist, tl, C, UNIFORM)
    assert not too_few
    for k in KS:
        assert np.array_equal(pred_all[k - 1], golden_pred(ds, k)), k
    want = np.stack([np.bincount(tl[r], minlength=C) for r in idx]).astype(np.float32)
    assert np.array_equal(bits(scores), bits(want))


@pytest.mark.parametrize("weights", [INV_DIST, INV_SQDIST])
def test_zero_rule(oracle, weights):
    """Queries copied from train rows that have duplicates under different labels: the vote for
    k > z (z zero-distance entries) is the vote over the first z."""
    rng = np.random.default_rng(8)
    tr = rng.standard_normal((200, 5)).astype(np.float32)
    tl = rng.integers(0, 4, 200).astype(np.int32)
    tr[100:103] = tr[7]                      # row 7 four times: labels 3, 0, 0, 2 -> vote 0
    tl[[7, 100, 101, 102]] = [3, 0, 0, 2]
    tr[150] = tr[9]                          # row 9 twice: labels 2, 1 -> tie, smallest label 1
    tl[[9, 150]] = [2, 1]
    te = np.stack([tr[7], tr[9], tr[11], tr[7] + np.float32(0.25)])
    bad, _, dist, idx = oracle.knn(tr, tl, te, 12, 4)
    assert bad == 0
    z = (dist == 0).sum(axis=1)
    assert z.tolist() == [4, 2, 1, 0]
    pred, scores, too_few = weighted_reference(idx, dist, tl, 4, weights)
    assert not too_few
    assert pred[:, 0].tolist() == [3, 0, 0] + [0] * 9      # 3 | 3,0 -> 0 (tie) | 3,0,0 | 3,0,0,2 | frozen
    assert pred[:, 1].tolist() == [2] + [1] * 11           # 2 | 2,1 -> 1 (tie) | frozen
    assert pred[:, 2].tolist() == [int(tl[11])] * 12
    assert np.array_equal(scores[0], np.array([2, 0, 1, 1], np.float32))
    assert np.array_equal(scores[1], np.array([0, 1, 1, 0], np.float32))
    assert scores[2].sum() == 1 and scores[2, tl[11]] == 1
    # no zero distance: ordinary weights, every entry counts
    assert (scores[3] > 0).sum() == len(set(tl[idx[3]].tolist())) and not float(scores[3].sum()).is_integer()
    want = weighted_definition(idx, dist, tl, 4, weights)
    assert np.array_equal(pred, want[0]) and np.array_equal(bits(scores), bits(want[1]))


def test_inf_tie_goes_to_the_smallest_label():
    labels = np.array([0, 1, 2, 3], np.int32)
    idx = np.array([[3, 1, 0]], np.int32)
    dist = np.array([[1e-40, 1e-40, 1.0]], np.float32)
    assert dist[0, 0] > 0                      # a subnormal, kept
    pred, scores, too_few = weighted_reference(idx, dist, labels, 4, INV_SQDIST)
    assert not too_few
    assert np.isinf(scores[0, 3]) and np.isinf(scores[0, 1]) and scores[0, 0] == 1
    assert pred[:, 0].tolist() == [3, 1, 1]
    want = weighted_definition(idx, dist, labels, 4, INV_SQDIST)
    assert np.array_equal(pred, want[0]) and np.array_equal(bits(scores), bits(want[1]))
    # 1 / sqrt(1e-40) is finite: two equal finite weights tie the same way
    pred, scores, _ = weighted_reference(idx, dist, labels, 4, INV_DIST)
    assert np.isfinite(scores).all() and scores[0, 3] == scores[0, 1]
    assert pred[:, 0].tolist() == [3, 1, 1]


@pytest.mark.parametrize("weights", KINDS)
def test_missing_entries(weights):
    idx = np.array([[0, 1, -1], [2, 1, 0]], np.int32)
    dist = np.array([[0.5, 2.0, 3e38], [0.25, 0.25, 4.0]], np.float32)
    pred, scores, too_few = weighted_reference(idx, dist, np.array([3, 1, 1], np.int32), 4, weights)
    assert too_few
    assert pred[:, 0].tolist() == [3, 3 if weights != UNIFORM else 1, 0]
    assert pred[:, 1].tolist() == [1, 1, 1]
    assert not scores[0].any() and scores[1].any()
    want = weighted_definition(idx, dist, np.array([3, 1, 1], np.int32), 4, weights)
    assert want[2] and np.array_equal(pred, want[0]) and np.array_equal(bits(scores), bits(want[1]))
