"""CPU-side checks of the k-sweep: the new entry points are exported, and the numpy
restatement of the sweep that the GPU tests check against (sweep_reference: prefix bincount
argmax with ties to the smallest label, and the leave-one-out self-removal rule) is itself
pinned to the reference's fixtures and to the oracle.  No GPU is needed here.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA, KS, PKG_DIR, REPO, golden_pred


def sweep_reference(idx, labels, C, self_base=None):
    """Host restatement of k_vote_sweep (test infrastructure).  idx [nq][kin]: each query's
    neighbour list, ascending by (distance, train index), -1 = none.  self_base: the entry
    equal to self_base + q is removed from query q's list; if none equals it the last entry
    is dropped.  Returns (pred_all int32 [kmax][nq], too_few): pred_all[k - 1][q] = argmax of
    the bincount of the first k labels, ties to the smallest label (main.cpp:64-78); a prefix
    that reaches a missing entry predicts 0 and sets too_few.  The argmax is kept
    incrementally: adding one label changes one count, so the new argmax is the old one or
    that label."""
    idx = np.asarray(idx)
    labels = np.asarray(labels)
    nq, kin = idx.shape
    kmax = kin - (0 if self_base is None else 1)
    pred = np.zeros((kmax, nq), np.int32)
    too_few = False
    for q in range(nq):
        row = idx[q]
        if self_base is not None:
            hit = np.nonzero(row == self_base + q)[0]
            row = np.delete(row, hit[0]) if len(hit) else row[:-1]
        counts = np.zeros(C, np.int64)
        best_c, best_l = 0, 0
        for j in range(kmax):
            if row[j] < 0:
                too_few = True
                break
            lab = int(labels[row[j]])
            counts[lab] += 1
            if counts[lab] > best_c or (counts[lab] == best_c and lab < best_l):
                best_c, best_l = int(counts[lab]), lab
            pred[j, q] = best_l
    return pred, too_few


def loo_oracle(oracle, train, labels, ks, C, rows=None):
    """Leave-one-out by definition: for every row i (of `rows`), the oracle's KNN of row i on
    the train set with row i deleted.  Returns {k: int32 [len(rows)]}."""
    rows = range(len(train)) if rows is None else rows
    out = {k: np.zeros(len(rows), np.int32) for k in ks}
    for n, i in enumerate(rows):
        tr = np.delete(train, i, axis=0)
        tl = np.delete(labels, i)
        for k in ks:
            bad, p, _, _ = oracle.knn(tr, tl, train[i:i + 1], k, C, threads=1, topk=False)
            assert bad == 0
            out[k][n] = p[0]
    return out


def test_sweep_symbols_in_header_and_library(knn):
    with open(os.path.join(REPO, "include", "knn_amd.h")) as f:
        declared = set(re.findall(r"\b(knn_[a-z_0-9]+)\s*\(", f.read()))
    lib = knn.load_library()
    for s in ("knn_vote_sweep_device", "knn_sweep_device", "knn_sweep"):
        assert s in declared, s
        assert hasattr(lib, s), s
    assert lib.knn_version() == 3
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(PKG_DIR, "libknn_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    for sig in ("KNN_sweep(ArffData*, ArffData*, int)", "KNN_sweep_loo(ArffData*, int)"):
        assert sig in out, sig
    for m in ("sweep_device", "vote_sweep_device", "sweep", "loo_device"):
        assert callable(getattr(knn.Context, m)), m


@pytest.mark.parametrize("ds", ["small", "medium"])
def test_restatement_matches_golden(oracle, ds):
    """Row k - 1 of the restatement on the oracle's top-100 lists is the reference's
    prediction vector for k, for every golden k."""
    tf, tl, d = oracle.read_arff(f"{DATA}/{ds}-train.arff")
    qf, _, _ = oracle.read_arff(f"{DATA}/{ds}-test.arff")
    C = int(tl.max()) + 1
    bad, _, _, idx = oracle.knn(tf, tl, qf, 100, C)
    assert bad == 0
    pred_all, too_few = sweep_reference(idx, tl, C)
    assert not too_few
    for k in KS:
        assert np.array_equal(pred_all[k - 1], golden_pred(ds, k)), k


def loo_set_300():
    """300 rows on a small integer grid (distance ties), 20 exact copies of earlier rows and
    one row repeated 12 times: with kin = 8 the later copies do not find themselves in their
    own list (the "drop the last" case)."""
    rng = np.random.default_rng(4)
    tr = rng.integers(-2, 3, size=(300, 6)).astype(np.float32)
    tl = rng.integers(0, 5, size=300).astype(np.int32)
    src = rng.integers(0, 100, size=20)
    tr[rng.permutation(np.arange(100, 300))[:20]] = tr[src]
    tr[np.arange(12) * 23 + 7] = np.float32(9.0)
    return tr, tl, 5


def test_restatement_leave_one_out_matches_oracle(oracle):
    tr, tl, C = loo_set_300()
    kmax = 7
    bad, _, _, idx = oracle.knn(tr, tl, tr, kmax + 1, C)
    assert bad == 0
    # both branches of the rule occur: self inside its list, and pushed out of it by ties
    inside = (idx == np.arange(300)[:, None]).any(axis=1)
    assert inside.any() and not inside.all()
    pred_all, too_few = sweep_reference(idx, tl, C, self_base=0)
    assert not too_few and pred_all.shape == (kmax, 300)
    want = loo_oracle(oracle, tr, tl, (1, 2, 3, 7), C)
    for k, w in want.items():
        assert np.array_equal(pred_all[k - 1], w), k


def test_restatement_missing_entries():
    idx = np.array([[0, 1, -1], [2, 1, 0]], np.int32)
    pred_all, too_few = sweep_reference(idx, np.array([3, 1, 1], np.int32), 4)
    assert too_few
    assert pred_all[:, 0].tolist() == [3, 1, 0] and pred_all[:, 1].tolist() == [1, 1, 1]


def test_best_k_ties_go_to_the_smallest_k(knn):
    assert knn.best_k(np.array([5, 9, 9, 3], np.int64)) == 2
    assert knn.best_k([7]) == 1
    assert knn.best_k(np.array([1, 2, 3, 3])) == 3
    assert knn.best_k(np.array([4, 4, 4])) == 1
    with pytest.raises(knn.KnnError):
        knn.best_k(np.zeros(0, np.int64))
