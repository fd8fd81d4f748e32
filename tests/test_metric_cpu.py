"""CPU-side checks of the Manhattan and Chebyshev metrics: the entry points are exported and
bound, and the numpy float32 restatement the GPU tests compare bits against (metric_reference)
is pinned to a scalar, definitional loop and to exact float64 arithmetic on an integer grid.
The input sets of tests/test_gpu_metric.py are made here too, with assertions that they can
tell a kernel that ran the wrong metric, or summed in another order, from a right one.  No GPU
is needed here.

The rules (include/knn_amd.h, "Metrics"): Manhattan D = sum |q_i - t_i| with sum = +0, then for
i ascending df = fl(q_i - t_i), sum = fl(sum + |df|) in IEEE binary32; Chebyshev m = +0, then
m = fmaxf(m, |fl(q_i - t_i)|), fmaxf ignoring a NaN operand like numpy.fmax.  Neighbours are the k
smallest (D, train index) pairs among the rows with D < FLT_MAX; the reported distance is D.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, REPO

EUCLIDEAN, MANHATTAN, CHEBYSHEV = 0, 1, 2
NAMES = {MANHATTAN: "manhattan", CHEBYSHEV: "chebyshev"}
FLT_MAX = np.finfo(np.float32).max


def bits(x):
    """float32 array -> its uint32 bit patterns (what the tests compare)."""
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def metric_distances(train, test, metric):
    """float32 [nq][nt] distances of the metric (test infrastructure): one feature at a time, in
    ascending order, every step rounded to float32.  EUCLIDEAN is the reference's squared form."""
    tr = np.ascontiguousarray(train, np.float32)
    te = np.ascontiguousarray(test, np.float32)
    acc = np.zeros((len(te), len(tr)), np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for i in range(tr.shape[1]):
            df = te[:, i:i + 1] - tr[None, :, i]
            if metric == MANHATTAN:
                acc = acc + np.abs(df)
            elif metric == CHEBYSHEV:
                acc = np.fmax(acc, np.abs(df))
            else:
                acc = acc + df * df
            assert df.dtype == np.float32 and acc.dtype == np.float32
    return acc


def metric_reference(train, test, k, metric):
    """Host restatement of a top-k pass under `metric`: (dist float32 [nq][k], idx int32 [nq][k]),
    each list ascending by (distance bits, train index) over the rows with D < FLT_MAX (NaN, inf
    and FLT_MAX never qualify); missing entries are FLT_MAX / -1."""
    D = metric_distances(train, test, metric)
    nq = len(D)
    dist = np.full((nq, k), FLT_MAX, np.float32)
    idx = np.full((nq, k), -1, np.int32)
    for q in range(nq):
        ok = np.nonzero(D[q] < FLT_MAX)[0]
        order = ok[np.lexsort((ok, bits(D[q, ok])))][:k]
        dist[q, :len(order)] = D[q, order]
        idx[q, :len(order)] = order
    return dist, idx


def vote_reference(idx, labels, C):
    """The reference's vote over full lists: bincount argmax, ties to the smallest label."""
    return np.array([np.argmax(np.bincount(labels[row], minlength=C)) for row in idx], np.int32)


def metric_definition(train, test, k, metric):
    """The definition with float32 scalars and plain Python control flow: no numpy ufunc decides a
    rounding, a NaN or an order."""
    zero = np.float32(0.0)
    nq, nt = len(test), len(train)
    dist = np.full((nq, k), FLT_MAX, np.float32)
    idx = np.full((nq, k), -1, np.int32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for q in range(nq):
            cand = []
            for t in range(nt):
                acc = zero
                for i in range(train.shape[1]):
                    df = np.float32(test[q, i]) - np.float32(train[t, i])
                    a = -df if df < zero else df       # |df|; NaN stays NaN, -0 and +0 compare equal
                    if metric == MANHATTAN:
                        acc = np.float32(acc + a)
                    elif a > acc:                      # fmaxf: a NaN never compares greater
                        acc = a
                if acc < FLT_MAX:                      # strict '<' against the sentinel; NaN fails
                    cand.append((int(np.float32(acc).view(np.uint32)), t))
            cand.sort()
            for j, (b, t) in enumerate(cand[:k]):
                dist[q, j] = np.array(b, np.uint32).view(np.float32)
                idx[q, j] = t
    return dist, idx


# ---------------------------------------------------------------------------------------
# the input sets of the GPU tests
# ---------------------------------------------------------------------------------------
def metric_set(oracle, kind, nt, nq, d, seed=5):
    """(train, labels, test): kind "float" = the generator's uniform fp32 rows (every sum rounds),
    "grid" = integers -2..2 (distance ties everywhere; both metrics exact in any order).  An
    eighth of the train rows is copied twice further up, so equal rows sit on both sides of their
    copies, and the first queries are copies of train rows (zero distances).  Labels are random
    in [0, 10)."""
    rng = np.random.default_rng(seed + 1000 * d + nt)
    if kind == "grid":
        tr = rng.integers(-2, 3, size=(nt, d)).astype(np.float32)
        te = rng.integers(-2, 3, size=(nq, d)).astype(np.float32)
    else:
        tr, _ = oracle.gen(seed + d, 0, 0, nt, d)
        te, _ = oracle.gen(seed + d, 1, 0, nq, d)
    m = nt // 8
    tr[nt // 2:nt // 2 + m] = tr[:m]
    tr[nt - m:] = tr[:m]
    c = min(nq // 4, m)
    te[:c] = tr[rng.integers(0, nt, size=c)]
    tl = rng.integers(0, 10, size=nt).astype(np.int32)
    return tr, tl, te


# ---------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------
def test_metric_symbols_and_bindings(knn):
    with open(os.path.join(REPO, "include", "knn_amd.h")) as f:
        src = f.read()
    declared = set(re.findall(r"\b(knn_[a-z_0-9]+)\s*\(", src))
    for name, v in (("KNN_METRIC_SQEUCLIDEAN", 0), ("KNN_METRIC_MANHATTAN", 1), ("KNN_METRIC_CHEBYSHEV", 2)):
        assert re.search(rf"\b{name} = {v}\b", src), name
    assert "numpy.fmax" in src            # the header says how a NaN difference is treated
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG_DIR, "libknn_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    lib = knn.load_library()
    for s in ("knn_set_metric", "knn_get_metric"):
        assert s in declared, s
        assert re.search(rf"\bT {s}$", out, re.M), s
        assert getattr(lib, s).argtypes is not None, s
    assert lib.knn_version() == 3
    assert knn.METRICS == {"euclidean": 0, "manhattan": 1, "chebyshev": 2}
    assert callable(knn.Context.set_metric) and isinstance(knn.Context.metric, property)
    with pytest.raises(knn.KnnError) as e:
        knn._metric_kind("cosine")
    assert e.value.status == knn.KNN_EINVAL
    # a NULL context: no crash, the default metric
    assert lib.knn_set_metric(None, 1) == knn.KNN_EINVAL
    assert lib.knn_get_metric(None) == 0


SUB = np.float32(2.0 ** -140)
TINY_CASES = {
    "d1": (np.array([[0.5], [-1.25], [0.5], [3.0]], np.float32), np.array([[0.5], [1.0]], np.float32)),
    "d3_subnormal": (np.array([[3, -5, 7], [1, 1, 1], [-2, 9, 4], [3, -5, 7], [0, 0, 0]], np.float32) * SUB,
                     np.array([[1, 2, 3], [0, 0, 0]], np.float32) * SUB),
    # row 0: the L1 sum overflows to inf (never listed) while its largest difference is finite;
    # row 2: one difference is FLT_MAX itself (not < FLT_MAX under either metric)
    "d3_huge": (np.array([[3e38, -3e38, 1], [1, 2, 3], [FLT_MAX, 0, 0], [2e38, 0, 1e38], [1, 2, 4]], np.float32),
                np.array([[0, 0, 0], [1, 2, 3]], np.float32)),
    # a NaN feature: the L1 sum is NaN (never listed), the Chebyshev maximum skips that feature
    "d5_nan": (np.array([[1, 2, np.nan, 4, 5], [1, 2, 3, 4, 5], [np.nan] * 5, [0, 2, 3, 4, 6], [1, 2, 3, 4, 5.5]],
                        np.float32),
               np.array([[1, 2, 3, 4, 5], [0, 0, np.nan, 0, 0]], np.float32)),
    "d5_mixed": (np.array([[1e-3, 1e3, -1e-3, 7, 1e-40], [0.1, 0.2, 0.3, 0.4, 0.5], [-0.1, 0.2, -0.3, 0.4, -0.5],
                           [0.1, 0.2, 0.3, 0.4, 0.5], [1e30, 1e-30, 1, -1, 0]], np.float32),
                 np.array([[0.1, 0.2, 0.3, 0.4, 0.5], [0.3, -0.7, 1e-7, 1e7, 3]], np.float32)),
}


@pytest.mark.parametrize("metric", [MANHATTAN, CHEBYSHEV])
@pytest.mark.parametrize("case", sorted(TINY_CASES))
def test_restatement_equals_definition(case, metric):
    tr, te = TINY_CASES[case]
    for k in (1, 3, len(tr)):
        dist, idx = metric_reference(tr, te, k, metric)
        ddist, didx = metric_definition(tr, te, k, metric)
        assert np.array_equal(idx, didx), (case, k)
        assert np.array_equal(bits(dist), bits(ddist)), (case, k)


def test_restatement_special_values():
    """What the tiny cases are there to show, spelled out."""
    tr, te = TINY_CASES["d3_huge"]
    d1, i1 = metric_reference(tr, te, 5, MANHATTAN)
    dc, ic = metric_reference(tr, te, 5, CHEBYSHEV)
    assert 0 not in i1[0] and 2 not in i1[0] and (i1[0] == -1).sum() == 2      # inf and FLT_MAX never listed
    assert 0 in ic[0] and 2 not in ic[0] and (ic[0] == -1).sum() == 1          # max 3e38 < FLT_MAX is
    assert i1[1, 0] == 1 and d1[1, 0] == 0 and ic[1, 0] == 1
    tr, te = TINY_CASES["d5_nan"]
    d1, i1 = metric_reference(tr, te, 5, MANHATTAN)
    dc, ic = metric_reference(tr, te, 5, CHEBYSHEV)
    assert 0 not in i1[0] and 2 not in i1[0]                       # a NaN sum never qualifies
    assert list(ic[0][:3]) == [0, 1, 2] and not dc[0][:3].any()     # NaN differences ignored: distance 0,
    assert (i1[1] == -1).all()                                      # ... lower index first; a NaN query feature
    assert (ic[1] >= 0).all()                                       # poisons every L1 sum, no Chebyshev maximum
    tr, te = TINY_CASES["d3_subnormal"]
    d1, _ = metric_reference(tr, te, 5, MANHATTAN)
    assert (d1[0] > 0).all() and (d1[0] < np.finfo(np.float32).tiny).all()     # subnormal sums kept


@pytest.mark.parametrize("d", [1, 3, 5])
def test_restatement_exact_on_integer_grid(d):
    rng = np.random.default_rng(d)
    tr = rng.integers(-2, 3, size=(300, d)).astype(np.float32)
    te = rng.integers(-2, 3, size=(20, d)).astype(np.float32)
    diff = np.abs(te[:, None, :].astype(np.float64) - tr[None, :, :].astype(np.float64))
    for metric, exact in ((MANHATTAN, diff.sum(axis=2)), (CHEBYSHEV, diff.max(axis=2))):
        assert np.array_equal(metric_distances(tr, te, metric).astype(np.float64), exact)
        dist, idx = metric_reference(tr, te, 7, metric)
        for q in range(len(te)):
            order = np.lexsort((np.arange(len(tr)), exact[q]))[:7]
            assert np.array_equal(idx[q], order)
            assert np.array_equal(dist[q].astype(np.float64), exact[q, order])
        ddist, didx = metric_definition(tr[:40], te[:3], 7, metric)
        rdist, ridx = metric_reference(tr[:40], te[:3], 7, metric)
        assert np.array_equal(didx, ridx) and np.array_equal(bits(ddist), bits(rdist))


def test_inputs_discriminate(oracle):
    """The GPU tests' sets (2,048 x 8, 257 queries, C = 10; and the L1 sums at d = 11 and 64): a
    kernel that silently ran Euclidean, or summed in another order, cannot pass on them."""
    K, C = 10, 10
    for kind in ("float", "grid"):
        tr, tl, te = metric_set(oracle, kind, 2048, 257, 8)
        _, eidx = metric_reference(tr, te, K, EUCLIDEAN)
        epred = vote_reference(eidx, tl, C)
        for metric in (MANHATTAN, CHEBYSHEV):
            dist, idx = metric_reference(tr, te, K, metric)
            assert (idx >= 0).all()
            sets_differ = np.mean([set(a) != set(b) for a, b in zip(idx.tolist(), eidx.tolist())])
            lists_differ = (idx != eidx).any(axis=1).mean()
            preds_differ = (vote_reference(idx, tl, C) != epred).mean()
            ties = (dist[:, 1:] == dist[:, :-1]).any(axis=1).mean()
            print(f"{kind} {NAMES[metric]}: neighbour sets differ {sets_differ:.3f}, lists differ "
                  f"{lists_differ:.3f}, predictions differ {preds_differ:.3f}, lists with ties {ties:.3f}")
            assert sets_differ >= 0.90, (kind, metric, sets_differ)
            if kind == "grid":
                assert ties >= 0.90, (metric, ties)
            assert preds_differ >= 0.25, (kind, metric, preds_differ)
    for d, least in ((11, 0.25), (64, 0.25)):
        tr, _, te = metric_set(oracle, "float", 1000, 9, d)
        ordered = metric_distances(tr, te, MANHATTAN)
        exact = np.abs(te[:, None, :].astype(np.float64) - tr[None, :, :].astype(np.float64)).sum(axis=2)
        sensitive = (bits(ordered) != bits(exact.astype(np.float32))).mean()
        print(f"d = {d}: ordered fp32 L1 sum differs from the correctly rounded sum on {sensitive:.3f} of pairs")
        assert sensitive >= least, (d, sensitive)
