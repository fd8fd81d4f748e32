"""CPU-side checks of the MFMA form of the radius pass (k_radius_gemm; include/knn_amd.h "Radius
neighbours", DESIGN.md "Radius neighbours", "The MFMA form"): the routing rule knn_radius_policy is
declared, exported, bound and follows its table, and a numpy model of the certificate band on the
input sets of tests/test_gpu_radius_mfma.py.  No GPU is needed here.

The band model.  The kernel multiplies rt = rn_bf16(t) by rq = rn_bf16(-2 q) / -2 and brackets the
reference's distance D by G -+ dl,
    G  = qn + tn - 2 rq.rt                         (binary64 here; the kernel's binary32 roundings
                                                    are what coef pays for)
    dl = coef (qn + tmax) + eta + 2 (|q| max|t - rt| + |q - rq| max|rt|),   coef = (9 d + 512) 2^-24,
                                                    eta = (8 d + 16) 2^-125,
with tmax and the two maxima taken over the row's 64-row tile.  The model asserts L <= D <= U for
every pair of every set (D: test_metric_cpu.metric_distances) and that the band -- the pairs with
L <= thr < U, which are the only ones the kernel must evaluate exactly for a count -- is at most
5 % of all pairs at every threshold the GPU tests use on the shapes of their first case.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, REPO
from test_metric_cpu import EUCLIDEAN, metric_distances, metric_set
from test_radius_cpu import radius_thresholds

# (d, nt, nq, kind) of the GPU tests' first case: one tile plus one row, partial last tiles, query
# blocks on both sides of 256
MFMA_SHAPES = [(64, 65, 9, "grid"), (64, 1000, 257, "float"), (128, 1000, 257, "float"), (128, 4096, 33, "grid"),
               (256, 1000, 33, "float"), (64, 4096, 257, "float")]
MFMA_DIMS = (64, 128, 256)
BAND_CAP = 0.05


def aligned_rows(d, nt=1000, nq=33):
    """The rows of test_gpu_parity.test_rounded_filter_aligned_rounding: every element just below
    a bf16 rounding midpoint, so every operand rounding error has the same sign."""
    rng = np.random.default_rng(31 + d)

    def rows(n):
        s = 2.0 ** rng.integers(0, 4, size=(n, d))                # binades [1, 16): spread distances
        m = 1.0 + rng.integers(0, 128, size=(n, d)) / 128.0      # bf16-exact grid in [1, 2)
        delta = rng.integers(1, 64, size=(n, d)) * 2.0 ** -22     # stay below the midpoint
        return ((m + 2.0 ** -8 - delta) * s).astype(np.float32)   # rounds down to m s

    tr, te = rows(nt), rows(nq)
    tl = rng.integers(0, 10, size=nt).astype(np.int32)
    return tr, tl, te


def bf16_set(oracle, d, nt=1000, nq=65):
    """bf16-exact rows (generator kind 1) with copies, the GPU tests' bf16 case."""
    tr, tl = oracle.gen(23, 0, 0, nt, d, kind=1)
    te, _ = oracle.gen(23, 1, 0, nq, d, kind=1)
    tr[500:600] = tr[:100]
    te[:16] = tr[:16]
    return tr, tl, te


def special_set(case, nt=1000, nq=33, d=64):
    """The GPU tests' special values: one NaN train feature, one inf query feature, rows with
    norms past 2^125 (the direct form runs: nothing to model), or everything scaled by 2^-70 (the
    MFMA form runs; products and distances are subnormal)."""
    rng = np.random.default_rng(31)
    tr = rng.standard_normal((nt, d)).astype(np.float32)
    te = rng.standard_normal((nq, d)).astype(np.float32)
    te[:8] = tr[:8]
    if case == "nan_train":
        tr[5, 3] = np.nan
    elif case == "inf_query":
        te[9, 23] = np.inf
    elif case == "huge_norm":
        tr[::7] *= np.float32(1.0e19)                 # squares near FLT_MAX: norms past 2^125
    else:
        assert case == "scaled"
        tr, te = tr * np.float32(2.0 ** -70), te * np.float32(2.0 ** -70)
    tl = rng.integers(0, 10, size=nt).astype(np.int32)
    return tr, tl, te


def special_thresholds(D):
    fin = np.sort(D[np.isfinite(D)])
    return [np.float32(0.0), fin[len(fin) // 20], fin[len(fin) // 2]]


def strided_set(oracle, d=64, nt=1000, nq=65):
    tr, tl = oracle.gen(53 + d, 0, 0, nt, d)
    te, _ = oracle.gen(53 + d, 1, 0, nq, d)
    te[:16] = tr[:16]
    return tr, tl, te


def routing_set(oracle, rows, queries, d=64):
    """(train, labels, test, thr) at AUTO's floors: thr is the largest 33rd-smallest distance of
    the first 16 queries, a few dozen neighbours per query."""
    tr, tl = oracle.gen(5 + d, 0, 0, rows, d)
    te, _ = oracle.gen(5 + d, 1, 0, queries, d)
    te[:8] = tr[:8]
    thr = np.float32(np.sort(metric_distances(tr, te[:16], EUCLIDEAN), axis=1)[:, 32].max())
    return tr, tl, te, thr


def rewritten_rows(tr):
    """The train cache case's in-place write."""
    tr2 = tr.copy()
    tr2[:400] = tr2[600:1000]
    return tr2


def rn_bf16(x):
    """float32 -> the nearest bf16 value (ties to even), as float32: bf16_rne of knn_device.h."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def band_model(tr, te):
    """(L, U) float64 [nq][nt] of the kernel's bracket, with the tile maxima."""
    d = tr.shape[1]
    coef = (9 * d + 512) * 2.0 ** -24
    eta = (8 * d + 16) * 2.0 ** -125
    t64, q64 = tr.astype(np.float64), te.astype(np.float64)
    rt = rn_bf16(tr).astype(np.float64)
    rq = rn_bf16(np.float32(-2) * te).astype(np.float64) / -2.0
    tn, qn = (t64 * t64).sum(axis=1), (q64 * q64).sum(axis=1)
    up = 1.0 + 2.0 ** -12                                          # norm_ub's factor
    et = np.sqrt(((t64 - rt) ** 2).sum(axis=1)) * up
    nrt = np.sqrt((rt * rt).sum(axis=1)) * up
    tile = np.arange(len(tr)) // 64
    ntile = tile[-1] + 1
    tmax = np.array([tn[tile == i].max() for i in range(ntile)])[tile]
    etmax = np.array([et[tile == i].max() for i in range(ntile)])[tile]
    rtmax = np.array([nrt[tile == i].max() for i in range(ntile)])[tile]
    nq_ = np.sqrt(qn) * up
    eq = np.sqrt(((q64 - rq) ** 2).sum(axis=1)) * up
    G = qn[:, None] + tn[None, :] - 2.0 * (rq @ rt.T)
    rho = 2.0 * (1.0 + 2.0 ** -17) * (nq_[:, None] * etmax[None, :] + eq[:, None] * rtmax[None, :])
    dl = coef * (qn[:, None] + tmax[None, :]) + eta + rho
    return G - dl, G + dl


def radius_floors(knn, d=64):
    """(row floor, query floor) of AUTO's MFMA form, found from knn_radius_policy itself."""
    def first(f):
        lo, hi = 0, 1 << 40                                        # f(lo) false, f(hi) true
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if f(mid) else (mid, hi)
        return hi
    big = 1 << 40
    assert knn.radius_policy("euclidean", "f32", d, big, big) == "mfma"
    rows = first(lambda n: knn.radius_policy("euclidean", "f32", d, n, big) == "mfma")
    queries = first(lambda n: knn.radius_policy("euclidean", "f32", d, big, n) == "mfma")
    return rows, queries


def test_policy_symbol_and_binding(knn):
    with open(os.path.join(REPO, "include", "knn_amd.h")) as f:
        src = f.read()
    assert re.search(r"\bint32_t\s+knn_radius_policy\s*\(", src)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG_DIR, "libknn_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT knn_radius_policy$", out, re.M)
    lib = knn.load_library()
    assert lib.knn_radius_policy.argtypes is not None and callable(knn.radius_policy)
    assert lib.knn_version() == 3
    assert lib.knn_radius_policy(0, 0, 64, 1, 1, 0, None) == knn.KNN_EINVAL          # no output
    for bad in ((3, "f32", 64, 1, 1, 0), (0, "f32", 0, 1, 1, 0), (0, "f32", 64, -1, 1, 0), (0, "f32", 64, 1, 1, 7)):
        with pytest.raises(knn.KnnError) as e:
            knn.radius_policy(*bad)
        assert e.value.status == knn.KNN_EINVAL


def test_policy_rule_table(knn):
    rows, queries = radius_floors(knn)
    print(f"AUTO's MFMA floors: {rows} train rows, {queries} queries")
    assert rows >= 16384 and queries >= 1
    assert radius_floors(knn, 128) == (rows, queries) and radius_floors(knn, 256) == (rows, queries)
    sides = [(rows, queries, True), (rows - 1, queries, False), (rows, queries - 1, False), (rows - 1, queries - 1, False),
             (1 << 30, 1 << 30, True), (1, 1, False)]
    for dtype in ("f32", "bf16"):
        for d in (63, 64, 128, 256, 260):
            ok_d = d in MFMA_DIMS
            for metric in ("euclidean", "manhattan", "chebyshev"):
                ok = ok_d and metric == "euclidean"
                for nt, nq, above in sides:
                    for algo in ("direct", "direct_scan"):
                        assert knn.radius_policy(metric, dtype, d, nt, nq, algo) == "direct"
                    want = "mfma" if ok else "direct"
                    assert knn.radius_policy(metric, dtype, d, nt, nq, "gemm_bf16") == want, (metric, d, nt, nq)
                    want = "mfma" if ok and above else "direct"
                    for algo in ("auto", "gemm", "gemm_split", "gemm_i8"):
                        assert knn.radius_policy(metric, dtype, d, nt, nq, algo) == want, (metric, d, nt, nq, algo)
    # every shape of the direct form's own tests stays on the direct form under AUTO, and an empty
    # set has nothing to filter
    for d in MFMA_DIMS:
        assert knn.radius_policy("euclidean", "f32", d, 4096, 1 << 30) == "direct"
        assert knn.radius_policy("euclidean", "f32", d, 0, 9, "gemm_bf16") == "direct"
        assert knn.radius_policy("euclidean", "f32", d, 9, 0, "gemm_bf16") == "direct"


def test_rn_bf16_model():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0e-39, 65280.0, 1.0 + 2.0 ** -8 - 2.0 ** -22], np.float32)
    r = rn_bf16(x)
    assert (r.view(np.uint32) & 0xffff == 0).all()
    assert r[0] == 1.0 and r[1] == 1.0 and r[2] == np.float32(1.015625)   # ties to even, both ways
    assert r[5] == 1.0 and np.all(np.abs(r - x) <= np.abs(x) * 2.0 ** -8 + 2.0 ** -133)


def _check_bracket(tr, te, what):
    D = metric_distances(tr, te, EUCLIDEAN).astype(np.float64)
    L, U = band_model(tr, te)
    assert (L <= D).all() and (D <= U).all(), what
    return D, L, U


def _shares(tr, te, thrs, what):
    """The bracket on every pair, then the band's share of all pairs at each threshold."""
    D, L, U = _check_bracket(tr, te, what)
    out = []
    for thr in thrs:
        t = float(thr)
        share = ((L <= t) & ~(U <= t)).mean()
        print(f"{what} thr={t:.6g}: band {100 * share:.3f} % of the pairs")
        out.append(share)
    return D, out


def _narrow(tr, te, thrs, what):
    for thr, share in zip(thrs, _shares(tr, te, thrs, what)[1]):
        assert share <= BAND_CAP, (what, float(thr), share)


def _thrs(tr, te):
    return radius_thresholds(metric_distances(tr, te, EUCLIDEAN))


@pytest.mark.parametrize("d,nt,nq,kind", MFMA_SHAPES + [(128, 4096, 257, "float")])
def test_band_shapes_and_segments(oracle, d, nt, nq, kind):
    """The shapes case, and with (128, 4096, 257) both sets of the forced-segments case; the
    consumers, errors, cross-form, cache and determinism cases run on these sets too."""
    tr, _, te = metric_set(oracle, kind, nt, nq, d)
    _narrow(tr, te, _thrs(tr, te), f"d={d} nt={nt} nq={nq} {kind}")


@pytest.mark.parametrize("d,kind", [(64, "grid"), (256, "float")])
def test_band_every_pair(oracle, d, kind):
    tr, _, te = metric_set(oracle, kind, 65, 9, d)
    _narrow(tr, te, [np.float32(3.0e38)], f"every pair d={d}")


@pytest.mark.parametrize("d", [64, 256])
def test_band_bf16_rows(oracle, d):
    tr, _, te = bf16_set(oracle, d)
    _narrow(tr, te, _thrs(tr, te), f"bf16 d={d}")


def test_band_leave_one_out(oracle):
    tr, _, _ = metric_set(oracle, "grid", 1000, 9, 64)
    thrs = _thrs(tr, tr)
    _narrow(tr, tr, [np.float32(0.0), thrs[2]], "loo")
    _narrow(tr, tr[100:357], [np.float32(0.0)], "loo window")


def test_band_strided_set(oracle):
    tr, _, te = strided_set(oracle)
    _narrow(tr, te, _thrs(tr, te)[1:], "strided")


def test_band_rewritten_rows(oracle):
    tr, _, te = metric_set(oracle, "float", 1000, 257, 64)
    _narrow(rewritten_rows(tr), te, [_thrs(tr, te)[2]], "rewritten rows")


def test_band_routing_set(knn, oracle):
    rows, queries = radius_floors(knn)
    tr, _, te, thr = routing_set(oracle, rows, queries)
    _narrow(tr, te, [thr], f"routing {rows} x {queries}")
    _narrow(tr[:rows - 64], te, [thr], "routing, one tile below")


@pytest.mark.parametrize("d", MFMA_DIMS)
def test_band_worst_case_rounding(d):
    """Every operand rounding error of one sign.  The bracket holds, and at the three lower
    thresholds the band keeps to the 5 % of the other sets.  At the 0.5 quantile it cannot: these
    rows are built so that the rounding term rho of dl, a Cauchy-Schwarz bound that random rounding
    errors stay 2-3 times under, is nearly attained, and the median is where the distances are
    densest (measured: 7.8 / 10.9 / 15.5 % of the pairs at d = 64 / 128 / 256).  The cap there is
    what the number formats allow.  A band pair has thr and D in [L, U], so |D - thr| <= 2 dl; and
    with |x - rn(x)| <= 2^-8 |x| per element of a normal bf16 rounding,
        dl <= dl_wc = coef (qn + tmax) + eta + 2^-6 (1 + 2^-8) |q| max|t|   (maxima over the tile),
    so the band is at most the share of the pairs with |D - thr| <= 2 dl_wc, computed from the
    reference distances and the rows' norms alone."""
    tr, _, te = aligned_rows(d)
    thrs = _thrs(tr, te)
    D, shares = _shares(tr, te, thrs, f"aligned d={d}")
    for thr, share in zip(thrs[:3], shares[:3]):
        assert share <= BAND_CAP, (d, float(thr), share)
    coef, eta = (9 * d + 512) * 2.0 ** -24, (8 * d + 16) * 2.0 ** -125
    tn, qn = (tr.astype(np.float64) ** 2).sum(axis=1), (te.astype(np.float64) ** 2).sum(axis=1)
    tile = np.arange(len(tr)) // 64
    tmax = np.array([tn[tile == i].max() for i in range(tile[-1] + 1)])[tile]
    dl_wc = coef * (qn[:, None] + tmax[None, :]) + eta + \
        2.0 ** -6 * (1 + 2.0 ** -8) * np.sqrt(qn)[:, None] * np.sqrt(tmax)[None, :]
    cap = (np.abs(D - float(thrs[3])) <= 2 * dl_wc).mean()
    print(f"aligned d={d} thr={float(thrs[3]):.6g}: band {100 * shares[3]:.3f} %, cap {100 * cap:.3f} %")
    assert shares[3] <= cap, (d, shares[3], cap)


def test_band_scaled_rows():
    """Rows scaled by 2^-70 with subnormal thresholds: the bracket holds, and the band is every
    pair at every threshold, not 5 % -- every distance is below 2^-126 while eta, which pays for
    products and partial sums flushed to zero, is (8 d + 16) 2^-125, so L < 0 <= thr < U for every
    pair.  That is what the GPU case is there for: the MFMA form runs and decides nothing."""
    tr, _, te = special_set("scaled")
    D = metric_distances(tr, te, EUCLIDEAN)
    thrs = special_thresholds(D)
    assert 0 < thrs[1] < thrs[2] < np.finfo(np.float32).tiny and D.max() < np.finfo(np.float32).tiny
    for share in _shares(tr, te, thrs, "scaled")[1]:
        assert share == 1.0


