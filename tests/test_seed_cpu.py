"""Host checks of the int8 filter's seeded thresholds (knn_seed.hip, DESIGN.md "Seeded
thresholds"), through the library's host exports of the functions the kernel runs.  No GPU.

  * knn_i8_seed_bound (knn_device.h): U of an accumulator value a = nq . nt - n_r, with the train
    set's maxima in place of a tile's statistics.  On int8 rows made from their fp32 originals
    (random, saturating queries, all-equal rows) U >= the fp32 direct-form distance and >= the
    exact one (rational arithmetic); U is non-increasing in a; a NaN or infinite query norm gives
    a non-finite U (which the kernel does not publish).
  * the group selection (knn_kth_largest_i32): the k-th largest of G group maxima equals numpy's
    and is <= the k-th largest value overall -- duplicates, fewer than k non-empty groups,
    k = 16 of 32 and k = 32 of 64.
  * the sample rule (knn_seed_sample): strided tile blocks inside the train set, at most an
    eighth of its rows, none for a train set too small.
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

F32 = np.float32
D = 128
COEF = F32((9 * D + 512) * 2.0 ** -24)   # certificate_fused (knn_capi.cpp)
ETA = F32((8 * D + 16) * 2.0 ** -125)
EMPTY = -(1 << 29)                        # KNN_SEED_EMPTY


@pytest.fixture(scope="module")
def lib(knn):
    lib = knn.load_library()
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    lib.knn_i8_debug_quant.argtypes = [P, LL, ctypes.c_float, P]
    lib.knn_i8_debug_quant.restype = I
    lib.knn_i8_debug_fast.argtypes = [P, P, P, LL, P]
    lib.knn_i8_debug_fast.restype = I
    lib.knn_debug_seed_bound.argtypes = [P, LL, P, P]
    lib.knn_debug_seed_bound.restype = I
    lib.knn_debug_seed_select.argtypes = [P, I, I, P]
    lib.knn_debug_seed_select.restype = I
    lib.knn_debug_seed_tiles.argtypes = [LL, I, LL, I, P, I, P]
    lib.knn_debug_seed_tiles.restype = I
    return lib


def quant(lib, x, s):
    x = np.ascontiguousarray(x, F32)
    out = np.zeros(x.shape, np.int8)
    assert lib.knn_i8_debug_quant(x.ctypes.data, x.size, ctypes.c_float(float(s)), out.ctypes.data) == 0
    return out


def seed_bound(lib, a, qn, qs, s2, smax):
    a = np.ascontiguousarray(a, np.int32)
    par = np.array([qn, qs[0], qs[1], s2, COEF, ETA, *smax], F32)
    out = np.zeros(len(a), F32)
    assert lib.knn_debug_seed_bound(a.ctypes.data, len(a), par.ctypes.data, out.ctypes.data) == 0
    return out


def up(x):
    """A float32 >= the real number x >= 0 (binary64 in, one step past its float32 rounding)."""
    return np.nextafter(F32(x), F32(np.inf))


def norm_up(v):
    """float32 upper bound of the Euclidean norm of the binary64 vector v."""
    return up(np.sqrt(np.sum(np.asarray(v, np.float64) ** 2)) * (1 + 1e-12))


def direct_fp32(q, t, fma):
    """The direct form in binary32, feature by feature: sum += (q_i - t_i)^2, separately rounded
    or contracted into an fma."""
    acc = F32(0)
    for i in range(len(q)):
        df = F32(q[i] - t[i])
        acc = F32(np.float64(df) * np.float64(df) + np.float64(acc)) if fma else F32(acc + F32(df * df))
    return acc


def _case(kind, rng):
    nt, nq = 48, 6
    t = rng.uniform(-1, 1, (nt, D)).astype(F32)
    q = rng.uniform(-1, 1, (nq, D)).astype(F32)
    if kind == "saturate":
        q = (q * 4).astype(F32)  # most query elements outside the train range: clamped to +-127
    elif kind == "all_equal":
        t[:] = t[0]
        q[:] = t[0]
        q[1] = t[0] + F32(1e-3)
    elif kind == "near":
        q[:] = t[:nq] + rng.uniform(-1e-3, 1e-3, (nq, D)).astype(F32)
    return t, q


@pytest.mark.parametrize("kind", ["random", "near", "saturate", "all_equal"])
def test_bound_covers_the_distance(lib, kind):
    rng = np.random.default_rng(["random", "near", "saturate", "all_equal"].index(kind) + 5)
    t, q = _case(kind, rng)
    s = F32(np.abs(t).max() / F32(127))
    s2 = F32(F32(2) * s) * s
    it, iq = quant(lib, t, s).astype(np.int64), quant(lib, q, s).astype(np.int64)
    t64, q64 = t.astype(np.float64), q.astype(np.float64)
    tn = np.sum(t64 * t64, axis=1).astype(F32)  # (the kernels' fmaf-chain norms differ from these by
    qn = np.sum(q64 * q64, axis=1).astype(F32)  #  less than the certificate's norm term allows)
    fast = np.zeros((len(tn), 3), np.int32)
    zero, s2v = np.zeros(len(tn), F32), np.full(len(tn), s2, F32)
    assert lib.knn_i8_debug_fast(tn.ctypes.data, zero.ctypes.data, s2v.ctypes.data, len(tn), fast.ctypes.data) == 0
    n_r, nu = fast[:, 0].astype(np.int64), fast[:, 1].copy().view(F32)
    rt, rq = it * np.float64(s), iq * np.float64(s)  # (exact: 24-bit s times 7-bit integers)
    smax = (tn.max(), max(norm_up(t64[r] - rt[r]) for r in range(len(t))),
            max(norm_up(rt[r]) for r in range(len(t))), nu.max())
    for qi in range(len(q)):
        a = iq[qi] @ it.T - n_r
        assert np.all(a > EMPTY) and np.all(np.abs(a) < 2 ** 31)
        qs = (norm_up(q64[qi]), norm_up(q64[qi] - rq[qi]))
        U = seed_bound(lib, a, qn[qi], qs, s2, smax)
        assert np.all(np.isfinite(U))
        for r in range(len(t)):
            exact = sum((Fraction(float(x)) - Fraction(float(y))) ** 2 for x, y in zip(q[qi], t[r]))
            assert Fraction(float(U[r])) >= exact, (kind, qi, r)
            assert U[r] >= direct_fp32(q[qi], t[r], False) and U[r] >= direct_fp32(q[qi], t[r], True), (kind, qi, r)


def test_bound_is_monotone_in_a(lib):
    rng = np.random.default_rng(11)
    smax = (F32(60.0), F32(0.05), F32(7.5), F32(1e-4))
    for qn in (F32(0.0), F32(42.7), F32(3e4)):
        for s2 in (F32(1.24e-4), F32(3.0)):
            a = np.unique(np.concatenate([rng.integers(-(1 << 22), 1 << 22, 4000), np.arange(-300, 300),
                                          (1 << 24) + np.arange(-40, 40), np.array([-(1 << 30), EMPTY, 2 ** 31 - 1])]))
            U = seed_bound(lib, a, qn, (F32(6.6), F32(0.03)), s2, smax)
            assert np.all(np.isfinite(U))
            assert np.all(np.diff(U) <= 0)  # a ascending: U never rises


@pytest.mark.parametrize("qn", [np.nan, np.inf, -np.inf])
def test_non_finite_query_norm_gives_no_seed(lib, qn):
    smax = (F32(60.0), F32(0.05), F32(7.5), F32(1e-4))
    for qs in ((F32(6.6), F32(0.03)), (F32(np.inf), F32(np.inf)), (F32(np.nan), F32(np.nan))):
        U = seed_bound(lib, np.array([-5000, 0, 123456]), F32(qn), qs, F32(1.24e-4), smax)
        assert not np.any(np.isfinite(U))
    # ... and so does a finite norm beside non-finite statistics
    U = seed_bound(lib, np.array([0]), F32(40.0), (F32(np.inf), F32(0.03)), F32(1.24e-4), smax)
    assert not np.any(np.isfinite(U))


def select(lib, m, k):
    m = np.ascontiguousarray(m, np.int32)
    out = ctypes.c_int32(0)
    ok = lib.knn_debug_seed_select(m.ctypes.data, len(m), k, ctypes.byref(out))
    assert ok in (0, 1)
    return ok, out.value


@pytest.mark.parametrize("G,k", [(32, 1), (32, 10), (32, 16), (64, 17), (64, 32), (32, 32), (64, 64)])
def test_group_selection(lib, G, k):
    rng = np.random.default_rng(G + k)
    for trial in range(40):
        rows = 1 + trial % 7
        span = 5 if trial % 3 == 0 else 1 << 21  # (a span of 5: many duplicates)
        vals = rng.integers(-span, span, (rows, G)).astype(np.int32)
        if trial % 5 == 4:
            vals[:, rng.integers(0, G, G // 4)] = -(1 << 30)  # some groups hold pad rows only
        m = vals.max(axis=0)
        ok, got = select(lib, m, k)
        assert got == np.sort(m)[-k]
        assert ok == int(np.sum(m > EMPTY) >= k)
        # k distinct rows lie at or above it: the k-th largest value overall is >= it
        if rows * G >= k:
            assert got <= np.sort(vals.reshape(-1))[-k]


def test_group_selection_too_few_groups(lib):
    m = np.full(32, np.iinfo(np.int32).min, np.int32)  # (the kernel's start value)
    assert select(lib, m, 1)[0] == 0
    m[:9] = [5, 5, 5, -7, 0, 3, 3, 2 ** 31 - 1, -(1 << 22)]
    assert select(lib, m, 9) == (1, -(1 << 22))
    assert select(lib, m, 3) == (1, 5)
    assert select(lib, m, 10)[0] == 0 and select(lib, m, 16)[0] == 0
    m[9:] = -(1 << 30)  # pad rows
    assert select(lib, m, 10) == (0, -(1 << 30))
    assert select(lib, m[:4], 5) == (0, np.iinfo(np.int32).min)  # fewer values than k


def sample(lib, nt, bn, nq, cus=256):
    out = np.zeros(4096, np.int64)
    info = np.zeros(3, np.int64)
    ns = lib.knn_debug_seed_tiles(nt, bn, nq, cus, out.ctypes.data, len(out), info.ctypes.data)
    assert ns == info[0]
    return out[:ns], info


@pytest.mark.parametrize("bn", [32, 64])
@pytest.mark.parametrize("nt", [1_000_000, 65_536, 16_447, 262_144, 8_191])
def test_sample_rule(lib, nt, bn):
    tiles, (ns, stride, slices) = sample(lib, nt, bn, 100_000)
    nblk = -(-nt // bn)
    assert ns > 0 and slices == 1
    assert ns * bn * 8 <= nt + 8 * bn                 # at most an eighth of the rows
    assert np.array_equal(tiles, np.arange(ns) * stride) and stride == nblk // ns
    assert tiles[-1] < nblk                           # inside the train set
    assert tiles[-1] >= nblk - stride - ns            # strided over all of it, not its first rows
    few = sample(lib, nt, bn, 64)[1]
    assert few[0] == ns and 1 <= few[2] <= ns         # few queries: the same sample in slices


@pytest.mark.parametrize("bn", [32, 64])
def test_sample_rule_too_few_rows(lib, bn):
    for nt in (1, 31, 255, 8 * 32 - 1):
        assert sample(lib, nt, bn, 1000)[1][0] == 0
    assert sample(lib, 0, bn, 1000)[1][0] == 0 and sample(lib, 5000, bn, 0)[1][0] == 0
