"""Host checks of the int8 filter operand class's rule (knn_device.h: knn_i8_quant, knn_i8_norm_q,
knn_i8_norm_res, knn_i8_fast_thr), through the library's host exports of the same functions the
kernels run.  No GPU.

  * the quantiser against a numpy restatement: n = clamp(rne(x / s), -127, 127), never -128;
  * the integer fast test: for every integer a with -s2 a <= tf, a >= knn_i8_fast_thr(tf, s2)
    (no false negative against the float test), and |tn - s2 n_r| <= knn_i8_norm_res, both in exact
    rational arithmetic; then the two together as the kernel uses them;
  * the certificate's operand-rounding term rho = 2 (|q| |t - rt| + |q - rq| |rt|) >=
    |2 (q.t - rq.rt)| in binary64, on random rows and on rows whose residuals all have their
    element's sign (each element just below a grid midpoint).
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

F32 = np.float32


@pytest.fixture(scope="module")
def lib(knn):
    lib = knn.load_library()
    P = ctypes.c_void_p
    lib.knn_i8_debug_quant.argtypes = [P, ctypes.c_longlong, ctypes.c_float, P]
    lib.knn_i8_debug_quant.restype = ctypes.c_int
    lib.knn_i8_debug_fast.argtypes = [P, P, P, ctypes.c_longlong, P]
    lib.knn_i8_debug_fast.restype = ctypes.c_int
    return lib


def quant(lib, x, s):
    x = np.ascontiguousarray(x, F32).reshape(-1)
    out = np.zeros(len(x), np.int8)
    assert lib.knn_i8_debug_quant(x.ctypes.data, len(x), ctypes.c_float(float(s)), out.ctypes.data) == 0
    return out


def fast(lib, tn, tf, s2):
    tn, tf, s2 = (np.ascontiguousarray(v, F32) for v in (tn, tf, s2))
    out = np.zeros((len(tn), 3), np.int32)
    assert lib.knn_i8_debug_fast(tn.ctypes.data, tf.ctypes.data, s2.ctypes.data, len(tn), out.ctypes.data) == 0
    return out[:, 0].astype(np.int64), out[:, 1].copy().view(F32), out[:, 2].astype(np.int64)


def quant_ref(x, s):
    with np.errstate(over="ignore"):
        return np.clip(np.rint(np.asarray(x, F32) / F32(s)), -127, 127).astype(np.int8)


def test_quantiser_matches_restatement(lib):
    rng = np.random.default_rng(5)
    for s in (F32(1.0 / 127.0), F32(0.0078125), F32(3.7e-3), F32(41.0), F32(2.0 ** -30)):
        x = (rng.uniform(-1.3, 1.3, 20000) * 127.0 * float(s)).astype(F32)
        got = quant(lib, x, s)
        assert np.array_equal(got, quant_ref(x, s))
        assert got.min() >= -127
    # exact midpoints tie to even (s a power of two: (n + 1/2) s is exact)
    s = F32(0.0078125)
    n = np.arange(-130, 131)
    mid = ((n + 0.5) * float(s)).astype(F32)
    want = np.clip(np.where((n % 2) == 0, n, n + 1), -127, 127)
    assert np.array_equal(quant(lib, mid, s).astype(np.int64), want)
    # +-max, past the range, zeros, subnormals, infinities
    edge = np.array([127 * float(s), -127 * float(s), 1e3, -1e3, 3.4e38, -3.4e38, 0.0, -0.0, 1e-45, -1e-45, 1e-39,
                     np.inf, -np.inf], F32)
    assert np.array_equal(quant(lib, edge, s), np.array([127, -127, 127, -127, 127, -127, 0, 0, 0, 0, 0, 127, -127]))
    assert quant(lib, np.array([np.nan], F32), s)[0] == -127  # defined; such a call leaves the GEMM form anyway


def _triples(rng, n):
    s = np.exp(rng.uniform(np.log(1e-6), np.log(50.0), n)).astype(F32)
    s2 = (F32(2.0) * s * s).astype(F32)
    # tn up to d 127^2 s^2 = 64516 s2 ... (d = 128: tn / s2 <= 1,032,256)
    tn = (s2.astype(np.float64) * rng.uniform(0, 1.04e6, n)).astype(F32)
    tf = (tn.astype(np.float64) * rng.uniform(-1.5, 1.5, n)).astype(F32)
    return tn, tf, s2


def test_fast_threshold_has_no_false_negative_exact(lib):
    """For every integer a: -s2 a <= tf  =>  a >= ti.  Checked at the boundary integers around
    -tf / s2 in exact arithmetic (a smaller a fails the premise a fortiori)."""
    rng = np.random.default_rng(7)
    tn, tf, s2 = _triples(rng, 4000)
    # boundary cases: tf = 0, tf an exact multiple of s2, tiny and huge ratios
    tf[:50] = 0.0
    tf[50:100] = (s2[50:100] * rng.integers(-2000, 2000, 50)).astype(F32)
    s2[100:120] = F32(2.0 ** -70)
    tf[120:140] = (s2[120:140].astype(np.float64) * -2.0 ** 30.5).astype(F32)
    tf[140:160] = (s2[140:160].astype(np.float64) * 2.0 ** 30.5).astype(F32)
    _, _, ti = fast(lib, tn, tf, s2)
    for i in range(len(tf)):
        x = -Fraction(float(tf[i])) / Fraction(float(s2[i]))  # a passes the float test iff a >= x
        amin = -(-x.numerator // x.denominator)                # ceil(x): the smallest passing integer
        # (a is an int32: below -2^31 the threshold is INT32_MIN, every accumulator passes)
        assert ti[i] <= max(amin, -2 ** 31), (i, float(tf[i]), float(s2[i]), int(ti[i]), amin)
        if abs(amin) < 2 ** 30:  # and it is not uselessly loose: within 2^-19 |x| + 3
            assert amin - ti[i] <= abs(x) * Fraction(1, 2 ** 19) + 3
    # infinities and NaN: nothing / everything passes
    inf = np.array([-np.inf, np.inf, np.nan, 0.0], F32)
    _, _, t2 = fast(lib, np.ones(4, F32), inf, np.full(4, 1e-4, F32))
    assert t2[0] == 2 ** 31 - 1 and t2[1] == -2 ** 31 and t2[2] == -2 ** 31
    assert -3 <= t2[3] <= 0


def test_norm_term_and_residual_exact(lib):
    rng = np.random.default_rng(8)
    tn, tf, s2 = _triples(rng, 4000)
    tn[:20] = 0.0
    nr, res, _ = fast(lib, tn, tf, s2)
    assert nr.min() >= 0 and nr.max() <= 2 ** 30
    for i in range(len(tn)):
        e = abs(Fraction(float(tn[i])) - Fraction(float(s2[i])) * int(nr[i]))
        assert e <= Fraction(float(res[i])), (i, float(tn[i]), float(s2[i]), int(nr[i]))
        # the term is the floor up to the division's rounding: the residual stays below ~s2
        assert Fraction(float(res[i])) <= Fraction(float(s2[i])) * Fraction(1001, 1000) + Fraction(float(tn[i])) / 2 ** 20 + Fraction(1, 2 ** 120)


def test_integer_test_is_superset_of_float_test(lib):
    """As the kernel composes them: accumulator a = p - n_r for the integer dot p; y* = tn - s2 p.
    With tf = tf0 + res rounded up, y* <= tf0 implies a >= ti."""
    rng = np.random.default_rng(9)
    tn, tf0, s2 = _triples(rng, 3000)
    nr, res, _ = fast(lib, tn, tf0, s2)
    tf = np.nextafter((tf0.astype(np.float64) + res.astype(np.float64) * (1 + 2.0 ** -20)).astype(F32), F32(np.inf))
    _, _, ti = fast(lib, tn, tf, s2)
    for i in range(len(tn)):
        # integer dots around the float test's boundary (tn - tf0) / s2, and the extremes
        pb = (Fraction(float(tn[i])) - Fraction(float(tf0[i]))) / Fraction(float(s2[i]))
        c = pb.numerator // pb.denominator
        for p in (c - 2, c - 1, c, c + 1, c + 2, -2064512, 2064512, 0):
            y = Fraction(float(tn[i])) - Fraction(float(s2[i])) * p
            if y <= Fraction(float(tf0[i])):
                assert p - int(nr[i]) >= ti[i], (i, p)


def _rho_holds(lib, q, t, s):
    nq_, nt_ = quant(lib, q, s).astype(np.float64).reshape(q.shape), quant(lib, t, s).astype(np.float64).reshape(t.shape)
    s64 = float(s)
    rq, rt = s64 * nq_, s64 * nt_
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    lhs = np.abs(2.0 * ((q64 * t64).sum(1) - (rq * rt).sum(1)))
    nrm = lambda v: np.sqrt((v * v).sum(1))
    rho = 2.0 * (nrm(q64) * nrm(t64 - rt) + nrm(q64 - rq) * nrm(rt))
    assert np.all(lhs <= rho * (1 + 1e-12) + 1e-300)
    return lhs, rho


def test_rho_bounds_the_operand_rounding(lib):
    rng = np.random.default_rng(10)
    d, n = 128, 2000
    t = rng.uniform(-1, 1, (n, d)).astype(F32)
    s = F32(np.abs(t).max() / F32(127.0))
    q = rng.uniform(-1, 1, (n, d)).astype(F32)
    _rho_holds(lib, q, t, s)
    _rho_holds(lib, (4.0 * q).astype(F32), t, s)  # saturating queries
    # residuals aligned with their element's sign: every |element| just below a grid midpoint
    g = rng.integers(0, 126, (n, d)) + 0.499
    sg = np.where(rng.random((n, d)) < 0.5, -1.0, 1.0)
    ta = (sg * g * float(s)).astype(F32)
    ta[0, 0] = 127 * float(s)  # the same scale
    qa = (np.where(rng.random((n, d)) < 0.5, -1.0, 1.0) * (rng.integers(0, 126, (n, d)) + 0.499) * float(s)).astype(F32)
    lhs, rho = _rho_holds(lib, qa, ta, s)
    _rho_holds(lib, ta[::-1].copy(), ta, s)
    # the bound is not vacuous on the worst rows: within a factor of the aligned error
    _, rho2 = _rho_holds(lib, ta, ta, s)
    assert np.all(rho2 > 0)
