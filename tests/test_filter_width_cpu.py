"""The MFMA candidate filter at any row width up to 4,096 features: what the host decides.

No GPU: knn_filter_policy's rule table and binding, the operand widths, the operand rows the
padding kernels write (their host view, knn_debug_operand_rows, which runs operand_quad's
per-element branch for every quad: on the device a whole quad inside the row takes the float4 load
instead, a path only the GPU suites' bit-exact results cover), and a float64 model of the
certificate on zero-padded operands.  The GPU side is
tests/test_gpu_filter_width.py, which shares this file's input sets (rows()).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, REPO
from test_metric_cpu import EUCLIDEAN, metric_distances
from test_radius_mfma_cpu import band_model, rn_bf16

SEED = 53
NT, NQ = 16_447, 517          # the GPU tests' small sets: tails on both axes, 258 tiles, nt % 64 != 0
DS = (1, 31, 32, 63, 64, 65, 100, 128, 129, 255, 256, 257, 384, 385, 4096, 4097)
BIG = 1 << 20                 # rows and queries far above every floor


def rows(oracle, n, d, stream, kind=0):
    """The generator's [n][d] rows and labels of the filter-width tests (kind 0 fp32, 1 bf16-exact)."""
    return oracle.gen(SEED + d, stream, 0, n, d, kind=kind)


def width_rule(d):
    """The operand width of the bf16 operand classes: the smallest of 64, 128, 256 that holds d;
    above 256 the next multiple of 128 (k_gemm_wide's chunk); none above 4,096."""
    if d <= 256:
        return next(w for w in (64, 128, 256) if w >= d)
    return (d + 127) // 128 * 128 if d <= 4096 else 0


def form_rule(dp, k):
    """fused wherever k_gemm_fused has a shape: every k <= 128 at 64 and 128, k <= 121 at 256 (256
    LDS heaps of heap_stride(k) = (k + 6) & ~3 floats beside two 32-row buffers of 512-byte rows,
    34,816 bytes, within 160 KiB - 256: 124 floats fit, 128 do not); wide above 256."""
    if dp > 256:
        return "wide"
    return "filter" if dp == 256 and k > 121 else "fused"


def test_symbol_and_binding(knn):
    with open(os.path.join(REPO, "include", "knn_amd.h")) as f:
        src = f.read()
    assert re.search(r"\bint32_t\s+knn_filter_policy\s*\(\s*int32_t\s+dtype,\s*int32_t\s+d,\s*int32_t\s+k,\s*int64_t\s+n_train,"
                     r"\s*int64_t\s+n_query,\s*int32_t\s+algo,\s*int32_t\*\s*form,\s*int32_t\*\s*operand_width\s*\)", src)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG_DIR, "libknn_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT knn_filter_policy$", out, re.M)
    for kept in ("knn_radius_policy", "knn_fused_debug_image", "knn_fused_debug_plan"):
        assert re.search(rf"\bT {kept}$", out, re.M)
    lib = knn.load_library()
    assert lib.knn_filter_policy.argtypes is not None and callable(knn.filter_policy)
    assert lib.knn_version() == 3
    f, w = ctypes.c_int32(), ctypes.c_int32()
    assert lib.knn_filter_policy(0, 64, 10, 1, 1, 0, None, ctypes.byref(w)) == knn.KNN_EINVAL
    assert lib.knn_filter_policy(0, 64, 10, 1, 1, 0, ctypes.byref(f), None) == knn.KNN_EINVAL
    for bad in (("f32", 0, 10, 1, 1, 0), ("f32", 64, 0, 1, 1, 0), ("f32", 64, 10, -1, 1, 0), ("f32", 64, 10, 1, -1, 0),
                ("f32", 64, 10, 1, 1, 7), ("f32", 64, 10, 1, 1, -1)):
        with pytest.raises(knn.KnnError) as e:
            knn.filter_policy(*bad)
        assert e.value.status == knn.KNN_EINVAL
    assert lib.knn_filter_policy(2, 64, 10, 1, 1, 0, ctypes.byref(f), ctypes.byref(w)) == knn.KNN_EINVAL  # dtype


def test_forced_bf16_operands_any_width(knn):
    """gemm_bf16 (and gemm on bf16 data) take the filter at any d <= 4096 and any size."""
    for dtype, algos in (("f32", ("gemm_bf16",)), ("bf16", ("gemm_bf16", "gemm", "gemm_split", "gemm_i8"))):
        for algo in algos:
            for d in DS:
                for k in (1, 10, 104, 121, 122, 128):
                    for nt, nq in ((BIG, BIG), (128, 1), (16_447, 517)):
                        dp = width_rule(d)
                        want = (form_rule(dp, k), dp) if dp else ("direct", 0)
                        assert knn.filter_policy(dtype, d, k, nt, nq, algo) == want, (dtype, algo, d, k, nt, nq)
                assert knn.filter_policy(dtype, d, 129, BIG, BIG, algo) == ("direct", 0)      # k > 128
                assert knn.filter_policy(dtype, d, 10, 9, BIG, algo) == ("direct", 0)         # k > n_train


def test_operand_widths(knn):
    for d in range(1, 4200, 7):
        form, w = knn.filter_policy("f32", d, 10, BIG, BIG, "gemm_bf16")
        if d > 4096:
            assert (form, w) == ("direct", 0)
        elif d <= 256:
            assert w in (64, 128, 256) and w >= d and (w == 64 or w // 2 < d) and form == "fused"
        else:
            assert w % 128 == 0 and d <= w < d + 128 and form == "wide"
    # the three widths the filter had keep the form and width that ran before
    for d in (64, 128, 256):
        for dtype in ("f32", "bf16"):
            assert knn.filter_policy(dtype, d, 10, BIG, BIG, "gemm_bf16") == ("fused", d)
            assert knn.filter_policy(dtype, d, 10, BIG, BIG, "auto") == ("fused", d)
    assert knn.filter_policy("f32", 256, 128, BIG, BIG, "gemm_bf16") == ("filter", 256)


def test_direct_algos(knn):
    for dtype in ("f32", "bf16"):
        for d in DS:
            for algo in ("direct", "direct_scan"):
                for nt, nq in ((BIG, BIG), (1, 1)):
                    assert knn.filter_policy(dtype, d, 10, nt, nq, algo) == ("direct", 0)


def test_auto_floors(knn):
    """AUTO: d >= 32, n_train >= 8192 and >= 10^9 pairs at any width up to 4096; the 16,384-row rule
    (any query count) stays with 64 / 128 / 256."""
    for dtype in ("f32", "bf16"):
        for d in DS:
            dp = width_rule(d)
            can = dp > 0 and d >= 32
            took = lambda nt, nq: knn.filter_policy(dtype, d, 10, nt, nq, "auto")[0] != "direct"  # noqa: E731
            # both sides of the pair floor (8192 x 122,071 = 1,000,005,632 pairs; one query fewer is below)
            assert took(8192, 122_071) == can, (dtype, d)
            assert not took(8192, 122_070)
            assert took(32_768, 32_768) == can
            # both sides of the row floor
            assert not took(8191, 1 << 30)
            assert took(8192, 1 << 30) == can
            # the 16,384-row rule
            assert took(16_384, 1) == (d in (64, 128, 256))
            assert not took(16_383, 1)
            if can:
                form, w = knn.filter_policy(dtype, d, 10, 32_768, 32_768, "auto")
                assert w == dp and form == form_rule(dp, 10)
    assert knn.filter_policy("f32", 31, 10, BIG, BIG, "auto") == ("direct", 0)
    assert knn.filter_policy("f32", 4097, 10, BIG, BIG, "auto") == ("direct", 0)


def test_other_operand_classes(knn):
    """fp32 gemm and gemm_split multiply the caller's rows: d = 32 / 64 / 128 only, the non-fused
    filter; a forced gemm_i8 context takes the bf16 operands at any width (its own at d = 128 only --
    the form and width are the fused filter's either way)."""
    for d in DS:
        for algo in ("gemm", "gemm_split"):
            want = ("filter", d) if d in (32, 64, 128) else ("direct", 0)
            assert knn.filter_policy("f32", d, 10, BIG, BIG, algo) == want, (algo, d)
        dp = width_rule(d)
        want = (form_rule(dp, 10), dp) if dp else ("direct", 0)
        assert knn.filter_policy("f32", d, 10, BIG, BIG, "gemm_i8") == want, d


def _operand_rows(knn, x, d, dp, scale, bf16=False):
    lib = knn.load_library()
    lib.knn_debug_operand_rows.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_float, ctypes.c_void_p]
    lib.knn_debug_operand_rows.restype = ctypes.c_int
    out = np.full((len(x), dp), 0xdead, np.uint16)
    assert lib.knn_debug_operand_rows(x.ctypes.data, 1 if bf16 else 0, len(x), x.shape[1], d, dp, scale, out.ctypes.data) == 0
    return out


def _bf16_bits(x):
    return (rn_bf16(x).view(np.uint32) >> 16).astype(np.uint16)


@pytest.mark.parametrize("scale", [1.0, -2.0])
def test_operand_rows(knn, scale):
    """Operand rows: rn(scale x) in columns < d, zero bits from d on, whatever the pad columns of the
    caller's rows hold (NaN, 3e38); at dp == d, d % 4 == 0 exactly the rows the kernels wrote before
    (rn(scale x) of every element, pitch d)."""
    rng = np.random.default_rng(5)
    for d, ld in ((64, 64), (128, 132), (256, 256), (5, 8), (33, 36), (70, 72), (100, 104), (255, 256), (260, 264), (770, 772)):
        dp = width_rule(d)
        for poison in (np.nan, 3.0e38):
            x = np.full((9, ld), poison, np.float32)
            x[:, :d] = rng.standard_normal((9, d)).astype(np.float32) * 3
            want = np.zeros((9, dp), np.uint16)
            want[:, :d] = _bf16_bits(np.float32(scale) * x[:, :d])
            got = _operand_rows(knn, x, d, dp, scale)
            assert np.array_equal(got, want), (d, ld, poison)
            if d % 4 == 0:  # the unpadded operand of before: the same bytes at pitch d
                assert np.array_equal(_operand_rows(knn, x, d, d, scale), want[:, :d])
    # bf16 data: the bits themselves at scale 1
    for d, ld in ((100, 104), (384, 384), (250, 256)):
        dp = width_rule(d)
        xb = np.full((7, ld), 0x7fc0, np.uint16)                      # NaN pad columns
        xb[:, :d] = _bf16_bits(rng.standard_normal((7, d)).astype(np.float32))
        want = np.zeros((7, dp), np.uint16)
        want[:, :d] = xb[:, :d] if scale == 1.0 else _bf16_bits(np.float32(scale) * (xb[:, :d].astype(np.uint32) << 16).view(np.float32))
        assert np.array_equal(_operand_rows(knn, xb, d, dp, scale, bf16=True), want)
    # a buffer that ends at (n - 1) ld + d elements: the last row's tail is read by element
    d, ld, n = 70, 72, 3
    flat = rng.standard_normal((n - 1) * ld + d).astype(np.float32)
    lib = knn.load_library()
    out = np.zeros((n, 128), np.uint16)
    assert lib.knn_debug_operand_rows(flat.ctypes.data, 0, n, ld, d, 128, ctypes.c_float(scale), out.ctypes.data) == 0
    assert np.array_equal(out[n - 1, :d], _bf16_bits(np.float32(scale) * flat[(n - 1) * ld:]))


CERT_BLOCK = 96  # queries per block: the fp32 D of a block is computed a feature at a time on [block][nt] arrays


@pytest.mark.parametrize("d", [100, 384, 770])
def test_certificate_on_padded_operands(oracle, d):
    """L <= D <= U on every (query, train row) pair of the GPU tests' small sets, all 517 queries
    against all 16,447 rows, in blocks of queries: D the reference's fp32 direct form, the operands
    exactly rounded bf16 rows padded with zeros to dp, float64 products, and the header's formulas
    with the coefficient for dp.  d = 100 runs the fused filter (certificate_fused with the rounding
    term of the tile statistics, band_model on the padded rows); 384 and 770 the wide kernel, which
    speaks k_gemm_filter's certificate: Delta = coef (qn + tn) + eta, coef = (6 dp + 131840) u,
    eta = (8 dp + 8) 2^-125."""
    tr, _ = rows(oracle, NT, d, 0)
    te_all, _ = rows(oracle, NQ, d, 1)
    dp = width_rule(d)
    trp = np.zeros((NT, dp), np.float32)
    trp[:, :d] = tr
    rt = rn_bf16(trp).astype(np.float64)
    tn = (tr.astype(np.float64) ** 2).sum(axis=1)
    widest, slack, pairs = 0.0, np.inf, 0
    for q0 in range(0, NQ, CERT_BLOCK):
        te = te_all[q0:q0 + CERT_BLOCK]
        D = metric_distances(tr, te, EUCLIDEAN).astype(np.float64)
        tep = np.zeros((len(te), dp), np.float32)
        tep[:, :d] = te
        if dp <= 256:
            L, U = band_model(trp, tep)
        else:
            coef, eta = (6 * dp + 131840) * 2.0 ** -24, (8 * dp + 8) * 2.0 ** -125
            rq = rn_bf16(tep).astype(np.float64)
            qn = (te.astype(np.float64) ** 2).sum(axis=1)
            s = qn[:, None] + tn[None, :]
            G = s - 2.0 * (rq @ rt.T)
            dl = coef * s + eta
            L, U = G - dl, G + dl
        assert (L <= D).all() and (D <= U).all(), (d, q0)
        widest = max(widest, float(np.max(U - L)))
        slack = min(slack, float(np.min(D - L)), float(np.min(U - D)))
        pairs += D.size
    assert pairs == NQ * NT
    print(f"d={d} dp={dp}: {pairs} pairs, widest band {widest:.4g}, smallest slack {slack:.4g}")
