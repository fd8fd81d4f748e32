"""The MFMA candidate filter at any row width up to 4,096 features, on the GPU.

Rows narrower than one of the filter's tile widths are padded with zero columns to 64 / 128 / 256
(k_tn_rows, k_round_rows); rows wider than 256 run the K-chunked kernel k_gemm_wide in chunks of
128 features.  Every case asserts indices, distance bits and predictions equal to the oracle, and
that the filter ran on the operands knn_filter_policy names: filter_operands, train_segments,
filter_width, filter_chunks (these stats are what a library without the feature fails).  On the
generator's kind-0 rows no query may need the exact fallback (a filter that overflows every list
would otherwise hide behind it).  The host side is tests/test_filter_width_cpu.py.
"""
import math
import os
import zlib

import numpy as np
import pytest

from conftest import DATA, DATASETS, GOLDEN, KS, golden_manifest, golden_topk, pred_sha
from test_filter_width_cpu import NQ, NT, rows, width_rule

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C = 10
_ref = {}


def _oracle(oracle, tr, tl, te, k, key=None):
    if key is None or key not in _ref:
        bad, pred, dist, idx = oracle.knn(tr, tl, te, k, C)
        assert bad == 0
        if key is None:
            return pred, dist.view(np.uint32), idx
        _ref[key] = (pred, dist.view(np.uint32), idx)
    return _ref[key]


def _dev_rows(x, bf16=False):
    """Device rows of the narrowest 16-byte-aligned pitch (zero pad columns, never read: the call
    passes the true d)."""
    import torch
    n, d = x.shape
    unit = 8 if bf16 else 4
    t = torch.zeros((n, (d + unit - 1) // unit * unit), dtype=torch.bfloat16 if bf16 else torch.float32)
    t[:, :d] = torch.from_numpy(np.ascontiguousarray(x))
    return t.to(DEV)[:, :d]


def _predict(ctx, train, labels, test, k):
    import torch
    nq = test.shape[0]
    pred = torch.empty(nq, dtype=torch.int32, device=DEV)
    dist = torch.empty((nq, k), dtype=torch.float32, device=DEV)
    idx = torch.empty((nq, k), dtype=torch.int32, device=DEV)
    ctx.predict_device(train, labels, test, k, C, pred, dist, idx)
    torch.cuda.synchronize()
    return (pred.cpu().numpy(), dist.cpu().numpy().view(np.uint32), idx.cpu().numpy()), ctx.stats()


def _same(got, want, what):
    assert np.array_equal(got[2], want[2]), f"{what}: indices"
    assert np.array_equal(got[1], want[1]), f"{what}: distance bits"
    assert np.array_equal(got[0], want[0]), f"{what}: predictions"


def _ran(knn, st, d, k, nt, nq, what, bf16=False, algo="gemm_bf16", clean=True, unsafe=False, may_fall_back=False):
    """The filter ran, at the policy's width and chunk count, on the expected operands."""
    form, width = knn.filter_policy("bf16" if bf16 else "f32", d, k, nt, nq, algo)
    print(what, form, width, {n: st[n] for n in ("filter_operands", "train_segments", "filter_width", "filter_chunks",
                                                 "fused_norm", "fallback_queries", "rerun_split")})
    assert width == width_rule(d) and form == ("wide" if d > 256 else form)
    assert st["filter_operands"] == ("bf16" if bf16 else "bf16 rounded"), (what, st)
    assert st["train_segments"] >= 1, (what, st)
    assert st["filter_width"] == width, (what, st)
    assert (st["filter_chunks"] == 1) if d <= 256 else (st["filter_chunks"] == width // 128 > 1), (what, st)
    assert st["fused_norm"] == (form == "fused"), (what, st)
    if clean:
        assert st["fallback_queries"] == 0 and not st["rerun_split"], (what, st)
    elif not unsafe and not may_fall_back:
        assert st["fallback_queries"] < nq, (what, st)


def _case(knn, oracle, tr, tl, te, ks, what, d=None, bf16=False, algo="gemm_bf16", clean=True, key=None, unsafe=False,
          may_fall_back=False, **kw):
    import torch
    d = tr.shape[1] if d is None else d
    ttr, tte = _dev_rows(tr, bf16), _dev_rows(te, bf16)
    lab = torch.from_numpy(np.ascontiguousarray(tl)).to(DEV)
    ctx = knn.Context(0, algo=algo, **kw)
    try:
        for k in ks:
            want = _oracle(oracle, tr, tl, te, k, None if key is None else key + (k,))
            got, st = _predict(ctx, ttr, lab, tte, k)
            _same(got, want, f"{what} k={k}")
            _ran(knn, st, d, k, len(tr), len(te), f"{what} k={k}", bf16, algo, clean, unsafe, may_fall_back)
            if unsafe:
                assert st["fallback_queries"] == len(te), st
    finally:
        ctx.close()


# 1. padded widths -------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 33, 70, 100, 129, 255])
def test_padded_widths(knn, oracle, d):
    tr, tl = rows(oracle, NT, d, 0)
    te, _ = rows(oracle, NQ, d, 1)
    _case(knn, oracle, tr, tl, te, (1, 10, 32, 100), f"padded d={d}", key=("small", d))


def test_padded_several_pieces(knn, oracle):
    tr, tl = rows(oracle, 70_001, 100, 0)
    te, _ = rows(oracle, 129, 100, 1)
    _case(knn, oracle, tr, tl, te, (3,), "padded 70,001 x 129")


def test_padded_nonfused_rounded_operands(knn, oracle):
    """d = 255, k = 128: no fused kernel at 256-wide operands with heaps this large; k_round_rows
    builds the padded operands of k_gemm_filter."""
    tr, tl = rows(oracle, NT, 255, 0)
    te, _ = rows(oracle, NQ, 255, 1)
    assert knn.filter_policy("f32", 255, 128, NT, NQ, "gemm_bf16") == ("filter", 256)
    _case(knn, oracle, tr, tl, te, (128,), "padded d=255 k=128", key=("small", 255))


# 2. the reference's data ----------------------------------------------------------------------------
@pytest.mark.parametrize("ds", DATASETS)
def test_arff_unpadded(knn, ds):
    """The ARFF pairs as they are (d = 7 and 11, no host-side padding) through gemm_bf16 at every k
    of the golden manifest."""
    tf, tl, Ct = knn.read_arff(os.path.join(DATA, f"{ds}-train.arff"))
    qf, ql, _ = knn.read_arff(os.path.join(DATA, f"{ds}-test.arff"))
    d = tf.shape[1]
    assert d in (7, 11)
    ctx = knn.Context(0, algo="gemm_bf16")
    try:
        for k in KS:
            pred, dist, idx = ctx.predict(tf, tl, qf, k, Ct, topk=True)
            st = ctx.stats()
            assert st["filter_operands"] == "bf16 rounded" and st["train_segments"] >= 1, st
            assert st["filter_width"] == 64 and st["filter_chunks"] == 1, st
            assert pred_sha(pred) == golden_manifest()[f"{ds}_k{k}"]["sha256"], (ds, k)
            if os.path.exists(os.path.join(GOLDEN, f"topk_{ds}_k{k}.bin")):
                gd, gi = golden_topk(ds, k)
                assert np.array_equal(idx, gi) and np.array_equal(dist.view(np.uint32), gd), (ds, k)
    finally:
        ctx.close()


# 3. wide widths -------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [260, 384, 512, 770, 1024])
def test_wide_widths(knn, oracle, d):
    tr, tl = rows(oracle, NT, d, 0)
    te, _ = rows(oracle, NQ, d, 1)
    _case(knn, oracle, tr, tl, te, (1, 10, 33, 128), f"wide d={d}", key=("small", d))


def test_wide_4096(knn, oracle):
    tr, tl = rows(oracle, 4_099, 4096, 0)
    te, _ = rows(oracle, 129, 4096, 1)
    _case(knn, oracle, tr, tl, te, (10,), "wide d=4096")


def test_wide_segments(knn, oracle):
    """train_splits = 3: three segments per query tile exchange thresholds through gthr."""
    import torch
    tr, tl = rows(oracle, 8_192, 1536, 0)
    te, _ = rows(oracle, 64, 1536, 1)
    ctx = knn.Context(0, algo="gemm_bf16", train_splits=3)
    try:
        got, st = _predict(ctx, _dev_rows(tr), torch.from_numpy(tl).to(DEV), _dev_rows(te), 10)
    finally:
        ctx.close()
    _same(got, _oracle(oracle, tr, tl, te, 10), "segments")
    _ran(knn, st, 1536, 10, 8_192, 64, "segments")
    assert st["train_segments"] == 3, st


# 4. signal only in the tail, in the last chunk, in the first chunk -------------------------------
def _signal_rows(n, d, lo, hi, flat, seed):
    """Rows equal to `flat` everywhere but in features [lo, hi), which are uniform in [0, 1)."""
    rng = np.random.default_rng(seed)
    x = np.full((n, d), flat, np.float32)
    x[:, lo:hi] = rng.random((n, hi - lo), dtype=np.float32)
    return x


@pytest.mark.parametrize("d,lo,hi,flat,falls_back", [
    (100, 96, 100, 0.125, False),       # the last d % 16 features (the scalar tail of the last quad's k-step)
    (770, 768, 770, 2.0 ** -6, False),  # the last d % 16 features = the last chunk's only columns
    (1024, 896, 1024, 0.0625, False),   # the last chunk only
    (770, 0, 128, 0.0625, False),       # the first chunk only
    (1024, 0, 128, 0.25, False),        # the first chunk only, larger equal values elsewhere
    # the first k-step only, large equal values elsewhere: built to fall back -- the band grows with
    # the norms, coef (qn + tn) = 1664 u x 10,752 = 1.07 against distances of 2.7 +- 0.8, so the lists
    # overflow and the exact scan answers
    (100, 0, 16, 8.0, True),
])
def test_signal_in_one_part(knn, oracle, d, lo, hi, flat, falls_back):
    """A dropped tail or a skipped chunk leaves every row at the same filter value: the bounds would
    be invalid and the neighbours wrong."""
    tr = _signal_rows(4_099, d, lo, hi, flat, 7 * d + lo)
    te = _signal_rows(129, d, lo, hi, flat, 7 * d + lo + 1)
    tl = (np.arange(4_099) % C).astype(np.int32)
    _case(knn, oracle, tr, tl, te, (1, 10), f"signal [{lo}, {hi}) of d={d}", clean=False, may_fall_back=falls_back)


# 5. adversarial rounding ------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [100, 768])
def test_aligned_rounding(knn, oracle, d):
    """Every element just below a bf16 rounding midpoint: every operand rounding error has the same
    sign (test_rounded_filter_aligned_rounding's construction)."""
    rng = np.random.default_rng(31 + d)

    def mk(n):
        s = 2.0 ** rng.integers(0, 4, size=(n, d))
        m = 1.0 + rng.integers(0, 128, size=(n, d)) / 128.0
        delta = rng.integers(1, 64, size=(n, d)) * 2.0 ** -22
        return ((m + 2.0 ** -8 - delta) * s).astype(np.float32)

    tr, te = mk(8_200), mk(96)
    tl = rng.integers(0, C, size=8_200).astype(np.int32)
    _case(knn, oracle, tr, tl, te, (1, 10, 33), f"aligned rounding d={d}", clean=False)


def test_duplicates_and_ties(knn, oracle):
    base, _ = rows(oracle, 300, 384, 2)
    rep = np.minimum(56, 1 + np.arange(300) % 60)
    tr = np.repeat(base, rep, axis=0)
    tl = (np.arange(len(tr)) % C).astype(np.int32)
    te = np.concatenate([base[:40], rows(oracle, 60, 384, 1)[0]])
    _case(knn, oracle, tr, tl, te, (1, 10, 57, 128), "duplicates d=384", clean=False)


def test_unsafe_norm_falls_back(knn, oracle):
    """One train row of norm >= 2^125: the filter is skipped (GEMM_UNSAFE), every query takes the exact
    fallback, results still bit-exact."""
    tr, tl = rows(oracle, 4_099, 384, 0)
    te, _ = rows(oracle, 129, 384, 1)
    tr = tr.copy()
    tr[1234, :] = np.float32(2.0 ** 59)        # 384 x 2^118 >= 2^125
    _case(knn, oracle, tr, tl, te, (10,), "unsafe norm d=384", clean=False, unsafe=True)


def test_nan_query(knn, oracle):
    """A NaN feature in two queries: no row ever passes their filter and they take the exact fallback,
    where no distance compares below the sentinel either -- the call reports KNN_ERANGE (fewer than k
    finite neighbours), as the direct form does, with every output written: all of them equal the
    direct form's, and every other query is the oracle's."""
    import torch
    tr, tl = rows(oracle, 4_099, 384, 0)
    te, _ = rows(oracle, 129, 384, 1)
    te = te.copy()
    te[5, 383] = np.nan
    te[77, 0] = np.nan
    ttr, tte, lab = _dev_rows(tr), _dev_rows(te), torch.from_numpy(tl).to(DEV)
    out = {}
    for algo in ("gemm_bf16", "direct"):
        ctx = knn.Context(0, algo=algo)
        try:
            pred = torch.zeros(129, dtype=torch.int32, device=DEV)
            dist = torch.zeros((129, 10), dtype=torch.float32, device=DEV)
            idx = torch.zeros((129, 10), dtype=torch.int32, device=DEV)
            with pytest.raises(knn.KnnError) as e:
                ctx.predict_device(ttr, lab, tte, 10, C, pred, dist, idx)
            assert e.value.status == knn.KNN_ERANGE, algo
            torch.cuda.synchronize()
            out[algo] = ((pred.cpu().numpy(), dist.cpu().numpy().view(np.uint32), idx.cpu().numpy()), ctx.stats())
        finally:
            ctx.close()
    got, st = out["gemm_bf16"]
    _same(got, out["direct"][0], "NaN query against the direct form")
    ok = np.setdiff1d(np.arange(129), [5, 77])
    _same(tuple(a[ok] for a in got), _oracle(oracle, tr, tl, te[ok], 10), "NaN query d=384")
    # (a call that ends in KNN_ERANGE does not add its pass to fallback_queries)
    _ran(knn, st, 384, 10, 4_099, 129, "NaN query d=384", clean=False)


# 6. strided, poisoned rows ----------------------------------------------------------------------------
def _view(x, ld, c0, poison, bf16=False, exact_end=False):
    """x inside a poisoned [n][ld] parent at column c0 (exact_end: storage of exactly (n - 1) ld + c0 + d
    elements, the view's last row ending the allocation)."""
    import torch
    n, d = x.shape
    dt = torch.bfloat16 if bf16 else torch.float32
    flat = torch.full(((n - 1) * ld + c0 + d if exact_end else n * ld,), poison, dtype=dt)
    v = torch.as_strided(flat, (n, d), (ld, 1), c0)
    v[:] = torch.from_numpy(np.ascontiguousarray(x))
    dev = flat.to(DEV)
    view = torch.as_strided(dev, (n, d), (ld, 1), c0)
    assert view.data_ptr() % 16 == 0 and (ld * flat.element_size()) % 16 == 0
    return view, dev, flat


@pytest.mark.parametrize("poison", [float("nan"), 3.0e38])
@pytest.mark.parametrize("d,bf16", [(70, False), (100, False), (384, False), (770, False), (100, True), (384, True)])
def test_strided_poisoned(knn, oracle, d, bf16, poison):
    import torch
    unit = 8 if bf16 else 4
    nt, nq = 4_099, 129
    tr, tl = rows(oracle, nt, d, 0, kind=1 if bf16 else 0)
    te, _ = rows(oracle, nq, d, 1, kind=1 if bf16 else 0)
    ld_t = (d // unit + 2) * unit
    ld_q = (d // unit + 5) * unit
    vt, dt_, ft = _view(tr, ld_t, 0, poison, bf16, exact_end=True)      # ends at (n - 1) ld + d
    vq, dq_, fq = _view(te, ld_q, 2 * unit, poison, bf16)
    lab = torch.from_numpy(tl).to(DEV)
    algo = "gemm" if bf16 else "gemm_bf16"
    ctx = knn.Context(0, algo=algo)
    try:
        for k in (10, 33):
            got, st = _predict(ctx, vt, lab, vq, k)
            _same(got, _oracle(oracle, tr, tl, te, k, ("strided", d, bf16, k)), f"strided d={d}")
            _ran(knn, st, d, k, nt, nq, f"strided d={d} bf16={bf16}", bf16, algo)
    finally:
        ctx.close()
    it = torch.int16 if bf16 else torch.int32
    assert torch.equal(dt_.cpu().view(it), ft.view(it)) and torch.equal(dq_.cpu().view(it), fq.view(it))


# 7. bf16 data -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [100, 512])
def test_bf16_data(knn, oracle, d):
    tr, tl = rows(oracle, NT, d, 0, kind=1)
    te, _ = rows(oracle, NQ, d, 1, kind=1)
    _case(knn, oracle, tr, tl, te, (10, 128), f"bf16 data d={d}", bf16=True, algo="gemm")


# 8. caches and contexts -----------------------------------------------------------------------------
def test_train_cache_across_widths(knn, oracle):
    """tprep / tpad keys keep the true d; the operand width is a function of it."""
    import torch
    sets = {}
    for d in (100, 384):
        tr, tl = rows(oracle, NT, d, 0)
        te, _ = rows(oracle, NQ, d, 1)
        sets[d] = (tr, tl, te, _dev_rows(tr), torch.from_numpy(tl).to(DEV), _dev_rows(te))
    ctx = knn.Context(0, algo="gemm_bf16", cache_train=True)
    try:
        for d, cached in ((100, False), (100, True), (384, False), (100, False), (100, True)):
            tr, tl, te, ttr, lab, tte = sets[d]
            got, st = _predict(ctx, ttr, lab, tte, 10)
            _same(got, _oracle(oracle, tr, tl, te, 10, ("small", d, 10)), f"cache d={d}")
            _ran(knn, st, d, 10, NT, NQ, f"cache d={d}")
            if d <= 256:   # (the fused filter's train operands are the cached ones)
                assert st["train_operands_cached"] == cached, (d, cached, st)
    finally:
        ctx.close()


@pytest.mark.parametrize("d", [96, 384])
def test_auto_above_floor(knn, oracle, d):
    """32,768 x 32,768 (> 10^9 pairs): AUTO takes the filter; 64 sampled queries against the oracle."""
    import torch
    n = 32_768
    ctx = knn.Context(0, algo="auto")
    try:
        train = torch.empty((n, d), dtype=torch.float32, device=DEV)
        labels = torch.empty(n, dtype=torch.int32, device=DEV)
        test = torch.empty((n, d), dtype=torch.float32, device=DEV)
        ctx.generate(train, labels, 0, d, 0, 3, 0, C)
        ctx.generate(test, None, 0, d, 0, 3, 1, C)
        got, st = _predict(ctx, train, labels, test, 10)
    finally:
        ctx.close()
    _ran(knn, st, d, 10, n, n, f"auto d={d}", algo="auto")
    tr, tl = oracle.gen(3, 0, 0, n, d)
    te, _ = oracle.gen(3, 1, 0, n, d)
    assert np.array_equal(train.cpu().numpy(), tr)
    qs = np.linspace(0, n - 1, 64).astype(np.int64)
    want = _oracle(oracle, tr, tl, te[qs], 10)
    _same(tuple(a[qs] for a in got), want, f"auto d={d}")


def test_auto_below_floor(knn, oracle):
    tr, tl = rows(oracle, NT, 100, 0)
    te, _ = rows(oracle, NQ, 100, 1)
    import torch
    ctx = knn.Context(0, algo="auto")
    try:
        got, st = _predict(ctx, _dev_rows(tr), torch.from_numpy(tl).to(DEV), _dev_rows(te), 10)
    finally:
        ctx.close()
    _same(got, _oracle(oracle, tr, tl, te, 10, ("small", 100, 10)), "auto below the floor")
    assert st["filter_operands"] is None and st["filter_width"] == 0 and st["filter_chunks"] == 0, st


# 9. list consumers ------------------------------------------------------------------------------------
def test_list_consumers(knn, oracle):
    """sweep, weighted vote and regression at d = 384 equal the same calls on a direct context."""
    import torch
    d = 384
    tr, tl = rows(oracle, NT, d, 0)
    te, _ = rows(oracle, NQ, d, 1)
    ttr, tte, lab = _dev_rows(tr), _dev_rows(te), torch.from_numpy(tl).to(DEV)
    targets = torch.from_numpy(np.sin(np.arange(NT, dtype=np.float32))).to(DEV)
    out = {}
    for algo in ("gemm_bf16", "direct"):
        ctx = knn.Context(0, algo=algo)
        try:
            pa, _ = ctx.sweep_device(ttr, lab, tte, 32, C)
            st = ctx.stats()
            pw, sc = ctx.predict_weighted_device(ttr, lab, tte, 10, C, weights="distance")
            rg = ctx.regress_device(ttr, targets, tte, 10)
            torch.cuda.synchronize()
            out[algo] = (pa.cpu().numpy(), pw.cpu().numpy(), sc.cpu().numpy().view(np.uint32), rg.cpu().numpy().view(np.uint32))
            if algo == "gemm_bf16":
                _ran(knn, st, d, 32, NT, NQ, "sweep d=384")
        finally:
            ctx.close()
    for a, b in zip(out["gemm_bf16"], out["direct"]):
        assert np.array_equal(a, b)


# 10. the hardware assumption at the wide kernel's chain lengths --------------------------------------
U = 2.0 ** -24


def _bf16(x):
    f = np.asarray(x, np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    bits = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    vals = (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return bits, vals


def _operands(case, K, rng):
    if case == "random":
        a = rng.uniform(-1, 1, (32, K))
        b = rng.uniform(-1, 1, (32, K))
    elif case == "cancel":
        a = rng.uniform(1, 2, (32, K)) * 2.0 ** rng.integers(10, 30, (32, K))
        b = rng.uniform(1, 2, (32, K)) * 2.0 ** rng.integers(10, 30, (32, K))
        a[:, 1::2] = a[:, 0::2]
        b[:, 1::2] = -b[:, 0::2]
        a[:, 0::16] = rng.uniform(-1, 1, (32, K // 16))
        b[:, 0::16] = rng.uniform(-1, 1, (32, K // 16))
    elif case == "mixed_exp":
        a = rng.uniform(-2, 2, (32, K)) * 2.0 ** rng.integers(-60, 60, (32, K))
        b = rng.uniform(-2, 2, (32, K)) * 2.0 ** rng.integers(-60, 60, (32, K))
    elif case == "subnormal":
        a = rng.uniform(-2, 2, (32, K)) * 2.0 ** -63
        b = rng.uniform(-2, 2, (32, K)) * 2.0 ** rng.integers(-70, -57, (32, K))
        a[:, ::5] *= 2.0 ** 40
    elif case == "same_sign":
        a = rng.uniform(0.5, 1, (32, K))
        b = rng.uniform(0.5, 1, (32, K))
    else:
        raise ValueError(case)
    return _bf16(a), _bf16(b)


@pytest.mark.parametrize("K", [1024, 4096])
@pytest.mark.parametrize("case", ["random", "cancel", "mixed_exp", "subnormal", "same_sign"])
def test_mfma_chain_bound_at_wide_lengths(knn, case, K):
    """|mfma - sum p_i| <= 2 u K sum |p_i| + K 2^-126 at the chain lengths of wide rows (one
    accumulator over K / 16 k-steps, as k_gemm_wide chains its chunks)."""
    import torch
    rng = np.random.default_rng(zlib.crc32(f"{case}-{K}".encode()))
    (ab, av), (bb, bv) = _operands(case, K, rng)
    ctx = knn.Context(0)
    try:
        ta = torch.from_numpy(ab.view(np.int16)).to(DEV).view(torch.bfloat16)
        tb = torch.from_numpy(bb.view(np.int16)).to(DEV).view(torch.bfloat16)
        got = ctx.mfma_probe_bf16(ta, tb).cpu().numpy().astype(np.float64)
    finally:
        ctx.close()
    worst = 0.0
    for i in range(32):
        for j in range(32):
            p = av[i] * bv[j]
            exact, mag = math.fsum(p), math.fsum(np.abs(p))
            err = abs(got[i, j] - exact)
            assert err <= 2 * U * K * mag + K * 2.0 ** -126, (case, K, i, j, got[i, j], exact, err)
            if mag > 0:
                worst = max(worst, err / (U * mag))
    print(f"[mfma bound] case={case} K={K}: max |err| / (u sum|p|) = {worst:.3f} (assumed <= {2 * K})")
