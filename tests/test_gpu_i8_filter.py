"""GPU checks of the int8 filter operand class (KNN_ALGO_GEMM_I8, Context(algo="gemm_i8");
DESIGN.md "int8 filter operands"): fp32 rows quantised to int8 for the candidate filter only, the
exact fp32 rescore unchanged -- so every output must equal the direct form's bit for bit.

  * the MFMA probe: v_mfma_i32_32x32x32_i8 over the filter's lane map sums exact integer dots;
  * parity (indices, distance bits, predictions) against the direct form on every query and the
    C oracle on a sample, at d = 128, k in {1, 10, 16, 17, 32}, both queries-per-wave shapes, on
    uniform / clustered / aligned-residual / duplicate / saturating / planted inputs, with tails on
    both axes, and on a shape whose query tiles are cut into many pieces (list exchange);
  * eligibility (non-finite rows, an outlier's scale), the operand cache and the scale rebuild.

Every parity case asserts stats()["filter_element"] == "i8": the form under test really ran.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, C = 128, 10
KINDS = ["uniform", "clustered", "aligned", "ties", "saturate", "saturate_mild", "planted"]
_data = {}
_ref = {}


def _inputs(knn, oracle, nt, nq, kind):
    """(train, labels, test) device tensors of one (shape, kind), built once."""
    import torch
    key = (nt, nq, kind)
    if key in _data:
        return _data[key]
    dev = "cuda:0"
    rng = np.random.default_rng(nt + 31 * nq + 7 * KINDS.index(kind))
    gen_kind = 2 if kind == "clustered" else 0
    c = knn.Context(0)
    try:
        train = torch.empty((nt, D), dtype=torch.float32, device=dev)
        labels = torch.empty(nt, dtype=torch.int32, device=dev)
        test = torch.empty((nq, D), dtype=torch.float32, device=dev)
        c.generate(train, labels, 0, D, gen_kind, 17, 0, C)
        c.generate(test, None, 0, D, gen_kind, 17, 1, C)
        torch.cuda.synchronize()
    finally:
        c.close()
    if kind == "aligned":
        # every element just below a midpoint of the int8 grid of step 1/127 (one element pins
        # the scale): all residuals have their element's sign, the certificate's worst rows
        s = 1.0 / 127.0
        def rows(n):
            sg = np.where(rng.random((n, D)) < 0.5, -1.0, 1.0)
            return (sg * (rng.integers(0, 126, (n, D)) + 0.499) * s).astype(np.float32)
        t = rows(nt)
        t[0, 0] = 1.0
        train = torch.from_numpy(t).to(dev)
        test = torch.from_numpy(rows(nq)).to(dev)
    elif kind == "ties":
        # duplicate train rows (equal distances: ties go to the smaller index) and queries that
        # are train rows (distance 0), some of them duplicated ones
        t = train.cpu().numpy()
        h = nt // 3
        t[h:h + 4000] = t[:4000]
        t[nt - 300:] = t[100:400]
        q = test.cpu().numpy()
        q[::3] = t[rng.integers(0, nt, len(q[::3]))]
        q[1::7] = t[rng.integers(0, 4000, len(q[1::7]))]
        train, test = torch.from_numpy(t).to(dev), torch.from_numpy(q).to(dev)
    elif kind == "saturate":
        test = test * 4.0  # outside the train range: the query operand saturates at +-127
    elif kind == "saturate_mild":
        # a few per cent of the query elements just past the train range: their residual is of the
        # order of the quantisation's own, so the int8 filter itself prunes (no fallback)
        test = test * 1.05
    elif kind == "planted":
        # near neighbours of the first queries planted at every place of a barrier group (eight
        # 32-row tiles or four 64-row ones: rows 0 .. 255 of a group), in the first group, a
        # middle one and the train set's last rows (the tail tile)
        t = train.cpu().numpy()
        q = test.cpu().numpy()
        places = [32 * p + o for p in range(8) for o in (0, 5, 31)]
        rows = places + [256 * (nt // 512) + r for r in places] + [nt - 1 - r for r in range(40)]
        for i, r in enumerate(rows):
            qi = i % 37
            t[r] = q[qi] + rng.uniform(-1e-3, 1e-3, D).astype(np.float32) * (1 + i % 5)
        train = torch.from_numpy(t).to(dev)
    _data[key] = (train, labels, test)
    return _data[key]


def _run(ctx, train, labels, test, k):
    import torch
    nq = test.shape[0]
    p = torch.empty(nq, dtype=torch.int32, device=test.device)
    dd = torch.empty((nq, k), dtype=torch.float32, device=test.device)
    ii = torch.empty((nq, k), dtype=torch.int32, device=test.device)
    ctx.predict_device(train, labels, test, k, C, p, dist=dd, idx=ii)
    torch.cuda.synchronize()
    return p.cpu().numpy(), dd.cpu().numpy().view(np.uint32), ii.cpu().numpy()


def _reference(knn, oracle, nt, nq, kind, k):
    """The direct form on every query (checked against the C oracle on a sample), once."""
    key = (nt, nq, kind, k)
    if key not in _ref:
        train, labels, test = _inputs(knn, oracle, nt, nq, kind)
        c = knn.Context(0, algo="direct")
        try:
            ref = _run(c, train, labels, test, k)
        finally:
            c.close()
        qs = np.unique(np.concatenate([np.arange(0, 4), np.linspace(0, nq - 1, 5).astype(np.int64)]))
        bad, op, od, oi = oracle.knn(train.cpu().numpy(), labels.cpu().numpy(), test.cpu().numpy()[qs], k, C)
        assert bad == 0
        assert np.array_equal(oi, ref[2][qs]) and np.array_equal(od.view(np.uint32), ref[1][qs])
        assert np.array_equal(op, ref[0][qs])
        _ref[key] = ref
    return _ref[key]


def _check_parity(knn, oracle, monkeypatch, nt, nq, kind, k, qg):
    monkeypatch.setenv("KNN_FUSED_QG", qg)  # snapshot at knn_create: both queries-per-wave shapes
    train, labels, test = _inputs(knn, oracle, nt, nq, kind)
    ref = _reference(knn, oracle, nt, nq, kind, k)
    c = knn.Context(0, algo="gemm_i8", profile=2)
    try:
        got = _run(c, train, labels, test, k)
        st = c.stats()
    finally:
        c.close()
    assert st["filter_element"] == "i8" and st["fused_norm"], st
    assert st["filter_operands"] == "bf16 rounded", st  # the class's code, unchanged
    assert st["queries_per_wave"] == 32 * int(qg), st
    assert np.array_equal(got[2], ref[2])
    assert np.array_equal(got[1], ref[1])
    assert np.array_equal(got[0], ref[0])
    if kind == "uniform":
        # the exact-scan fallback must not stand in for a broken filter
        assert st["fallback_queries"] == 0, st
    # candidates per query below the list's capacity: 64 * KNN_RESCORE_CAPW entries times 8 for
    # query sets this small (run_gemm cuts their few query tiles into up to 32 pieces, each with
    # its own threshold warm-up, and gives them the 8x list).  Saturating queries are the
    # exception by construction: their measured residual is of the order of the distances.
    if kind != "saturate":
        assert st["candidates"] / nq < 8 * 2048, st
    if kind == "saturate_mild":
        assert st["fallback_queries"] <= nq // 64, st
    return st


@pytest.mark.parametrize("qg", ["1", "2"])
@pytest.mark.parametrize("k", [1, 10, 16, 17, 32])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nt,nq", [(65_536, 1024), (16_447, 517)])
def test_i8_parity(knn, oracle, monkeypatch, nt, nq, kind, k, qg):
    _check_parity(knn, oracle, monkeypatch, nt, nq, kind, k, qg)


@pytest.mark.parametrize("qg", ["1", "2"])
@pytest.mark.parametrize("kind", KINDS)
def test_i8_parity_many_pieces(knn, oracle, monkeypatch, kind, qg):
    """262,144 x 300: one or two query tiles cut into many pieces (threshold and list exchange)."""
    st = _check_parity(knn, oracle, monkeypatch, 262_144, 300, kind, 10, qg)
    assert st["train_segments"] > 1, st


def test_mfma_probe_i8(knn):
    """The filter's own chain and lane map at K = 128: every one of the 32 x 32 sums is the
    integer dot product, on random and on all-+-127 operands."""
    import torch
    rng = np.random.default_rng(3)
    c = knn.Context(0)
    try:
        cases = [(rng.integers(-127, 128, (32, 128)), rng.integers(-127, 128, (32, 128))),
                 (np.full((32, 128), 127), np.full((32, 128), 127)),
                 (np.full((32, 128), -127), np.full((32, 128), 127)),
                 (np.where(rng.random((32, 128)) < 0.5, -127, 127), np.where(rng.random((32, 128)) < 0.5, -127, 127)),
                 (np.arange(32 * 128).reshape(32, 128) % 255 - 127, (np.arange(32 * 128).reshape(32, 128) * 7) % 255 - 127)]
        for a, b in cases:
            ta = torch.from_numpy(a.astype(np.int8)).cuda()
            tb = torch.from_numpy(b.astype(np.int8)).cuda()
            out = c.mfma_probe_i8(ta, tb).cpu().numpy()
            assert np.array_equal(out.astype(np.int64), a.astype(np.int64) @ b.astype(np.int64).T)
    finally:
        c.close()


def _pair(knn, algo, train, labels, test, k, **kw):
    c = knn.Context(0, algo=algo, **kw)
    try:
        return _run(c, train, labels, test, k), c.stats()
    finally:
        c.close()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_nonfinite_train_runs_bf16(knn, oracle):
    """Non-finite train elements: the int8 class has no scale for them; the call runs the bf16
    operands (whose norm check sends it to the exact path) and equals the direct form."""
    nt, nq, k = 65_536, 1024, 10
    train, labels, test = _inputs(knn, oracle, nt, nq, "uniform")
    t2 = train.clone()
    t2[5, 3] = float("nan")
    t2[40_000, 0] = float("inf")
    got, st = _pair(knn, "gemm_i8", t2, labels, test, k)
    assert st["filter_element"] == "bf16", st
    ref, _ = _pair(knn, "direct", t2, labels, test, k)
    assert _same(got, ref)


def test_nonfinite_queries_forced_i8(knn, oracle):
    """Non-finite query elements with int8 forced: such a query has no finite distance, so the
    call ends in KNN_ERANGE like the direct form's (main.cpp:47 never lists a row for it); the
    query norms' range check sends the call to the exact path, and every other query's outputs
    equal the direct form's."""
    import torch
    nt, nq, k = 65_536, 1024, 10
    train, labels, test = _inputs(knn, oracle, nt, nq, "uniform")
    q2 = test.clone()
    bad = [3, 500, 1023]
    q2[3, 7] = float("nan")
    q2[500, 0] = float("inf")
    q2[1023, 127] = float("-inf")
    out = {}
    for algo in ("gemm_i8", "direct"):
        c = knn.Context(0, algo=algo)
        try:
            p = torch.zeros(nq, dtype=torch.int32, device=q2.device)
            dd = torch.zeros((nq, k), dtype=torch.float32, device=q2.device)
            ii = torch.zeros((nq, k), dtype=torch.int32, device=q2.device)
            with pytest.raises(knn.KnnError) as e:
                c.predict_device(train, labels, q2, k, C, p, dist=dd, idx=ii)
            assert e.value.status == knn.KNN_ERANGE
            torch.cuda.synchronize()
            out[algo] = (p.cpu().numpy(), dd.cpu().numpy().view(np.uint32), ii.cpu().numpy())
        finally:
            c.close()
    ok = np.setdiff1d(np.arange(nq), bad)
    assert all(np.array_equal(x[ok], y[ok]) for x, y in zip(out["gemm_i8"], out["direct"]))
    assert _same(tuple(x[ok] for x in out["direct"]), tuple(x[ok] for x in _reference(knn, oracle, nt, nq, "uniform", k)))


def test_outlier_scale_stays_exact(knn, oracle):
    """One train element of 1e4 among unit-range rows sets the scale: nearly every element
    quantises to 0 and the filter keeps almost nothing out -- results are exact all the same
    (overflowing queries finish on the exact scan)."""
    nt, nq, k = 65_536, 1024, 10
    train, labels, test = _inputs(knn, oracle, nt, nq, "uniform")
    t2 = train.clone()
    t2[1234, 5] = 1e4
    got, st = _pair(knn, "gemm_i8", t2, labels, test, k)
    ref, _ = _pair(knn, "direct", t2, labels, test, k)
    assert _same(got, ref)


def test_auto_takes_i8_on_unit_range_rows(knn, oracle):
    """AUTO at a filter size (d = 128, k <= 32, fp32): the int8 form, under the class's code."""
    nt, nq, k = 65_536, 1024, 10
    train, labels, test = _inputs(knn, oracle, nt, nq, "uniform")
    got, st = _pair(knn, "auto", train, labels, test, k, cache_train=True)
    assert st["filter_element"] == "i8" and st["filter_operands"] == "bf16 rounded", st
    assert st["fallback_queries"] == 0, st
    assert _same(got, _reference(knn, oracle, nt, nq, "uniform", k))


def test_auto_outlier_scale_runs_bf16(knn, oracle):
    """One train element of 1e4 among unit-range rows: the int8 residual is far above the bf16
    one (E8 > R Ebf), AUTO keeps to the bf16 operands."""
    nt, nq, k = 65_536, 1024, 10
    train, labels, test = _inputs(knn, oracle, nt, nq, "uniform")
    t2 = train.clone()
    t2[1234, 5] = 1e4
    got, st = _pair(knn, "auto", t2, labels, test, k, cache_train=True)
    # (the bf16 pass's own tile term sees the outlier too: AUTO may end in its split re-run,
    # whose operands are bf16 all the same)
    assert st["filter_element"] == "bf16", st
    ref, _ = _pair(knn, "direct", t2, labels, test, k)
    assert _same(got, ref)


def test_auto_nonfinite_train_runs_bf16(knn, oracle):
    nt, nq, k = 65_536, 1024, 10
    train, labels, test = _inputs(knn, oracle, nt, nq, "uniform")
    t2 = train.clone()
    t2[9, 100] = float("-inf")
    t2[60_000, 1] = float("nan")
    got, st = _pair(knn, "auto", t2, labels, test, k, cache_train=True)
    assert st["filter_element"] == "bf16", st
    ref, _ = _pair(knn, "direct", t2, labels, test, k)
    assert _same(got, ref)


def test_auto_without_train_cache_keeps_bf16(knn, oracle):
    """A context that keeps no train operands has nowhere to keep the scale or the demotion mark:
    AUTO runs the bf16 operands there, on every call -- on unit-range rows and on the rows that
    overflow the int8 lists alike (the x8 hook set: no int8 pass to repeat).  Equal bits."""
    nt, nq, k = 65_536, 8192, 10
    train, labels, test = _inputs(knn, oracle, nt, nq, "aligned")
    ref = _reference(knn, oracle, nt, nq, "aligned", k)
    c = knn.Context(0, algo="auto")
    try:
        c._set_i8_coarsen(8)
        for _ in range(3):
            got = _run(c, train, labels, test, k)
            st = c.stats()
            assert st["filter_element"] == "bf16" and not st["rerun_split"], st
            assert st["fallback_queries"] == 0, st
            assert _same(got, ref)
    finally:
        c.close()
    tr2, lab2, te2 = _inputs(knn, oracle, 65_536, 1024, "uniform")
    got, st = _pair(knn, "auto", tr2, lab2, te2, k)
    assert st["filter_element"] == "bf16", st
    assert _same(got, _reference(knn, oracle, 65_536, 1024, "uniform", k))


def test_auto_demotes_a_misjudged_train_set(knn, oracle):
    """The aligned-residual rows at the forced x8 step on a caching AUTO context: the lists of
    2048 entries overflow, more than 1/64 of the queries finish on the exact scan -- once.  The
    train set is marked, and the next call runs the bf16 operands.  Equal bits both times."""
    nt, nq, k = 65_536, 8192, 10
    train, labels, test = _inputs(knn, oracle, nt, nq, "aligned")
    ref = _reference(knn, oracle, nt, nq, "aligned", k)
    c = knn.Context(0, algo="auto", cache_train=True)
    try:
        c._set_i8_coarsen(8)
        a = _run(c, train, labels, test, k)
        st = c.stats()
        # (past 1/16 of the queries AUTO re-runs the call with the split operands on the spot and
        # reports that pass; either way the int8 pass overflowed)
        assert st["rerun_split"] or (st["filter_element"] == "i8" and st["fallback_queries"] > nq // 64), st
        assert _same(a, ref)
        b = _run(c, train, labels, test, k)
        st = c.stats()
        assert st["filter_element"] == "bf16", st
        assert _same(b, ref)
    finally:
        c.close()


def test_coarser_step_stays_exact(knn, oracle):
    """The test hook's coarser steps (x2, x4, x8): wider certificates, the same bits."""
    nt, nq, k = 65_536, 1024, 10
    train, labels, test = _inputs(knn, oracle, nt, nq, "aligned")
    ref = _reference(knn, oracle, nt, nq, "aligned", k)
    c = knn.Context(0, algo="gemm_i8", profile=2)
    try:
        for mul in (1, 2, 4, 8):
            c._set_i8_coarsen(mul)
            got = _run(c, train, labels, test, k)
            st = c.stats()
            assert st["filter_element"] == "i8", st
            assert _same(got, ref)
    finally:
        c.close()


def test_operand_cache_and_scale_rebuild(knn, oracle):
    """A second call on a caching context takes the train operands and the scale from the cache
    and gives the same bits; changed train contents rebuild both."""
    import torch
    nt, nq, k = 65_536, 1024, 10
    train, labels, test = _inputs(knn, oracle, nt, nq, "uniform")
    tr = train.clone()
    c = knn.Context(0, algo="gemm_i8", cache_train=True)
    try:
        a = _run(c, tr, labels, test, k)
        assert not c.stats()["train_operands_cached"] and c.stats()["filter_element"] == "i8"
        b = _run(c, tr, labels, test, k)
        st = c.stats()
        assert st["train_operands_cached"] and st["filter_element"] == "i8", st
        assert _same(a, b) and _same(a, _reference(knn, oracle, nt, nq, "uniform", k))
        # new contents, a much larger range: the scale of the old rows would saturate them all
        tr.mul_(16.0)
        tr[7, 7] = 50.0
        torch.cuda.synchronize()
        got = _run(c, tr, labels, test, k)
        st = c.stats()
        assert not st["train_operands_cached"] and st["filter_element"] == "i8", st
        ref, _ = _pair(knn, "direct", tr, labels, test, k)
        assert _same(got, ref)
        # and the bf16 form on the same context and rows keeps its own operands apart
        d = knn.Context(0, algo="gemm_bf16", cache_train=True)
        try:
            assert _same(_run(d, tr, labels, test, k), ref)
            assert d.stats()["filter_element"] == "bf16"
        finally:
            d.close()
    finally:
        c.close()
