"""GPU checks of the MFMA form of the radius pass (k_radius_gemm) behind knn_radius_count_device and
knn_radius_fill_device and everything built on them.

Bar: exact equality everywhere, floats compared as uint32 bits.  The yardstick is the numpy
restatement of test_radius_cpu.py on the float32 distance matrix of metric_distances; the inputs
are metric_set's, the thresholds radius_thresholds' (entries of the matrix: every non-zero one has
a pair with D == thr inside the certificate band).  Contexts are algo="gemm_bf16" (the MFMA form at
any size) unless a test says otherwise, and every call asserts the form that ran
(stats()["radius_form"]).
"""
import ctypes

import numpy as np
import pytest

from test_gpu_strided_rows import Strided, _layout, _packed
from test_metric_cpu import EUCLIDEAN, FLT_MAX, MANHATTAN, bits, metric_distances, metric_reference, metric_set
from test_radius_cpu import (count_vote_reference, radius_reference, radius_regress_reference, radius_thresholds,
                             radius_vote_reference)
from test_radius_mfma_cpu import (MFMA_DIMS, MFMA_SHAPES, aligned_rows, bf16_set, radius_floors, rewritten_rows,
                                  routing_set, special_set, special_thresholds, strided_set)

pytestmark = pytest.mark.gpu

C = 10
OUTLIER = -7


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def _np(t):
    return None if t is None else t.cpu().numpy()


def _qlabels(nq):
    return np.random.default_rng(nq).integers(0, C, size=nq).astype(np.int32)


@pytest.fixture(scope="module")
def ctx(knn):
    c = knn.Context(0, algo="gemm_bf16", profile=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def direct(knn):
    c = knn.Context(0, algo="direct", profile=1)
    yield c
    c.close()


_sets = {}


def _set(oracle, d, nt, nq, kind):
    """(tr, tl, te, D, [(thr, reference)]) of one input set, made once."""
    key = (d, nt, nq, kind)
    if key not in _sets:
        tr, tl, te = aligned_rows(d, nt, nq) if kind == "aligned" else metric_set(oracle, kind, nt, nq, d)
        D = metric_distances(tr, te, EUCLIDEAN)
        refs = [(thr, radius_reference(tr, te, thr, EUCLIDEAN, labels=tl, C=C, D=D)) for thr in radius_thresholds(D)]
        _sets[key] = (tr, tl, te, D, refs)
    return _sets[key]


def _run(ctx, d_tr, d_tl, d_te, thr, form="mfma", ql=None, self_base=None, d=None):
    """The count pass with every output, then the fill with distances: numpy arrays, and the exact
    evaluations each pass reports (profile = 2 contexts; 0 otherwise)."""
    count, pred, correct, cc, off = ctx.radius_count_device(
        d_tr, d_tl, d_te, threshold=thr, num_classes=C, query_labels=None if ql is None else _dev(ql),
        self_base=self_base, outlier_label=OUTLIER, class_counts=True, offsets=True, d=d)
    st = ctx.stats()
    assert st["radius_form"] == form, st
    ex_count = st["radius_exact_pairs"]
    idx, dist = ctx.radius_fill_device(d_tr, d_te, off, threshold=thr, self_base=self_base, d=d)
    st = ctx.stats()
    assert st["radius_form"] == form, st
    return (_np(count), _np(pred), _np(correct), _np(cc), _np(off), _np(idx), _np(dist)), ex_count, st["radius_exact_pairs"]


def _assert_matches(got, ref, ql, what):
    count, pred, correct, cc, off, idx, dist = got
    rcount, roff, ridx, rdist, rcc = ref
    assert np.array_equal(count, rcount), f"{what}: count"
    assert np.array_equal(cc, rcc), f"{what}: class counts"
    rpred = count_vote_reference(rcc, OUTLIER)
    assert np.array_equal(pred, rpred), f"{what}: pred"
    if ql is not None:
        assert correct.dtype == np.int64 and correct[0] == (rpred == ql).sum(), f"{what}: correct"
    assert off.dtype == np.int64 and np.array_equal(off, roff), f"{what}: offsets"
    assert idx.dtype == np.int32 and np.array_equal(idx, ridx), f"{what}: idx"
    assert np.array_equal(bits(dist), bits(rdist)), f"{what}: dist bits"


def _same(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)


# 1
@pytest.mark.parametrize("d,nt,nq,kind", MFMA_SHAPES)
def test_mfma_shapes(ctx, oracle, d, nt, nq, kind):
    tr, tl, te, D, refs = _set(oracle, d, nt, nq, kind)
    ql = _qlabels(nq)
    d_tr, d_tl, d_te = _dev(tr), _dev(tl), _dev(te)
    for thr, ref in refs:
        got, ex_count, ex_fill = _run(ctx, d_tr, d_tl, d_te, float(thr), ql=ql)
        _assert_matches(got, ref, ql, f"thr={thr!r}")
        total = int(ref[1][-1])
        print(f"d={d} nt={nt} nq={nq} {kind} thr={float(thr):.6g}: exact pairs {ex_count} of {nq * nt} in the count, "
              f"{ex_fill} in the fill of {total}")
        # a filter, not a kernel that evaluates everything: at most twice the CPU model's cap
        assert 1 <= ex_count <= 0.10 * nq * nt, (thr, ex_count)
        assert ex_fill >= total, (thr, ex_fill, total)
    assert ctx.stage_times().keys() >= {"radius_norms", "radius_operands", "radius_fill"}


# 2
@pytest.mark.parametrize("d", [64, 256])
def test_mfma_every_pair_and_distance_bits(ctx, oracle, d):
    nt, nq = 65, 9
    tr, tl, te = metric_set(oracle, "grid" if d == 64 else "float", nt, nq, d)
    off, idx, dist = ctx.radius_neighbors_device(_dev(tr), _dev(te), threshold=3.0e38)
    assert ctx.stats()["radius_form"] == "mfma"
    assert np.array_equal(_np(off), np.arange(nq + 1) * nt) and np.array_equal(_np(idx), np.tile(np.arange(nt), nq))
    want = np.array([[oracle.lib.oracle_distance(oracle.p(te[q]), oracle.p(tr[t]), d) for t in range(nt)]
                     for q in range(nq)], np.float32)
    assert np.array_equal(bits(_np(dist).reshape(nq, nt)), bits(want))


# 3
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("splits", [1, 3, 7, 32])
def test_mfma_segments(knn, oracle, splits, d):
    tr, tl, te, D, refs = _set(oracle, d, 4096, 257, "float")
    ql = _qlabels(len(te))
    d_tr, d_tl, d_te = _dev(tr), _dev(tl), _dev(te)
    c = knn.Context(0, algo="gemm_bf16", train_splits=splits)
    try:
        for thr, ref in refs:
            got, _, _ = _run(c, d_tr, d_tl, d_te, float(thr), ql=ql)
            assert c.stats()["train_segments"] == splits
            _assert_matches(got, ref, ql, f"splits={splits} thr={thr!r}")
    finally:
        c.close()


# 4
@pytest.mark.parametrize("d", [64, 256])
def test_mfma_bf16_rows(ctx, oracle, d):
    import torch
    tr, tl, te = bf16_set(oracle, d)
    nq = len(te)
    b_tr, b_te = _dev(tr).to(torch.bfloat16), _dev(te).to(torch.bfloat16)
    assert torch.equal(b_tr.to(torch.float32).cpu(), torch.from_numpy(tr))   # bf16-exact values
    D = metric_distances(tr, te, EUCLIDEAN)
    ql = _qlabels(nq)
    for thr in radius_thresholds(D):
        got, _, _ = _run(ctx, b_tr, _dev(tl), b_te, float(thr), ql=ql)
        _assert_matches(got, radius_reference(tr, te, thr, EUCLIDEAN, labels=tl, C=C, D=D), ql, f"bf16 thr={thr!r}")


# 5
@pytest.mark.parametrize("d", MFMA_DIMS)
def test_mfma_worst_case_rounding(ctx, oracle, d):
    tr, tl, te, D, refs = _set(oracle, d, 1000, 33, "aligned")
    d_tr, d_tl, d_te = _dev(tr), _dev(tl), _dev(te)
    for thr, ref in refs:
        got, _, _ = _run(ctx, d_tr, d_tl, d_te, float(thr))
        _assert_matches(got, ref, None, f"aligned thr={thr!r}")


# 6
@pytest.mark.parametrize("case", ["nan_train", "inf_query", "huge_norm", "scaled"])
def test_mfma_special_values(ctx, case):
    tr, tl, te = special_set(case)
    form = "mfma" if case == "scaled" else "unsafe"
    if case == "huge_norm":
        assert (tr[::7].astype(np.float64) ** 2).sum(axis=1).min() >= 2.0 ** 125
    D = metric_distances(tr, te, EUCLIDEAN)
    thrs = special_thresholds(D)
    if case == "scaled":
        assert 0 < thrs[1] < thrs[2] < np.finfo(np.float32).tiny        # subnormal thresholds
    d_tr, d_tl, d_te = _dev(tr), _dev(tl), _dev(te)
    for thr in thrs:
        ref = radius_reference(tr, te, thr, EUCLIDEAN, labels=tl, C=C, D=D)
        got, _, _ = _run(ctx, d_tr, d_tl, d_te, float(thr), form=form)
        _assert_matches(got, ref, None, f"{case} thr={thr!r}")


# 7
def test_mfma_self_base_and_loo(ctx, oracle):
    tr, tl, _ = metric_set(oracle, "grid", 1000, 9, 64)              # duplicated rows
    d_tr, d_tl = _dev(tr), _dev(tl)
    D = metric_distances(tr, tr, EUCLIDEAN)
    for thr in (np.float32(0.0), radius_thresholds(D)[2]):
        ref = radius_reference(tr, tr, thr, EUCLIDEAN, self_base=0, labels=tl, C=C, D=D)
        got, _, _ = _run(ctx, d_tr, d_tl, d_tr, float(thr), ql=tl, self_base=0)
        _assert_matches(got, ref, tl, f"loo thr={thr!r}")
        off, idx = got[4], got[5]
        for q in range(len(tr)):
            seg = idx[off[q]:off[q + 1]]
            assert q not in seg
            copies = np.nonzero((tr == tr[q]).all(axis=1))[0]
            assert set(copies) - {q} <= set(seg)                    # equal copies of the row stay
        pred, _, count, correct = ctx.radius_loo_device(d_tr, d_tl, threshold=float(thr), num_classes=C,
                                                        outlier_label=OUTLIER)
        assert ctx.stats()["radius_form"] == "mfma"
        assert np.array_equal(_np(pred), got[1]) and np.array_equal(_np(count), got[0])
        assert _np(correct)[0] == got[2][0]
    # a window of queries further up: self rows 100 + q
    ref = radius_reference(tr, tr[100:357], 0.0, EUCLIDEAN, self_base=100, labels=tl, C=C)
    got, _, _ = _run(ctx, d_tr, d_tl, d_tr[100:357], 0.0, self_base=100)
    _assert_matches(got, ref, None, "loo window")


# 8
def test_mfma_consumers_equal_direct(ctx, direct, oracle):
    tr, tl, te, D, refs = _set(oracle, 128, 1000, 257, "float")
    targets = np.random.default_rng(77).standard_normal(len(tr)).astype(np.float32)
    ql = _qlabels(len(te))
    d_tr, d_tl, d_te, d_y, d_ql = _dev(tr), _dev(tl), _dev(te), _dev(targets), _dev(ql)
    for thr, ref in refs:
        rcount, roff, ridx, rdist, _ = ref
        for w, wk in (("uniform", 0), ("distance", 1)):
            out = {}
            for name, c in (("mfma", ctx), ("direct", direct)):
                # (the vote / regression calls behind the passes leave the passes' form readable)
                pred, scores, count, correct = c.radius_predict_device(
                    d_tr, d_tl, d_te, threshold=float(thr), num_classes=C, weights=w, outlier_label=OUTLIER,
                    query_labels=d_ql)
                assert c.stats()["radius_form"] == name
                reg, rc = c.radius_regress_device(d_tr, d_y, d_te, threshold=float(thr), weights=w)
                assert c.stats()["radius_form"] == name
                out[name] = [_np(pred), _np(scores), _np(count), _np(correct), _np(reg), _np(rc)]
            _same(out["mfma"], out["direct"])
            rpred, _ = radius_vote_reference(roff, ridx, rdist, tl, C, wk, EUCLIDEAN, OUTLIER)
            rreg = radius_regress_reference(roff, ridx, rdist, targets, wk, EUCLIDEAN)
            assert np.array_equal(out["mfma"][0], rpred) and np.array_equal(out["mfma"][2], rcount)
            ne = rcount > 0
            assert np.array_equal(bits(out["mfma"][4][ne]), bits(rreg[ne])) and np.isnan(out["mfma"][4][~ne]).all()


# 9
def test_mfma_strided_rows(ctx, oracle):
    tr, tl, te = strided_set(oracle)
    d, nq = tr.shape[1], len(te)
    (tld, tc0), (qld, qc0) = _layout("offset", d)
    T, Q = Strided(tr, tld, tc0, float("nan")), Strided(te, qld, qc0, float("nan"))
    D = metric_distances(tr, te, EUCLIDEAN)
    ql = _qlabels(nq)
    d_tl = _dev(tl)
    for thr in radius_thresholds(D)[1:]:
        ref = radius_reference(tr, te, thr, EUCLIDEAN, labels=tl, C=C, D=D)
        got, _, _ = _run(ctx, T.view, d_tl, Q.view, float(thr), ql=ql)
        _assert_matches(got, ref, ql, f"strided thr={thr!r}")
        packed, _, _ = _run(ctx, _packed(T.view), d_tl, _packed(Q.view), float(thr), ql=ql)
        _same(got, packed)
    assert T.intact() and Q.intact()


# 10
def test_mfma_errors(knn, ctx, oracle):
    import torch
    tr, tl, te, D, refs = _set(oracle, 64, 1000, 257, "float")
    nt, nq = len(tr), len(te)
    d_tr, d_tl, d_te = _dev(tr), _dev(tl), _dev(te)
    small, big = float(refs[2][0]), float(refs[3][0])
    # a label outside [0, C) on a row that is nobody's neighbour
    far = int(np.argmax(D.min(axis=0)))
    assert D[:, far].min() > small
    bad = tl.copy()
    bad[far] = C
    with pytest.raises(knn.KnnError) as e:
        ctx.radius_count_device(d_tr, _dev(bad), d_te, threshold=small, num_classes=C)
    assert e.value.status == knn.KNN_EINVAL and ctx.stats()["radius_form"] == "mfma"
    for thr in (float("nan"), -1.0e-30, float(FLT_MAX), float("inf")):
        with pytest.raises(knn.KnnError) as e:
            ctx.radius_count_device(d_tr, d_tl, d_te, threshold=thr, num_classes=C)
        assert e.value.status == knn.KNN_EINVAL, thr
    # offsets of another call: KNN_EINVAL, and the guard words around idx / dist are left alone
    off = ctx.radius_count_device(d_tr, None, d_te, threshold=small, offsets=True)[4]
    total = int(off[-1].item())
    G = 1024
    idx = torch.full((total + 2 * G,), -5, dtype=torch.int32, device=d_te.device)
    dist = torch.full((total + 2 * G,), -5.0, dtype=torch.float32, device=d_te.device)
    trd, ted = knn._device_dataset(d_tr, None, None), knn._device_dataset(d_te, None, None)
    torch.cuda.synchronize()                     # (the raw calls below run on the context's own stream)
    st = ctx.lib.knn_radius_fill_device(ctx.h, ctypes.byref(trd), ctypes.byref(ted), big, -1, off.data_ptr(),
                                        idx[G:].data_ptr(), dist[G:].data_ptr(), None)
    assert st == knn.KNN_EINVAL and "offsets" in ctx.lib.knn_last_error(ctx.h).decode()
    for buf, v in ((idx, -5), (dist, -5.0)):
        assert (buf[:G] == v).all() and (buf[G + total:] == v).all()
    _, roff, ridx, _, _ = refs[3][1]
    h_off, h_idx = _np(off), _np(idx[G:G + total])
    for q in range(nq):
        seg = h_idx[h_off[q]:h_off[q + 1]]
        assert set(seg[seg != -5]) <= set(ridx[roff[q]:roff[q + 1]])
    # the right threshold on the same buffers
    st = ctx.lib.knn_radius_fill_device(ctx.h, ctypes.byref(trd), ctypes.byref(ted), small, -1, off.data_ptr(),
                                        idx[G:].data_ptr(), dist[G:].data_ptr(), None)
    assert st == knn.KNN_OK
    assert np.array_equal(_np(idx[G:G + total]), refs[2][1][2])
    assert np.array_equal(bits(_np(dist[G:G + total])), bits(refs[2][1][3]))
    assert (idx[:G] == -5).all() and (idx[G + total:] == -5).all()


# 11
@pytest.mark.parametrize("splits", [0, 3])
def test_mfma_cross_form_fill(knn, oracle, splits):
    """Offsets from one form's count, lists from the other form's fill: the same lists both ways."""
    tr, tl, te, D, refs = _set(oracle, 64, 4096, 257, "float")
    d_tr, d_te = _dev(tr), _dev(te)
    a = knn.Context(0, algo="gemm_bf16", train_splits=splits)
    b = knn.Context(0, algo="direct", train_splits=splits)
    try:
        for thr, ref in refs[1:]:
            for cnt, fill, form in ((a, b, "direct"), (b, a, "mfma")):
                off = cnt.radius_count_device(d_tr, None, d_te, threshold=float(thr), offsets=True)[4]
                idx, dist = fill.radius_fill_device(d_tr, d_te, off, threshold=float(thr))
                assert fill.stats()["radius_form"] == form
                assert np.array_equal(_np(off), ref[1]) and np.array_equal(_np(idx), ref[2])
                assert np.array_equal(bits(_np(dist)), bits(ref[3]))
    finally:
        a.close()
        b.close()


# 12
def test_mfma_train_cache(knn, oracle):
    import torch
    tr, tl, te, D, refs = _set(oracle, 64, 1000, 257, "float")
    thr, ref = refs[2]
    d_tr, d_tl, d_te = _dev(tr), _dev(tl), _dev(te)
    c = knn.Context(0, algo="gemm_bf16", cache_train=True)
    try:
        for call in range(2):
            got, _, _ = _run(c, d_tr, d_tl, d_te, float(thr))
            _assert_matches(got, ref, None, f"call {call}")
            assert c.stats()["train_operands_cached"]              # (the fill after the count)
            count = c.radius_count_device(d_tr, None, d_te, threshold=float(thr))[0]
            assert c.stats()["train_operands_cached"] and np.array_equal(_np(count), ref[0])
        # a GEMM top-k call between two radius calls: all three right
        k = 5
        pred = torch.empty(len(te), dtype=torch.int32, device=d_te.device)
        kd = torch.empty((len(te), k), dtype=torch.float32, device=d_te.device)
        ki = torch.empty((len(te), k), dtype=torch.int32, device=d_te.device)
        c.predict_device(d_tr, d_tl, d_te, k, C, pred, kd, ki)
        assert c.stats()["fused_norm"]
        rd, ri = metric_reference(tr, te, k, EUCLIDEAN)
        assert np.array_equal(_np(ki), ri) and np.array_equal(bits(_np(kd)), bits(rd))
        got, _, _ = _run(c, d_tr, d_tl, d_te, float(thr))
        _assert_matches(got, ref, None, "after top-k")
        c.predict_device(d_tr, d_tl, d_te, k, C, pred, kd, ki)
        assert np.array_equal(_np(ki), ri) and np.array_equal(bits(_np(kd)), bits(rd))
        # an in-place write to train rows: the results follow the new rows
        d_tr[:400] = d_tr[600:1000]
        tr2 = rewritten_rows(tr)
        count, _, _, _, off = c.radius_count_device(d_tr, None, d_te, threshold=float(thr), offsets=True)
        assert not c.stats()["train_operands_cached"]
        ref2 = radius_reference(tr2, te, thr, EUCLIDEAN)
        assert not np.array_equal(ref2[0], ref[0])
        idx, dist = c.radius_fill_device(d_tr, d_te, off, threshold=float(thr))
        assert np.array_equal(_np(count), ref2[0]) and np.array_equal(_np(idx), ref2[2])
        assert np.array_equal(bits(_np(dist)), bits(ref2[3]))
    finally:
        c.close()


# 13
def test_mfma_routing(knn, direct, oracle):
    rows, queries = radius_floors(knn)
    d = 64
    tr, tl, te, thr = routing_set(oracle, rows, queries, d)
    thr = float(thr)
    d_tr, d_tl, d_te = _dev(tr), _dev(tl), _dev(te)
    auto = knn.Context(0, algo="auto")
    try:
        want, _, _ = _run(direct, d_tr, d_tl, d_te, thr, form="direct")
        assert want[0].sum() > 0
        got, _, _ = _run(auto, d_tr, d_tl, d_te, thr, form="mfma")
        _same(got, want)
        # one 64-row tile below the row floor, and one query below the query floor
        below, _, _ = _run(direct, d_tr[:rows - 64], d_tl[:rows - 64], d_te, thr, form="direct")
        got, _, _ = _run(auto, d_tr[:rows - 64], d_tl[:rows - 64], d_te, thr, form="direct")
        _same(got, below)
        if queries > 1:
            got, _, _ = _run(auto, d_tr, d_tl, d_te[:queries - 1], thr, form="direct")
            _same(got[:1], [want[0][:queries - 1]])
    finally:
        auto.close()
    # a non-Euclidean context never takes the MFMA form (and a GEMM algo refuses such a metric)
    man = knn.Context(0, algo="auto", metric="manhattan")
    try:
        Dm = metric_distances(tr[:4096], te[:33], MANHATTAN)
        tm = radius_thresholds(Dm)[2]
        count = man.radius_count_device(d_tr[:4096], None, d_te[:33], threshold=float(tm))[0]
        assert man.stats()["radius_form"] == "direct"
        assert np.array_equal(_np(count), radius_reference(tr[:4096], te[:33], tm, MANHATTAN, D=Dm)[0])
        count = man.radius_count_device(d_tr, None, d_te, threshold=float(tm))[0]
        assert man.stats()["radius_form"] == "direct" and knn.radius_policy("manhattan", "f32", d, rows, queries) == "direct"
    finally:
        man.close()
    with pytest.raises(knn.KnnError) as e:
        knn.Context(0, algo="gemm_bf16", metric="manhattan")
    assert e.value.status == knn.KNN_EINVAL


# 14
def test_mfma_same_call_twice(ctx, oracle):
    tr, tl, te, D, refs = _set(oracle, 64, 4096, 257, "float")
    d_tr, d_tl, d_te = _dev(tr), _dev(tl), _dev(te)
    thr = float(refs[3][0])
    runs = [_run(ctx, d_tr, d_tl, d_te, thr)[0] for _ in range(2)]
    _same(runs[0], runs[1])
