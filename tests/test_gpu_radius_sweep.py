"""GPU checks of the radius sweep (k_radius_sweep_tile, k_radius_sweep_finish, k_radius_vote_sweep;
include/knn_amd.h "Radius sweep") through every entry point: the counts, class counts, uniform
vote, correct and outlier sums of every threshold from one pass; threshold lists of every kind;
forced train segments; bf16 and strided rows; leave-one-out; query blocks and the row pitch; the
vote sweep on held lists; bad arguments; routing between the two forms of the pass; determinism.

Bar: exact equality everywhere, floats compared as uint32 bits -- against the numpy restatement of
test_radius_sweep_cpu.py (pinned there to scalar definitions) AND against R single-threshold calls
on an algo="direct" context.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_strided_rows import Strided, _layout
from test_metric_cpu import EUCLIDEAN, FLT_MAX, MANHATTAN, bits, metric_distances, metric_set
from test_radius_cpu import (INV_DIST, INV_SQDIST, METRIC_NAMES, METRICS, UNIFORM, WEIGHT_NAMES, radius_reference,
                             radius_thresholds)
from test_radius_mfma_cpu import (MFMA_SHAPES, aligned_rows, bf16_set, radius_floors, routing_set, special_set,
                                  special_thresholds, strided_set)
from test_radius_sweep_cpu import SWEEP_SHAPES, filter_lists, radius_sweep_reference, radius_vote_sweep_reference

pytestmark = pytest.mark.gpu

C = 10
OUTLIER = -7


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def _pad4(x):
    """Device rows are 16-byte aligned: zero columns up to a multiple of 4 (the call passes the
    true d, so they are never read as features)."""
    return np.pad(x, ((0, 0), (0, -x.shape[1] % 4)))


def _np(t):
    return None if t is None else t.cpu().numpy()


def _qlabels(nq, C=C):
    return np.random.default_rng(nq).integers(0, C, size=nq).astype(np.int32)


@pytest.fixture(scope="module")
def ctxs(knn):
    """Per metric: an AUTO context, the algo="direct" context the single-threshold calls run on,
    and (Euclidean) an algo="gemm_bf16" context, which takes the MFMA form at any size."""
    cs = {(m, a): knn.Context(0, algo=a, profile=1, metric=METRIC_NAMES[m]) for m in METRICS
          for a in ("auto", "direct")}
    cs[EUCLIDEAN, "gemm_bf16"] = knn.Context(0, algo="gemm_bf16", profile=2)
    yield cs
    for c in cs.values():
        c.close()


def _sweep(ctx, d_tr, d_tl, d_te, thr, d, ql=None, self_base=None, query_block=None, C=C):
    """radius_sweep_device with every output: numpy (count, cc, pred, correct, outliers)."""
    count, pred, correct, outliers, cc = ctx.radius_sweep_device(
        d_tr, d_tl, d_te, thresholds=thr, num_classes=C, query_labels=None if ql is None else _dev(ql),
        self_base=self_base, outlier_label=OUTLIER, class_counts=True, query_block=query_block, d=d)
    st = ctx.stage_times()
    assert "radius_sweep" in st and "radius_sweep_finish" in st and "radius_count" not in st, st
    return _np(count), _np(cc), _np(pred), _np(correct), _np(outliers)


def _singles(ctx, d_tr, d_tl, d_te, thr, d, ql=None, self_base=None, C=C):
    """The R single-threshold calls the sweep replaces, stacked like the sweep's outputs."""
    rows = [ctx.radius_count_device(d_tr, d_tl, d_te, threshold=float(t), num_classes=C,
                                    query_labels=None if ql is None else _dev(ql), self_base=self_base,
                                    outlier_label=OUTLIER, class_counts=True, d=d) for t in thr]
    count = np.stack([_np(r[0]) for r in rows])
    correct = None if ql is None else np.array([_np(r[2])[0] for r in rows], np.int64)
    return (count, np.stack([_np(r[3]) for r in rows]), np.stack([_np(r[1]) for r in rows]), correct,
            (count == 0).sum(axis=1).astype(np.int64))


def _assert_same(got, want, what):
    for name, g, w in zip(("count", "class_counts", "pred", "correct", "outliers"), got, want):
        if w is None:
            assert g is None, f"{what}: {name}"
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} {g.dtype} {g.shape}"
        assert np.array_equal(g, w), f"{what}: {name}"


def _check(ctxs, metric, algo, tr, tl, te, thr, d, ql=None, self_base=None, query_block=None, what="", D=None,
           d_tr=None, d_te=None):
    """One sweep against the restatement and against the direct context's single calls."""
    D = metric_distances(tr, te, metric) if D is None else D
    thr = np.float32(thr)
    d_tr = _dev(_pad4(tr)) if d_tr is None else d_tr
    d_te = _dev(_pad4(te)) if d_te is None else d_te
    d_tl = _dev(tl)
    got = _sweep(ctxs[metric, algo], d_tr, d_tl, d_te, thr, d, ql, self_base, query_block)
    _assert_same(got, radius_sweep_reference(D, thr, self_base, tl, C, OUTLIER, ql), f"{what} vs restatement")
    _assert_same(got, _singles(ctxs[metric, "direct"], d_tr, d_tl, d_te, thr, d, ql, self_base),
                 f"{what} vs single calls")
    return got


# 1. the direct form, three metrics
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,nt,nq,kind", SWEEP_SHAPES)
def test_sweep_shapes(ctxs, oracle, d, nt, nq, kind, metric):
    import torch
    tr, tl, te = metric_set(oracle, kind, nt, nq, d)
    D = metric_distances(tr, te, metric)
    thr = radius_thresholds(D)
    _check(ctxs, metric, "auto", tr, tl, te, thr, d, _qlabels(nq), what=f"f32 d={d}", D=D)
    assert ctxs[metric, "auto"].stats()["radius_form"] == "direct"


@pytest.mark.parametrize("metric", METRICS)
def test_sweep_bf16(ctxs, oracle, metric):
    import torch
    tr, tl, te = bf16_set(oracle, 72)
    b_tr, b_te = _dev(tr).to(torch.bfloat16), _dev(te).to(torch.bfloat16)
    assert torch.equal(b_tr.to(torch.float32).cpu(), torch.from_numpy(tr))   # bf16-exact values
    D = metric_distances(tr, te, metric)
    _check(ctxs, metric, "auto", tr, tl, te, radius_thresholds(D), 72, _qlabels(len(te)), what="bf16", D=D,
           d_tr=b_tr, d_te=b_te)


# 2. the MFMA form
@pytest.mark.parametrize("d,nt,nq,kind", MFMA_SHAPES + [(128, 4096, 257, "float")])
def test_sweep_mfma_shapes(ctxs, oracle, d, nt, nq, kind):
    tr, tl, te = metric_set(oracle, kind, nt, nq, d)
    D = metric_distances(tr, te, EUCLIDEAN)
    _check(ctxs, EUCLIDEAN, "gemm_bf16", tr, tl, te, radius_thresholds(D), d, _qlabels(nq), what=f"mfma d={d}", D=D)
    st = ctxs[EUCLIDEAN, "gemm_bf16"].stats()                        # (profile = 2)
    assert st["radius_form"] == "mfma"
    print(f"d={d} nt={nt} nq={nq} {kind}: {st['radius_exact_pairs']} exact pairs of {nt * nq}")
    assert st["radius_exact_pairs"] >= 1
    if kind == "float":
        assert st["radius_exact_pairs"] <= 0.10 * nt * nq


@pytest.mark.parametrize("case", ["bf16", "aligned", "scaled"])
def test_sweep_mfma_hard_rows(ctxs, oracle, case):
    """bf16 rows; rows whose operand rounding errors all have one sign; rows scaled by 2^-70, where
    every pair is undecided and the result must still be right."""
    import torch
    kw = {}
    if case == "bf16":
        tr, tl, te = bf16_set(oracle, 64)
        kw = dict(d_tr=_dev(tr).to(torch.bfloat16), d_te=_dev(te).to(torch.bfloat16))
    elif case == "aligned":
        tr, tl, te = aligned_rows(128)
    else:
        tr, tl, te = special_set(case)
    D = metric_distances(tr, te, EUCLIDEAN)
    thr = special_thresholds(D) if case == "scaled" else radius_thresholds(D)
    _check(ctxs, EUCLIDEAN, "gemm_bf16", tr, tl, te, thr, tr.shape[1], _qlabels(len(te)), what=case, D=D, **kw)
    st = ctxs[EUCLIDEAN, "gemm_bf16"].stats()
    assert st["radius_form"] == "mfma"
    if case == "scaled":
        assert st["radius_exact_pairs"] == D.size                    # every pair is in the band


# 3. unsafe norms: the direct sweep kernel behind the gate
@pytest.mark.parametrize("case", ["nan_train", "inf_query", "huge_norm"])
def test_sweep_unsafe_norms(ctxs, case):
    tr, tl, te = special_set(case)
    D = metric_distances(tr, te, EUCLIDEAN)
    _check(ctxs, EUCLIDEAN, "gemm_bf16", tr, tl, te, special_thresholds(D), tr.shape[1], _qlabels(len(te)), what=case,
           D=D)
    assert ctxs[EUCLIDEAN, "gemm_bf16"].stats()["radius_form"] == "unsafe"


# 4. threshold lists
@pytest.fixture(scope="module")
def list_set(oracle):
    tr, tl, te = metric_set(oracle, "float", 1000, 257, 11)
    return tr, tl, te, {m: metric_distances(tr, te, m) for m in METRICS}


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", ["one", "thirty_two", "all_equal", "zero", "every_pair"])
def test_sweep_threshold_lists(ctxs, list_set, kind, metric):
    tr, tl, te, Ds = list_set
    D = Ds[metric]
    flat = np.sort(D, axis=None)
    if kind == "one":
        thr = [radius_thresholds(D)[2]]
    elif kind == "thirty_two":
        # 32 sorted matrix entries up to the 0.5 quantile, every fourth one doubled
        pos = (np.linspace(0.0, 0.5, 24) * (flat.size - 1)).astype(np.int64)
        thr = np.sort(np.concatenate([flat[pos], flat[pos[::3]]]))
        assert len(thr) == 32 and (np.diff(thr) == 0).sum() >= 8
    elif kind == "all_equal":
        thr = [radius_thresholds(D)[2]] * 5
    elif kind == "zero":
        thr = [0.0]
    else:
        thr = [0.0, radius_thresholds(D)[1], 3.0e38]
    ql = _qlabels(len(te))
    got = _check(ctxs, metric, "auto", tr, tl, te, thr, 11, ql, what=kind, D=D)
    if kind == "one":
        # R = 1 is the single call
        single = ctxs[metric, "auto"].radius_count_device(_dev(_pad4(tr)), _dev(tl), _dev(_pad4(te)),
                                                          threshold=float(thr[0]), num_classes=C, d=11,
                                                          outlier_label=OUTLIER)
        assert np.array_equal(got[0][0], _np(single[0])) and np.array_equal(got[2][0], _np(single[1]))
    if kind == "all_equal":
        assert all(np.array_equal(got[0][0], got[0][r]) and np.array_equal(got[1][0], got[1][r]) for r in range(5))
    if kind == "every_pair":
        assert (got[0][2] == np.isfinite(D).sum(axis=1)).all() and got[4][2] == 0


# 5. forced segments
@pytest.mark.parametrize("algo", ["auto", "gemm_bf16"])
def test_sweep_segments(knn, ctxs, oracle, algo):
    tr, tl, te = metric_set(oracle, "float", 4096, 257, 128)
    D = metric_distances(tr, te, EUCLIDEAN)
    thr = np.float32(radius_thresholds(D))
    ql = _qlabels(257)
    ctx = knn.Context(0, algo=algo, profile=1, train_splits=3)
    try:
        got = _sweep(ctx, _dev(tr), _dev(tl), _dev(te), thr, 128, ql)
        assert ctx.stats()["train_segments"] == 3
        assert ctx.stats()["radius_form"] == ("mfma" if algo == "gemm_bf16" else "direct")
        _assert_same(got, radius_sweep_reference(D, thr, None, tl, C, OUTLIER, ql), f"splits=3 {algo}")
        _assert_same(got, _singles(ctxs[EUCLIDEAN, "direct"], _dev(tr), _dev(tl), _dev(te), thr, 128, ql),
                     f"splits=3 {algo} vs single calls")
    finally:
        ctx.close()


# 6. leave-one-out
@pytest.mark.parametrize("metric", METRICS)
def test_sweep_leave_one_out(knn, ctxs, oracle, metric):
    tr, tl, _ = metric_set(oracle, "grid", 1000, 9, 3)              # duplicated rows, many equal distances
    assert len(np.unique(tr, axis=0)) < len(tr)                      # a self row with an exact copy
    D = metric_distances(tr, tr, metric)
    thr = np.float32([0.0] + list(radius_thresholds(D)[2:]))
    got = _check(ctxs, metric, "auto", tr, tl, tr, thr, 3, tl, self_base=0, what="loo", D=D)
    ctx = ctxs[metric, "auto"]
    d_tr, d_tl = _dev(_pad4(tr)), _dev(tl)
    count, pred, correct, outliers = ctx.radius_sweep_loo_device(d_tr, d_tl, thresholds=thr, num_classes=C,
                                                                outlier_label=OUTLIER, d=3)
    assert np.array_equal(_np(count), got[0]) and np.array_equal(_np(pred), got[2])
    assert np.array_equal(_np(correct), got[3]) and np.array_equal(_np(outliers), got[4])
    # at thr = 0 a row's neighbours are its copies: the self row is out, they are in
    copies = np.array([(tr == tr[q]).all(axis=1).sum() - 1 for q in range(len(tr))])
    assert np.array_equal(got[0][0], copies) and copies.any()
    # a window of queries further up: self rows 100 + q
    _check(ctxs, metric, "auto", tr, tl, tr[100:357], thr, 3, None, self_base=100, what="loo window", D=D[100:357],
           d_tr=d_tr, d_te=d_tr[100:357])
    with pytest.raises(knn.KnnError) as e:
        ctx.radius_sweep_device(d_tr, d_tl, d_tr[:257], thresholds=thr, num_classes=C, self_base=1000 - 256, d=3)
    assert e.value.status == knn.KNN_EINVAL


# 7. strided rows
@pytest.mark.parametrize("metric,algo", [(m, "auto") for m in METRICS] + [(EUCLIDEAN, "gemm_bf16")])
def test_sweep_strided_rows(ctxs, oracle, metric, algo):
    """Rows inside a wider, NaN-poisoned parent ("offset" layout: train and query strides differ,
    both column offsets non-zero), the parent unchanged."""
    d = 64 if algo == "gemm_bf16" else 24
    tr, tl, te = strided_set(oracle, d)
    (tld, tc0), (qld, qc0) = _layout("offset", d)
    T, Q = Strided(tr, tld, tc0, float("nan")), Strided(te, qld, qc0, float("nan"))
    D = metric_distances(tr, te, metric)
    _check(ctxs, metric, algo, tr, tl, te, radius_thresholds(D), None, _qlabels(len(te)), what="strided", D=D,
           d_tr=T.view, d_te=Q.view)
    assert ctxs[metric, algo].stats()["radius_form"] == ("mfma" if algo == "gemm_bf16" else "direct")
    assert T.intact() and Q.intact()


# 8. query blocks
def test_sweep_query_blocks(knn, ctxs, list_set):
    import torch
    tr, tl, te, Ds = list_set
    D = Ds[EUCLIDEAN]
    thr = np.float32(radius_thresholds(D))
    ql = _qlabels(len(te))
    whole = _check(ctxs, EUCLIDEAN, "auto", tr, tl, te, thr, 11, ql, what="unblocked", D=D)
    ctx = ctxs[EUCLIDEAN, "auto"]
    d_tr, d_tl, d_te = _dev(_pad4(tr)), _dev(tl), _dev(_pad4(te))
    _assert_same(_sweep(ctx, d_tr, d_tl, d_te, thr, 11, ql, query_block=64), whole, "query_block=64")
    # leave-one-out in blocks: the self row of a block's query q is self_base + q of the whole call
    Dl = metric_distances(tr, tr[:257], EUCLIDEAN)
    got = _sweep(ctx, d_tr, d_tl, d_tr[:257], thr, 11, tl[:257], self_base=0, query_block=100)
    _assert_same(got, radius_sweep_reference(Dl, thr, 0, tl, C, OUTLIER, tl[:257]), "loo blocks")
    # ld_out > nq through the C entry: the guard columns stay as they were, correct / outliers are added to
    nq, R, ld = len(te), len(thr), len(te) + 7
    trd, ted = knn._device_dataset(d_tr, d_tl, 11), knn._device_dataset(d_te, None, 11)
    count = torch.full((R, ld), -5, dtype=torch.int32, device=d_te.device)
    pred = torch.full((R, ld), -5, dtype=torch.int32, device=d_te.device)
    cc = torch.full((R, ld, C), -5, dtype=torch.int32, device=d_te.device)
    correct = torch.full((R,), 1000, dtype=torch.int64, device=d_te.device)
    outliers = torch.full((R,), 2000, dtype=torch.int64, device=d_te.device)
    tp = thr.ctypes.data_as(ctypes.c_void_p)
    st = ctx.lib.knn_radius_sweep_count_device(ctx.h, ctypes.byref(trd), ctypes.byref(ted), tp, R, C, -1, OUTLIER,
                                               _dev(ql).data_ptr(), ld, count.data_ptr(), cc.data_ptr(),
                                               pred.data_ptr(), correct.data_ptr(), outliers.data_ptr(), None)
    assert st == knn.KNN_OK
    assert (count[:, nq:] == -5).all() and (pred[:, nq:] == -5).all() and (cc[:, nq:] == -5).all()
    _assert_same((_np(count[:, :nq]), _np(cc[:, :nq]), _np(pred[:, :nq]), _np(correct) - 1000, _np(outliers) - 2000),
                 whole, "ld_out")


def test_sweep_budget(knn, list_set, monkeypatch):
    """A call sized past the workspace budget: KNN_ERANGE naming the largest nq that fits, nothing
    launched; radius_sweep_device walks the queries in blocks of that many by itself."""
    import torch
    tr, tl, te, Ds = list_set
    thr = np.float32(radius_thresholds(Ds[EUCLIDEAN]))
    d_tr, d_tl, d_te = _dev(_pad4(tr)), _dev(tl), _dev(_pad4(te))
    ql = _qlabels(len(te))
    monkeypatch.setenv("KNN_WS_QUERIES", "1")                        # read at knn_create: 24,640 bytes of budget
    ctx = knn.Context(0, profile=1)
    try:
        fit = ctx.lib.knn_radius_sweep_max_queries(ctx.h, len(thr), C)
        assert fit == 24640 // ((len(thr) + 1) * (1 + C) * 4) and 1 <= fit < len(te)
        trd, ted = knn._device_dataset(d_tr, d_tl, 11), knn._device_dataset(d_te, None, 11)
        count = torch.full((len(thr), len(te)), -5, dtype=torch.int32, device=d_te.device)
        pred = torch.full((len(thr), len(te)), -5, dtype=torch.int32, device=d_te.device)
        outliers = torch.full((len(thr),), 2000, dtype=torch.int64, device=d_te.device)
        st = ctx.lib.knn_radius_sweep_count_device(ctx.h, ctypes.byref(trd), ctypes.byref(ted),
                                                   thr.ctypes.data_as(ctypes.c_void_p), len(thr), C, -1, OUTLIER, None,
                                                   len(te), count.data_ptr(), None, pred.data_ptr(), None,
                                                   outliers.data_ptr(), None)
        assert st == knn.KNN_ERANGE and f"nq={fit} " in ctx.lib.knn_last_error(ctx.h).decode()
        assert (count == -5).all() and (pred == -5).all() and (outliers == 2000).all()
        got = _sweep(ctx, d_tr, d_tl, d_te, thr, 11, ql)             # blocks of `fit` queries
        _assert_same(got, radius_sweep_reference(Ds[EUCLIDEAN], thr, None, tl, C, OUTLIER, ql), "budget blocks")
    finally:
        ctx.close()


# 9. the vote sweep on held lists
VOTE_KINDS = [(EUCLIDEAN, UNIFORM), (EUCLIDEAN, INV_DIST), (EUCLIDEAN, INV_SQDIST), (MANHATTAN, INV_DIST)]


@pytest.mark.parametrize("metric,weights", VOTE_KINDS)
def test_vote_sweep(ctxs, list_set, metric, weights):
    """Lists at thr[R - 1]; per r against the restatement and against radius_vote_device on the
    numpy-filtered sub-lists.  The queries that are copies of train rows have a zero distance among
    non-zero ones (the zero rule switches on inside the sub-list); the float set has queries with
    no neighbour at the small thresholds."""
    tr, tl, te, Ds = list_set
    D = Ds[metric]
    thr = np.float32(radius_thresholds(D))
    ctx = ctxs[metric, "auto"]
    ql = _qlabels(len(te))
    wname = WEIGHT_NAMES[weights]
    d_tr, d_tl, d_te, d_ql = _dev(_pad4(tr)), _dev(tl), _dev(_pad4(te)), _dev(ql)
    off, idx, dist = ctx.radius_neighbors_device(d_tr, d_te, threshold=float(thr[-1]), d=11)
    h_off, h_idx, h_dist = _np(off), _np(idx), _np(dist)
    segs = [h_dist[h_off[q]:h_off[q + 1]] for q in range(len(te))]
    assert any((s == 0).any() and (s != 0).any() for s in segs)     # the zero rule is exercised ...
    assert any(len(s) and not (s <= thr[1]).any() for s in segs)    # ... and a query empty at small r
    pred, correct, scores = ctx.radius_vote_sweep_device(off, idx, dist, d_tl, C, thresholds=thr, weights=wname,
                                                         outlier_label=OUTLIER, query_labels=d_ql)
    assert "radius_vote_sweep" in ctx.stage_times()
    pred, correct, scores = _np(pred), _np(correct), _np(scores)
    rpred, rscores = radius_vote_sweep_reference(h_off, h_idx, h_dist, tl, C, weights, metric, OUTLIER, thr)
    assert np.array_equal(pred, rpred) and np.array_equal(bits(scores), bits(rscores)), wname
    assert correct.dtype == np.int64 and np.array_equal(correct, (rpred == ql[None, :]).sum(axis=1))
    for r, t in enumerate(thr):
        so, si, sd = filter_lists(h_off, h_idx, h_dist, t)
        # (at least one element: an empty tensor has no address to hand to the library)
        vp, vc, vs = ctx.radius_vote_device(_dev(so), _dev(np.append(si, 0).astype(np.int32)),
                                            _dev(np.append(sd, 0).astype(np.float32)), d_tl, C, wname, OUTLIER, d_ql)
        assert np.array_equal(pred[r], _np(vp)) and np.array_equal(bits(scores[r]), bits(_np(vs))), (wname, r)
        assert correct[r] == _np(vc)[0]
    count, cpred, ccorrect, _ = ctx.radius_sweep_device(d_tr, d_tl, d_te, thresholds=thr, num_classes=C,
                                                        query_labels=d_ql, outlier_label=OUTLIER, d=11)
    if weights == UNIFORM:
        # the uniform vote sweep is the count sweep's vote
        assert np.array_equal(pred, _np(cpred)) and np.array_equal(correct, _np(ccorrect))
    # radius_sweep_predict_device: the same rows, and the counts
    ppred, pscores, pcount, pcorrect = ctx.radius_sweep_predict_device(
        d_tr, d_tl, d_te, thresholds=thr, num_classes=C, weights=wname, outlier_label=OUTLIER, query_labels=d_ql, d=11)
    assert np.array_equal(_np(ppred), pred) and np.array_equal(bits(_np(pscores)), bits(scores))
    assert np.array_equal(_np(pcount), _np(count)) and np.array_equal(_np(pcorrect), correct)


# 10. errors
def test_sweep_bad_arguments(knn, ctxs, list_set):
    import torch
    tr, tl, te, Ds = list_set
    d_tr, d_tl, d_te = _dev(_pad4(tr)), _dev(tl), _dev(_pad4(te))
    ctx = ctxs[EUCLIDEAN, "auto"]
    nq = len(te)
    trd, ted = knn._device_dataset(d_tr, d_tl, 11), knn._device_dataset(d_te, None, 11)
    guard = torch.full((32, nq), -5, dtype=torch.int32, device=d_te.device)
    outl = torch.full((32,), 2000, dtype=torch.int64, device=d_te.device)
    off, idx, dist = ctx.radius_neighbors_device(d_tr, d_te, threshold=1.0, d=11)

    def count_call(thr, R=None, ld=nq, out=True):
        thr = np.float32(thr)
        return ctx.lib.knn_radius_sweep_count_device(
            ctx.h, ctypes.byref(trd), ctypes.byref(ted), thr.ctypes.data_as(ctypes.c_void_p),
            len(thr) if R is None else R, C, -1, OUTLIER, None, ld, guard.data_ptr() if out else None, None, None, None,
            outl.data_ptr() if out else None, None)

    def vote_call(thr, R=None, ld=nq, out=True, weights=0):
        thr = np.float32(thr)
        return ctx.lib.knn_radius_vote_sweep_device(
            ctx.h, nq, len(tr), off.data_ptr(), idx.data_ptr(), dist.data_ptr(), d_tl.data_ptr(), C, weights,
            thr.ctypes.data_as(ctypes.c_void_p), len(thr) if R is None else R, OUTLIER, None, ld,
            guard.data_ptr() if out else None, None, None, None)

    cases = [dict(thr=[1.0], R=0), dict(thr=[1.0] * 33), dict(thr=[0.5, float("nan")]), dict(thr=[-1.0e-30, 1.0]),
             dict(thr=[0.5, float(FLT_MAX)]), dict(thr=[0.5, float("inf")]), dict(thr=[1.0, 0.5]),
             dict(thr=[0.5, 1.0], out=False), dict(thr=[0.5, 1.0], ld=nq - 1)]
    for call in (count_call, vote_call):
        for kw in cases:
            assert call(**kw) == knn.KNN_EINVAL, (call.__name__, kw)
            assert ctx.lib.knn_last_error(ctx.h).decode() != ""
    assert vote_call([0.5, 1.0], weights=3) == knn.KNN_EINVAL       # what weights_check refuses
    assert (guard == -5).all() and (outl == 2000).all()
    with pytest.raises(knn.KnnError):
        ctx.radius_sweep_device(d_tr, d_tl, d_te, radii=[1.0], thresholds=[1.0], num_classes=C, d=11)
    # a Manhattan context has no 1 / D^2 kind
    with pytest.raises(knn.KnnError) as e:
        ctxs[MANHATTAN, "auto"].radius_vote_sweep_device(off, idx, dist, d_tl, C, thresholds=[1.0], weights="sqdist")
    assert e.value.status == knn.KNN_EINVAL and "KNN_W_INV_SQDIST" in str(e.value)
    # a label outside [0, C), nobody's neighbour need it be: the single-threshold pass's status
    bad = tl.copy()
    bad[999] = C
    with pytest.raises(knn.KnnError) as e:
        ctx.radius_sweep_device(d_tr, _dev(bad), d_te, thresholds=[0.0, 1.0], num_classes=C, d=11)
    assert e.value.status == knn.KNN_EINVAL and "label" in str(e.value)
    with pytest.raises(knn.KnnError) as e1:
        ctx.radius_count_device(d_tr, _dev(bad), d_te, threshold=1.0, num_classes=C, d=11)
    assert str(e1.value) == str(e.value)
    # poisoned lists: the statuses of radius_vote_device
    for what in ("nan", "negative", "index", "offsets", "label"):
        o2, i2, d2, l2 = off.clone(), idx.clone(), dist.clone(), d_tl
        if what == "nan":
            d2[5] = float("nan")
        elif what == "negative":
            d2[5] = -1.0
        elif what == "index":
            i2[7] = len(tr)                                          # must not be followed
        elif what == "offsets":
            o2[3] = o2[4] + 1                                        # offsets that decrease
        else:
            l2 = _dev(bad)
            i2[7] = 999
        with pytest.raises(knn.KnnError) as e:
            ctx.radius_vote_sweep_device(o2, i2, d2, l2, C, thresholds=[0.25, 1.0], weights="distance")
        with pytest.raises(knn.KnnError) as e1:
            ctx.radius_vote_device(o2, i2, d2, l2, C, "distance", OUTLIER)
        assert e.value.status == knn.KNN_EINVAL and str(e.value) == str(e1.value), what
    # ... and the context still works
    count = ctx.radius_sweep_device(d_tr, None, d_te, thresholds=[0.0, 1.0], d=11)[0]
    assert np.array_equal(_np(count), radius_sweep_reference(Ds[EUCLIDEAN], np.float32([0.0, 1.0]))[0])


# 11. routing
def test_sweep_routing(knn, ctxs, oracle):
    """AUTO at and one below the floors takes the form knn_radius_policy states; a Manhattan
    context takes the direct form."""
    rows, queries = radius_floors(knn)
    tr, tl, te, thr1 = routing_set(oracle, rows, queries)
    thr = np.float32([0.0, thr1 / 2, thr1])
    d_tr, d_tl, d_te = _dev(tr), _dev(tl), _dev(te)
    ctx = ctxs[EUCLIDEAN, "auto"]
    for nt, nq in ((rows, queries), (rows - 1, queries), (rows, queries - 1)):
        got = _sweep(ctx, d_tr[:nt], d_tl[:nt], d_te[:nq], thr, 64)
        form = knn.radius_policy("euclidean", "f32", 64, nt, nq)
        assert form == ("mfma" if (nt, nq) == (rows, queries) else "direct")
        assert ctx.stats()["radius_form"] == form, (nt, nq)
        _assert_same(got, _singles(ctxs[EUCLIDEAN, "direct"], d_tr[:nt], d_tl[:nt], d_te[:nq], thr, 64),
                     f"routing {nt} x {nq}")
        assert got[0][2].sum() > 0
    assert knn.radius_policy("manhattan", "f32", 64, rows, queries) == "direct"
    _sweep(ctxs[MANHATTAN, "auto"], d_tr, d_tl, d_te, thr, 64)
    assert ctxs[MANHATTAN, "auto"].stats()["radius_form"] == "direct"


# 12. determinism
def test_sweep_determinism_and_empty(knn, ctxs, oracle, list_set):
    import torch
    tr, tl, te, Ds = list_set
    thr = np.float32(radius_thresholds(Ds[EUCLIDEAN]))
    d_tr, d_tl, d_te = _dev(_pad4(tr)), _dev(tl), _dev(_pad4(te))
    ctx = ctxs[EUCLIDEAN, "auto"]
    runs = []
    for _ in range(2):
        a = _sweep(ctx, d_tr, d_tl, d_te, thr, 11, _qlabels(len(te)))
        p, s, c = ctx.radius_sweep_predict_device(d_tr, d_tl, d_te, thresholds=thr, num_classes=C, weights="distance",
                                                  d=11)
        runs.append(list(a) + [_np(p), bits(_np(s)), _np(c)])
        pred = torch.empty(len(te), dtype=torch.int32, device=d_te.device)
        ctx.predict_device(d_tr, d_tl, d_te, 5, C, pred, d=11)      # a top-k call in between
    for x, y in zip(*runs):
        assert x.tobytes() == y.tobytes()
    # the MFMA form twice on a caching context, a top-k GEMM call in between: the same bytes, and the
    # radius pass's train operands are still valid behind the top-k call
    tr2, tl2, te2 = metric_set(oracle, "float", 1000, 257, 64)
    thr2 = np.float32(radius_thresholds(metric_distances(tr2, te2, EUCLIDEAN)))
    m_tr, m_tl, m_te = _dev(tr2), _dev(tl2), _dev(te2)
    mctx = knn.Context(0, algo="gemm_bf16", profile=1, cache_train=True)
    try:
        first = _sweep(mctx, m_tr, m_tl, m_te, thr2, 64, _qlabels(257))
        assert mctx.stats()["radius_form"] == "mfma" and not mctx.stats()["train_operands_cached"]
        pred = torch.empty(257, dtype=torch.int32, device=m_te.device)
        mctx.predict_device(m_tr, m_tl, m_te, 5, C, pred)
        again = _sweep(mctx, m_tr, m_tl, m_te, thr2, 64, _qlabels(257))
        assert mctx.stats()["radius_form"] == "mfma" and mctx.stats()["train_operands_cached"]
        for x, y in zip(first, again):
            assert x.tobytes() == y.tobytes()
    finally:
        mctx.close()
    # nq = 0
    none = d_te[:0]
    count, pred, correct, outliers, cc = ctx.radius_sweep_device(d_tr, d_tl, none, thresholds=thr, num_classes=C,
                                                                 query_labels=_dev(_qlabels(0)), class_counts=True, d=11)
    assert count.shape == (4, 0) and pred.shape == (4, 0) and cc.shape == (4, 0, C)
    assert not _np(correct).any() and not _np(outliers).any()
