"""GPU checks of k-NN regression (k_regress_sweep / k_regress_reduce): the predictions for every
k <= K under the three weight kinds, the error sums, leave-one-out, the GEMM path, the metrics, the
entry points against each other, status codes and the CLI.

Bar: exact equality with the numpy float64 restatement in test_regress_cpu.py (which the CPU tests
pin to the definition, sklearn and hand cases), fed with the oracle's neighbour lists.  Predictions
compare as uint32 bits with NaN positions equal; the error sums are bounded against math.fsum of
the restatement's float32 predictions: every term is non-negative, so a binary64 sum in any order
errs by at most (nq - 1) 2^-53 relative, and squaring adds one more rounding: nq 2^-52 in all.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR
from test_gpu_sweep import D, NQ, NQS, NT, _dev
from test_gpu_weighted import loo_ref, sets  # noqa: F401  (module fixtures: the two sets, the leave-one-out lists)
from test_metric_cpu import CHEBYSHEV, MANHATTAN, metric_reference, metric_set
from test_metric_cpu import NAMES as METRIC_NAMES
from test_regress_cpu import error_sums, fbits, regress_reference
from test_weighted_cpu import INV_DIST, INV_SQDIST, KINDS, UNIFORM, list_weights, remove_self

pytestmark = pytest.mark.gpu

NAMES = {UNIFORM: "uniform", INV_DIST: "distance", INV_SQDIST: "sqdist"}
KMAXS = (1, 63, 64, 65, 128, 129, 1024)   # both sides of each register boundary, and the cap


@pytest.fixture(scope="module")
def ctx(knn):
    c = knn.Context(0, algo="direct")
    yield c
    c.close()


def _targets(n, seed):
    """Standard normal scaled by 100: both signs (the sums cancel), no two rows alike -- the
    duplicated rows of the sets carry different values."""
    return (np.random.default_rng(seed).standard_normal(n) * 100).astype(np.float32)


def _same(got, want):
    return np.array_equal(fbits(got.cpu().numpy() if hasattr(got, "cpu") else got), fbits(want))


def _check_sums(sse, sae, pred_ref, qt, nq):
    """The kernel's sums against fsum of the restatement's predictions: nq 2^-52 relative."""
    sse = sse.cpu().numpy() if hasattr(sse, "cpu") else sse
    sae = sae.cpu().numpy() if hasattr(sae, "cpu") else sae
    rse, rae = error_sums(pred_ref, qt)
    assert sse.dtype == np.float64 and sae.dtype == np.float64
    for got, want in ((sse, rse), (sae, rae)):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert (np.abs(got[ok] - want[ok]) <= nq * 2.0 ** -52 * want[ok]).all(), (got, want)


def _ref32(idx, dist, targets, weights):
    """A WRONG restatement that accumulates in float32: what an fp32 shortcut in the kernel gives."""
    w = list_weights(idx, dist, weights)
    y = targets[np.maximum(idx, 0)]
    N = np.zeros(len(idx), np.float32)
    Dn = np.zeros(len(idx), np.float32)
    out = np.empty((idx.shape[1], len(idx)), np.float32)
    for j in range(idx.shape[1]):
        N = N + w[:, j] * y[:, j]
        Dn = Dn + w[:, j]
        out[j] = N / Dn
    assert out.dtype == np.float32 and N.dtype == np.float32
    return out


def test_inputs_discriminate(sets):
    """CPU only, by the restatement alone (float set, K = 128): the inputs can tell a wrong kernel
    from a right one.  Measured here: 100 % of the queries change prediction bits between uniform
    and distance at k = 128, and 76 % (uniform) / 62 % (distance) of all predictions differ in
    bits from the float32-accumulated form."""
    K = 128
    s = sets["float"]
    idx, dist = s["idx"][:, :K], s["dist"][:, :K]
    y = _targets(NT, 5)
    assert (dist[:64, :2] == 0).all(axis=1).sum() >= 32                # several zero distances per list ...
    assert (y[idx[:32, 0]] != y[idx[:32, 1]]).all()                    # ... under different targets
    uni = regress_reference(idx, dist, y, UNIFORM)[0]
    dis = regress_reference(idx, dist, y, INV_DIST)[0]
    moved = (fbits(uni[K - 1]) != fbits(dis[K - 1])).mean()
    print(f"queries whose k = {K} prediction differs between uniform and distance: {moved:.3f}")
    assert moved >= 0.25, moved
    for weights, ref in ((UNIFORM, uni), (INV_DIST, dis)):
        short = (fbits(ref) != fbits(_ref32(idx, dist, y, weights))).mean()
        print(f"{NAMES[weights]}: predictions that differ from float32 accumulation: {short:.3f}")
        assert short >= 0.10, (weights, short)


@pytest.mark.parametrize("weights", KINDS)
@pytest.mark.parametrize("name", ["grid", "float"])
def test_regress_shapes(ctx, sets, name, weights):
    s = sets[name]
    idx, dist = s["idx"], s["dist"]
    y = _targets(NT, 5)
    qt = _targets(NQ, 6)
    ref, too_few = regress_reference(idx, dist, y, weights)
    assert not too_few
    d_y, d_qt = _dev(y), _dev(qt)
    for kmax in KMAXS:
        for nq in NQS:
            pa, sse, sae = ctx.regress_sweep_device(s["d_tr"], d_y, s["d_te"][:nq], kmax, weights,
                                                    query_targets=d_qt[:nq])
            assert pa.shape == (kmax, nq) and _same(pa, ref[:kmax, :nq]), (kmax, nq)
            _check_sums(sse, sae, ref[:kmax, :nq], qt[:nq], nq)
    # stride > kin: the kernel alone on the first kin entries of the 1024-wide lists
    for kin in (1, 63, 65, 200, 1024):
        for nq in (1, 65, 257):
            pa, sse, sae = ctx.regress_vote_device(s["d_idx"][:nq], s["d_dist"][:nq], d_y, weights,
                                                   query_targets=d_qt[:nq], kin=kin)
            assert _same(pa, ref[:kin, :nq]), (kin, nq)
            _check_sums(sse, sae, ref[:kin, :nq], qt[:nq], nq)
    if weights == UNIFORM:
        pa, _, _ = ctx.regress_vote_device(s["d_idx"], None, d_y, "uniform", kin=200)
        assert _same(pa, ref[:200])
    # without query targets the call returns no sums
    pa, sse, sae = ctx.regress_sweep_device(s["d_tr"], d_y, s["d_te"], 5, weights)
    assert sse is None and sae is None and _same(pa, ref[:5])


# ---------------------------------------------------------------------------------------
# leave-one-out
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [INV_DIST, UNIFORM])
@pytest.mark.parametrize("kmax", [1, 31, 32, 64])
def test_leave_one_out_regress(knn, ctx, loo_ref, kmax, weights):
    import torch
    tr, tl, C, odist, oidx, ddist, didx = loo_ref
    y = _targets(600, 9)
    d_tr, d_y = _dev(tr), _dev(y)
    dist = torch.empty((600, kmax), dtype=torch.float32, device=d_tr.device)
    idx = torch.empty((600, kmax), dtype=torch.int32, device=d_tr.device)
    pa, sse, sae = ctx.regress_loo_device(d_tr, d_y, kmax, weights, dist=dist, idx=idx)
    ref, too_few = regress_reference(oidx[:, :kmax + 1], odist[:, :kmax + 1], y, weights, self_base=0)
    assert not too_few and _same(pa, ref)
    _check_sums(sse, sae, ref, y, 600)
    ri, rd = remove_self(oidx[:, :kmax + 1], odist[:, :kmax + 1], 0)
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(fbits(dist.cpu().numpy()), fbits(rd))
    pa = pa.cpu().numpy()
    # the definition: the prediction on the train set with the row deleted
    for k in (1, 31):
        if k <= kmax:
            dref, _ = regress_reference(didx[:, :k], ddist[:, :k], y, weights)
            assert _same(pa[k - 1], dref[k - 1]), k
    # a slice of the train rows as the queries: self_base is the slice's first row
    ps, ses, sas = ctx.regress_sweep_device(d_tr, d_y, d_tr[200:333], kmax, weights, query_targets=d_y[200:333],
                                            self_base=200)
    assert _same(ps, pa[:, 200:333])
    _check_sums(ses, sas, ref[:, 200:333], y[200:333], 133)
    # the host entry point: the same bits, sums included (one batch, the device path's order)
    ph, seh, sah = ctx.regress_sweep(tr, y, tr, kmax, weights, query_targets=y, self_base=0)
    assert _same(ph, pa)
    assert np.array_equal(seh, sse.cpu().numpy()) and np.array_equal(sah, sae.cpu().numpy())
    assert knn.best_k_error(sse) == int(np.argmin(sse.cpu().numpy())) + 1


def test_gemm_bf16_equals_direct(knn, oracle):
    """The bf16 MFMA filter + exact rescore under the regression: 16,384 rows, d = 64, kmax = 32,
    leave-one-out, with duplicated rows (zero distances).  Every row against the direct form, 128
    sampled rows against the restatement on the oracle's lists."""
    nt, d, kmax = 16384, 64, 32
    tr, tl = oracle.gen(41, 0, 0, nt, d)
    tr[9000:9040] = tr[100:140]
    rep = 50 + 300 * np.arange(40)
    tr[rep] = tr[50]
    y = _targets(nt, 13)
    d_tr, d_y = _dev(tr), _dev(y)
    out = {}
    for algo in ("direct", "gemm_bf16"):
        c = knn.Context(0, algo=algo)
        try:
            pa, sse, sae = c.regress_loo_device(d_tr, d_y, kmax, "distance")
            out[algo] = (pa.cpu().numpy(), sse.cpu().numpy(), sae.cpu().numpy(), c.stats())
        finally:
            c.close()
    assert out["gemm_bf16"][3]["filter_operands"] == "bf16 rounded"
    for i in range(3):
        assert np.array_equal(out["gemm_bf16"][i].view(np.uint8), out["direct"][i].view(np.uint8)), i
    pa = out["gemm_bf16"][0]
    rows = np.unique(np.concatenate([np.linspace(0, nt - 1, 100).astype(np.int64), rep[:4], rep[-12:],
                                     [100, 139, 9000, 9039]]))[:128]
    bad, _, odist, oidx = oracle.knn(tr, tl, tr[rows], kmax + 1, 10)
    assert bad == 0
    li = np.empty((len(rows), kmax), np.int32)
    ld = np.empty((len(rows), kmax), np.float32)
    for n, i in enumerate(rows):
        hit = np.nonzero(oidx[n] == i)[0]
        at = hit[0] if len(hit) else kmax
        li[n], ld[n] = np.delete(oidx[n], at), np.delete(odist[n], at)
    assert (ld[:, 0] == 0).any() and (ld[:, 0] > 0).any()
    ref, too_few = regress_reference(li, ld, y, INV_DIST)
    assert not too_few and _same(pa[:, rows], ref)


# ---------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [MANHATTAN, CHEBYSHEV])
def test_regress_metrics(knn, oracle, metric):
    """weights="distance" is 1 / D on the metric's distance: the restatement's inverse-of-the-value
    kind on test_metric_cpu's numpy lists.  "sqdist" is refused."""
    K = 65
    tr, _, te = metric_set(oracle, "float", 1000, 65, 8)
    y, qt = _targets(1000, 17), _targets(65, 18)
    rdist, ridx = metric_reference(tr, te, K, metric)
    assert (rdist[:, 0] == 0).any() and (rdist[:, 0] > 0).any()
    ref, too_few = regress_reference(ridx, rdist, y, INV_SQDIST)
    assert not too_few
    c = knn.Context(0, metric=METRIC_NAMES[metric])
    try:
        d_tr, d_te, d_y, d_qt = _dev(tr), _dev(te), _dev(y), _dev(qt)
        pa, sse, sae = c.regress_sweep_device(d_tr, d_y, d_te, K, "distance", query_targets=d_qt)
        assert _same(pa, ref)
        _check_sums(sse, sae, ref, qt, 65)
        pv, _, _ = c.regress_vote_device(_dev(ridx), _dev(rdist), d_y, "distance")
        assert _same(pv, ref)
        pu, _, _ = c.regress_sweep_device(d_tr, d_y, d_te, K, "uniform")
        assert _same(pu, regress_reference(ridx, rdist, y, UNIFORM)[0])
        for call in (lambda: c.regress_sweep_device(d_tr, d_y, d_te, K, "sqdist"),
                     lambda: c.regress_device(d_tr, d_y, d_te, K, "sqdist"),
                     lambda: c.regress_vote_device(_dev(ridx), _dev(rdist), d_y, "sqdist"),
                     lambda: c.regress_sweep(tr, y, te, K, "sqdist")):
            with pytest.raises(knn.KnnError) as e:
                call()
            assert e.value.status == knn.KNN_EINVAL
    finally:
        c.close()


# ---------------------------------------------------------------------------------------
# the entry points agree
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", KINDS)
def test_entry_points_agree(knn, ctx, sets, weights):
    import torch
    s = sets["float"]
    kmax = 65
    y, qt = _targets(NT, 5), _targets(NQ, 6)
    d_y, d_qt, d_tr, d_te = _dev(y), _dev(qt), s["d_tr"], s["d_te"]
    pa, sse, sae = ctx.regress_sweep_device(d_tr, d_y, d_te, kmax, weights, query_targets=d_qt)
    ref, _ = regress_reference(s["idx"][:, :kmax], s["dist"][:, :kmax], y, weights)
    assert _same(pa, ref)
    # the single-k form is row k - 1
    dist = torch.empty((NQ, kmax), dtype=torch.float32, device=d_tr.device)
    idx = torch.empty((NQ, kmax), dtype=torch.int32, device=d_tr.device)
    pred = ctx.regress_device(d_tr, d_y, d_te, kmax, weights, dist=dist, idx=idx)
    assert pred.shape == (NQ,) and _same(pred, ref[kmax - 1])
    assert np.array_equal(idx.cpu().numpy(), s["idx"][:, :kmax])
    assert np.array_equal(fbits(dist.cpu().numpy()), fbits(s["dist"][:, :kmax]))
    for k in (1, 7, 64):
        assert _same(ctx.regress_device(d_tr, d_y, d_te, k, weights), ref[k - 1]), k
    # the regression alone on the lists the single-k call returned: the sweep, sums included
    pv, sev, sav = ctx.regress_vote_device(idx, dist, d_y, weights, query_targets=d_qt)
    assert _same(pv, ref) and torch.equal(sev, sse) and torch.equal(sav, sae)
    # two train shards merged: global indices, the whole target array, no new collective
    zl = torch.zeros(NT, dtype=torch.int32, device=d_tr.device)
    rec = torch.empty((2, NQ, 3, kmax), dtype=torch.int32, device=d_tr.device)
    ctx.shard_topk_device(d_tr[:1000], zl[:1000], d_te, kmax, 1, 0, rec[0])
    ctx.shard_topk_device(d_tr[1000:], zl[1000:], d_te, kmax, 1, 1000, rec[1])
    pred2 = torch.empty(NQ, dtype=torch.int32, device=d_tr.device)
    dist2 = torch.empty((NQ, kmax), dtype=torch.float32, device=d_tr.device)
    idx2 = torch.empty((NQ, kmax), dtype=torch.int32, device=d_tr.device)
    ctx.merge_vote_device(rec, kmax, 1, pred2, dist2, idx2)
    pm, sem, sam = ctx.regress_vote_device(idx2, dist2, d_y, weights, query_targets=d_qt)
    assert _same(pm, ref) and torch.equal(sem, sse) and torch.equal(sam, sae)


def test_host_regress_over_several_batches(knn, sets, monkeypatch):
    """Context.regress_sweep on numpy arrays equals the device result in every bit, sse / sae
    included, when the host path needs several batches: batches of 4,096 queries, here 2 x 4,096 +
    37 (three batches: the sums stay on the device and continue the same chain)."""
    s = sets["grid"]
    kmax, nq = 5, 2 * 4096 + 37
    monkeypatch.setenv("KNN_BATCH_ROWS", "4096")
    c = knn.Context(0, algo="direct")
    try:
        rng = np.random.default_rng(5)
        te = rng.integers(-2, 3, size=(nq, D)).astype(np.float32)
        te[4090:4100] = s["tr"][1500:1510]         # zero-rule lists on both sides of the batch edge
        y, qt = _targets(NT, 5), _targets(nq, 7)
        ph, seh, sah = c.regress_sweep(s["tr"], y, te, kmax, "distance", query_targets=qt)
        pd, sed, sad = c.regress_sweep_device(s["d_tr"], _dev(y), _dev(te), kmax, "distance", query_targets=_dev(qt))
        assert _same(ph, pd.cpu().numpy()) and not np.isnan(ph).any()
        assert np.array_equal(seh, sed.cpu().numpy()) and np.array_equal(sah, sad.cpu().numpy())
        _check_sums(seh, sah, ph, qt, nq)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------
# error sums over many blocks
# ---------------------------------------------------------------------------------------
def _synthetic(nq, kin, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, NT, size=(nq, kin)).astype(np.int32)
    dist = np.sort(rng.random((nq, kin)).astype(np.float32) + np.float32(0.01), axis=1)
    return idx, dist, _targets(NT, 5), _targets(nq, seed + 1)


@pytest.mark.parametrize("nq,kin", [(300000, 3), (5000, 300), (257 * 4096 + 5, 1)])
def test_error_sums_over_many_blocks(ctx, nq, kin):
    """The regression alone on synthetic lists.  This launcher gives every block one chunk of 16
    queries (so that the order of the sums depends on the query numbers alone), in tiles of 16,
    16, 16, 8 or 4 queries by list length: 300,000 x 3 is 18,750 blocks and 74 spans of the
    reduce; 5,000 x 300 is the shape at which one block takes several tiles (two of 8); and
    257 x 4,096 + 5 queries x 1 takes the reduce past one round of 256 spans.  Predictions equal
    the restatement, the sums are within nq 2^-52, and the same call twice gives the same bits."""
    import torch
    idx, dist, y, qt = _synthetic(nq, kin, 23)
    weights = UNIFORM if kin == 1 else INV_DIST
    ref, too_few = regress_reference(idx, dist, y, weights)
    assert not too_few
    d_idx, d_dist, d_y, d_qt = _dev(idx), _dev(dist), _dev(y), _dev(qt)
    pa, sse, sae = ctx.regress_vote_device(d_idx, d_dist, d_y, weights, query_targets=d_qt)
    assert _same(pa, ref)
    _check_sums(sse, sae, ref, qt, nq)
    pa2, sse2, sae2 = ctx.regress_vote_device(d_idx, d_dist, d_y, weights, query_targets=d_qt)
    assert torch.equal(sse2.view(torch.int64), sse.view(torch.int64))
    assert torch.equal(sae2.view(torch.int64), sae.view(torch.int64))
    assert torch.equal(pa2.view(torch.int32), pa.view(torch.int32))


# ---------------------------------------------------------------------------------------
# status: every case is an argument the host or the kernel's status word rejects
# ---------------------------------------------------------------------------------------
def test_regress_status(knn, ctx):
    import torch
    rng = np.random.default_rng(3)
    tr = rng.standard_normal((100, 8)).astype(np.float32)
    te = rng.standard_normal((9, 8)).astype(np.float32)
    y, qt = _targets(100, 1), _targets(9, 2)
    d_tr, d_te, d_y, d_qt = _dev(tr), _dev(te), _dev(y), _dev(qt)
    dist = torch.empty((9, 10), dtype=torch.float32, device=d_tr.device)
    idx = torch.empty((9, 10), dtype=torch.int32, device=d_tr.device)
    # (the train tensor goes in with labels = None: regression has no classes)
    assert knn._device_dataset(d_tr, None).labels is None
    pa0, sse0, _ = ctx.regress_sweep_device(d_tr, d_y, d_te, 10, "distance", query_targets=d_qt, dist=dist, idx=idx)
    assert pa0.shape == (10, 9) and sse0.shape == (10,) and not torch.isnan(pa0).any()
    # only 5 rows at a finite distance, kmax = 10: KNN_ERANGE, NaN from that prefix on
    far = tr.copy()
    far[5:, 0] = np.float32(3e38)
    pa = torch.zeros((10, 9), dtype=torch.float32, device=d_tr.device)
    with pytest.raises(knn.KnnError) as e:
        ctx.regress_sweep_device(_dev(far), d_y, d_te, 10, "distance", pred_all=pa)
    assert e.value.status == knn.KNN_ERANGE
    assert not torch.isnan(pa[:5]).any() and torch.isnan(pa[5:]).all()
    p5, _, _ = ctx.regress_sweep_device(_dev(far), d_y, d_te, 5, "distance")
    assert torch.equal(p5.view(torch.int32), pa[:5].view(torch.int32))
    # an unknown kind, by number and by name
    for call in (lambda: ctx.regress_sweep_device(d_tr, d_y, d_te, 10, 7),
                 lambda: ctx.regress_device(d_tr, d_y, d_te, 10, 7),
                 lambda: ctx.regress_vote_device(idx, dist, d_y, 7),
                 lambda: ctx.regress_sweep(tr, y, te, 10, -1),
                 lambda: ctx.regress_sweep_device(d_tr, d_y, d_te, 10, "nearest")):
        with pytest.raises(knn.KnnError) as e:
            call()
        assert e.value.status == knn.KNN_EINVAL
    # kin > 1024 on the regression alone; kin > n_train, kmax + the self row > n_train, kmax = 0
    wide_i = torch.zeros((9, 1025), dtype=torch.int32, device=d_tr.device)
    wide_d = torch.zeros((9, 1025), dtype=torch.float32, device=d_tr.device)
    with pytest.raises(knn.KnnError) as e:
        ctx.regress_vote_device(wide_i, wide_d, d_y)
    assert e.value.status == knn.KNN_EINVAL
    for kmax, sb in ((101, None), (100, 0), (0, None)):
        with pytest.raises(knn.KnnError) as e:
            ctx.regress_sweep_device(d_tr, d_y, d_tr[:9], kmax, self_base=sb)
        assert e.value.status == knn.KNN_EINVAL
    with pytest.raises(knn.KnnError) as e:
        ctx.regress_sweep(tr, y, tr[:9], 100, self_base=0)
    assert e.value.status == knn.KNN_EINVAL
    # all outputs NULL; sse without the query targets
    lib = knn.load_library()
    dtr, dte = knn._device_dataset(d_tr), knn._device_dataset(d_te)
    out = torch.zeros(10, dtype=torch.float64, device=d_tr.device)
    assert lib.knn_regress_sweep_device(ctx.h, ctypes.byref(dtr), ctypes.byref(dte), d_y.data_ptr(), 3, 1, -1,
                                        d_qt.data_ptr(), None, None, None, None, None, None) == knn.KNN_EINVAL
    assert lib.knn_regress_device(ctx.h, ctypes.byref(dtr), ctypes.byref(dte), d_y.data_ptr(), 3, 1, None, None, None,
                                  None) == knn.KNN_EINVAL
    assert lib.knn_regress_vote_device(ctx.h, 9, 3, idx.data_ptr(), dist.data_ptr(), 10, d_y.data_ptr(), 1, -1,
                                       d_qt.data_ptr(), None, None, None, None) == knn.KNN_EINVAL
    assert lib.knn_regress_sweep(ctx.h, ctypes.byref(dtr), ctypes.byref(dte), d_y.data_ptr(), 3, 1, -1, None, None,
                                 None, None) == knn.KNN_EINVAL
    assert lib.knn_regress_sweep_device(ctx.h, ctypes.byref(dtr), ctypes.byref(dte), d_y.data_ptr(), 3, 1, -1, None,
                                        pa.data_ptr(), out.data_ptr(), None, None, None, None) == knn.KNN_EINVAL
    assert lib.knn_regress_vote_device(ctx.h, 9, 3, idx.data_ptr(), dist.data_ptr(), 10, d_y.data_ptr(), 1, -1,
                                       None, pa.data_ptr(), None, out.data_ptr(), None) == knn.KNN_EINVAL
    # the weighted kinds need the distances; dist must match idx
    assert lib.knn_regress_vote_device(ctx.h, 9, 3, idx.data_ptr(), None, 10, d_y.data_ptr(), 1, -1,
                                       None, pa.data_ptr(), None, None, None) == knn.KNN_EINVAL
    with pytest.raises(knn.KnnError) as e:
        ctx.regress_vote_device(idx, dist[:, :5], d_y)
    assert e.value.status == knn.KNN_EINVAL
    # a NaN or negative distance on the regression-alone entry
    for v in (float("nan"), -1.0):
        bad_d = dist.clone()
        bad_d[4, 3] = v
        with pytest.raises(knn.KnnError) as e:
            ctx.regress_vote_device(idx, bad_d, d_y, "distance")
        assert e.value.status == knn.KNN_EINVAL
    # targets of another dtype, or not contiguous: no silent cast
    for call in (lambda: ctx.regress_sweep_device(d_tr, d_y.double(), d_te, 10),
                 lambda: ctx.regress_sweep_device(d_tr, d_y, d_te, 10, query_targets=d_qt.double()),
                 lambda: ctx.regress_device(d_tr, d_y.double(), d_te, 10),
                 lambda: ctx.regress_vote_device(idx, dist, d_y.double()),
                 lambda: ctx.regress_vote_device(idx, dist, torch.stack([d_y, d_y], dim=1)[:, 0]),
                 lambda: ctx.regress_sweep(tr, y.astype(np.float64), te, 10),
                 lambda: ctx.regress_sweep(tr, np.stack([y, y], axis=1)[:, 0], te, 10)):
        with pytest.raises(knn.KnnError) as e:
            call()
        assert e.value.status == knn.KNN_EINVAL
    # the context still works
    pa2, sse2, _ = ctx.regress_vote_device(idx, dist, d_y, "distance", query_targets=d_qt)
    assert torch.equal(pa2.view(torch.int32), pa0.view(torch.int32)) and torch.equal(sse2, sse0)
    pa3, _, _ = ctx.regress_sweep_device(d_tr, d_y, d_te, 10, "distance")
    assert torch.equal(pa3.view(torch.int32), pa0.view(torch.int32))


def test_stage_is_named_regress(knn, sets):
    s = sets["grid"]
    c = knn.Context(0, algo="direct", profile=True)
    try:
        c.regress_sweep_device(s["d_tr"], _dev(_targets(NT, 5)), s["d_te"], 8, "distance")
        st = c.stage_times()
        assert "regress" in st and "vote_weighted" not in st and "vote_sweep" not in st
    finally:
        c.close()


# ---------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------
def _write_arff(path, feat, y):
    with open(path, "w") as f:
        f.write("@RELATION r\n")
        for i in range(feat.shape[1]):
            f.write(f"@ATTRIBUTE f{i} NUMERIC\n")
        f.write("@ATTRIBUTE y NUMERIC\n@DATA\n")
        for row, t in zip(feat, y):
            f.write(",".join(f"{v:.9g}" for v in row) + f",{t:.9g}\n")


def test_cli_regress(knn, oracle, tmp_path):
    rng = np.random.default_rng(29)
    tr = rng.standard_normal((200, 4)).astype(np.float32)
    te = rng.standard_normal((40, 4)).astype(np.float32)
    te[:5] = tr[10:15]                                     # zero distances
    y = (rng.standard_normal(200) * 10).astype(np.float32)
    qy = (rng.standard_normal(40) * 10).astype(np.float32)
    assert (y < 0).any() and (y != np.round(y)).all()
    _write_arff(tmp_path / "train.arff", tr, y)
    _write_arff(tmp_path / "test.arff", te, qy)
    f2, y2 = knn.read_arff_targets(str(tmp_path / "train.arff"))
    assert np.array_equal(f2, tr) and np.array_equal(y2, y)
    exe = os.path.join(PKG_DIR, "knn_cli")
    K = 10
    args = [exe, str(tmp_path / "train.arff"), str(tmp_path / "test.arff"), str(K)]
    out = tmp_path / "pred.txt"

    def run(*flags):
        r = subprocess.run(args + list(flags), capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, KNN_CLI_PRED_OUT=str(out)))
        assert r.returncode == 0, r.stderr
        return r.stdout.strip().split("\n")

    def check(lines, ref, qt, ks, ntest):
        rse, rae = error_sums(ref, qt)
        assert len(lines) == len(ks)
        for ln, k in zip(lines, ks):
            m = re.fullmatch(rf"The {k}-NN regressor for {ntest} test instances on 200 train instances required "
                             r"\d+ ms CPU time\. RMSE was (\S+), MAE (\S+)", ln)
            assert m, ln
            assert m.group(1) == f"{np.sqrt(rse[k - 1] / ntest):.4f}" and m.group(2) == f"{rae[k - 1] / ntest:.4f}", ln

    zl = np.zeros(200, np.int32)
    bad, _, dist, idx = oracle.knn(tr, zl, te, K, 1)
    assert bad == 0
    ks = list(range(1, K + 1))
    ref, _ = regress_reference(idx, dist, y, UNIFORM)
    check(run("--regress", "--sweep"), ref, qy, ks, 40)
    rows = out.read_text().strip().split("\n")
    assert len(rows) == K
    for k in range(K):
        assert np.array_equal(fbits(np.array(rows[k].split(), np.float32)), fbits(ref[k])), k
    ref, _ = regress_reference(idx, dist, y, INV_DIST)
    check(run("--regress", "--weights=distance"), ref, qy, [K], 40)
    assert np.array_equal(fbits(np.array(out.read_text().split("\n")[:-1], np.float32)), fbits(ref[K - 1]))   # one per line
    bad, _, sdist, sidx = oracle.knn(tr, zl, tr, K + 1, 1)
    assert bad == 0
    ref, _ = regress_reference(sidx, sdist, y, UNIFORM, self_base=0)
    check(run("--regress", "--sweep=loo"), ref, y, ks, 200)
    mdist, midx = metric_reference(tr, te, K, MANHATTAN)
    ref, _ = regress_reference(midx, mdist, y, INV_SQDIST)
    check(run("--regress", "--metric=manhattan", "--weights=distance", "--sweep"), ref, qy, ks, 40)
    ref, _ = regress_reference(midx, mdist, y, UNIFORM)
    check(run("--regress", "--metric=manhattan"), ref, qy, [K], 40)
