"""GPU checks of what the three consumers of the exact top-k lists -- the k-sweep, the weighted
vote and regression -- share: the GEMM path's query passes (KNN_WS_QUERIES), the empty query
set, and the texts of the argument errors.

Bar: exact equality.  A context whose passes are cut short gives the bits of a default context
(one pass) on the same data; the error texts are the library's, character for character.
"""
import ctypes
import os

import numpy as np
import pytest

from test_gpu_sweep import _dev

pytestmark = pytest.mark.gpu

# test_gpu_host_path's KNN_WS_QUERIES shape: 60,000 rows x 128 under "gemm_bf16" run a GEMM filter
NT, D, C, KMAX, SEED = 60000, 128, 10, 10, 67
NQ_CLASS = 1000           # KNN_WS_QUERIES=333: passes of 333, 333, 333 and 1
NQ_REGRESS = 4096 + 500   # KNN_WS_QUERIES=5000: cut to the reduce span, passes of 4,096 and 500


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else t
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want):
    assert len(got) == len(want)
    return all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))


def _calls(c, data):
    """The pass-loop calls under test on one context: every output, as host arrays."""
    import torch
    tr, tl, te, ql, y, qy = data
    q, dev = te[:NQ_CLASS], tr.device

    def lists(nq):
        return (torch.empty((nq, KMAX), dtype=torch.float32, device=dev),
                torch.empty((nq, KMAX), dtype=torch.int32, device=dev))

    out = {}
    dist, idx = lists(NQ_CLASS)
    pa, corr = c.sweep_device(tr, tl, q, KMAX, C, query_labels=ql, dist=dist, idx=idx)
    assert c.stats()["filter_operands"] == "bf16 rounded"     # (a GEMM filter ran)
    out["sweep"] = [x.cpu().numpy() for x in (pa, corr, dist, idx)]
    dist, idx = lists(NQ_CLASS)
    pa, corr, sc = c.sweep_weighted_device(tr, tl, q, KMAX, C, "distance", query_labels=ql, dist=dist, idx=idx)
    out["sweep_weighted"] = [x.cpu().numpy() for x in (pa, corr, sc, dist, idx)]
    dist, idx = lists(NQ_CLASS)
    pred, sc = c.predict_weighted_device(tr, tl, q, KMAX, C, "distance", dist=dist, idx=idx)
    out["predict_weighted"] = [x.cpu().numpy() for x in (pred, sc, dist, idx)]
    return out


def _regress_call(c, data):
    tr, tl, te, ql, y, qy = data
    pa, sse, sae = c.regress_sweep_device(tr, y, te, KMAX, "distance", query_targets=qy)
    assert c.stats()["filter_operands"] == "bf16 rounded"
    return [x.cpu().numpy() for x in (pa, sse, sae)]


@pytest.fixture(scope="module")
def one_pass(knn, oracle):
    """The data on the device, and a default context's results (every query in one pass)."""
    assert "KNN_WS_QUERIES" not in os.environ
    tr, tl = oracle.gen(SEED, 0, 0, NT, D)
    te, _ = oracle.gen(SEED, 1, 0, NQ_REGRESS, D)
    rng = np.random.default_rng(SEED)
    ql = rng.integers(0, C, size=NQ_CLASS).astype(np.int32)
    y = (rng.standard_normal(NT) * 100).astype(np.float32)
    qy = (rng.standard_normal(NQ_REGRESS) * 100).astype(np.float32)
    data = tuple(_dev(x) for x in (tr, tl, te, ql, y, qy))
    c = knn.Context(0, algo="gemm_bf16")
    try:
        ref = _calls(c, data)
        ref["regress"] = _regress_call(c, data)
    finally:
        c.close()
    return data, ref, ql


def test_gemm_passes_class_votes(knn, one_pass, monkeypatch):
    """sweep_device, sweep_weighted_device and predict_weighted_device in GEMM passes of 333
    queries: pred_all / pred, scores and the returned lists are a single pass's bits, and
    correct is the sum over all four passes."""
    data, ref, ql = one_pass
    monkeypatch.setenv("KNN_WS_QUERIES", "333")
    c = knn.Context(0, algo="gemm_bf16")
    try:
        got = _calls(c, data)
    finally:
        c.close()
    for name in ("sweep", "sweep_weighted", "predict_weighted"):
        assert _same(got[name], ref[name]), name
    for name in ("sweep", "sweep_weighted"):
        pa, corr = got[name][:2]
        assert corr.dtype == np.int64 and np.array_equal(corr, (pa == ql[None, :]).sum(axis=1)), name
        assert corr.sum() > 0
    assert np.array_equal(got["predict_weighted"][0], got["sweep_weighted"][0][KMAX - 1])


def test_gemm_passes_regression(knn, one_pass, monkeypatch):
    """regress_sweep_device with KNN_WS_QUERIES=5000: the pass is cut to the reduce's span (4,096
    queries), and pred_all, sse and sae over 4,096 + 500 queries are a single pass's bits."""
    data, ref, _ = one_pass
    monkeypatch.setenv("KNN_WS_QUERIES", "5000")
    c = knn.Context(0, algo="gemm_bf16")
    try:
        got = _regress_call(c, data)
    finally:
        c.close()
    assert got[0].shape == (KMAX, NQ_REGRESS) and got[1].dtype == np.float64
    assert _same(got, ref["regress"])
    assert (got[1] > 0).all() and (got[2] > 0).all() and not np.isnan(got[0]).any()


# ---------------------------------------------------------------------------------------
# the empty query set and the argument errors, through the C ABI itself
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(knn):
    """100 train rows x 8 on the device and on the host, as knn_dataset pairs (train, no queries)."""
    rng = np.random.default_rng(3)
    tr = rng.standard_normal((100, 8)).astype(np.float32)
    tl = rng.integers(0, 4, size=100).astype(np.int32)
    y = rng.standard_normal(100).astype(np.float32)
    d_tr, d_tl, d_y = _dev(tr), _dev(tl), _dev(y)
    dev = (knn._device_dataset(d_tr, d_tl), knn._device_dataset(d_tr[:9]), d_y)
    dev[1].n = 0
    host = (knn._dataset(tr, tl)[0], knn._dataset(tr[:9])[0], y)
    host[1].n = 0
    c = knn.Context(0, algo="direct")
    yield c, knn.load_library(), dev, host, (tr, tl, y, d_tr, d_tl, d_y)
    c.close()


def test_empty_query_set(knn, small):
    """nq = 0 through the three *_sweep_device calls and the three host calls: KNN_OK, and the
    accumulators -- full of sevens going in -- come back all zero."""
    import torch
    c, lib, (dtr, dte, d_y), (htr, hte, y), _ = small
    ref = ctypes.byref
    kmax, dev = 5, torch.device("cuda", 0)
    ql = torch.zeros(4, dtype=torch.int32, device=dev)
    qt = torch.zeros(4, dtype=torch.float32, device=dev)
    pa = torch.zeros(4, dtype=torch.int32, device=dev)
    corr = torch.full((kmax,), 7, dtype=torch.int64, device=dev)
    sse = torch.full((kmax,), 7.0, dtype=torch.float64, device=dev)
    sae = torch.full((kmax,), 7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    assert lib.knn_sweep_device(c.h, ref(dtr), ref(dte), kmax, 4, -1, ql.data_ptr(), pa.data_ptr(), corr.data_ptr(),
                                None, None, None) == knn.KNN_OK
    assert (corr.cpu().numpy() == 0).all()
    corr.fill_(7)
    torch.cuda.synchronize()
    assert lib.knn_sweep_weighted_device(c.h, ref(dtr), ref(dte), kmax, 4, 1, -1, ql.data_ptr(), pa.data_ptr(),
                                         corr.data_ptr(), None, None, None, None) == knn.KNN_OK
    assert (corr.cpu().numpy() == 0).all()
    assert lib.knn_regress_sweep_device(c.h, ref(dtr), ref(dte), d_y.data_ptr(), kmax, 1, -1, qt.data_ptr(),
                                        pa.data_ptr(), sse.data_ptr(), sae.data_ptr(), None, None, None) == knn.KNN_OK
    assert (sse.cpu().numpy() == 0).all() and (sae.cpu().numpy() == 0).all()
    # the host calls
    hql, hqt = np.zeros(4, np.int32), np.zeros(4, np.float32)
    hpa = np.zeros(4, np.int32)
    hcorr = np.full(kmax, 7, np.int64)
    hsse, hsae = np.full(kmax, 7.0), np.full(kmax, 7.0)
    p = knn._ptr
    assert lib.knn_sweep(c.h, ref(htr), ref(hte), kmax, 4, -1, p(hql), p(hpa), p(hcorr)) == knn.KNN_OK
    assert (hcorr == 0).all()
    hcorr[:] = 7
    assert lib.knn_sweep_weighted(c.h, ref(htr), ref(hte), kmax, 4, 1, -1, p(hql), p(hpa), p(hcorr),
                                  None) == knn.KNN_OK
    assert (hcorr == 0).all()
    assert lib.knn_regress_sweep(c.h, ref(htr), ref(hte), p(y), kmax, 1, -1, p(hqt), p(hpa), p(hsse),
                                 p(hsae)) == knn.KNN_OK
    assert (hsse == 0).all() and (hsae == 0).all()


def _device_entry(prefix, lib, c, dtr, dte, d_y, kmax, ql, pa, acc):
    ref = ctypes.byref
    if prefix == "sweep":
        return lib.knn_sweep_device(c.h, ref(dtr), ref(dte), kmax, 4, -1, ql, pa, acc, None, None, None)
    if prefix == "weighted vote":
        return lib.knn_sweep_weighted_device(c.h, ref(dtr), ref(dte), kmax, 4, 1, -1, ql, pa, acc, None, None, None,
                                             None)
    return lib.knn_regress_sweep_device(c.h, ref(dtr), ref(dte), d_y.data_ptr(), kmax, 1, -1, ql, pa, acc, None,
                                        None, None, None)


def _host_entry(prefix, lib, c, htr, hte, y, kmax, ql, pa, acc):
    ref = ctypes.byref
    if prefix == "sweep":
        return lib.knn_sweep(c.h, ref(htr), ref(hte), kmax, 4, -1, ql, pa, acc)
    if prefix == "weighted vote":
        return lib.knn_sweep_weighted(c.h, ref(htr), ref(hte), kmax, 4, 1, -1, ql, pa, acc, None)
    return lib.knn_regress_sweep(c.h, ref(htr), ref(hte), knn_ptr(y), kmax, 1, -1, ql, pa, acc, None)


def knn_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


MESSAGES = {
    "sweep": ("sweep: kmax=0 must be >= 1", "sweep: query labels, pred_all and correct are all NULL"),
    "weighted vote": ("weighted vote: kmax=0 must be >= 1",
                      "weighted vote: query labels, pred_all, correct and scores are all NULL"),
    "regression": ("regression: kmax=0 must be >= 1", "regression: pred_all, sse and sae are all NULL"),
}


@pytest.mark.parametrize("prefix", sorted(MESSAGES))
def test_argument_error_texts(knn, small, prefix):
    """kmax = 0, and every output NULL, through a device and a host entry point of each consumer:
    KNN_EINVAL and the library's text, character for character."""
    import torch
    c, lib, (dtr, dte, d_y), (htr, hte, y), _ = small
    dev = torch.device("cuda", 0)
    ql = torch.zeros(16, dtype=torch.int32, device=dev).data_ptr()
    buf = torch.zeros(64, dtype=torch.float64, device=dev)
    hbuf = np.zeros(64, np.float64)
    no_k, no_out = MESSAGES[prefix]
    dte9, hte9 = knn.knn_dataset.from_buffer_copy(dte), knn.knn_dataset.from_buffer_copy(hte)
    dte9.n = hte9.n = 9
    for entry, args, some in ((_device_entry, (lib, c, dtr, dte9, d_y), buf.data_ptr()),
                              (_host_entry, (lib, c, htr, hte9, y), knn_ptr(hbuf))):
        assert entry(prefix, *args, 0, None, some, None) == knn.KNN_EINVAL
        assert lib.knn_last_error(c.h).decode() == no_k
        assert entry(prefix, *args, 3, None, None, None) == knn.KNN_EINVAL
        assert lib.knn_last_error(c.h).decode() == no_out
    # (the query side input alone is not an output: regression reports the missing outputs)
    if prefix == "regression":
        assert _device_entry(prefix, lib, c, dtr, dte9, d_y, 3, ql, None, None) == knn.KNN_EINVAL
        assert lib.knn_last_error(c.h).decode() == no_out
