"""GPU checks of the Manhattan and Chebyshev metrics (k_metric_tile) through every entry point:
predict and top-k export, forced train segments, bf16 rows, special values, the k-sweep,
leave-one-out, the weighted vote, train shards + merge, the host path, metric switching, the
ARFF pair and the CLI.

Bar: exact equality everywhere, floats compared as uint32 bits.  The yardstick is the numpy
float32 restatement in test_metric_cpu.py (pinned there to a scalar definition), fed through the
existing restatements of the vote (test_sweep_cpu.py, test_weighted_cpu.py).
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA, PKG_DIR
from test_metric_cpu import (CHEBYSHEV, FLT_MAX, MANHATTAN, NAMES, bits, metric_reference, metric_set,
                             vote_reference)
from test_sweep_cpu import sweep_reference
from test_weighted_cpu import INV_SQDIST, remove_self, weighted_reference

pytestmark = pytest.mark.gpu

METRICS = (MANHATTAN, CHEBYSHEV)
C = 10


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def _pad4(x):
    """Device rows are 16-byte aligned: zero columns up to a multiple of 4 (the call passes the
    true d, so they are never read as features)."""
    return np.pad(x, ((0, 0), (0, -x.shape[1] % 4)))


@pytest.fixture(scope="module")
def ctxs(knn):
    cs = {m: knn.Context(0, algo="direct", profile=1, metric=NAMES[m]) for m in METRICS}
    yield cs
    for c in cs.values():
        c.close()


def _topk(ctx, tr, tl, te, k, d=None):
    """predict_device with the lists exported: (pred, dist, idx) as numpy arrays."""
    import torch
    d = tr.shape[1] if d is None else d
    d_tr, d_te = (tr, te) if hasattr(tr, "is_cuda") else (_dev(_pad4(tr)), _dev(_pad4(te)))
    nq = d_te.shape[0]
    pred = torch.empty(nq, dtype=torch.int32, device=d_te.device)
    dist = torch.empty((nq, k), dtype=torch.float32, device=d_te.device)
    idx = torch.empty((nq, k), dtype=torch.int32, device=d_te.device)
    ctx.predict_device(d_tr, _dev(tl), d_te, k, C, pred, dist, idx, d=d)
    return pred.cpu().numpy(), dist.cpu().numpy(), idx.cpu().numpy()


def _check(ctx, metric, tr, tl, te, k, dev=None):
    """The context's lists and predictions against the restatement; returns the reference lists."""
    rdist, ridx = metric_reference(tr, te, k, metric)
    assert (ridx >= 0).all()
    pred, dist, idx = _topk(ctx, *(dev or (tr, tl, te)), k)
    assert np.array_equal(idx, ridx)
    assert np.array_equal(bits(dist), bits(rdist))
    assert np.array_equal(pred, vote_reference(ridx, tl, C))
    st = ctx.stage_times()
    assert "metric_tile" in st and "direct_tile" not in st, st
    return rdist, ridx


# ---------------------------------------------------------------------------------------
# shapes.  d: 1-3 trailing features, one chunk, more than DT_MAX_DC = 128; nt: a partial last
# tile; nq: a partial query block; k: every list register count, both insert paths, k = nt and
# k = 1024.  (11, 1000, 257, 5) is the Euclidean rows form's shape.
# ---------------------------------------------------------------------------------------
SHAPES = [(1, 65, 1, 1, "float"), (1, 1000, 9, 16, "grid"), (3, 65, 9, 17, "float"), (3, 1000, 257, 64, "grid"),
          (11, 1000, 257, 5, "float"), (11, 4096, 9, 16, "grid"), (11, 65, 257, 65, "float"),
          (64, 1000, 9, 129, "float"), (64, 4096, 257, 17, "grid"), (64, 4096, 9, 1024, "float"),
          (129, 65, 1, 64, "grid"), (129, 1000, 257, 1, "float"), (129, 4096, 9, 65, "float"),
          (260, 1000, 9, 16, "float"), (260, 4096, 1, 129, "grid"), (260, 65, 257, 17, "float"),
          (3, 4096, 9, 1024, "grid"), (1, 4096, 257, 129, "float"), (11, 1000, 1, 1, "grid"),
          (64, 65, 9, 65, "grid")]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,nt,nq,k,kind", SHAPES)
def test_metric_shapes(ctxs, oracle, d, nt, nq, k, kind, metric):
    tr, tl, te = metric_set(oracle, kind, nt, nq, d)
    _check(ctxs[metric], metric, tr, tl, te, k)


@pytest.fixture(scope="module")
def seg_set(oracle):
    tr, tl, te = metric_set(oracle, "float", 4096, 257, 11)
    refs = {(m, k): metric_reference(tr, te, k, m) for m in METRICS for k in (5, 65)}
    return tr, tl, te, refs


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("splits", [1, 3, 7, 32])
def test_metric_segments(knn, seg_set, splits, metric):
    """Forced train segments: per-segment records merged by k_merge_vote; the copies of a row sit
    in other segments, so the lower-index rule has to survive the merge."""
    tr, tl, te, refs = seg_set
    ctx = knn.Context(0, algo="direct", profile=1, train_splits=splits, metric=NAMES[metric])
    try:
        for k in (5, 65):
            rdist, ridx = refs[metric, k]
            pred, dist, idx = _topk(ctx, tr, tl, te, k)
            assert np.array_equal(idx, ridx) and np.array_equal(bits(dist), bits(rdist))
            assert np.array_equal(pred, vote_reference(ridx, tl, C))
            st = ctx.stage_times()
            assert "metric_tile" in st and "direct_tile" not in st
            assert ("merge_vote" in st) == (splits > 1)
            assert ctx.stats()["train_segments"] == splits
    finally:
        ctx.close()


@pytest.mark.parametrize("metric", METRICS)
def test_metric_bf16(ctxs, oracle, metric):
    import torch
    tr, tl = oracle.gen(23, 0, 0, 1000, 72, kind=1)
    te, _ = oracle.gen(23, 1, 0, 65, 72, kind=1)
    tr[500:600] = tr[:100]
    b_tr, b_te = _dev(tr).to(torch.bfloat16), _dev(te).to(torch.bfloat16)
    assert torch.equal(b_tr.to(torch.float32).cpu(), torch.from_numpy(tr))   # bf16-exact values
    for k in (7, 100):
        _check(ctxs[metric], metric, tr, tl, te, k, dev=(b_tr, tl, b_te))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("case", ["subnormal", "wide_range"])
def test_metric_numerics(ctxs, case, metric):
    rng = np.random.default_rng(31)
    nt, nq, d = 1000, 33, 24
    if case == "subnormal":
        tr = (rng.standard_normal((nt, d)) * 2.0 ** -140).astype(np.float32)
        te = (rng.standard_normal((nq, d)) * 2.0 ** -140).astype(np.float32)
    else:
        sc = np.float32(2.0) ** rng.integers(-60, 60, size=(1, d)).astype(np.float32)
        tr = (rng.standard_normal((nt, d)).astype(np.float32) * sc).astype(np.float32)
        te = (rng.standard_normal((nq, d)).astype(np.float32) * sc).astype(np.float32)
    tl = rng.integers(0, C, size=nt).astype(np.int32)
    for k in (1, 9, 40):
        rdist, _ = _check(ctxs[metric], metric, tr, tl, te, k)
        if case == "subnormal":
            assert (rdist > 0).all() and (rdist < np.finfo(np.float32).tiny).all()    # every distance is subnormal


def test_metric_overflow_and_nan(knn, ctxs):
    """Row 7's L1 sum overflows to inf while its largest difference stays below FLT_MAX; row 11 has
    a NaN feature and otherwise equals query 0.  Under L1 neither is ever listed (k = nt - 2 lists
    every other row, k = nt - 1 is KNN_ERANGE); under Chebyshev both are ordinary rows and the NaN
    difference is ignored, so row 11 is query 0's nearest at distance 0."""
    rng = np.random.default_rng(41)
    nt, nq, d = 200, 9, 5
    tr = rng.standard_normal((nt, d)).astype(np.float32)
    te = rng.standard_normal((nq, d)).astype(np.float32)
    tl = rng.integers(0, C, size=nt).astype(np.int32)
    tr[7] = [3e38, -3e38, 1, 2, 3]
    tr[11] = te[0]
    tr[11, 2] = np.nan
    rdist, ridx = _check(ctxs[MANHATTAN], MANHATTAN, tr, tl, te, nt - 2)
    assert 7 not in ridx and 11 not in ridx
    with pytest.raises(knn.KnnError) as e:
        _topk(ctxs[MANHATTAN], tr, tl, te, nt - 1)
    assert e.value.status == knn.KNN_ERANGE
    rdist, ridx = _check(ctxs[CHEBYSHEV], CHEBYSHEV, tr, tl, te, nt)
    assert ridx[0, 0] == 11 and rdist[0, 0] == 0
    assert (ridx[:, -1] == 7).all() and (rdist[:, -1] < FLT_MAX).all()


# ---------------------------------------------------------------------------------------
# composition: the restatement's lists through the existing restatements of the votes
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def comp_set(oracle):
    """1,000 x 8 on the grid (ties, duplicated rows, one row 43 times) and 65 queries; top-33 lists per metric, for
    the queries and for the train rows themselves (leave-one-out)."""
    tr, tl, te = metric_set(oracle, "grid", 1000, 65, 8)
    tr[900:940] = tr[0]          # 43 equal rows: the later ones are outside their own top-33
    lists = {m: metric_reference(tr, te, 33, m) for m in METRICS}
    self_lists = {m: metric_reference(tr, tr, 33, m) for m in METRICS}
    rng = np.random.default_rng(3)
    ql = rng.integers(0, C, size=len(te)).astype(np.int32)
    return tr, tl, te, ql, lists, self_lists


@pytest.mark.parametrize("metric", METRICS)
def test_metric_sweep_and_loo(ctxs, comp_set, metric):
    import torch
    tr, tl, te, ql, lists, self_lists = comp_set
    ctx = ctxs[metric]
    d_tr, d_tl, d_te = _dev(tr), _dev(tl), _dev(te)
    K = 32
    rdist, ridx = lists[metric]
    ref, too_few = sweep_reference(ridx[:, :K], tl, C)
    assert not too_few
    dist = torch.empty((len(te), K), dtype=torch.float32, device=d_tr.device)
    idx = torch.empty((len(te), K), dtype=torch.int32, device=d_tr.device)
    pa, corr = ctx.sweep_device(d_tr, d_tl, d_te, K, C, query_labels=_dev(ql), dist=dist, idx=idx)
    assert np.array_equal(pa.cpu().numpy(), ref)
    assert np.array_equal(corr.cpu().numpy(), (ref == ql[None, :]).sum(axis=1))
    assert np.array_equal(idx.cpu().numpy(), ridx[:, :K]) and np.array_equal(bits(dist.cpu().numpy()), bits(rdist[:, :K]))
    st = ctx.stage_times()
    assert "metric_tile" in st and "vote_sweep" in st and "direct_tile" not in st
    # leave-one-out: the self row (or, past a run of earlier duplicates, the last entry) leaves
    sdist, sidx = self_lists[metric]
    inside = (sidx == np.arange(len(tr))[:, None]).any(axis=1)
    assert inside.any() and not inside.all()
    ref, too_few = sweep_reference(sidx, tl, C, self_base=0)
    assert not too_few
    oi, od = remove_self(sidx, sdist, 0)
    dist = torch.empty((len(tr), K), dtype=torch.float32, device=d_tr.device)
    idx = torch.empty((len(tr), K), dtype=torch.int32, device=d_tr.device)
    pa, corr = ctx.loo_device(d_tr, d_tl, K, C, dist=dist, idx=idx)
    assert np.array_equal(pa.cpu().numpy(), ref)
    assert np.array_equal(corr.cpu().numpy(), (ref == tl[None, :]).sum(axis=1))
    assert np.array_equal(idx.cpu().numpy(), oi) and np.array_equal(bits(dist.cpu().numpy()), bits(od))


@pytest.mark.parametrize("metric", METRICS)
def test_metric_weighted(knn, ctxs, comp_set, metric):
    """weights="distance" is 1 / D on the metric's distance: the restatement's inverse-of-the-value
    kind on the restatement's lists.  "sqdist" has no meaning here and is refused."""
    import torch
    tr, tl, te, ql, lists, _ = comp_set
    ctx = ctxs[metric]
    d_tr, d_tl, d_te = _dev(tr), _dev(tl), _dev(te)
    K = 32
    rdist, ridx = lists[metric]
    rdist, ridx = rdist[:, :K], ridx[:, :K]
    ref, rsc, too_few = weighted_reference(ridx, rdist, tl, C, INV_SQDIST)
    assert not too_few
    assert (rdist[:, 0] == 0).any() and (rdist[:, 0] > 0).any()      # the zero rule and the 1 / D weights both run
    uni, _ = sweep_reference(ridx, tl, C)
    assert (ref != uni).any()
    pa, corr, sc = ctx.sweep_weighted_device(d_tr, d_tl, d_te, K, C, "distance", query_labels=_dev(ql))
    assert np.array_equal(pa.cpu().numpy(), ref)
    assert np.array_equal(bits(sc.cpu().numpy()), bits(rsc))
    assert np.array_equal(corr.cpu().numpy(), (ref == ql[None, :]).sum(axis=1))
    assert "metric_tile" in ctx.stage_times() and "vote_weighted" in ctx.stage_times()
    pred, sc1 = ctx.predict_weighted_device(d_tr, d_tl, d_te, K, C, "distance")
    assert np.array_equal(pred.cpu().numpy(), ref[K - 1]) and np.array_equal(bits(sc1.cpu().numpy()), bits(rsc))
    # lists the caller holds follow the context's metric too
    pa2, _, sc2 = ctx.vote_weighted_device(_dev(ridx), _dev(rdist), d_tl, C, "distance")
    assert np.array_equal(pa2.cpu().numpy(), ref) and np.array_equal(bits(sc2.cpu().numpy()), bits(rsc))
    for call in (lambda: ctx.sweep_weighted_device(d_tr, d_tl, d_te, K, C, "sqdist"),
                 lambda: ctx.predict_weighted_device(d_tr, d_tl, d_te, K, C, "sqdist"),
                 lambda: ctx.vote_weighted_device(_dev(ridx), _dev(rdist), d_tl, C, "sqdist")):
        with pytest.raises(knn.KnnError) as e:
            call()
        assert e.value.status == knn.KNN_EINVAL
    pa3, _, _ = ctx.sweep_weighted_device(d_tr, d_tl, d_te, K, C, "uniform")
    assert np.array_equal(pa3.cpu().numpy(), uni)


@pytest.mark.parametrize("metric", METRICS)
def test_metric_shards_and_host_path(ctxs, comp_set, metric):
    import torch
    tr, tl, te, _, lists, _ = comp_set
    ctx = ctxs[metric]
    k = 33
    rdist, ridx = lists[metric]
    rpred = vote_reference(ridx, tl, C)
    d_te = _dev(te)
    cuts = [0, 300, 301, 1000]              # a one-row shard: k exceeds its rows
    rec = torch.empty((3, len(te), 3, k), dtype=torch.int32, device=d_te.device)
    for s in range(3):
        a, b = cuts[s], cuts[s + 1]
        ctx.shard_topk_device(_dev(tr[a:b]), _dev(tl[a:b]), d_te, k, C, a, rec[s])
        assert "metric_tile" in ctx.stage_times()
    pred = torch.empty(len(te), dtype=torch.int32, device=d_te.device)
    dist = torch.empty((len(te), k), dtype=torch.float32, device=d_te.device)
    idx = torch.empty((len(te), k), dtype=torch.int32, device=d_te.device)
    ctx.merge_vote_device(rec, k, C, pred, dist, idx)
    assert np.array_equal(idx.cpu().numpy(), ridx) and np.array_equal(bits(dist.cpu().numpy()), bits(rdist))
    assert np.array_equal(pred.cpu().numpy(), rpred)
    upred, udist, uidx = _topk(ctx, tr, tl, te, k)
    assert np.array_equal(uidx, ridx) and np.array_equal(bits(udist), bits(rdist)) and np.array_equal(upred, rpred)
    # host arrays in and out (knn_predict), d = 8 and an unpadded d = 7 view
    hpred, hdist, hidx = ctx.predict(tr, tl, te, k, C, topk=True)
    assert np.array_equal(hidx, ridx) and np.array_equal(bits(hdist), bits(rdist)) and np.array_equal(hpred, rpred)
    r7d, r7i = metric_reference(tr[:, :7], te[:, :7], 5, metric)
    hpred, hdist, hidx = ctx.predict(tr[:, :7], tl, te[:, :7], 5, C, topk=True)
    assert np.array_equal(hidx, r7i) and np.array_equal(bits(hdist), bits(r7d))
    assert np.array_equal(hpred, vote_reference(r7i, tl, C))
    pa, corr = ctx.sweep(tr, tl, te, 32, C)
    assert np.array_equal(pa, sweep_reference(ridx[:, :32], tl, C)[0])


def test_metric_switching(knn, oracle):
    """One context: euclidean, manhattan, euclidean.  The Euclidean results are the oracle's before
    and after (the default path is untouched, whatever AUTO picks), the Manhattan ones the
    restatement's; bad metrics and contexts that cannot take one are refused."""
    tr, tl, te = metric_set(oracle, "float", 16384, 65, 64)     # (AUTO's Euclidean choice here is a GEMM form)
    bad, opred, odist, oidx = oracle.knn(tr, tl, te, 10, C)
    assert bad == 0
    ctx = knn.Context(0, profile=1)
    try:
        assert ctx.metric == "euclidean"
        first = _topk(ctx, tr, tl, te, 10)
        assert "metric_tile" not in ctx.stage_times()
        ctx.set_metric("manhattan")
        assert ctx.metric == "manhattan"
        rdist, ridx = metric_reference(tr, te, 10, MANHATTAN)
        pred, dist, idx = _topk(ctx, tr, tl, te, 10)
        assert np.array_equal(idx, ridx) and np.array_equal(bits(dist), bits(rdist))
        assert "metric_tile" in ctx.stage_times() and ctx.stats()["filter_operands"] is None
        assert (ridx != oidx).any()
        with pytest.raises(knn.KnnError) as e:
            ctx.set_metric(7)
        assert e.value.status == knn.KNN_EINVAL
        assert ctx.metric == "manhattan"                 # a refused metric changes nothing
        ctx.set_metric(0)
        assert ctx.metric == "euclidean"
        last = _topk(ctx, tr, tl, te, 10)
        assert "metric_tile" not in ctx.stage_times()
        for a, b, o in zip(first, last, (opred, odist, oidx)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert np.array_equal(a.view(np.uint32), o.view(np.uint32))
    finally:
        ctx.close()
    for algo in ("gemm", "gemm_split", "gemm_bf16", "direct_scan"):
        c = knn.Context(0, algo=algo)
        try:
            with pytest.raises(knn.KnnError) as e:
                c.set_metric("manhattan")
            assert e.value.status == knn.KNN_EINVAL
            assert c.metric == "euclidean"
            c.set_metric("euclidean")
        finally:
            c.close()
        with pytest.raises(knn.KnnError) as e:
            knn.Context(0, algo=algo, metric="chebyshev")
        assert e.value.status == knn.KNN_EINVAL


# ---------------------------------------------------------------------------------------
# ARFF data and the CLI
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_metric_arff_medium(knn, ctxs, metric):
    tf, tl, Ctr = knn.read_arff(f"{DATA}/medium-train.arff")
    qf, ql, _ = knn.read_arff(f"{DATA}/medium-test.arff")
    rdist, ridx = metric_reference(tf, qf, 5, metric)
    import torch
    d_te = _dev(_pad4(qf))
    pred = torch.empty(len(qf), dtype=torch.int32, device=d_te.device)
    dist = torch.empty((len(qf), 5), dtype=torch.float32, device=d_te.device)
    idx = torch.empty((len(qf), 5), dtype=torch.int32, device=d_te.device)
    ctxs[metric].predict_device(_dev(_pad4(tf)), _dev(tl), d_te, 5, Ctr, pred, dist, idx, d=tf.shape[1])
    assert np.array_equal(idx.cpu().numpy(), ridx) and np.array_equal(bits(dist.cpu().numpy()), bits(rdist))
    assert np.array_equal(pred.cpu().numpy(), vote_reference(ridx, tl, Ctr))
    assert "metric_tile" in ctxs[metric].stage_times()


def test_metric_cli(oracle, tmp_path):
    exe = os.path.join(PKG_DIR, "knn_cli")
    args = [exe, f"{DATA}/small-train.arff", f"{DATA}/small-test.arff", "5"]
    out = tmp_path / "pred.txt"

    def run(*flags):
        return subprocess.run(args + list(flags), capture_output=True, text=True, timeout=120,
                              env=dict(os.environ, KNN_CLI_PRED_OUT=str(out)))

    tf, tl, _ = oracle.read_arff(f"{DATA}/small-train.arff")
    qf, ql, _ = oracle.read_arff(f"{DATA}/small-test.arff")
    Ctr = int(tl.max()) + 1
    _, ridx = metric_reference(tf, qf, 5, MANHATTAN)
    ref, _ = sweep_reference(ridx, tl, Ctr)
    acc = [np.float32((ref[k] == ql).sum()) / np.float32(len(ql)) for k in range(5)]
    _, eidx = metric_reference(tf, qf, 5, 0)
    assert (sweep_reference(eidx, tl, Ctr)[0][4] != ref[4]).any()       # the flag matters on this pair
    r = run("--metric=manhattan")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 1 and lines[0].startswith("The 5-NN classifier for ")
    assert lines[0].endswith(f"Accuracy was {acc[4]:.4f}"), lines[0]
    assert np.array_equal(np.array(out.read_text().split(), np.int32), ref[4])
    r = run("--metric=manhattan", "--sweep")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 5
    for k, ln in enumerate(lines, 1):
        assert ln.startswith(f"The {k}-NN classifier for ") and ln.endswith(f"Accuracy was {acc[k - 1]:.4f}"), ln
    r = run("--metric=bogus")
    assert r.returncode != 0 and "bogus" in r.stderr and r.stdout == ""
    r = run("--metric=chebyshev", "--weights=sqdist")
    assert r.returncode == 1 and "KNN_W_INV_SQDIST" in r.stderr and r.stdout == "", (r.returncode, r.stderr)
