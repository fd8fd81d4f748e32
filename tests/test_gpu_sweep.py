"""GPU checks of the k-sweep (k_vote_sweep behind one top-K pass): predictions and correct
counts for every k <= K, leave-one-out with self-removal, the three entry points and the CLI.

Bar: exact equality everywhere.  The yardsticks are the reference's golden fixtures, the
oracle (oracle/knn_oracle.c), and the numpy restatement of the sweep in test_sweep_cpu.py,
which the CPU tests pin to both.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import (DATA, DATASETS, KS, PKG_DIR, golden_cm, golden_manifest, golden_pred,
                      pred_sha)
from test_sweep_cpu import loo_oracle, sweep_reference

pytestmark = pytest.mark.gpu


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))


def _pad4(x):
    """Device rows are 16-byte aligned: zero columns up to a multiple of 4 (the call passes the
    true d, so they are never read as features)."""
    return np.pad(x, ((0, 0), (0, -x.shape[1] % 4)))


def _remove_self(a, idx, self_base):
    """Rows of a [nq][kin] with the entry where idx == self_base + q removed (else the last)."""
    nq, kin = idx.shape
    out = np.empty((nq, kin - 1), a.dtype)
    for q in range(nq):
        hit = np.nonzero(idx[q] == self_base + q)[0]
        out[q] = np.delete(a[q], hit[0] if len(hit) else kin - 1)
    return out


@pytest.fixture(scope="module")
def ctx(knn):
    c = knn.Context(0, algo="direct")
    yield c
    c.close()


# ---------------------------------------------------------------------------------------
# golden fixtures
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ds", DATASETS)
def test_sweep_golden(knn, oracle, ds):
    tf, tl, C = knn.read_arff(f"{DATA}/{ds}-train.arff")
    qf, ql, Cq = knn.read_arff(f"{DATA}/{ds}-test.arff")
    c = knn.Context(0, algo="auto")
    try:
        pa, corr = c.sweep_device(_dev(_pad4(tf)), _dev(tl), _dev(_pad4(qf)), 100, C, query_labels=_dev(ql),
                                  d=tf.shape[1])
        pa, corr = pa.cpu().numpy(), corr.cpu().numpy()
    finally:
        c.close()
    assert pa.shape == (100, len(qf)) and corr.shape == (100,)
    for k in KS:
        assert np.array_equal(pa[k - 1], golden_pred(ds, k)), k
        assert pred_sha(pa[k - 1]) == golden_manifest()[f"{ds}_k{k}"]["sha256"], k
        assert corr[k - 1] == np.trace(golden_cm(ds, k)[1]), k
    assert np.array_equal(corr, (pa == ql[None, :]).sum(axis=1))
    if ds == "small":
        for k in range(1, 101):
            if k not in KS:
                _, op, _, _ = oracle.knn(tf, tl, qf, k, C, topk=False)
                assert np.array_equal(pa[k - 1], op), k
        assert knn.best_k(corr) == int(np.argmax(corr)) + 1


# ---------------------------------------------------------------------------------------
# kernel shapes: 2,048 train rows on a small integer grid (distance ties and vote ties are
# common), the oracle's top-1024 lists fed to the restatement
# ---------------------------------------------------------------------------------------
NT, NQ, D = 2048, 257, 8
KMAXS = (1, 63, 64, 65, 128, 1024)   # both sides of each 64-entry register boundary, and the cap
NQS = (1, 63, 65, 257)               # partial tiles of the transposed store


@pytest.fixture(scope="module")
def grid(oracle):
    rng = np.random.default_rng(7)
    tr = rng.integers(-2, 3, size=(NT, D)).astype(np.float32)
    te = rng.integers(-2, 3, size=(NQ, D)).astype(np.float32)
    bad, _, _, idx = oracle.knn(tr, np.zeros(NT, np.int32), te, 1024, 1)
    assert bad == 0
    return tr, te, idx, _dev(tr), _dev(te), _dev(idx)


def _grid_labels(idx, C):
    rng = np.random.default_rng(100 + C)
    lab = rng.integers(0, C, size=NT).astype(np.int32)
    lab[idx[::8, 1]] = C - 1            # the highest label sits inside the lists
    return lab


@pytest.mark.parametrize("C", [2, 10, 1025, 16384])
def test_sweep_shapes(ctx, grid, C):
    tr, te, idx, d_tr, d_te, d_idx = grid
    lab = _grid_labels(idx, C)
    ref, too_few = sweep_reference(idx, lab, C)
    assert not too_few
    # (CPU, before the GPU is used) the reference output is no constant: at least a quarter of
    # the queries change prediction between some pair of consecutive k -- on the whole block
    # and on the smallest multi-row block run below -- and the top label is in use
    assert (ref[1:] != ref[:-1]).any(axis=0).mean() >= 0.25
    assert (ref[1:63, :63] != ref[:62, :63]).any(axis=0).mean() >= 0.25
    assert (lab[idx] == C - 1).any() and (ref == C - 1).any()
    rng = np.random.default_rng(C)
    ql = np.where(rng.random(NQ) < 0.5, ref[rng.integers(0, 1024, NQ), np.arange(NQ)],
                  rng.integers(0, C, NQ)).astype(np.int32)
    d_lab, d_ql = _dev(lab), _dev(ql)
    for kmax in KMAXS:
        for nq in NQS:
            pa, corr = ctx.sweep_device(d_tr, d_lab, d_te[:nq], kmax, C, query_labels=d_ql[:nq])
            want = ref[:kmax, :nq]
            assert np.array_equal(pa.cpu().numpy(), want), (kmax, nq)
            assert np.array_equal(corr.cpu().numpy(), (want == ql[None, :nq]).sum(axis=1)), (kmax, nq)
    # idx_stride > kin: the kernel alone on the first kin entries of the 1024-wide lists
    for kin in (1, 63, 65, 200, 1024):
        for nq in (1, 65, 257):
            pa, corr = ctx.vote_sweep_device(d_idx[:nq], d_lab, C, query_labels=d_ql[:nq], kin=kin)
            assert np.array_equal(pa.cpu().numpy(), ref[:kin, :nq]), (kin, nq)
            assert np.array_equal(corr.cpu().numpy(), (ref[:kin, :nq] == ql[None, :nq]).sum(axis=1)), (kin, nq)
    # without query labels there is no count
    pa, corr = ctx.sweep_device(d_tr, d_lab, d_te, 5, C)
    assert corr is None and np.array_equal(pa.cpu().numpy(), ref[:5])


def test_context_reused_with_more_queries(knn, grid):
    """One context, growing query counts, on the short-row direct kernel with several train
    segments (d = 8, k <= 16): the per-group arrival counters of its in-kernel segment merge
    must be zero again when their buffer grows in place.  Lists against the oracle."""
    import torch
    tr, te, oidx, d_tr, d_te, _ = grid
    d_lab = _dev(np.zeros(NT, np.int32))
    c = knn.Context(0, algo="direct")
    try:
        for k in (1, 5):
            for nq in (1, 63, 65, 257):
                pred = torch.empty(nq, dtype=torch.int32, device=d_tr.device)
                idx = torch.full((nq, k), -7, dtype=torch.int32, device=d_tr.device)
                c.predict_device(d_tr, d_lab, d_te[:nq], k, 1, pred, None, idx)
                assert c.stats()["train_segments"] > 1
                assert np.array_equal(idx.cpu().numpy(), oidx[:nq, :k]), (k, nq)
    finally:
        c.close()


# ---------------------------------------------------------------------------------------
# leave-one-out
# ---------------------------------------------------------------------------------------
def _loo_set():
    """600 rows, d = 8, on an integer grid; 40 exact copies of earlier rows (the self row sits
    before its duplicate for the original and after it for the copy); one value repeated 70
    times: for kmax = 64 the later copies fall outside their own top-65 ("drop the last")."""
    rng = np.random.default_rng(11)
    tr = rng.integers(-3, 4, size=(600, 8)).astype(np.float32)
    tl = rng.integers(0, 6, size=600).astype(np.int32)
    dst = 100 + rng.permutation(500)[:40]
    tr[dst] = tr[rng.integers(0, 100, size=40)]
    tr[5 + 8 * np.arange(70)] = np.float32(9.0)
    return tr, tl, 6


@pytest.fixture(scope="module")
def loo_ref(oracle):
    tr, tl, C = _loo_set()
    want = loo_oracle(oracle, tr, tl, (1, 31, 32, 64), C)
    bad, _, dist, idx = oracle.knn(tr, tl, tr, 65, C)
    assert bad == 0
    inside = (idx == np.arange(600)[:, None]).any(axis=1)
    assert inside.any() and not inside.all()
    return tr, tl, C, want, dist, idx


@pytest.mark.parametrize("kmax", [1, 31, 32, 64])
def test_leave_one_out_direct(knn, ctx, loo_ref, kmax):
    import torch
    tr, tl, C, want, odist, oidx = loo_ref
    d_tr, d_tl = _dev(tr), _dev(tl)
    dist = torch.empty((600, kmax), dtype=torch.float32, device=d_tr.device)
    idx = torch.empty((600, kmax), dtype=torch.int32, device=d_tr.device)
    pa, corr = ctx.loo_device(d_tr, d_tl, kmax, C, dist=dist, idx=idx)
    pa, corr = pa.cpu().numpy(), corr.cpu().numpy()
    for k, w in want.items():
        if k <= kmax:
            assert np.array_equal(pa[k - 1], w), k
    ref, too_few = sweep_reference(oidx[:, :kmax + 1], tl, C, self_base=0)
    assert not too_few and np.array_equal(pa, ref)
    assert np.array_equal(corr, (pa == tl[None, :]).sum(axis=1))
    assert np.array_equal(idx.cpu().numpy(), _remove_self(oidx[:, :kmax + 1], oidx[:, :kmax + 1], 0))
    assert np.array_equal(dist.cpu().numpy().view(np.uint32),
                          _remove_self(odist[:, :kmax + 1].view(np.uint32), oidx[:, :kmax + 1], 0))
    # a slice of the train rows as the queries: self_base is the slice's first row
    ps, cs = ctx.sweep_device(d_tr, d_tl, d_tr[200:333], kmax, C, query_labels=d_tl[200:333], self_base=200)
    assert np.array_equal(ps.cpu().numpy(), pa[:, 200:333])
    assert np.array_equal(cs.cpu().numpy(), (pa[:, 200:333] == tl[None, 200:333]).sum(axis=1))
    # the host entry point
    ph, ch = ctx.sweep(tr, tl, tr, kmax, C, query_labels=tl, self_base=0)
    assert np.array_equal(ph, pa) and np.array_equal(ch, corr)


def test_leave_one_out_gemm_bf16(knn, oracle):
    """The bf16 MFMA filter + exact rescore under the sweep: 16,384 rows, d = 64, kmax = 32
    (kin = 33 crosses the fused filter's 32-entry list shape).  128 sampled rows against the
    per-row oracle, every row against the direct form."""
    nt, d, C, kmax = 16384, 64, 10, 32
    tr, tl = oracle.gen(41, 0, 0, nt, d)
    tr[9000:9040] = tr[100:140]
    rep = 50 + 300 * np.arange(40)
    tr[rep] = tr[50]
    d_tr, d_tl = _dev(tr), _dev(tl)
    out = {}
    for algo in ("direct", "gemm_bf16"):
        c = knn.Context(0, algo=algo)
        try:
            pa, corr = c.loo_device(d_tr, d_tl, kmax, C)
            out[algo] = (pa.cpu().numpy(), corr.cpu().numpy(), c.stats())
        finally:
            c.close()
    assert out["gemm_bf16"][2]["filter_operands"] == "bf16 rounded"
    assert np.array_equal(out["gemm_bf16"][0], out["direct"][0])
    assert np.array_equal(out["gemm_bf16"][1], out["direct"][1])
    pa, corr = out["gemm_bf16"][:2]
    assert np.array_equal(corr, (pa == tl[None, :]).sum(axis=1))
    rows = np.unique(np.concatenate([np.linspace(0, nt - 1, 100).astype(np.int64), rep[:4], rep[-12:],
                                     [100, 139, 9000, 9039]]))[:128]
    want = loo_oracle(oracle, tr, tl, (1, 5, 32), C, rows=rows)
    for k, w in want.items():
        assert np.array_equal(pa[k - 1, rows], w), k


# ---------------------------------------------------------------------------------------
# the entry points agree
# ---------------------------------------------------------------------------------------
def test_entry_points_agree(knn, ctx, grid):
    import torch
    tr, te, oidx, d_tr, d_te, _ = grid
    C, kmax = 10, 65
    lab = _grid_labels(oidx, C)
    d_lab = _dev(lab)
    pa, _ = ctx.sweep_device(d_tr, d_lab, d_te, kmax, C)
    pred = torch.empty(NQ, dtype=torch.int32, device=d_tr.device)
    idx = torch.empty((NQ, kmax), dtype=torch.int32, device=d_tr.device)
    ctx.predict_device(d_tr, d_lab, d_te, kmax, C, pred, None, idx)
    pv, _ = ctx.vote_sweep_device(idx, d_lab, C)
    assert torch.equal(pv, pa) and torch.equal(pa[kmax - 1], pred)
    # two train shards merged: global indices, the whole label array
    rec = torch.empty((2, NQ, 3, kmax), dtype=torch.int32, device=d_tr.device)
    ctx.shard_topk_device(d_tr[:1000], d_lab[:1000], d_te, kmax, C, 0, rec[0])
    ctx.shard_topk_device(d_tr[1000:], d_lab[1000:], d_te, kmax, C, 1000, rec[1])
    pred2 = torch.empty(NQ, dtype=torch.int32, device=d_tr.device)
    idx2 = torch.empty((NQ, kmax), dtype=torch.int32, device=d_tr.device)
    ctx.merge_vote_device(rec, kmax, C, pred2, None, idx2)
    pm, _ = ctx.vote_sweep_device(idx2, d_lab, C)
    assert torch.equal(pm, pa) and torch.equal(pred2, pred)


def test_host_sweep_over_several_batches(knn, ctx, grid):
    """Context.sweep on numpy arrays equals the device result, on more queries (131,109) than
    one batch of the host path holds (131,072; the batch size has no knob but an environment
    variable, so the test brings the queries instead)."""
    tr, _, oidx, d_tr, _, _ = grid
    C, kmax, nq = 10, 5, 131072 + 37
    lab = _grid_labels(oidx, C)
    rng = np.random.default_rng(5)
    te = rng.integers(-2, 3, size=(nq, D)).astype(np.float32)
    ql = rng.integers(0, C, size=nq).astype(np.int32)
    ph, ch = ctx.sweep(tr, lab, te, kmax, C, query_labels=ql)
    pd, cd = ctx.sweep_device(d_tr, _dev(lab), _dev(te), kmax, C, query_labels=_dev(ql))
    assert np.array_equal(ph, pd.cpu().numpy())
    assert np.array_equal(ch, cd.cpu().numpy())
    assert np.array_equal(ch, (ph == ql[None, :]).sum(axis=1))


def batch_case(self_base):
    """2,000 train rows x 20 on an integer grid (ties), 7 classes, and 1,500 queries: two full
    host batches of 700 and a ragged one.  With self_base the queries are train rows
    [self_base, self_base + 1500) and score against their own labels."""
    rng = np.random.default_rng(31)
    tr = rng.integers(-3, 4, size=(2000, 20)).astype(np.float32)
    lab = rng.integers(0, 7, size=2000).astype(np.int32)
    if self_base is None:
        return tr, lab, rng.integers(-3, 4, size=(1500, 20)).astype(np.float32), \
            rng.integers(0, 7, size=1500).astype(np.int32)
    return tr, lab, tr[self_base:self_base + 1500].copy(), lab[self_base:self_base + 1500].copy()


@pytest.mark.parametrize("self_base", [None, 300])
def test_host_sweep_batches_of_700(knn, monkeypatch, self_base):
    """Context.sweep in host batches of 700 (KNN_BATCH_ROWS; 700 + 700 + 100 queries) equals
    sweep_device on the same data in one call: pred_all and the correct counts summed over the
    batches, with and without the self rows."""
    C, kmax = 7, 9
    tr, lab, te, ql = batch_case(self_base)
    monkeypatch.setenv("KNN_BATCH_ROWS", "700")
    c = knn.Context(0, algo="direct")
    try:
        ph, ch = c.sweep(tr, lab, te, kmax, C, query_labels=ql, self_base=self_base)
        pd, cd = c.sweep_device(_dev(tr), _dev(lab), _dev(te), kmax, C, query_labels=_dev(ql), self_base=self_base)
        assert c.stats()["h2d_query_bytes"] == 0     # (the device call moves nothing)
    finally:
        c.close()
    assert ph.shape == (kmax, 1500) and np.array_equal(ph, pd.cpu().numpy())
    assert np.array_equal(ch, cd.cpu().numpy()) and np.array_equal(ch, (ph == ql[None, :]).sum(axis=1))
    assert (ph[1:] != ph[:-1]).any(axis=0).mean() >= 0.25   # the predictions move with k


# ---------------------------------------------------------------------------------------
# status
# ---------------------------------------------------------------------------------------
def test_sweep_status(knn, ctx):
    import torch
    rng = np.random.default_rng(3)
    tr = rng.standard_normal((100, 8)).astype(np.float32)
    te = rng.standard_normal((9, 8)).astype(np.float32)
    tl = rng.integers(0, 4, size=100).astype(np.int32)
    d_tr, d_tl, d_te = _dev(tr), _dev(tl), _dev(te)
    pa, _ = ctx.sweep_device(d_tr, d_tl, d_te, 10, 4)   # the shapes themselves are fine
    assert pa.shape == (10, 9)
    # only 5 rows at a finite distance, kmax = 10
    far = tr.copy()
    far[5:, 0] = np.float32(3e38)
    with pytest.raises(knn.KnnError) as e:
        ctx.sweep_device(_dev(far), d_tl, d_te, 10, 4)
    assert e.value.status == knn.KNN_ERANGE
    pa, _ = ctx.sweep_device(_dev(far), d_tl, d_te, 5, 4)
    assert pa.shape == (5, 9)
    # a train label equal to C
    bad = tl.copy()
    bad[:] = 4
    with pytest.raises(knn.KnnError) as e:
        ctx.sweep_device(d_tr, _dev(bad), d_te, 10, 4)
    assert e.value.status == knn.KNN_EINVAL
    # self rows past the train set, kin > n_train, kin > 1024
    with pytest.raises(knn.KnnError) as e:
        ctx.sweep_device(d_tr, d_tl, d_tr[:9], 3, 4, self_base=92)
    assert e.value.status == knn.KNN_EINVAL
    for kmax, sb in ((101, None), (100, 0), (0, None)):
        with pytest.raises(knn.KnnError) as e:
            ctx.sweep_device(d_tr, d_tl, d_tr[:9], kmax, 4, self_base=sb)
        assert e.value.status == knn.KNN_EINVAL
    # all three outputs NULL
    lib = knn.load_library()
    dtr, dte = knn._device_dataset(d_tr, d_tl), knn._device_dataset(d_te)
    st = lib.knn_sweep_device(ctx.h, ctypes.byref(dtr), ctypes.byref(dte), 3, 4, -1, None, None, None, None, None,
                              None)
    assert st == knn.KNN_EINVAL
    idx = torch.zeros((9, 3), dtype=torch.int32, device=d_tr.device)
    st = lib.knn_vote_sweep_device(ctx.h, 9, 3, 4, idx.data_ptr(), 3, d_tl.data_ptr(), -1, None, None, None, None)
    assert st == knn.KNN_EINVAL
    assert lib.knn_sweep(ctx.h, ctypes.byref(dtr), ctypes.byref(dte), 3, 4, -1, None, None, None) == knn.KNN_EINVAL
    # the context still works
    pa2, _ = ctx.sweep_device(d_tr, d_tl, d_te, 10, 4)
    assert pa2.shape == (10, 9)


# ---------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------
def test_cli_sweep(tmp_path):
    exe = os.path.join(PKG_DIR, "knn_cli")
    args = [exe, f"{DATA}/small-train.arff", f"{DATA}/small-test.arff", "10"]
    out = tmp_path / "pred.txt"
    r = subprocess.run(args + ["--sweep"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, KNN_CLI_PRED_OUT=str(out)))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 10
    for k, ln in enumerate(lines, 1):
        assert ln.startswith(f"The {k}-NN classifier for ") and "ms CPU time. Accuracy was " in ln, ln
        if k in (1, 3, 5, 10):
            assert ln.endswith(f"Accuracy was {golden_manifest()[f'small_k{k}']['accuracy']:.4f}"), ln
    rows = out.read_text().strip().split("\n")
    assert len(rows) == 10
    for k in (1, 3, 5, 10):
        assert np.array_equal(np.array(rows[k - 1].split(), np.int32), golden_pred("small", k))
    # without the flag: the single report line, as before
    r1 = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r1.returncode == 0, r1.stderr
    one = r1.stdout.strip().split("\n")
    assert len(one) == 1 and one[0].startswith("The 10-NN classifier for ")
    assert one[0].endswith(lines[9][lines[9].index("Accuracy was"):])
    # leave-one-out on the train file: the test path is not read
    r2 = subprocess.run(args[:2] + ["/nonexistent.arff", "4", "--sweep=loo"], capture_output=True, text=True,
                        timeout=120)
    assert r2.returncode == 0, r2.stderr
    assert len(r2.stdout.strip().split("\n")) == 4
