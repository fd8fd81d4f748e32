"""GPU checks of the weighted vote (k_vote_weighted): predictions, correct counts and per-class
scores for every k <= K under the three weight kinds, leave-one-out, the GEMM path, the entry
points against each other, status codes and the CLI.

Bar: exact equality everywhere, floats compared as uint32 bits.  The yardstick is the numpy
float32 restatement in test_weighted_cpu.py (which the CPU tests pin to the definition, the
uniform sweep's restatement and the golden fixtures), fed with the oracle's neighbour lists.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA, PKG_DIR, golden_manifest, golden_pred, pred_sha
from test_gpu_sweep import D, KMAXS, NQ, NQS, NT, _dev, _grid_labels, _loo_set, _pad4, batch_case
from test_weighted_cpu import (INV_DIST, INV_SQDIST, KINDS, UNIFORM, bits, list_weights, remove_self,
                               weighted_reference)

pytestmark = pytest.mark.gpu

NAMES = {UNIFORM: "uniform", INV_DIST: "distance", INV_SQDIST: "sqdist"}


@pytest.fixture(scope="module")
def ctx(knn):
    c = knn.Context(0, algo="direct")
    yield c
    c.close()


# ---------------------------------------------------------------------------------------
# kernel shapes.  Two sets of 2,048 train rows x 8 and 257 queries: test_gpu_sweep's integer
# grid -2..2 (distance ties, exact score ties) and the generator's floats (every sum rounds,
# so the summation order shows).  In both, the first 64 queries are copies of train rows, and
# 32 of those rows have a second copy in the train set under its own random label: zero
# distances, several per list, with mixed labels.  Lists are the oracle's top-1024.
# ---------------------------------------------------------------------------------------
def _with_copies(tr, te):
    rng = np.random.default_rng(19)
    src = rng.permutation(1000)[:64]
    te[:64] = tr[src]
    tr[1500:1532] = tr[src[:32]]
    return tr, te


@pytest.fixture(scope="module")
def sets(oracle):
    rng = np.random.default_rng(7)
    gtr = rng.integers(-2, 3, size=(NT, D)).astype(np.float32)
    gte = rng.integers(-2, 3, size=(NQ, D)).astype(np.float32)
    ftr, _ = oracle.gen(77, 0, 0, NT, D)
    fte, _ = oracle.gen(77, 1, 0, NQ, D)
    out = {}
    for name, (tr, te) in (("grid", (gtr, gte)), ("float", (ftr, fte))):
        tr, te = _with_copies(tr, te)
        bad, _, dist, idx = oracle.knn(tr, np.zeros(NT, np.int32), te, 1024, 1)
        assert bad == 0
        out[name] = dict(tr=tr, te=te, dist=dist, idx=idx, d_tr=_dev(tr), d_te=_dev(te), d_dist=_dev(dist),
                         d_idx=_dev(idx))
    return out


def _prefix_scores(idx, dist, labels, C, weights, dtype=np.float32):
    """S_c(k) for every k: [kmax][nq][C], summed in list order in `dtype` (small C and kmax)."""
    w = list_weights(idx, dist, weights).astype(dtype)
    nq, kmax = idx.shape
    S = np.zeros((nq, C), dtype)
    out = np.zeros((kmax, nq, C), dtype)
    ar = np.arange(nq)
    for j in range(kmax):
        S[ar, labels[idx[:, j]]] += w[:, j]
        out[j] = S
    return out


def test_inputs_discriminate(sets):
    """CPU only, by the restatement alone (K = 128, C = 10): the inputs can tell a wrong kernel
    from a right one."""
    K, C = 128, 10
    for name, s in sets.items():
        idx, dist = s["idx"][:, :K], s["dist"][:, :K]
        lab = _grid_labels(s["idx"], C)
        uni = weighted_reference(idx, dist, lab, C, UNIFORM)[0]
        # zero distances: several per list, with mixed labels
        z = (dist == 0).sum(axis=1)
        mixed = [q for q in range(NQ) if z[q] >= 2 and len(set(lab[idx[q, :z[q]]].tolist())) > 1]
        assert len(mixed) >= 8, (name, len(mixed))
        for weights in (INV_DIST, INV_SQDIST):
            pred, _, too_few = weighted_reference(idx, dist, lab, C, weights)
            assert not too_few
            differs = (pred != uni).mean()
            moves = (pred[1:] != pred[:-1]).any(axis=0).mean()
            S = _prefix_scores(idx, dist, lab, C, weights)
            top2 = np.sort(S, axis=2)[:, :, -2:]
            ties = (top2[:, :, 0] == top2[:, :, 1])[:, dist[:, 0] > 0].mean()   # (lists under the zero rule aside)
            S64 = _prefix_scores(idx, dist, lab, C, weights, np.float64)
            with np.errstate(over="ignore"):
                order = (bits(S.max(axis=2)) != bits(S64.max(axis=2).astype(np.float32))).mean()
            print(f"{name} {NAMES[weights]}: differs from uniform {differs:.3f}, queries that move {moves:.3f}, "
                  f"top-score ties {ties:.4f}, order-sensitive top scores {order:.3f}")
            assert differs >= 0.05, (name, weights, differs)
            assert moves >= 0.25, (name, weights, moves)
            if name == "grid":
                assert ties > 0, (weights, ties)
            else:
                assert order >= 0.10, (weights, order)


@pytest.mark.parametrize("weights", KINDS)
@pytest.mark.parametrize("C", [2, 10, 1025, 16384])
@pytest.mark.parametrize("name", ["grid", "float"])
def test_weighted_shapes(ctx, sets, name, C, weights):
    s = sets[name]
    idx, dist = s["idx"], s["dist"]
    lab = _grid_labels(idx, C)
    refs = {k: weighted_reference(idx[:, :k], dist[:, :k], lab, C, weights) for k in set(KMAXS) | {63, 65, 200}}
    ref = refs[1024][0]
    assert not refs[1024][2]
    assert (lab[idx] == C - 1).any() and (ref == C - 1).any()
    rng = np.random.default_rng(C)
    ql = np.where(rng.random(NQ) < 0.5, ref[rng.integers(0, 1024, NQ), np.arange(NQ)],
                  rng.integers(0, C, NQ)).astype(np.int32)
    d_lab, d_ql = _dev(lab), _dev(ql)
    for kmax in KMAXS:
        for nq in NQS:
            pa, corr, sc = ctx.sweep_weighted_device(s["d_tr"], d_lab, s["d_te"][:nq], kmax, C, weights,
                                                     query_labels=d_ql[:nq])
            want = ref[:kmax, :nq]
            assert np.array_equal(pa.cpu().numpy(), want), (kmax, nq)
            assert np.array_equal(corr.cpu().numpy(), (want == ql[None, :nq]).sum(axis=1)), (kmax, nq)
            assert np.array_equal(bits(sc.cpu().numpy()), bits(refs[kmax][1][:nq])), (kmax, nq)
    # stride > kin: the kernel alone on the first kin entries of the 1024-wide lists
    for kin in (1, 63, 65, 200, 1024):
        for nq in (1, 65, 257):
            pa, corr, sc = ctx.vote_weighted_device(s["d_idx"][:nq], s["d_dist"][:nq], d_lab, C, weights,
                                                    query_labels=d_ql[:nq], kin=kin)
            assert np.array_equal(pa.cpu().numpy(), ref[:kin, :nq]), (kin, nq)
            assert np.array_equal(corr.cpu().numpy(), (ref[:kin, :nq] == ql[None, :nq]).sum(axis=1)), (kin, nq)
            assert np.array_equal(bits(sc.cpu().numpy()), bits(refs[kin][1][:nq])), (kin, nq)
    # without query labels there is no count; without scores no score tensor
    pa, corr, sc = ctx.sweep_weighted_device(s["d_tr"], d_lab, s["d_te"], 5, C, weights, scores=False)
    assert corr is None and sc is None and np.array_equal(pa.cpu().numpy(), ref[:5])


# ---------------------------------------------------------------------------------------
# leave-one-out
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loo_ref(oracle):
    """test_gpu_sweep's leave-one-out set, the oracle's top-65 lists on it, and -- the
    definition -- the oracle's top-31 lists of every row on the train set with that row deleted,
    renumbered to the whole set's rows (deleting a row keeps the order of the others)."""
    tr, tl, C = _loo_set()
    bad, _, dist, idx = oracle.knn(tr, tl, tr, 65, C)
    assert bad == 0
    inside = (idx == np.arange(600)[:, None]).any(axis=1)
    assert inside.any() and not inside.all()
    didx = np.zeros((600, 31), np.int32)
    ddist = np.zeros((600, 31), np.float32)
    for i in range(600):
        bad, _, dd, ii = oracle.knn(np.delete(tr, i, axis=0), np.delete(tl, i), tr[i:i + 1], 31, C, threads=1)
        assert bad == 0
        didx[i], ddist[i] = ii[0] + (ii[0] >= i), dd[0]
    return tr, tl, C, dist, idx, ddist, didx


@pytest.mark.parametrize("weights", [INV_DIST, INV_SQDIST])
@pytest.mark.parametrize("kmax", [1, 31, 32, 64])
def test_leave_one_out_weighted(knn, ctx, loo_ref, kmax, weights):
    import torch
    tr, tl, C, odist, oidx, ddist, didx = loo_ref
    d_tr, d_tl = _dev(tr), _dev(tl)
    dist = torch.empty((600, kmax), dtype=torch.float32, device=d_tr.device)
    idx = torch.empty((600, kmax), dtype=torch.int32, device=d_tr.device)
    pa, corr, sc = ctx.loo_weighted_device(d_tr, d_tl, kmax, C, weights, dist=dist, idx=idx)
    pa, corr, sc = pa.cpu().numpy(), corr.cpu().numpy(), sc.cpu().numpy()
    ref, rsc, too_few = weighted_reference(oidx[:, :kmax + 1], odist[:, :kmax + 1], tl, C, weights, self_base=0)
    assert not too_few
    assert np.array_equal(pa, ref) and np.array_equal(bits(sc), bits(rsc))
    assert np.array_equal(corr, (pa == tl[None, :]).sum(axis=1))
    ri, rd = remove_self(oidx[:, :kmax + 1], odist[:, :kmax + 1], 0)
    assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(bits(dist.cpu().numpy()), bits(rd))
    # the definition: the vote on the train set with the row deleted
    for k in (1, 31):
        if k <= kmax:
            dref, dsc, _ = weighted_reference(didx[:, :k], ddist[:, :k], tl, C, weights)
            assert np.array_equal(pa[k - 1], dref[k - 1]), k
            if k == kmax:
                assert np.array_equal(bits(sc), bits(dsc))
    # a slice of the train rows as the queries: self_base is the slice's first row
    ps, cs, ss = ctx.sweep_weighted_device(d_tr, d_tl, d_tr[200:333], kmax, C, weights, query_labels=d_tl[200:333],
                                           self_base=200)
    assert np.array_equal(ps.cpu().numpy(), pa[:, 200:333])
    assert np.array_equal(cs.cpu().numpy(), (pa[:, 200:333] == tl[None, 200:333]).sum(axis=1))
    assert np.array_equal(bits(ss.cpu().numpy()), bits(sc[200:333]))
    # the host entry point
    ph, ch, sh = ctx.sweep_weighted(tr, tl, tr, kmax, C, weights, query_labels=tl, self_base=0)
    assert np.array_equal(ph, pa) and np.array_equal(ch, corr) and np.array_equal(bits(sh), bits(sc))


@pytest.mark.parametrize("weights", [INV_DIST, INV_SQDIST])
def test_gemm_bf16_equals_direct(knn, oracle, weights):
    """The bf16 MFMA filter + exact rescore under the weighted vote: 16,384 rows, d = 64,
    kmax = 32, leave-one-out, with duplicated rows (zero distances).  Every row against the
    direct form, 128 sampled rows against the restatement on the oracle's lists."""
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
            pa, corr, sc = c.loo_weighted_device(d_tr, d_tl, kmax, C, weights)
            out[algo] = (pa.cpu().numpy(), corr.cpu().numpy(), sc.cpu().numpy(), c.stats())
        finally:
            c.close()
    assert out["gemm_bf16"][3]["filter_operands"] == "bf16 rounded"
    assert np.array_equal(out["gemm_bf16"][0], out["direct"][0])
    assert np.array_equal(out["gemm_bf16"][1], out["direct"][1])
    assert np.array_equal(bits(out["gemm_bf16"][2]), bits(out["direct"][2]))
    pa, corr, sc = out["gemm_bf16"][:3]
    assert np.array_equal(corr, (pa == tl[None, :]).sum(axis=1))
    rows = np.unique(np.concatenate([np.linspace(0, nt - 1, 100).astype(np.int64), rep[:4], rep[-12:],
                                     [100, 139, 9000, 9039]]))[:128]
    bad, _, odist, oidx = oracle.knn(tr, tl, tr[rows], kmax + 1, C)
    assert bad == 0
    li = np.empty((len(rows), kmax), np.int32)
    ld = np.empty((len(rows), kmax), np.float32)
    for n, i in enumerate(rows):
        hit = np.nonzero(oidx[n] == i)[0]
        at = hit[0] if len(hit) else kmax
        li[n], ld[n] = np.delete(oidx[n], at), np.delete(odist[n], at)
    assert (ld[:, 0] == 0).any() and (ld[:, 0] > 0).any()
    ref, rsc, too_few = weighted_reference(li, ld, tl, C, weights)
    assert not too_few
    assert np.array_equal(pa[:, rows], ref) and np.array_equal(bits(sc[rows]), bits(rsc))


# ---------------------------------------------------------------------------------------
# the entry points agree
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", KINDS)
def test_entry_points_agree(knn, ctx, sets, weights):
    import torch
    s = sets["float"]
    C, kmax = 10, 65
    lab = _grid_labels(s["idx"], C)
    d_lab, d_tr, d_te = _dev(lab), s["d_tr"], s["d_te"]
    pa, _, sc = ctx.sweep_weighted_device(d_tr, d_lab, d_te, kmax, C, weights)
    ref, rsc, _ = weighted_reference(s["idx"][:, :kmax], s["dist"][:, :kmax], lab, C, weights)
    assert np.array_equal(pa.cpu().numpy(), ref) and np.array_equal(bits(sc.cpu().numpy()), bits(rsc))
    # the single-k form is row k - 1 and the same scores
    dist = torch.empty((NQ, kmax), dtype=torch.float32, device=d_tr.device)
    idx = torch.empty((NQ, kmax), dtype=torch.int32, device=d_tr.device)
    pred, psc = ctx.predict_weighted_device(d_tr, d_lab, d_te, kmax, C, weights, dist=dist, idx=idx)
    assert torch.equal(pred, pa[kmax - 1]) and torch.equal(psc.view(torch.int32), sc.view(torch.int32))
    assert np.array_equal(idx.cpu().numpy(), s["idx"][:, :kmax])
    assert np.array_equal(bits(dist.cpu().numpy()), bits(s["dist"][:, :kmax]))
    for k in (1, 7, 64):
        p1, s1 = ctx.predict_weighted_device(d_tr, d_lab, d_te, k, C, weights)
        assert torch.equal(p1, pa[k - 1]), k
        assert np.array_equal(bits(s1.cpu().numpy()),
                              bits(weighted_reference(s["idx"][:, :k], s["dist"][:, :k], lab, C, weights)[1])), k
    # the vote alone on the lists the single-k call returned
    pv, _, sv = ctx.vote_weighted_device(idx, dist, d_lab, C, weights)
    assert torch.equal(pv, pa) and torch.equal(sv.view(torch.int32), sc.view(torch.int32))
    # two train shards merged: global indices, the whole label array, no new collective
    rec = torch.empty((2, NQ, 3, kmax), dtype=torch.int32, device=d_tr.device)
    ctx.shard_topk_device(d_tr[:1000], d_lab[:1000], d_te, kmax, C, 0, rec[0])
    ctx.shard_topk_device(d_tr[1000:], d_lab[1000:], d_te, kmax, C, 1000, rec[1])
    pred2 = torch.empty(NQ, dtype=torch.int32, device=d_tr.device)
    dist2 = torch.empty((NQ, kmax), dtype=torch.float32, device=d_tr.device)
    idx2 = torch.empty((NQ, kmax), dtype=torch.int32, device=d_tr.device)
    ctx.merge_vote_device(rec, kmax, C, pred2, dist2, idx2)
    pm, _, sm = ctx.vote_weighted_device(idx2, dist2, d_lab, C, weights)
    assert torch.equal(pm, pa) and torch.equal(sm.view(torch.int32), sc.view(torch.int32))


def test_uniform_is_the_existing_vote(knn, ctx, sets):
    """KNN_W_UNIFORM through every new entry point: the existing sweep_device / predict_device
    output, and the golden sha256 on `small`."""
    import torch
    s = sets["grid"]
    C, kmax = 10, 128
    lab = _grid_labels(s["idx"], C)
    d_lab, d_tr, d_te = _dev(lab), s["d_tr"], s["d_te"]
    old, _ = ctx.sweep_device(d_tr, d_lab, d_te, kmax, C)
    pa, _, sc = ctx.sweep_weighted_device(d_tr, d_lab, d_te, kmax, C, "uniform")
    assert torch.equal(pa, old)
    want = np.stack([np.bincount(lab[r], minlength=C) for r in s["idx"][:, :kmax]]).astype(np.float32)
    assert np.array_equal(bits(sc.cpu().numpy()), bits(want))
    pv, _, _ = ctx.vote_weighted_device(s["d_idx"], None, d_lab, C, "uniform", kin=kmax)
    assert torch.equal(pv, old)
    pv, _, _ = ctx.vote_weighted_device(s["d_idx"], s["d_dist"], d_lab, C, "uniform", kin=kmax)
    assert torch.equal(pv, old)
    oldp = torch.empty(NQ, dtype=torch.int32, device=d_tr.device)
    ctx.predict_device(d_tr, d_lab, d_te, 33, C, oldp)
    p1, _ = ctx.predict_weighted_device(d_tr, d_lab, d_te, 33, C, "uniform")
    assert torch.equal(p1, oldp)
    ph, _, _ = ctx.sweep_weighted(s["tr"], lab, s["te"], kmax, C, "uniform")
    assert np.array_equal(ph, old.cpu().numpy())
    # golden
    tf, tl, Cs = knn.read_arff(f"{DATA}/small-train.arff")
    qf, ql, _ = knn.read_arff(f"{DATA}/small-test.arff")
    d_tf, d_tl, d_qf = _dev(_pad4(tf)), _dev(tl), _dev(_pad4(qf))
    pa, corr, _ = ctx.sweep_weighted_device(d_tf, d_tl, d_qf, 100, Cs, "uniform", query_labels=_dev(ql),
                                            d=tf.shape[1])
    pa = pa.cpu().numpy()
    for k in (1, 3, 5, 10, 32, 100):
        assert pred_sha(pa[k - 1]) == golden_manifest()[f"small_k{k}"]["sha256"], k
        pk, _ = ctx.predict_weighted_device(d_tf, d_tl, d_qf, k, Cs, "uniform", d=tf.shape[1])
        assert pred_sha(pk.cpu().numpy()) == golden_manifest()[f"small_k{k}"]["sha256"], k
    assert np.array_equal(corr.cpu().numpy(), (pa == ql[None, :]).sum(axis=1))
    ph, _, _ = ctx.sweep_weighted(tf, tl, qf, 100, Cs, "uniform")
    assert np.array_equal(ph, pa)


def test_host_sweep_weighted_over_several_batches(knn, ctx, sets):
    """Context.sweep_weighted on numpy arrays equals the device result when the host path needs
    several batches: with scores and C = 16,384 a batch holds 4,096 queries, here 4,096 + 37."""
    s = sets["grid"]
    C, kmax, nq = 16384, 5, 4096 + 37
    lab = _grid_labels(s["idx"], C)
    rng = np.random.default_rng(5)
    te = rng.integers(-2, 3, size=(nq, D)).astype(np.float32)
    te[4090:4100] = s["tr"][1500:1510]         # zero-rule lists on both sides of the batch edge
    ql = rng.integers(0, C, size=nq).astype(np.int32)
    ph, ch, sh = ctx.sweep_weighted(s["tr"], lab, te, kmax, C, "distance", query_labels=ql)
    pd, cd, sd = ctx.sweep_weighted_device(s["d_tr"], _dev(lab), _dev(te), kmax, C, "distance", query_labels=_dev(ql))
    assert np.array_equal(ph, pd.cpu().numpy())
    assert np.array_equal(ch, cd.cpu().numpy()) and np.array_equal(ch, (ph == ql[None, :]).sum(axis=1))
    assert np.array_equal(bits(sh), bits(sd.cpu().numpy()))
    zr = sh[4090:4100]                          # under the zero rule the scores are counts, 2 or more in all
    assert np.array_equal(zr, np.round(zr)) and (zr.sum(axis=1) >= 2).all() and (sh > 0).any(axis=1).all()
    p = knn.proba(sd)
    assert np.allclose(p.cpu().numpy(), knn.proba(sh), rtol=1e-6, atol=0)   # (a helper: the row sums' order is torch's)
    assert np.allclose(p.sum(dim=1).cpu().numpy(), 1.0, rtol=0, atol=1e-6)


@pytest.mark.parametrize("self_base", [None, 300])
@pytest.mark.parametrize("weights", KINDS)
def test_host_sweep_weighted_batches_of_700(knn, monkeypatch, weights, self_base):
    """Context.sweep_weighted in host batches of 700 (KNN_BATCH_ROWS; test_gpu_sweep's batch_case)
    equals sweep_weighted_device on the same data in one call: pred_all, the correct counts summed
    over the batches and every batch's rows of the scores, in every bit."""
    C, kmax = 7, 9
    tr, lab, te, ql = batch_case(self_base)
    monkeypatch.setenv("KNN_BATCH_ROWS", "700")
    c = knn.Context(0, algo="direct")
    try:
        ph, ch, sh = c.sweep_weighted(tr, lab, te, kmax, C, weights, query_labels=ql, self_base=self_base,
                                      scores=True)
        pd, cd, sd = c.sweep_weighted_device(_dev(tr), _dev(lab), _dev(te), kmax, C, weights,
                                             query_labels=_dev(ql), self_base=self_base, scores=True)
    finally:
        c.close()
    assert ph.shape == (kmax, 1500) and np.array_equal(ph, pd.cpu().numpy())
    assert np.array_equal(ch, cd.cpu().numpy()) and np.array_equal(ch, (ph == ql[None, :]).sum(axis=1))
    assert sh.shape == (1500, C) and np.array_equal(bits(sh), bits(sd.cpu().numpy()))
    assert (sh > 0).any(axis=1).all()


# ---------------------------------------------------------------------------------------
# status: every case is an argument the host or the kernel's status word rejects
# ---------------------------------------------------------------------------------------
def test_weighted_status(knn, ctx):
    import torch
    rng = np.random.default_rng(3)
    tr = rng.standard_normal((100, 8)).astype(np.float32)
    te = rng.standard_normal((9, 8)).astype(np.float32)
    tl = rng.integers(0, 4, size=100).astype(np.int32)
    d_tr, d_tl, d_te = _dev(tr), _dev(tl), _dev(te)
    dist = torch.empty((9, 10), dtype=torch.float32, device=d_tr.device)
    idx = torch.empty((9, 10), dtype=torch.int32, device=d_tr.device)
    pa0, _, sc = ctx.sweep_weighted_device(d_tr, d_tl, d_te, 10, 4, dist=dist, idx=idx)  # the shapes are fine
    assert pa0.shape == (10, 9) and sc.shape == (9, 4)
    # only 5 rows at a finite distance, kmax = 10: KNN_ERANGE, the score rows all zero
    far = tr.copy()
    far[5:, 0] = np.float32(3e38)
    sc = torch.ones((9, 4), dtype=torch.float32, device=d_tr.device)
    with pytest.raises(knn.KnnError) as e:
        ctx.sweep_weighted_device(_dev(far), d_tl, d_te, 10, 4, scores=sc)
    assert e.value.status == knn.KNN_ERANGE
    assert not sc.cpu().numpy().any()
    pa, _, sc = ctx.sweep_weighted_device(_dev(far), d_tl, d_te, 5, 4)
    assert pa.shape == (5, 9) and (sc.cpu().numpy() > 0).any(axis=1).all()
    # a train label equal to C
    bad = tl.copy()
    bad[:] = 4
    with pytest.raises(knn.KnnError) as e:
        ctx.sweep_weighted_device(d_tr, _dev(bad), d_te, 10, 4)
    assert e.value.status == knn.KNN_EINVAL
    with pytest.raises(knn.KnnError) as e:
        ctx.vote_weighted_device(idx, dist, _dev(bad), 4)
    assert e.value.status == knn.KNN_EINVAL
    # an unknown kind, by number and by name
    for call in (lambda: ctx.sweep_weighted_device(d_tr, d_tl, d_te, 10, 4, 7),
                 lambda: ctx.predict_weighted_device(d_tr, d_tl, d_te, 10, 4, 7),
                 lambda: ctx.vote_weighted_device(idx, dist, d_tl, 4, 7),
                 lambda: ctx.sweep_weighted(tr, tl, te, 10, 4, -1),
                 lambda: ctx.sweep_weighted_device(d_tr, d_tl, d_te, 10, 4, "nearest")):
        with pytest.raises(knn.KnnError) as e:
            call()
        assert e.value.status == knn.KNN_EINVAL
    # kin > 1024 on the vote alone; kin > n_train, kmax + the self row > n_train, kmax = 0
    wide_i = torch.zeros((9, 1025), dtype=torch.int32, device=d_tr.device)
    wide_d = torch.zeros((9, 1025), dtype=torch.float32, device=d_tr.device)
    with pytest.raises(knn.KnnError) as e:
        ctx.vote_weighted_device(wide_i, wide_d, d_tl, 4)
    assert e.value.status == knn.KNN_EINVAL
    for kmax, sb in ((101, None), (100, 0), (0, None)):
        with pytest.raises(knn.KnnError) as e:
            ctx.sweep_weighted_device(d_tr, d_tl, d_tr[:9], kmax, 4, self_base=sb)
        assert e.value.status == knn.KNN_EINVAL
    # all outputs NULL
    lib = knn.load_library()
    dtr, dte = knn._device_dataset(d_tr, d_tl), knn._device_dataset(d_te)
    assert lib.knn_sweep_weighted_device(ctx.h, ctypes.byref(dtr), ctypes.byref(dte), 3, 4, 1, -1, None, None, None,
                                         None, None, None, None) == knn.KNN_EINVAL
    assert lib.knn_predict_weighted_device(ctx.h, ctypes.byref(dtr), ctypes.byref(dte), 3, 4, 1, None, None, None,
                                           None, None) == knn.KNN_EINVAL
    assert lib.knn_vote_weighted_device(ctx.h, 9, 3, 4, idx.data_ptr(), dist.data_ptr(), 10, d_tl.data_ptr(), 1, -1,
                                        None, None, None, None, None) == knn.KNN_EINVAL
    assert lib.knn_sweep_weighted(ctx.h, ctypes.byref(dtr), ctypes.byref(dte), 3, 4, 1, -1, None, None, None,
                                  None) == knn.KNN_EINVAL
    # the weighted kinds need the distances; dist must match idx
    assert lib.knn_vote_weighted_device(ctx.h, 9, 3, 4, idx.data_ptr(), None, 10, d_tl.data_ptr(), 1, -1,
                                        None, wide_i.data_ptr(), None, None, None) == knn.KNN_EINVAL
    with pytest.raises(knn.KnnError) as e:
        ctx.vote_weighted_device(idx, dist[:, :5], d_tl, 4)
    assert e.value.status == knn.KNN_EINVAL
    # a NaN or negative distance on the vote-alone entry
    for v in (float("nan"), -1.0):
        bad_d = dist.clone()
        bad_d[4, 3] = v
        with pytest.raises(knn.KnnError) as e:
            ctx.vote_weighted_device(idx, bad_d, d_tl, 4)
        assert e.value.status == knn.KNN_EINVAL
    # the context still works
    pa2, _, _ = ctx.vote_weighted_device(idx, dist, d_tl, 4)
    assert torch.equal(pa2, pa0)
    pa3, _, _ = ctx.sweep_weighted_device(d_tr, d_tl, d_te, 10, 4)
    assert torch.equal(pa3, pa0)


# ---------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------
def _untimed(out):
    return re.sub(r"required \d+ ms", "required N ms", out)


def test_cli_weights(knn, oracle, tmp_path):
    exe = os.path.join(PKG_DIR, "knn_cli")
    args = [exe, f"{DATA}/small-train.arff", f"{DATA}/small-test.arff", "10"]
    out = tmp_path / "pred.txt"

    def run(*flags):
        r = subprocess.run(args + list(flags), capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, KNN_CLI_PRED_OUT=str(out)))
        assert r.returncode == 0, r.stderr
        return r.stdout

    # --weights=uniform changes nothing, with and without --sweep
    lines = run("--weights=uniform", "--sweep").strip().split("\n")
    assert _untimed("\n".join(lines)) == _untimed(run("--sweep").strip())
    assert len(lines) == 10
    for k, ln in enumerate(lines, 1):
        assert ln.startswith(f"The {k}-NN classifier for ") and "ms CPU time. Accuracy was " in ln, ln
        if k in (1, 3, 5, 10):
            assert ln.endswith(f"Accuracy was {golden_manifest()[f'small_k{k}']['accuracy']:.4f}"), ln
    assert _untimed(run("--weights=uniform")) == _untimed(run())
    # --weights=distance: the restatement's accuracies
    tf, tl, _ = oracle.read_arff(f"{DATA}/small-train.arff")
    qf, ql, _ = oracle.read_arff(f"{DATA}/small-test.arff")
    C = int(tl.max()) + 1
    bad, _, dist, idx = oracle.knn(tf, tl, qf, 10, C)
    assert bad == 0
    ref, _, _ = weighted_reference(idx, dist, tl, C, INV_DIST)
    acc = [np.float32((ref[k] == ql).sum()) / np.float32(len(ql)) for k in range(10)]
    lines = run("--weights=distance", "--sweep").strip().split("\n")
    assert len(lines) == 10
    for k, ln in enumerate(lines, 1):
        assert ln.startswith(f"The {k}-NN classifier for ") and ln.endswith(f"Accuracy was {acc[k - 1]:.4f}"), ln
    rows = out.read_text().strip().split("\n")
    assert len(rows) == 10
    for k in range(10):
        assert np.array_equal(np.array(rows[k].split(), np.int32), ref[k]), k
    one = run("--weights=distance").strip().split("\n")
    assert len(one) == 1 and one[0].startswith("The 10-NN classifier for ")
    assert one[0].endswith(f"Accuracy was {acc[9]:.4f}")
    assert np.array_equal(np.array(out.read_text().split("\n")[:-1], np.int32), ref[9])   # one per line
    assert (ref != weighted_reference(idx, dist, tl, C, UNIFORM)[0]).any()              # the flag matters here
    assert np.array_equal(ref[0], golden_pred("small", 1))   # k = 1: one neighbour, any weight
