"""The Euclidean direct forms at every list-register class, on the GPU: the counterpart of
test_gpu_metric.py's SHAPES for k_direct_tile, k_direct_rows (algo="direct") and k_exact_scan
(algo="direct_scan"), fp32 and bf16 rows.

knn_list_regs picks the kernel instance by k (lists of 1, 2, 4, 8 or 16 registers of 64 entries:
k <= 64, 128, 256, 512, 1024), so k runs on both sides of every class, of the 16-entry rows form
(k_direct_rows takes d <= 16 with k <= 16: 16 | 17 crosses both of its limits) and at the largest
k; nt = k (every row, in order), a partial tile, a partial last tile of many and 4,096 rows; one
query, a partial query group and a partial block; d = 1, a row of trailing features, the rows
form's own shape, one staging chunk, just over one (DT_MAX_DC = 128) and over two.  Forced train
segments run k_merge_vote with 1, 2 and 4 list registers; a quarter of the train rows are exact
copies of earlier rows, so copies sit in other segments and the lower-index rule has to survive
the merge.

The reference is the C oracle, bit for bit: one call per (d, dtype, nt) at min(nt, 1024)
neighbours for all 257 queries -- a smaller k and fewer queries are prefixes of its lists
(test_plan_lattice_cpu.py::test_reference_prefixes pins that property of the oracle).
"""
import numpy as np
import pytest

from test_plan_lattice_cpu import list_classes, votes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C = 10
SEED = 83
KS = (1, 16, 17, 64, 65, 128, 129, 256, 257, 512, 513, 1024)
NTS = (65, 1000, 4096)
NQS = (1, 9, 257)
DS = (1, 3, 11, 64, 129, 260)
SPLITS = (1, 3, 7)
SPLIT_KS = (64, 65, 128, 129, 256, 257)
NT_MAX, NQ_MAX, K_MAX = max(NTS), max(NQS), 1024
_sets, _refs = {}, {}


def _rows(oracle, d, bf16):
    """4,096 train rows and 257 queries of one (d, dtype) on the device and the host (kind 1: exact
    in bf16, the oracle runs on the widened floats).  Every fourth train row is a copy of row
    r // 3, every fourth query one of the first 64 train rows."""
    import torch
    key = (d, bf16)
    if key not in _sets:
        tr, tl = oracle.gen(SEED + d, 0, 0, NT_MAX, d, kind=1 if bf16 else 0, C=C)
        te, _ = oracle.gen(SEED + d, 1, 0, NQ_MAX, d, kind=1 if bf16 else 0, C=C)
        for r in range(3, NT_MAX, 4):
            tr[r] = tr[r // 3]             # (ascending: a copy of the row as it stands)
        q = np.arange(0, NQ_MAX, 4)
        te[q] = tr[(5 * q) % 64]
        unit = 8 if bf16 else 4
        pitch = -(-d // unit) * unit       # (16-byte rows; the call passes the true d)

        def dev(x):
            t = torch.zeros((len(x), pitch), dtype=torch.bfloat16 if bf16 else torch.float32)
            t[:, :d] = torch.from_numpy(x)
            t = t.to(DEV)
            assert torch.equal(t[:, :d].to(torch.float32).cpu(), torch.from_numpy(x))
            return t

        _sets[key] = (tr, tl, te, dev(tr), torch.from_numpy(tl).to(DEV), dev(te))
    return _sets[key]


def _reference(oracle, d, bf16, nt):
    key = (d, bf16, nt)
    if key not in _refs:
        tr, tl, te = _rows(oracle, d, bf16)[:3]
        bad, _, dist, idx = oracle.knn(tr[:nt], tl[:nt], te, min(nt, K_MAX), C)
        assert bad == 0
        _refs[key] = (dist.view(np.uint32), idx)
    return _refs[key]


def _check(ctx, oracle, d, bf16, nt, nq, k, what):
    import torch
    tr, tl, te, dtr, dtl, dte = _rows(oracle, d, bf16)
    rdist, ridx = _reference(oracle, d, bf16, nt)
    rdist, ridx = rdist[:nq, :k], ridx[:nq, :k]
    pred = torch.empty(nq, dtype=torch.int32, device=DEV)
    dist = torch.empty((nq, k), dtype=torch.float32, device=DEV)
    idx = torch.empty((nq, k), dtype=torch.int32, device=DEV)
    ctx.predict_device(dtr[:nt], dtl[:nt], dte[:nq], k, C, pred, dist, idx, d=d)
    assert np.array_equal(idx.cpu().numpy(), ridx), f"{what}: indices"
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), rdist), f"{what}: distance bits"
    assert np.array_equal(pred.cpu().numpy(), votes(ridx, tl, C)), f"{what}: predictions"
    st = ctx.stats()
    assert st["filter_operands"] is None and st["filter_width"] == 0 and st["fallback_queries"] == 0, (what, st)
    return st


def test_k_edges_are_the_list_classes():
    """KS holds both sides of every class of knn_list_regs and its largest k."""
    tops = list_classes()
    assert tops[-1] == K_MAX == max(KS)
    for top in tops[:-1]:
        assert top in KS and top + 1 in KS
    assert 16 in KS and 17 in KS and 1 in KS           # the rows form's k limit
    assert any(d <= 16 for d in DS) and any(d > 16 for d in DS)


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("algo", ["direct", "direct_scan"])
def test_direct_lattice(knn, oracle, algo, bf16, d):
    ctx = knn.Context(0, algo=algo)
    try:
        for k in KS:
            for nt in sorted({k, *NTS}):
                if nt < k:
                    continue
                for nq in NQS:
                    _check(ctx, oracle, d, bf16, nt, nq, k, f"{algo} bf16={bf16} d={d} k={k} nt={nt} nq={nq}")
    finally:
        ctx.close()


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("splits", SPLITS)
def test_direct_segments_lattice(knn, oracle, splits, bf16, d):
    """Forced train segments at both sides of k = 64, 128 and 256: k_merge_vote with 1, 2 and 4 list
    registers, pieces with fewer rows than k, copies of rows in other segments."""
    ctx = knn.Context(0, algo="direct", train_splits=splits)
    try:
        for k in SPLIT_KS:
            for nt in sorted({k, *NTS}):
                if nt < k:
                    continue
                for nq in NQS:
                    st = _check(ctx, oracle, d, bf16, nt, nq, k, f"splits={splits} bf16={bf16} d={d} k={k} nt={nt} nq={nq}")
                    assert st["train_segments"] == splits, st
    finally:
        ctx.close()


@pytest.mark.parametrize("algo", ["direct", "direct_scan"])
def test_k_above_the_largest_class(knn, oracle, algo):
    import torch
    _, _, _, dtr, dtl, dte = _rows(oracle, 11, False)
    ctx = knn.Context(0, algo=algo)
    try:
        pred = torch.empty(9, dtype=torch.int32, device=DEV)
        with pytest.raises(knn.KnnError) as e:
            ctx.predict_device(dtr, dtl, dte[:9], K_MAX + 1, C, pred, d=11)
        assert e.value.status == knn.KNN_EINVAL
    finally:
        ctx.close()
