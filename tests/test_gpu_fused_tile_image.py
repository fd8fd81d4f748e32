"""The fused filter's tile copy and schedule on the device (k_gemm_fused): every shape of the
register-list plans, at sizes that put real rows in every corner of the LDS image and run
every kind of block of the balanced schedule, against the oracle (main.cpp:40-82): indices,
distance bits and predictions of every query, except in the balanced-schedule test, which
checks a sample (its docstring).

* nt = 16,384 + 64 * 3 + 17: the last tile is partial and the last barrier group is mostly pad
  tiles.
* nt = 40,000 with nq = 3 * 512 + 17: every query tile is cut into pieces and the last query
  tile is partial (so few queries get the small-set segments, knn_capi.cpp); with 20 * 512 + 17
  queries the host takes the balanced schedule: two-piece blocks, and blocks whose range lies
  inside one query tile (these start beside the second sweep and wrap: knn_fused_range_piece),
  all paced per XCD (fused_pace).
* Planted rows: the true nearest neighbour of 256 queries sits at each of the 32 row positions
  of each of the 8 tile places of a barrier group, so a slot copied from the wrong place, a
  piece no wave issued or a header read from the wrong tile changes a result, not only a
  candidate count.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = {"tail": (16_384 + 64 * 3 + 17, 600), "pieces": (40_000, 3 * 512 + 17)}
_data, _want = {}, {}


def _rows(knn, size, d, dtype, plant=False):
    """Train rows, labels and queries of a case (device tensors), generated once and shared."""
    import torch
    key = (size, d, dtype, plant)
    if key not in _data:
        nt, nq = SIZES[size]
        kind = 1 if dtype == "bf16" else 0
        tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
        g = knn.Context(0)
        train = torch.empty((nt, d), dtype=tdt, device=DEV)
        labels = torch.empty(nt, dtype=torch.int32, device=DEV)
        test = torch.empty((nq, d), dtype=tdt, device=DEV)
        g.generate(train, labels, 0, d, kind, 53 + d, 0, 10)
        g.generate(test, None, 0, d, kind, 53 + d, 1, 10)
        if plant:
            # query p's own row at train row base + p: 256 consecutive rows cover every (row of a
            # tile, tile of a group) once, in the first groups and (unaligned) in the last ones
            train[512:768] = test[:256]
            train[nt - 273:nt - 17] = test[256:512]
        torch.cuda.synchronize()
        g.close()
        _data[key] = (train, labels, test)
    return _data[key]


def _oracle(oracle, knn, size, d, dtype, k, plant=False):
    key = (size, d, dtype, k, plant)
    if key not in _want:
        train, labels, test = _rows(knn, size, d, dtype, plant)
        bad, pred, dist, idx = oracle.knn(train.float().cpu().numpy(), labels.cpu().numpy(),
                                          test.float().cpu().numpy(), k, 10)
        assert bad == 0
        _want[key] = (pred, dist.view(np.uint32), idx)
    return _want[key]


def _run(knn, monkeypatch, train, labels, test, k, qg, splits=0):
    import torch
    if qg is None:
        monkeypatch.delenv("KNN_FUSED_QG", raising=False)
    else:
        monkeypatch.setenv("KNN_FUSED_QG", qg)  # (snapshot at knn_create)
    ctx = knn.Context(0, algo="gemm_bf16", train_splits=splits)
    try:
        nq = test.shape[0]
        pred = torch.empty(nq, dtype=torch.int32, device=DEV)
        dist = torch.empty((nq, k), dtype=torch.float32, device=DEV)
        idx = torch.empty((nq, k), dtype=torch.int32, device=DEV)
        ctx.predict_device(train, labels, test, k, 10, pred, dist, idx)
        torch.cuda.synchronize()
        return pred.cpu().numpy(), dist.cpu().numpy().view(np.uint32), idx.cpu().numpy(), ctx.stats()
    finally:
        ctx.close()


def _check(got, want, qg):
    st = got[3]
    assert st["fused_norm"] and st["fallback_queries"] == 0, st
    if qg is not None:
        assert st["queries_per_wave"] == 32 * int(qg), st
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0])


CASES = [(d, k, "f32", qg) for d in (64, 128) for k in (10, 32) for qg in ("1", "2")]
CASES += [(256, 10, "f32", None), (256, 32, "f32", None), (256, 100, "bf16", None)]


@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("d,k,dtype,qg", CASES)
def test_fused_shapes_match_oracle(knn, oracle, monkeypatch, size, d, k, dtype, qg):
    train, labels, test = _rows(knn, size, d, dtype)
    got = _run(knn, monkeypatch, train, labels, test, k, qg)
    _check(got, _oracle(oracle, knn, size, d, dtype, k), qg)
    if size == "pieces" and k <= 32:
        assert got[3]["train_segments"] > 1, got[3]   # pieces of a query tile, not whole tiles


@pytest.mark.parametrize("qg", ["1", "2"])
def test_balanced_schedule_with_rotated_blocks(knn, oracle, monkeypatch, qg):
    """Enough query tiles (20 * 512 + 17 queries) that the host takes the balanced schedule
    rather than the small-set segments: 51 ranges of ~257 units over 21 query tiles of 625 --
    two-piece blocks, and one-piece blocks that start at unit 368 of their tile and wrap.

    This is a SAMPLE, not every query: the oracle checks 517 of the 10,257 queries (500 spread
    over every query tile, and the last, partial tile whole); every query would cost the oracle
    ~10 s at the smallest size that takes this schedule (35 tiles of 256 queries on 40,000
    rows).  The other queries are only compared between the two wave shapes, of which only the
    64-query one is paced (fused_pace); stats() does not report whether a launch was paced, so
    the test relies on the host's rule (one round of blocks, d = 128, 64-query register lists),
    which this size meets."""
    import torch
    nt, nq, d, k = 40_000, 20 * 512 + 17, 128, 10
    key = ("balanced",)
    if key not in _data:
        g = knn.Context(0)
        train = torch.empty((nt, d), dtype=torch.float32, device=DEV)
        labels = torch.empty(nt, dtype=torch.int32, device=DEV)
        test = torch.empty((nq, d), dtype=torch.float32, device=DEV)
        g.generate(train, labels, 0, d, 0, 59, 0, 10)
        g.generate(test, None, 0, d, 0, 59, 1, 10)
        torch.cuda.synchronize()
        g.close()
        qs = np.unique(np.concatenate([np.linspace(0, nq - 1, 500).astype(np.int64), np.arange(nq - 17, nq)]))
        bad, pred, dist, idx = oracle.knn(train.cpu().numpy(), labels.cpu().numpy(), test.cpu().numpy()[qs], k, 10)
        assert bad == 0
        _data[key] = (train, labels, test, qs, (pred, dist.view(np.uint32), idx))
    train, labels, test, qs, want = _data[key]
    got = _run(knn, monkeypatch, train, labels, test, k, qg)
    assert got[3]["train_segments"] > 1, got[3]
    _check((got[0][qs], got[1][qs], got[2][qs], got[3]), want, qg)
    other = _data.setdefault(("balanced", "got"), got)
    assert all(np.array_equal(x, y) for x, y in zip(got[:3], other[:3]))


@pytest.mark.parametrize("qg", ["1", "2"])
def test_fused_segments_with_scan_cursor(knn, oracle, monkeypatch, qg):
    """train_splits > 1: the segment schedule, whose blocks rotate their scan to the per-XCD
    cursor (any tile of the piece, not whole groups)."""
    train, labels, test = _rows(knn, "pieces", 64, "f32")
    got = _run(knn, monkeypatch, train, labels, test, 32, qg, splits=3)
    assert got[3]["train_segments"] == 3, got[3]
    _check(got, _oracle(oracle, knn, "pieces", 64, "f32", 32), qg)


@pytest.mark.parametrize("d,k,dtype,qg", [(128, 10, "f32", "1"), (128, 10, "f32", "2"), (64, 32, "f32", "2"),
                                          (256, 100, "bf16", None)])
def test_planted_neighbours_at_every_tile_position(knn, oracle, monkeypatch, d, k, dtype, qg):
    train, labels, test = _rows(knn, "tail", d, dtype, plant=True)
    nt = train.shape[0]
    want = _oracle(oracle, knn, "tail", d, dtype, k, plant=True)
    # the plants are what the oracle finds: distance 0 at the planted row
    assert np.array_equal(want[2][:256, 0], 512 + np.arange(256))
    assert np.array_equal(want[2][256:512, 0], nt - 273 + np.arange(256))
    assert (want[1][:512, 0] == 0).all()
    _check(_run(knn, monkeypatch, train, labels, test, k, qg), want, qg)
