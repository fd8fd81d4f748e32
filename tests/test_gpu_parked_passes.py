"""GPU checks of the int8 filter's parked passes (k_gemm_fused<..., PARK>, DESIGN.md "Parked
passes"): a tile that passes the fast test is copied into a per-lane slot in LDS and visited
later, in batches.  The exact fp32 rescore is unchanged, so every output must equal the direct
form's bit for bit -- with the parked path (KNN_FUSED_PARK=1) and with the immediate one
(KNN_FUSED_PARK=0), which stays in the library.

Every case asserts, for both settings: indices, distance bits and predictions equal to the direct
form on every query (the direct form checked against the C oracle on a sample),
stats()["filter_element"] == "i8", parked_passes > 0 with the parked path and == 0 without,
and no exact-scan fallback on uniform rows.

Shapes: the smallest at which each mechanism is reached -- 65,536 x 1,024 and 16,447 x 517
(tails on both axes), both queries-per-wave shapes, k = 1 (passes sparse from a few thousand rows
on: most of the scan parks) to 32 (the longer lists); neighbours planted where the ring fills,
where a record holds two values, on both sides of a share tile and in the last rows; a shape
whose query tiles are cut into many pieces (list exchange, two pieces per block); and one context
called twice with different query counts.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, C = 128, 10
KINDS = ["uniform", "ties", "saturate_mild", "planted_park"]
_data = {}
_ref = {}


def planted_rows(nt):
    """(train row, query) pairs of the "planted_park" kind.  Tile numbers are those of one piece
    over the whole train set (train_splits = 1): 32-row tiles on the 64-query shape, 64-row
    tiles (two accumulators of 32 rows) on the 32-query one; threshold exchanges fall on tiles
    63, 127, ... of a piece.  Row r of a tile belongs to lane half (r >> 2) & 1."""
    pairs = []
    # (a) three neighbours of one query in one lane half of three consecutive 32-row tiles inside
    # one 64-tile interval (tiles 1290 .. 1292; 64-row tiles 645, 645, 646): one more record than
    # the lane has slots
    pairs += [(32 * t + 5, 0) for t in (1290, 1291, 1292)]
    # (b) two in one tile and one lane half (rows 1 and 9): two values in one record
    pairs += [(32 * 1400 + 1, 1), (32 * 1400 + 9, 1)]
    # (c) the tile before and the tile after a share tile: tiles 63 / 64 and 1471 / 1472 of 32
    # rows, 63 / 64 and 703 / 704 of 64 rows
    pairs += [(32 * 63 + 6, 2), (32 * 64 + 6, 2), (32 * 1471 + 6, 3), (32 * 1472 + 6, 3)]
    pairs += [(64 * 63 + 6, 4), (64 * 64 + 6, 4), (64 * 703 + 38, 5), (64 * 704 + 38, 5)]
    # (d) one in each of the train set's last 40 rows: pending at the drain, the row_end tail
    pairs += [(nt - 1 - r, (6 + r) % 37) for r in range(40)]
    # (e) every place of a barrier group (eight 32-row tiles or four 64-row ones), first group and
    # a middle one
    places = [32 * p + o for p in range(8) for o in (0, 5, 31)]
    pairs += [(r, (9 + i) % 37) for i, r in enumerate(places + [256 * (nt // 512) + r for r in places])]
    return pairs


def _inputs(knn, nt, nq, kind):
    """(train, labels, test) device tensors of one (shape, kind), built once."""
    import torch
    key = (nt, nq, kind)
    if key in _data:
        return _data[key]
    dev = "cuda:0"
    rng = np.random.default_rng(nt + 31 * nq + 7 * KINDS.index(kind))
    c = knn.Context(0)
    try:
        train = torch.empty((nt, D), dtype=torch.float32, device=dev)
        labels = torch.empty(nt, dtype=torch.int32, device=dev)
        test = torch.empty((nq, D), dtype=torch.float32, device=dev)
        c.generate(train, labels, 0, D, 0, 17, 0, C)
        c.generate(test, None, 0, D, 0, 17, 1, C)
        torch.cuda.synchronize()
    finally:
        c.close()
    if kind == "ties":
        # duplicate train rows (ties go to the smaller index) and queries that are train rows
        t = train.cpu().numpy()
        h = nt // 3
        t[h:h + 4000] = t[:4000]
        t[nt - 300:] = t[100:400]
        q = test.cpu().numpy()
        q[::3] = t[rng.integers(0, nt, len(q[::3]))]
        q[1::7] = t[rng.integers(0, 4000, len(q[1::7]))]
        train, test = torch.from_numpy(t).to(dev), torch.from_numpy(q).to(dev)
    elif kind == "saturate_mild":
        test = test * 1.05  # a few per cent of the query elements just past the train range
    elif kind == "planted_park":
        t = train.cpu().numpy()
        q = test.cpu().numpy()
        for i, (r, qi) in enumerate(planted_rows(nt)):
            assert 0 <= r < nt
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
        train, labels, test = _inputs(knn, nt, nq, kind)
        c = knn.Context(0, algo="direct")
        try:
            ref = _run(c, train, labels, test, k)
        finally:
            c.close()
        qs = np.unique(np.concatenate([np.arange(0, 6), np.linspace(0, nq - 1, 5).astype(np.int64)]))
        bad, op, od, oi = oracle.knn(train.cpu().numpy(), labels.cpu().numpy(), test.cpu().numpy()[qs], k, C)
        assert bad == 0
        assert np.array_equal(oi, ref[2][qs]) and np.array_equal(od.view(np.uint32), ref[1][qs])
        assert np.array_equal(op, ref[0][qs])
        _ref[key] = ref
    return _ref[key]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _check(knn, oracle, monkeypatch, nt, nq, kind, k, qg, train_splits=0):
    """Both settings of the hook on one input; returns the parked run's stats."""
    monkeypatch.setenv("KNN_FUSED_QG", qg)  # snapshots at knn_create
    train, labels, test = _inputs(knn, nt, nq, kind)
    ref = _reference(knn, oracle, nt, nq, kind, k)
    stats = {}
    for park in ("1", "0"):
        monkeypatch.setenv("KNN_FUSED_PARK", park)
        c = knn.Context(0, algo="gemm_i8", profile=2, train_splits=train_splits)
        try:
            got = _run(c, train, labels, test, k)
            st = stats[park] = c.stats()
        finally:
            c.close()
        print(f"park={park} nt={nt} nq={nq} {kind} k={k} qg={qg}: candidates/query "
              f"{st['candidates'] / nq:.1f} parked {st['parked_passes']} fallback {st['fallback_queries']} "
              f"segments {st['train_segments']}")
        assert st["filter_element"] == "i8" and st["fused_norm"], st
        assert st["queries_per_wave"] == 32 * int(qg), st
        assert np.array_equal(got[2], ref[2])
        assert np.array_equal(got[1], ref[1])
        assert np.array_equal(got[0], ref[0])
        if kind in ("uniform", "planted_park"):
            assert st["fallback_queries"] == 0, st  # the exact scan must not stand in for the filter
        if park == "1":
            assert st["parked_passes"] > 0, st
        else:
            assert st["parked_passes"] == 0, st
    return stats["1"]


@pytest.mark.parametrize("qg", ["1", "2"])
@pytest.mark.parametrize("k", [1, 10, 17, 32])
@pytest.mark.parametrize("nt,nq", [(65_536, 1024), (16_447, 517)])
def test_parked_parity_uniform(knn, oracle, monkeypatch, nt, nq, k, qg):
    _check(knn, oracle, monkeypatch, nt, nq, "uniform", k, qg)


@pytest.mark.parametrize("qg", ["1", "2"])
@pytest.mark.parametrize("train_splits", [1, 0])
def test_parked_parity_planted(knn, oracle, monkeypatch, qg, train_splits):
    """Planted neighbours (planted_rows): as one piece over the whole train set, where the tile
    numbers are the planted ones, and under the schedule's own pieces."""
    st = _check(knn, oracle, monkeypatch, 65_536, 1024, "planted_park", 10, qg, train_splits)
    if train_splits == 1:
        assert st["train_segments"] == 1, st


@pytest.mark.parametrize("qg", ["1", "2"])
def test_parked_parity_many_pieces(knn, oracle, monkeypatch, qg):
    """262,144 x 300: query tiles cut into many pieces, blocks running two pieces, the list
    exchange on the 32-query shape."""
    st = _check(knn, oracle, monkeypatch, 262_144, 300, "uniform", 10, qg)
    assert st["train_segments"] > 1, st


@pytest.mark.parametrize("qg", ["1", "2"])
@pytest.mark.parametrize("kind", ["ties", "saturate_mild"])
def test_parked_parity_kinds(knn, oracle, monkeypatch, kind, qg):
    nq = 1024
    st = _check(knn, oracle, monkeypatch, 65_536, nq, kind, 10, qg)
    assert st["candidates"] / nq < 8 * 2048, st
    if kind == "saturate_mild":
        assert st["fallback_queries"] <= nq // 64, st


@pytest.mark.parametrize("qg", ["1", "2"])
def test_one_context_two_query_counts(knn, oracle, monkeypatch, qg):
    """1,024 queries, then 517 on the same context: nothing of a call's ring survives."""
    monkeypatch.setenv("KNN_FUSED_QG", qg)
    monkeypatch.setenv("KNN_FUSED_PARK", "1")
    k = 10
    tr, lab, te = _inputs(knn, 65_536, 1024, "uniform")
    tr2, lab2, te2 = _inputs(knn, 16_447, 517, "uniform")
    c = knn.Context(0, algo="gemm_i8", profile=2)
    try:
        for train, labels, test, shape in ((tr, lab, te, (65_536, 1024)), (tr2, lab2, te2, (16_447, 517)),
                                           (tr, lab, te[:517], None)):
            got = _run(c, train, labels, test, k)
            st = c.stats()
            assert st["filter_element"] == "i8" and st["parked_passes"] > 0 and st["fallback_queries"] == 0, st
            ref = _reference(knn, oracle, *shape, "uniform", k) if shape else \
                tuple(x[:517] for x in _reference(knn, oracle, 65_536, 1024, "uniform", k))
            assert _same(got, ref)
    finally:
        c.close()
