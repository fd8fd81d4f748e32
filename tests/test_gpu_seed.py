"""GPU checks of the int8 filter's seeded thresholds (k_seed_thr, DESIGN.md "Seeded thresholds"): a
pass over a strided sample of the train tile blocks lowers every query's start threshold from
+inf to an upper bound of its k-th distance before k_gemm_fused runs.  The exact fp32 rescore is
unchanged, so every output must equal the direct form's bit for bit, with the seed
(KNN_FUSED_SEED=1) and without it (KNN_FUSED_SEED=0).

Every case runs algo="gemm_i8", profile=2, both settings of the hook, and asserts: indices,
distance bits and predictions equal to the direct form on every query (the direct form checked
against the C oracle on a sample); seeded_queries == 0 with the hook off; and, with it on, every
published seed (Context.last_seed) >= the direct form's k-th distance, compared as floats.

Shapes are the parked-pass tests' own: 65,536 x 1,024 and 16,447 x 517 (tails on both axes), both
queries-per-wave shapes, k = 1 .. 32 on both sides of the 32 / 64-group threshold (k = 16 | 17).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, C = 128, 10
KINDS = ["uniform", "ties", "saturate", "saturate_mild", "planted_seed", "nonfinite"]
_data = {}
_ref = {}
# How far a seed can lie above the k-th distance when k rows of k distinct groups are sampled:
# U - D <= 2 dl with dl = coef (qn + max tn) + eta + rho + nu, rows in [-1, 1)^128 (norms <= 128),
# coef = 1664 2^-24, rho <= 2 (|q| max|t - rt| + |q - rq| max|rt|) <= 4 sqrt(128) (s / 2) sqrt(128)
# = 256 s with s = 1 / 127 (every element rounds by at most s / 2), nu <= s2 = 2 s^2:
# 2 (0.0254 + 2.016 + 0.0002) < 4.1.  The unplanted k-th distance of these shapes is above 40.
SEED_BAND = 4.1


def _num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def sampled_tiles(knn, nt, bn, nq):
    """The tile blocks (of bn rows) the seed pass samples: the host's own rule."""
    lib = knn.load_library()
    fn = lib.knn_debug_seed_tiles
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                   ctypes.c_void_p]
    out = np.zeros(4096, np.int64)
    info = np.zeros(3, np.int64)
    ns = fn(nt, bn, nq, _num_cus(), out.ctypes.data, len(out), info.ctypes.data)
    return out[:ns]


def planted_rows(knn, nt, nq, k):
    """(train row, query, scale) triples of the "planted_seed" kind, k = 10.  A row's group is its
    place in its 32-row tile (64-row tile blocks are sampled as two 32-row tiles); rows are
    planted in tile blocks both shapes sample (32-row block 2 b and 64-row block b cover the same
    rows when both are sampled: the two rules are checked for a common set below)."""
    s32 = set(sampled_tiles(knn, nt, 32, nq).tolist())
    s64 = sampled_tiles(knn, nt, 64, nq)
    both = [int(b) for b in s64 if 2 * int(b) in s32]          # 64-row blocks whose first half both sample
    assert len(both) >= k + 2, (len(s32), len(s64), len(both))
    un = [b for b in range(nt // 64 - 2) if b not in set(s64.tolist()) and 2 * b not in s32 and 2 * b + 1 not in s32]
    assert len(un) >= k
    trip = []
    # (a query tile's sample may be cut into slices, each a subset of the sampled tile blocks with a
    # bound of its own: rows that must meet in one selection are planted in one tile)
    # query 0: its k nearest rows all in one group (place 5 of k sampled tiles): the group's maximum
    # is one row, the seed comes from the other groups -- valid, far above D_(k)
    trip += [(64 * both[i] + 5, 0, 1) for i in range(k)]
    # query 1: spread over k groups (places 0, 3, 6, ... of one sampled tile): seed within the band
    trip += [(64 * both[k] + 3 * i, 1, 1) for i in range(k)]
    # query 2: k + 1 exact duplicates in k + 1 groups of one sampled tile
    trip += [(64 * both[k + 1] + 12 + i, 2, 0) for i in range(k + 1)]
    # query 3: neighbours in unsampled tiles only
    trip += [(64 * un[i] + 7 + i, 3, 1) for i in range(k)]
    # queries 6 ..: one in each of the train set's last 40 rows
    trip += [(nt - 1 - r, 6 + r % 31, 1) for r in range(40)]
    return trip


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
    elif kind == "saturate":
        test = test * 4.0  # most query elements far outside the train range: a valid, useless seed
    elif kind == "saturate_mild":
        test = test * 1.05
    elif kind == "planted_seed":
        t = train.cpu().numpy()
        q = test.cpu().numpy()
        for i, (r, qi, sc) in enumerate(planted_rows(knn, nt, nq, 10)):
            assert 0 <= r < nt
            t[r] = q[qi] + rng.uniform(-1e-3, 1e-3, D).astype(np.float32) * sc * (1 + i % 5)
            if sc == 0:
                t[r] = q[qi] + np.float32(2e-3)  # (the duplicates: one row, k + 1 times)
        train = torch.from_numpy(t).to(dev)
    elif kind == "nonfinite":
        q = test.cpu().numpy()
        q[3, 17] = np.nan
        q[64, :] = np.nan
        q[100, 5] = np.inf
        q[101, 6] = -np.inf
        q[515, 0], q[515, 127] = np.inf, -np.inf
        test = torch.from_numpy(q).to(dev)
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


def _check(knn, oracle, monkeypatch, nt, nq, kind, k, qg, train_splits=0, sampled=True):
    """Both settings of the hook on one input; returns ({hook: stats}, the seeds of the run with it).
    sampled = False: a train set the sample rule takes nothing from -- the pass must not run."""
    monkeypatch.setenv("KNN_FUSED_QG", qg)  # snapshots at knn_create
    train, labels, test = _inputs(knn, nt, nq, kind)
    ref = _reference(knn, oracle, nt, nq, kind, k)
    dk = ref[1].view(np.float32)[:, k - 1]
    stats, seeds = {}, None
    for seed in ("1", "0"):
        monkeypatch.setenv("KNN_FUSED_SEED", seed)
        c = knn.Context(0, algo="gemm_i8", profile=2, train_splits=train_splits)
        try:
            got = _run(c, train, labels, test, k)
            st = stats[seed] = c.stats()
            sd = c.last_seed(nq)
        finally:
            c.close()
        print(f"seed={seed} nt={nt} nq={nq} {kind} k={k} qg={qg}: candidates/query {st['candidates'] / nq:.1f} "
              f"seeded {st['seeded_queries']} fallback {st['fallback_queries']} segments {st['train_segments']}")
        assert st["filter_element"] == "i8" and st["fused_norm"], st
        assert st["queries_per_wave"] == 32 * int(qg), st
        assert np.array_equal(got[2], ref[2])
        assert np.array_equal(got[1], ref[1])
        assert np.array_equal(got[0], ref[0])
        if kind in ("uniform", "planted_seed"):
            assert st["fallback_queries"] == 0, st  # the exact scan must not stand in for the filter
        if seed == "1" and not sampled:
            assert st["seeded_queries"] == 0 and len(sd) == 0, st
        elif seed == "1":
            seeds = sd
            assert len(sd) == nq and not np.any(np.isnan(sd))
            assert st["seeded_queries"] == int(np.sum(np.isfinite(sd))), st
            # validity, directly: no seed below the exact k-th distance
            with np.errstate(divide="ignore", invalid="ignore"):
                print(f"  seed / D_(k): min {np.nanmin(sd / dk):.4f} median {np.nanmedian(sd / dk):.4f}")
            assert np.all(sd >= dk)
        else:
            assert st["seeded_queries"] == 0 and len(sd) == 0, st
    return stats, seeds


@pytest.mark.parametrize("qg", ["1", "2"])
@pytest.mark.parametrize("k", [1, 10, 16, 17, 32])
@pytest.mark.parametrize("nt,nq", [(65_536, 1024), (16_447, 517)])
def test_seed_parity_uniform(knn, oracle, monkeypatch, nt, nq, k, qg):
    stats, _ = _check(knn, oracle, monkeypatch, nt, nq, "uniform", k, qg)
    assert stats["1"]["seeded_queries"] == nq, stats["1"]


@pytest.mark.parametrize("qg", ["1", "2"])
@pytest.mark.parametrize("kind", ["ties", "saturate", "saturate_mild"])
def test_seed_valid_on_kinds(knn, oracle, monkeypatch, kind, qg):
    """Duplicate rows and queries that are train rows; queries far (x4) and just (x1.05) outside the
    train range -- the seed stays at or above the k-th distance, the outputs stay the direct form's."""
    _check(knn, oracle, monkeypatch, 65_536, 1024, kind, 10, qg)


@pytest.mark.parametrize("qg", ["1", "2"])
@pytest.mark.parametrize("train_splits", [1, 0])
def test_seed_planted(knn, oracle, monkeypatch, qg, train_splits):
    """Neighbours planted by the host's own sample rule (planted_rows)."""
    nt, nq, k = 65_536, 1024, 10
    stats, sd = _check(knn, oracle, monkeypatch, nt, nq, "planted_seed", k, qg, train_splits)
    dk = _reference(knn, oracle, nt, nq, "planted_seed", k)[1].view(np.float32)[:, k - 1]
    assert stats["1"]["seeded_queries"] == nq
    assert dk[0] < 1e-2 and dk[1] < 1e-2 and dk[2] < 1e-2 and dk[3] < 1e-2, dk[:4]  # the planted rows are the neighbours
    print(f"planted: seeds {sd[:4]} D_(k) {dk[:4]}")
    assert sd[0] > 10.0          # one group: the seed is another group's row
    assert sd[1] <= dk[1] + SEED_BAND  # k groups: the seed is the k-th planted row's bound
    assert sd[2] <= dk[2] + SEED_BAND  # k + 1 duplicates in k + 1 groups
    assert sd[3] > 10.0          # unsampled tiles: nothing planted is seen


@pytest.mark.parametrize("qg", ["1", "2"])
def test_seed_only_lowers_thresholds(knn, oracle, monkeypatch, qg):
    """One piece per query tile: the filter keeps no more rows with the seed than without it."""
    stats, _ = _check(knn, oracle, monkeypatch, 65_536, 1024, "uniform", 10, qg, train_splits=1)
    assert stats["1"]["train_segments"] == 1 and stats["0"]["train_segments"] == 1
    assert stats["1"]["candidates"] <= stats["0"]["candidates"], (stats["1"], stats["0"])


@pytest.mark.parametrize("qg", ["1", "2"])
def test_seed_too_few_rows(knn, oracle, monkeypatch, qg):
    """255 train rows: the sample rule yields nothing (an eighth of the rows is under 64)."""
    assert len(sampled_tiles(knn, 255, 32 if qg == "2" else 64, 517)) == 0
    stats, _ = _check(knn, oracle, monkeypatch, 255, 517, "uniform", 10, qg, sampled=False)
    assert stats["1"]["seeded_queries"] == 0


@pytest.mark.parametrize("qg", ["1", "2"])
def test_seed_many_pieces(knn, oracle, monkeypatch, qg):
    """262,144 x 300: query tiles cut into many pieces, the sample cut into slices."""
    stats, _ = _check(knn, oracle, monkeypatch, 262_144, 300, "uniform", 10, qg)
    assert stats["1"]["train_segments"] > 1 and stats["1"]["seeded_queries"] == 300, stats["1"]


@pytest.mark.parametrize("qg", ["1", "2"])
def test_seed_non_finite_queries(knn, monkeypatch, qg):
    """Query rows holding a NaN or +-inf: the same status (such a query has fewer than k finite
    distances: KNN_ERANGE) and identical outputs on the other queries with the hook on and off,
    and no seed for those rows."""
    monkeypatch.setenv("KNN_FUSED_QG", qg)
    train, labels, test = _inputs(knn, 16_447, 517, "nonfinite")
    bad = [3, 64, 100, 101, 515]
    out = {}
    for seed in ("1", "0"):
        monkeypatch.setenv("KNN_FUSED_SEED", seed)
        c = knn.Context(0, algo="gemm_i8", profile=2)
        try:
            import torch
            p = torch.zeros(517, dtype=torch.int32, device=test.device)
            dd = torch.zeros((517, 10), dtype=torch.float32, device=test.device)
            ii = torch.zeros((517, 10), dtype=torch.int32, device=test.device)
            status = None
            try:
                c.predict_device(train, labels, test, 10, C, p, dist=dd, idx=ii)
            except knn.KnnError as e:
                status = e.status
            torch.cuda.synchronize()
            out[seed] = (status,) + tuple(np.delete(x.cpu().numpy(), bad, axis=0) for x in (p, dd.view(torch.int32), ii))
            if seed == "1":
                sd = c.last_seed(517)
                assert not np.any(np.isnan(sd))
                assert len(sd) == 0 or not np.any(np.isfinite(sd[bad])), sd[bad]
        finally:
            c.close()
    print(f"status {out['1'][0]}")
    assert out["1"][0] == out["0"][0]
    assert _same(out["1"][1:], out["0"][1:])


@pytest.mark.parametrize("qg", ["1", "2"])
def test_seed_one_context_reused(knn, oracle, monkeypatch, qg):
    """1,024 queries, then 517 on another train set, then 517 on the first: nothing of a call's
    seed survives."""
    monkeypatch.setenv("KNN_FUSED_QG", qg)
    monkeypatch.setenv("KNN_FUSED_SEED", "1")
    k = 10
    tr, lab, te = _inputs(knn, 65_536, 1024, "uniform")
    tr2, lab2, te2 = _inputs(knn, 16_447, 517, "uniform")
    c = knn.Context(0, algo="gemm_i8", profile=2)
    try:
        for train, labels, test, shape in ((tr, lab, te, (65_536, 1024)), (tr2, lab2, te2, (16_447, 517)),
                                           (tr, lab, te[:517], None)):
            nq = test.shape[0]
            got = _run(c, train, labels, test, k)
            st = c.stats()
            assert st["filter_element"] == "i8" and st["seeded_queries"] == nq and st["fallback_queries"] == 0, st
            ref = _reference(knn, oracle, *shape, "uniform", k) if shape else \
                tuple(x[:517] for x in _reference(knn, oracle, 65_536, 1024, "uniform", k))
            assert _same(got, ref)
            sd = c.last_seed(nq)
            assert len(sd) == nq and np.all(sd >= ref[1].view(np.float32)[:, k - 1])
    finally:
        c.close()
