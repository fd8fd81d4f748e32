"""Every device path on strided rows: [n][ld] with ld > d, the pad columns poisoned.

Every entry point takes rows as [n][ld], ld >= d, and the device wrappers accept column views
(x[:, c0:c0 + d]) of a wider tensor, so the row stride is part of the contract (bench.py itself
runs d = 11 at ld = 12).  Each case copies the generator's contiguous rows into a view of a
poisoned parent

    parent = full((n + 1, LD), poison);  view = parent[:n, c0:c0 + d]

(the spare row keeps any over-read inside the allocation) and asserts

  * indices, distance bits and predictions equal a reference computed from the contiguous CPU
    rows (the oracle for squared Euclidean, test_metric_cpu's restatement for the other metrics,
    the exactly widened floats for bf16 data);
  * the same call on .contiguous() copies (d % 4 != 0: the narrowest 16-byte-aligned rows, zero
    padded), on a context of the same kind, gives the same arrays;
  * for the filter paths: the filter ran (train_segments), on the expected operands, and sent no
    query to the exact fallback scan -- on the strided run and on the contiguous run, asserted
    separately.  A norm or an int8 scale that picks up a pad column does not give a wrong answer
    (the lists overflow or the norm check trips and the exact scan delivers the right bits): only
    these counters show that the filter did not do its job;
  * the parent is unchanged, bit for bit (nothing writes through the caller's pointer).

Poisons: NaN (a pad element that reaches a norm, a scale, a distance or an MFMA operand shows
up; fmaxf ignores it, so under Chebyshev it does not) and 1.0e3 (finite: inflates norms and
distances, and gives the int8 filter a scale of about 7.9, so unit-range rows quantise to 0).

Layouts, in units of u = 4 floats / 8 bf16 elements (rows stay 16-byte aligned):
    pad     train and queries LD = d + u (d % 4 != 0: LD = d rounded up to 4), c0 = 0
    offset  train LD = d + 2u, c0 = u;  queries LD = d + 5u, c0 = 2u (the two strides differ)
    half    train LD = 2d, c0 = d (the right half of a wider table);  queries contiguous
"""
import ctypes

import numpy as np
import pytest

from test_metric_cpu import CHEBYSHEV, MANHATTAN, bits, metric_reference, vote_reference
from test_metric_cpu import NAMES as METRIC_NAMES
from test_regress_cpu import error_sums, fbits, regress_reference
from test_sweep_cpu import sweep_reference
from test_weighted_cpu import INV_DIST, remove_self, weighted_reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C = 10
POISONS = {"nan": float("nan"), "1e3": 1.0e3}
NT, NQ = 16_447, 517        # tails on both axes; nt % 64 != 0 reaches the fp32 filter's 64-row pad copy
SEED = 53

_rows_cache = {}
_ref_cache = {}


def _rows(oracle, n, d, stream, kind=0):
    """The generator's contiguous [n][d] rows and labels (kind 0: fp32 grid, 1: bf16-exact), once."""
    key = (n, d, stream, kind)
    if key not in _rows_cache:
        f, lab = oracle.gen(SEED + d, stream, 0, n, d, kind=kind)
        _rows_cache[key] = (f, lab)
    return _rows_cache[key]


def _oracle(oracle, tr, tl, te, k, key):
    """(pred, dist bits, idx) of the oracle on contiguous CPU rows, once per key."""
    if key not in _ref_cache:
        bad, pred, dist, idx = oracle.knn(tr, tl, te, k, C)
        assert bad == 0
        _ref_cache[key] = (pred, dist.view(np.uint32), idx)
    return _ref_cache[key]


def _layout(name, d, unit=4):
    """((LD, c0) of train, (LD, c0) of the queries)."""
    if name == "pad":
        ld = (d // unit + 1) * unit
        return (ld, 0), (ld, 0)
    if name == "offset":
        return (d + 2 * unit, unit), (d + 5 * unit, 2 * unit)
    assert name == "half"
    return (2 * d, d), (d, 0)


class Strided:
    """rows [n][d] (numpy float32) inside a poisoned parent [n + 1][LD] at column c0: the CPU
    parent (what must still be there after the calls), its device copy and the device view."""

    def __init__(self, rows, ld, c0, poison, bf16=False):
        import torch
        n, d = rows.shape
        assert c0 + d <= ld
        self.cpu = torch.full((n + 1, ld), poison, dtype=torch.bfloat16 if bf16 else torch.float32)
        self.cpu[:n, c0:c0 + d] = torch.from_numpy(np.array(rows))
        if bf16:  # the rows are bf16-exact: the reference runs on the same numbers
            assert np.array_equal(self.cpu[:n, c0:c0 + d].float().numpy(), rows)
        self.dev = self.cpu.to(DEV)
        self.view = self.dev[:n, c0:c0 + d]
        assert self.view.data_ptr() % 16 == 0 and (ld * self.cpu.element_size()) % 16 == 0

    def intact(self):
        import torch
        it = torch.int16 if self.cpu.dtype == torch.bfloat16 else torch.int32
        return torch.equal(self.dev.cpu().view(it), self.cpu.view(it))


def _packed(view):
    """The view's contiguous copy; for d % 4 != 0, where device rows of d floats are not 16-byte
    aligned, the narrowest aligned rows instead: zero columns up to a multiple of 4, never read
    (the call passes the true d)."""
    import torch
    n, d = view.shape
    if (d * view.element_size()) % 16 == 0:
        return view.contiguous()
    out = torch.zeros((n, d + -d % 4), dtype=view.dtype, device=view.device)
    out[:, :d] = view
    return out


def _predict(ctx, train, labels, test, k, d=None):
    import torch
    nq = test.shape[0]
    pred = torch.empty(nq, dtype=torch.int32, device=DEV)
    dist = torch.empty((nq, k), dtype=torch.float32, device=DEV)
    idx = torch.empty((nq, k), dtype=torch.int32, device=DEV)
    ctx.predict_device(train, labels, test, k, C, pred, dist, idx, d=d)
    torch.cuda.synchronize()
    return (pred.cpu().numpy(), dist.cpu().numpy().view(np.uint32), idx.cpu().numpy()), ctx.stats()


def _assert_same(got, want, what):
    assert np.array_equal(got[2], want[2]), f"{what}: indices"
    assert np.array_equal(got[1], want[1]), f"{what}: distance bits"
    assert np.array_equal(got[0], want[0]), f"{what}: predictions"


def _assert_filter(st, expect, what):
    """The filter ran, on the expected operands, and needed no exact fallback scan."""
    operands, element, fused = expect
    print(what, {k: st[k] for k in ("train_segments", "filter_operands", "filter_element", "fused_norm",
                                    "fallback_queries")})
    assert st["train_segments"] >= 1, (what, st)
    assert st["filter_operands"] == operands and st["filter_element"] == element, (what, st)
    assert st["fused_norm"] == fused, (what, st)
    assert st["fallback_queries"] == 0, (what, st)


def _check(knn, make_ctx, tr, tl, te, ks, tlay, qlay, poison, ref_of, expect=None, bf16=False, qpw=None):
    """One case: the strided run against the reference and against the contiguous run on a
    context of the same kind, the filter's counters of both runs, the parents untouched."""
    import torch
    st_tr = Strided(tr, *tlay, poison, bf16)
    st_te = Strided(te, *qlay, poison, bf16)
    lab = torch.from_numpy(np.array(tl)).to(DEV)
    c_tr, c_te = _packed(st_tr.view), _packed(st_te.view)
    assert st_tr.view.stride(0) == tlay[0] and st_te.view.stride(0) == qlay[0]
    ctx_s, ctx_c = make_ctx(), make_ctx()
    try:
        for k in ks:
            want = ref_of(k)
            got, st = _predict(ctx_s, st_tr.view, lab, st_te.view, k)
            cont, st_c = _predict(ctx_c, c_tr, lab, c_te, k, d=tr.shape[1])
            _assert_same(cont, want, f"contiguous k={k}")
            _assert_same(got, want, f"strided k={k}")
            if expect is not None:
                _assert_filter(st_c, expect, f"contiguous k={k}")
                _assert_filter(st, expect, f"strided k={k}")
            if qpw is not None:
                assert st["queries_per_wave"] == qpw and st_c["queries_per_wave"] == qpw, (st, st_c)
    finally:
        ctx_s.close()
        ctx_c.close()
    assert st_tr.intact() and st_te.intact()


# ---------------------------------------------------------------------------------------
# 1. filter paths, predict_device.  16,447 x 517: both axes have tails, and for "gemm" (the fp32
# MFMA filter, which DMAs the caller's rows into LDS at pitch ld) nt % 64 != 0 takes the copy
# onto the 64-row grid; 16,384 x 300 lets its DMA read the caller's rows with no copy between.
# gemm_bf16 at d = 256, k = 128 is the one shape of the rounded operands with no fused kernel
# (the LDS heaps of k > 116 do not fit beside 512-byte rows): k_round_rows builds the operands.
# (algo, d, nt, nq, ks, context arguments, (filter_operands, filter_element, fused_norm))
# ---------------------------------------------------------------------------------------
FILTERS = [
    ("gemm", 32, NT, NQ, (10, 32), {}, ("f32", None, False)),
    ("gemm", 128, NT, NQ, (10, 32), {}, ("f32", None, False)),
    ("gemm", 32, 16_384, 300, (10, 32), {}, ("f32", None, False)),
    ("gemm", 128, 16_384, 300, (10, 32), {}, ("f32", None, False)),
    ("gemm_split", 64, NT, NQ, (10, 32), {}, ("bf16x3 split", "bf16", False)),
    ("gemm_bf16", 64, NT, NQ, (10, 32), {}, ("bf16 rounded", "bf16", True)),
    ("gemm_bf16", 256, NT, NQ, (10, 32), {}, ("bf16 rounded", "bf16", True)),
    ("gemm_bf16", 256, NT, NQ, (128,), {}, ("bf16 rounded", "bf16", False)),
    ("gemm_i8", 128, NT, NQ, (10, 32), {"profile": 2}, ("bf16 rounded", "i8", True)),
    ("auto", 128, NT, NQ, (10, 32), {"cache_train": True}, ("bf16 rounded", "i8", True)),
]


def _filter_case(knn, oracle, algo, d, nt, nq, ks, kw, expect, layout, poison, qpw=None):
    tr, tl = _rows(oracle, nt, d, 0)
    te, _ = _rows(oracle, nq, d, 1)
    tlay, qlay = _layout(layout, d)
    _check(knn, lambda: knn.Context(0, algo=algo, **kw), tr, tl, te, ks, tlay, qlay, POISONS[poison],
           lambda k: _oracle(oracle, tr, tl, te, k, (nt, nq, d, 0, k)), expect, qpw=qpw)


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("layout", ["pad", "offset", "half"])
@pytest.mark.parametrize("algo,d,nt,nq,ks,kw,expect", FILTERS,
                         ids=[f"{f[0]}-d{f[1]}-{f[2]}x{f[3]}-k{'_'.join(map(str, f[4]))}" for f in FILTERS])
def test_filter_paths(knn, oracle, algo, d, nt, nq, ks, kw, expect, layout, poison):
    _filter_case(knn, oracle, algo, d, nt, nq, ks, kw, expect, layout, poison)


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("park", ["0", "1"])
@pytest.mark.parametrize("qg", ["1", "2"])
def test_i8_filter_shapes(knn, oracle, monkeypatch, qg, park, poison):
    """The int8 filter's queries-per-wave shapes, with its parked passes off and on (the hooks are
    read at knn_create), on layout "offset"."""
    monkeypatch.setenv("KNN_FUSED_QG", qg)
    monkeypatch.setenv("KNN_FUSED_PARK", park)
    _filter_case(knn, oracle, "gemm_i8", 128, NT, NQ, (10, 32), {"profile": 2}, ("bf16 rounded", "i8", True),
                 "offset", poison, qpw=32 * int(qg))


# ---------------------------------------------------------------------------------------
# 2. bf16 data (torch.bfloat16 views; u = 8 elements) on the direct form and on "gemm": the fused
# bf16 filter at d = 64 / 128; at d = 256, k = 128 it has no kernel, and k_gemm_filter DMAs the
# caller's bf16 rows (through the 64-row pad copy: nt % 64 != 0).  The reference runs on the
# exactly widened values.
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("layout", ["pad", "offset"])
@pytest.mark.parametrize("d,k,fused", [(64, 10, True), (128, 10, True), (256, 128, False)])
@pytest.mark.parametrize("algo", ["direct", "gemm"])
def test_bf16_rows(knn, oracle, algo, d, k, fused, layout, poison):
    tr, tl = _rows(oracle, NT, d, 0, kind=1)
    te, _ = _rows(oracle, NQ, d, 1, kind=1)
    tlay, qlay = _layout(layout, d, unit=8)
    _check(knn, lambda: knn.Context(0, algo=algo), tr, tl, te, (k,), tlay, qlay, POISONS[poison],
           lambda kk: _oracle(oracle, tr, tl, te, kk, (NT, NQ, d, 1, kk)),
           ("bf16", "bf16", fused) if algo == "gemm" else None, bf16=True)


# ---------------------------------------------------------------------------------------
# 3. direct forms.  k_direct_rows (d <= 16, k <= 16): (11, 12) is the benchmark's own layout; for
# d % 4 != 0 the poison sits in the 1 to 3 columns directly behind the row.  k_direct_tile: one
# and several 128-feature chunks' worth of row, d % 4 == 0 with a float4 tail.  (d, LD), c0 = 0,
# and layout "offset" where d % 4 == 0.
# ---------------------------------------------------------------------------------------
def _direct_case(knn, oracle, algo, d, nt, nq, ks, tlay, qlay, poison):
    tr, tl = _rows(oracle, nt, d, 0)
    te, _ = _rows(oracle, nq, d, 1)
    _check(knn, lambda: knn.Context(0, algo=algo), tr, tl, te, ks, tlay, qlay, POISONS[poison],
           lambda k: _oracle(oracle, tr, tl, te, k, (nt, nq, d, 0, k)))


def _direct_layouts(shapes):
    out = []
    for d, ld in shapes:
        out.append((d, (ld, 0), (ld, 0)))
        if d % 4 == 0:
            out.append((d,) + _layout("offset", d))
    return out


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("d,tlay,qlay", _direct_layouts([(11, 12), (7, 8), (16, 20)]))
def test_direct_rows(knn, oracle, d, tlay, qlay, poison):
    _direct_case(knn, oracle, "direct", d, 3_000, 33, (1, 16), tlay, qlay, poison)


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("d,tlay,qlay", _direct_layouts([(32, 48), (100, 104), (128, 132), (40, 48)]))
def test_direct_tile(knn, oracle, d, tlay, qlay, poison):
    _direct_case(knn, oracle, "direct", d, 9_000, 257, (5, 100), tlay, qlay, poison)


@pytest.mark.parametrize("poison", list(POISONS))
def test_direct_scan(knn, oracle, poison):
    tlay, qlay = _layout("offset", 100)
    _direct_case(knn, oracle, "direct_scan", 100, 5_000, 130, (10,), tlay, qlay, poison)


# ---------------------------------------------------------------------------------------
# 4. metrics (k_metric_tile), on a direct context.  Under Chebyshev a NaN that is read is ignored
# by fmaxf: the 1.0e3 poison is the one that bites there.
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("d,ld", [(11, 12), (128, 136)])
@pytest.mark.parametrize("metric", [MANHATTAN, CHEBYSHEV], ids=lambda m: METRIC_NAMES[m])
def test_metrics(knn, oracle, metric, d, ld, poison):
    nt, nq, k = 9_000, 257, 10
    tr, tl = _rows(oracle, nt, d, 0)
    te, _ = _rows(oracle, nq, d, 1)

    def ref(kk):
        key = (nt, nq, d, "metric", metric, kk)
        if key not in _ref_cache:
            rdist, ridx = metric_reference(tr, te, kk, metric)
            assert (ridx >= 0).all()
            _ref_cache[key] = (vote_reference(ridx, tl, C), bits(rdist), ridx)
        return _ref_cache[key]

    _check(knn, lambda: knn.Context(0, algo="direct", metric=METRIC_NAMES[metric]), tr, tl, te, (k,),
           (ld, 0), (ld, 0), POISONS[poison], ref)


# ---------------------------------------------------------------------------------------
# 5. other entry points: d = 128, layout "offset", NaN poison, a gemm_i8 context, 16,447 x 517
# ---------------------------------------------------------------------------------------
I8 = ("bf16 rounded", "i8", True)


@pytest.fixture(scope="module")
def entry(knn, oracle):
    import torch
    d = 128
    tr, tl = _rows(oracle, NT, d, 0)
    te, _ = _rows(oracle, NQ, d, 1)
    tlay, qlay = _layout("offset", d)
    s_tr = Strided(tr, *tlay, POISONS["nan"])
    s_te = Strided(te, *qlay, POISONS["nan"])
    lab = torch.from_numpy(np.array(tl)).to(DEV)
    ctx = knn.Context(0, algo="gemm_i8", profile=2)
    yield ctx, tr, tl, te, s_tr, s_te, lab
    ctx.close()
    assert s_tr.intact() and s_te.intact()


def test_shards_of_one_strided_parent(knn, oracle, entry):
    """shard_topk_device on two row slices of the strided train view (idx_base 0 and 8,000: views
    whose pointer is not the parent's), then merge_vote_device: the whole train set's reference."""
    import torch
    ctx, tr, tl, te, s_tr, s_te, lab = entry
    k = 10
    want = _oracle(oracle, tr, tl, te, k, (NT, NQ, 128, 0, k))
    rec = torch.empty((2, NQ, 3, k), dtype=torch.int32, device=DEV)
    for s, (a, b) in enumerate(((0, 8_000), (8_000, NT))):
        part = s_tr.view[a:b]
        assert part.data_ptr() != s_tr.dev.data_ptr() and part.stride(0) == s_tr.dev.shape[1]
        ctx.shard_topk_device(part, lab[a:b], s_te.view, k, C, a, rec[s])
        _assert_filter(ctx.stats(), I8, f"shard {s}")
    pred = torch.empty(NQ, dtype=torch.int32, device=DEV)
    dist = torch.empty((NQ, k), dtype=torch.float32, device=DEV)
    idx = torch.empty((NQ, k), dtype=torch.int32, device=DEV)
    ctx.merge_vote_device(rec, k, C, pred, dist, idx)
    torch.cuda.synchronize()
    _assert_same((pred.cpu().numpy(), dist.cpu().numpy().view(np.uint32), idx.cpu().numpy()), want, "merged shards")
    assert s_tr.intact() and s_te.intact()


def _targets(n):
    return (np.random.default_rng(9).standard_normal(n) * 100).astype(np.float32)


@pytest.mark.parametrize("kind", ["sweep", "weighted", "regress"])
def test_leave_one_out_on_a_strided_table(knn, oracle, entry, kind):
    """The sweeps with self_base = 4,000 and the query set train_view[4000:4517] (leave-one-out on
    a slice of a strided table), kmax = 16: predictions, counts and the exported lists against the
    restatements on the oracle's top-17 lists.  The three consumers share the pass."""
    import torch
    ctx, tr, tl, te, s_tr, s_te, lab = entry
    kmax, base, nq = 16, 4_000, NQ
    key = ("loo", kmax)
    if key not in _ref_cache:
        bad, _, odist, oidx = oracle.knn(tr, tl, tr[base:base + nq], kmax + 1, C)
        assert bad == 0
        _ref_cache[key] = (odist, oidx)
    odist, oidx = _ref_cache[key]
    ri, rd = remove_self(oidx, odist, base)
    q = s_tr.view[base:base + nq]
    ql = tl[base:base + nq]
    dist = torch.empty((nq, kmax), dtype=torch.float32, device=DEV)
    idx = torch.empty((nq, kmax), dtype=torch.int32, device=DEV)
    if kind == "sweep":
        pa, corr = ctx.sweep_device(s_tr.view, lab, q, kmax, C, query_labels=lab[base:base + nq], self_base=base,
                                    dist=dist, idx=idx)
        ref, too_few = sweep_reference(oidx, tl, C, self_base=base)
        assert not too_few and np.array_equal(pa.cpu().numpy(), ref)
        assert np.array_equal(corr.cpu().numpy(), (ref == ql[None, :]).sum(axis=1))
    elif kind == "weighted":
        pa, corr, sc = ctx.sweep_weighted_device(s_tr.view, lab, q, kmax, C, "distance",
                                                 query_labels=lab[base:base + nq], self_base=base, dist=dist, idx=idx)
        ref, rsc, too_few = weighted_reference(oidx, odist, tl, C, INV_DIST, self_base=base)
        assert not too_few and np.array_equal(pa.cpu().numpy(), ref)
        assert np.array_equal(bits(sc.cpu().numpy()), bits(rsc))
        assert np.array_equal(corr.cpu().numpy(), (ref == ql[None, :]).sum(axis=1))
    else:
        y = _targets(NT)
        d_y = torch.from_numpy(y).to(DEV)
        pa, sse, sae = ctx.regress_sweep_device(s_tr.view, d_y, q, kmax, "distance", query_targets=d_y[base:base + nq],
                                                self_base=base, dist=dist, idx=idx)
        ref, too_few = regress_reference(oidx, odist, y, INV_DIST, self_base=base)
        assert not too_few and np.array_equal(fbits(pa.cpu().numpy()), fbits(ref))
        # the kernel's fixed-order binary64 sums against fsum of the restatement's predictions:
        # nq 2^-52 relative (test_gpu_regress's bound)
        for got, want in zip((sse, sae), error_sums(ref, y[base:base + nq])):
            assert (np.abs(got.cpu().numpy() - want) <= nq * 2.0 ** -52 * want).all(), (got, want)
    _assert_filter(ctx.stats(), I8, kind)
    assert np.array_equal(idx.cpu().numpy(), ri)
    assert np.array_equal(bits(dist.cpu().numpy()), bits(rd))
    assert s_tr.intact()


def test_d_argument_on_a_wide_tensor(knn, oracle, entry):
    """predict_device(..., d=128) on contiguous 136-wide poisoned tensors (no view): the pad
    columns are part of the tensor the caller hands over; the result is the view's."""
    import torch
    ctx, tr, tl, te, s_tr, s_te, lab = entry
    k = 10
    want = _oracle(oracle, tr, tl, te, k, (NT, NQ, 128, 0, k))
    w_tr = Strided(tr, 136, 0, POISONS["nan"])
    w_te = Strided(te, 136, 0, POISONS["nan"])
    wide_tr, wide_te = w_tr.dev[:NT], w_te.dev[:NQ]
    assert wide_tr.is_contiguous() and wide_tr.shape[1] == 136
    got, st = _predict(ctx, wide_tr, lab, wide_te, k, d=128)
    _assert_same(got, want, "d=128 of 136")
    _assert_filter(st, I8, "d=128 of 136")
    view, st = _predict(ctx, s_tr.view, lab, s_te.view, k)
    _assert_same(view, got, "the view")
    _assert_filter(st, I8, "the view")
    assert w_tr.intact() and w_te.intact()


# ---------------------------------------------------------------------------------------
# 6. cache keys.  One buffer of 2n x 136 floats seen as [2n][136][:n, :128] (A, ld = 136) and as
# [n][272][:, :128] (B, ld = 272): the same pointer, n and d, other rows -- B's row i is the
# buffer's 136-block 2i, so its first half repeats A's even rows and its second half are blocks
# n and up, which hold another generator stream (A's rows stay what they were).  The calls go
# through the C ABI with one generation: the wrapper would bump the generation for another tensor
# object, and the library's own keys (which include ld) would never be asked.
# ---------------------------------------------------------------------------------------
def _raw_predict(knn, ctx, train, labels, test, k):
    import torch
    nq = test.shape[0]
    pred = torch.empty(nq, dtype=torch.int32, device=DEV)
    dist = torch.empty((nq, k), dtype=torch.float32, device=DEV)
    idx = torch.empty((nq, k), dtype=torch.int32, device=DEV)
    tr = knn._device_dataset(train, labels)
    te = knn._device_dataset(test)
    torch.cuda.synchronize()
    ctx._check(ctx.lib.knn_predict_device(ctx.h, ctypes.byref(tr), ctypes.byref(te), k, C, pred.data_ptr(),
                                          dist.data_ptr(), idx.data_ptr(), None))
    torch.cuda.synchronize()
    return (pred.cpu().numpy(), dist.cpu().numpy().view(np.uint32), idx.cpu().numpy()), ctx.stats()


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("algo,element", [("gemm_i8", "i8"), ("gemm_bf16", "bf16")])
def test_cache_keys_include_the_stride(knn, oracle, algo, element, poison):
    import torch
    n, d, k = NT, 128, 10
    rows_a, tl = _rows(oracle, n, d, 0)
    rows_2, _ = _rows(oracle, n, d, 2)
    te, _ = _rows(oracle, NQ, d, 1)
    flat = torch.full(((2 * n + 1) * 136,), POISONS[poison], dtype=torch.float32)
    blocks = flat[:2 * n * 136].view(2 * n, 136)
    blocks[:n, :d] = torch.from_numpy(np.array(rows_a))
    blocks[n:, :d] = torch.from_numpy(np.array(rows_2))
    rows_b = flat[:2 * n * 136].view(n, 272)[:, :d].contiguous().numpy()
    assert np.array_equal(rows_b[:4], rows_a[:8:2]) and np.array_equal(rows_b[-1], rows_2[n - 2])
    dev = flat.to(DEV)
    view_a = dev[:2 * n * 136].view(2 * n, 136)[:n, :d]
    view_b = dev[:2 * n * 136].view(n, 272)[:, :d]
    assert view_a.data_ptr() == view_b.data_ptr() and view_a.shape == view_b.shape
    assert (view_a.stride(0), view_b.stride(0)) == (136, 272)
    lab = torch.from_numpy(np.array(tl)).to(DEV)
    test = torch.from_numpy(np.array(te)).to(DEV)
    want_a = _oracle(oracle, rows_a, tl, te, k, (NT, NQ, d, 0, k))
    want_b = _oracle(oracle, rows_b, tl, te, k, (NT, NQ, d, "B", k))
    assert not np.array_equal(want_a[2], want_b[2])
    ctx = knn.Context(0, algo=algo, profile=True, cache_train=True)
    try:
        for view, want, cached in ((view_a, want_a, False), (view_a, want_a, True), (view_b, want_b, False),
                                   (view_b, want_b, True), (view_a, want_a, False)):
            got, st = _raw_predict(knn, ctx, view, lab, test, k)
            assert st["train_operands_cached"] == cached, st
            _assert_same(got, want, f"ld={view.stride(0)} cached={cached}")
            _assert_filter(st, ("bf16 rounded", element, True), f"ld={view.stride(0)}")
    finally:
        ctx.close()
    it = torch.int32
    assert torch.equal(dev.cpu().view(it), flat.view(it))


# ---------------------------------------------------------------------------------------
# 7. host path with a pitch: knn_predict and knn_sweep through the C ABI (the Python wrapper
# always passes ld = d) on numpy parents [n + 1][d + 3], pad columns poisoned (host rows need no
# alignment).  The train upload and the three query uploads -- knn_predict's one-batch copy, its
# pipelined batches (KNN_BATCH_ROWS = 100: the range [100, 400) is three of them, and the slice's
# offset is multiplied by ld) and knn_sweep's batches -- are 2-D copies from the host pitch.
# ---------------------------------------------------------------------------------------
def _host_parent(rows, ld, poison):
    n, d = rows.shape
    parent = np.full((n + 1, ld), poison, np.float32)
    parent[:n, :d] = rows
    return parent


def _host_ds(knn, parent, n, d, ld, labels=None):
    return knn.knn_dataset(parent.ctypes.data, None if labels is None else labels.ctypes.data, n, d, ld, knn.KNN_F32)


def _host_predict(knn, ctx, tr, te, k, q0, q1):
    nq = q1 - q0
    pred = np.zeros(nq, np.int32)
    dist = np.zeros((nq, k), np.float32)
    idx = np.zeros((nq, k), np.int32)
    ctx._check(ctx.lib.knn_predict(ctx.h, ctypes.byref(tr), ctypes.byref(te), k, C, q0, q1, knn._ptr(pred),
                                   knn._ptr(dist), knn._ptr(idx)))
    return (pred, dist.view(np.uint32), idx), ctx.stats()


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("batch", [None, "100"])
@pytest.mark.parametrize("algo,d,kw", [("direct", 11, {}), ("auto", 128, {"cache_train": True})],
                         ids=["direct-d11", "auto-cached-d128"])
def test_host_path_with_a_pitch(knn, oracle, monkeypatch, algo, d, kw, batch, poison):
    nt, nq, k, ld = 9_000, NQ, 10, d + 3
    if batch:
        monkeypatch.setenv("KNN_BATCH_ROWS", batch)
    rows, tl = _rows(oracle, nt, d, 0)
    te, _ = _rows(oracle, nq, d, 1)
    want = _oracle(oracle, rows, tl, te, k, (nt, nq, d, 0, k))
    p_tr, p_te = _host_parent(rows, ld, POISONS[poison]), _host_parent(te, ld, POISONS[poison])
    keep_tr, keep_te = p_tr.copy(), p_te.copy()
    labels = np.array(tl)
    ds_tr, ds_te = _host_ds(knn, p_tr, nt, d, ld, labels), _host_ds(knn, p_te, nq, d, ld)
    ctx = knn.Context(0, algo=algo, **kw)
    try:
        for q0, q1 in ((0, nq), (100, 400)):
            got, st = _host_predict(knn, ctx, ds_tr, ds_te, k, q0, q1)
            _assert_same(got, tuple(w[q0:q1] for w in want), f"queries [{q0}, {q1})")
            assert st["h2d_query_bytes"] == 4 * d * (q1 - q0), st
            first = q0 == 0 or not kw
            assert st["h2d_train_bytes"] == ((4 * d + 4) * nt if first else 0), st
        # knn_sweep: every k <= kmax from the top-kmax lists, the queries in batches
        kmax = 16
        wantk = _oracle(oracle, rows, tl, te, kmax, (nt, nq, d, 0, kmax))
        ref, too_few = sweep_reference(wantk[2], tl, C)
        pred_all = np.zeros((kmax, nq), np.int32)
        ctx._check(ctx.lib.knn_sweep(ctx.h, ctypes.byref(ds_tr), ctypes.byref(ds_te), kmax, C, -1, None,
                                     knn._ptr(pred_all), None))
        assert not too_few and np.array_equal(pred_all, ref)
        assert ctx.stats()["h2d_query_bytes"] == 4 * d * nq
    finally:
        ctx.close()
    for parent, keep in ((p_tr, keep_tr), (p_te, keep_te)):
        assert np.array_equal(parent.view(np.uint32), keep.view(np.uint32))


@pytest.mark.parametrize("poison", list(POISONS))
def test_host_train_cache_keyed_by_the_pitch(knn, oracle, poison):
    """The same host pointer, n and d at ld = 131 and at ld = 262 (every second 131-block: other
    rows) on a caching context: each change of the pitch uploads again and matches its own
    reference; the same pitch again moves no train bytes."""
    nt, nq, d, k, ld = 9_000, NQ, 128, 10, 131
    rows_a, tl = _rows(oracle, nt, d, 0)
    rows_2, _ = _rows(oracle, nt, d, 2)
    te, _ = _rows(oracle, nq, d, 1)
    buf = np.full((2 * nt + 1, ld), POISONS[poison], np.float32)
    buf[:nt, :d] = rows_a
    buf[nt:2 * nt, :d] = rows_2
    rows_b = np.ascontiguousarray(buf[:2 * nt].reshape(nt, 2 * ld)[:, :d])
    keep = buf.copy()
    labels = np.array(tl)
    ds_a, ds_b = _host_ds(knn, buf, nt, d, ld, labels), _host_ds(knn, buf, nt, d, 2 * ld, labels)
    p_te = _host_parent(te, ld, POISONS[poison])
    ds_te = _host_ds(knn, p_te, nq, d, ld)
    want_a = _oracle(oracle, rows_a, tl, te, k, (nt, nq, d, 0, k))
    want_b = _oracle(oracle, rows_b, tl, te, k, (nt, nq, d, "B", k))
    assert not np.array_equal(want_a[2], want_b[2])
    ctx = knn.Context(0, algo="auto", cache_train=True)
    try:
        for ds, want, upload in ((ds_a, want_a, True), (ds_a, want_a, False), (ds_b, want_b, True),
                                 (ds_b, want_b, False), (ds_a, want_a, True)):
            got, st = _host_predict(knn, ctx, ds, ds_te, k, 0, nq)
            assert st["h2d_train_bytes"] == ((4 * d + 4) * nt if upload else 0), (ds.ld, st)
            _assert_same(got, want, f"ld={ds.ld} upload={upload}")
    finally:
        ctx.close()
    assert np.array_equal(buf.view(np.uint32), keep.view(np.uint32))
