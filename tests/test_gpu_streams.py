"""Every device entry point on a busy caller stream.

The header promises that a device call enqueues its work on `hip_stream` and returns after that
stream has drained.  Every other GPU test runs on torch's default stream, the legacy null stream,
which every blocking stream is ordered after: an enqueue on the wrong stream cannot be seen there.
Here every wrapper with a `stream=` parameter runs while its inputs are still being produced.

The protocol, per case (an entry point, a context, its inputs):

* reference: the call on the default stream with the real inputs in fresh tensors.  Its primary
  outputs must equal the CPU restatement of the feature's own test, so the file does not compare
  the library with itself.
* decoy: a second valid input set of the same shapes, and its reference.  It differs in values
  that cannot index memory (feature rows, labels, targets, distances); index and offset tensors
  keep a valid structure of the same sizes.  The list-building radius calls take a decoy whose
  train rows are the real ones in another order and whose queries are the real ones: every
  neighbourhood keeps its size, so whatever mixture a wrongly ordered call read, the offsets it
  used fit the lists it wrote.  The decoy's reference must differ from the real one.
* the input buffers hold the decoy, the outputs a guard value.  Then, with no synchronisation
  between the steps: a device-side wait of T ms, `buf.copy_(real)` for every input, the call.
  - `current`: all three under `torch.cuda.stream(s)`, no `stream=`;
  - `explicit`: wait and copies on s, the call made with `stream=s.cuda_stream` while torch's
    current stream is another side stream x with a wait of 1.5 T pending -- longer than s is
    busy, so a zero fill a wrapper left on x lands after the call wrote its result;
  - `null`: wait and copies on the default stream, the call with no `stream=` (it runs on the
    context's own blocking stream).
* after `torch.cuda.synchronize()` every output of every variant equals the real reference bit
  for bit, and the guard words past every pre-allocated output are intact.

Sensitivity control: the same producer on s, the call handed to the context's own stream while
torch's current stream is idle.  That call is NOT ordered after s, so it must return the decoy's
reference.  Streams that share a hardware queue serialise and would hide the race, so s is the
first of at most 4 fresh side streams that shows the decoy, and x the first of at most 4 whose
wait overlaps a wait on s; the module fails when there is none.  (The control speaks for the direct
context's own stream; another context's stream may still share a queue with s.)

Measured on one MI355X (five runs): torch.cuda._sleep runs 2.39e6 to 2.41e6 cycles per ms; the longest
default-stream reference call took 16.1 to 18.6 ms, so T = 200 ms, the cap (20 x the longest, floor
20 ms, cap 200 ms).  The fixture measures both again on every run and prints them.
"""
import functools
import inspect
import math
import sys
import time

import numpy as np
import pytest

from conftest import merge_lists_reference
from test_dbscan_cpu import dbscan_case, dbscan_set, distances
from test_dbscan_sweep_cpu import Q4, sweep_case, thresholds_of
from test_lof_cpu import lof_novelty_reference, lof_reference
from test_metric_cpu import EUCLIDEAN, FLT_MAX, MANHATTAN, bits, metric_distances, metric_set, vote_reference
from test_mst_cpu import mst_case, mst_cut, mst_reference
from test_radius_cpu import (METRIC_NAMES, count_vote_reference, radius_reference, radius_regress_reference,
                             radius_thresholds, radius_vote_reference)
from test_radius_sweep_cpu import radius_sweep_reference, radius_vote_sweep_reference
from test_regress_cpu import _targets, fbits, regress_reference
from test_sweep_cpu import sweep_reference
from test_weighted_cpu import INV_DIST, weighted_reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C = 10
K = 5
OUTLIER = -7
GUARD = -777
GUARD_WORDS = 64
LOF_K = (3, 5)
VARIANTS = ("current", "explicit", "null")
# (train rows, queries, features) of the feature-row sets
SHAPES = {"dir": (1000, 65, 11), "bf": (4096, 517, 64), "i8": (4096, 517, 128)}
# (rows, features) of the self-join sets (test_dbscan_cpu.dbscan_set)
SELF_SHAPES = {"s11": (1000, 11), "s3": (1000, 3), "s64": (4096, 64)}
# (the direct contexts run one train segment; "dir3" forces three)
CONTEXTS = {"dir": dict(algo="direct", train_splits=1), "dir3": dict(algo="direct", train_splits=3),
            "bf": dict(algo="gemm_bf16"), "i8": dict(algo="gemm_i8"),
            "man": dict(algo="direct", train_splits=1, metric="manhattan")}
_FIX = {}  # the session's oracle and package (the fixtures), for the cached builders below


def _torch():
    import torch
    return torch


def _dev(x):
    return _torch().from_numpy(np.ascontiguousarray(x)).to(DEV)


def _pad4(x):
    """Device rows are 16-byte aligned: zero columns up to a multiple of 4 (the calls pass the true d)."""
    return np.ascontiguousarray(np.pad(x, ((0, 0), (0, -x.shape[1] % 4))))


def _ubits(a):
    """A host array as unsigned words of its element size: what the variants are compared by."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _nbits(a):
    """_ubits with every NaN mapped to one pattern: the restatements fix NaN positions, not payloads."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return fbits(a)
    if a.dtype == np.float64:
        return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))
    return _ubits(a)


# ---------------------------------------------------------------------------------------
# input sets (cached; "real", "decoy" = another seed, "perm" = the real train rows in another order
# against the real queries, with the decoy's labels and targets)
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _set(tag, which):
    nt, nq, d = SHAPES[tag]
    if which == "perm":
        real, decoy = _set(tag, "real"), _set(tag, "decoy")
        p = np.random.default_rng(3).permutation(nt)
        s = dict(decoy, tr=real["tr"][p], te=real["te"])
    else:
        seed = 5 if which == "real" else 6
        tr, tl, te = metric_set(_FIX["oracle"], "float", nt, nq, d, seed=seed)
        s = dict(d=d, tr=tr, te=te, labels=tl,
                 qlabels=np.random.default_rng(nq + seed).integers(0, C, size=nq).astype(np.int32),
                 targets=_targets(nt, 26 + seed), qtargets=_targets(nq, 36 + seed))
    s["train"], s["test"] = _pad4(s["tr"]), _pad4(s["te"])
    return s


@functools.lru_cache(maxsize=None)
def _D(tag, which, pair, metric=EUCLIDEAN):
    """float32 distances of a set: "qt" queries against train rows, "tt" the train rows against themselves."""
    s = _set(tag, which)
    return metric_distances(s["tr"], s["te"] if pair == "qt" else s["tr"], metric)


def _lists(D, k):
    """test_metric_cpu.metric_reference's selection on a distance matrix that is shared between the
    cases: ascending (distance bits, train index) over the rows with D < FLT_MAX."""
    nq = len(D)
    dist = np.full((nq, k), FLT_MAX, np.float32)
    idx = np.full((nq, k), -1, np.int32)
    for q in range(nq):
        ok = np.nonzero(D[q] < FLT_MAX)[0]
        order = ok[np.lexsort((ok, bits(D[q, ok])))][:k]
        dist[q, :len(order)] = D[q, order]
        idx[q, :len(order)] = order
    return dist, idx


@functools.lru_cache(maxsize=None)
def _topk(tag, which, pair, k, metric=EUCLIDEAN):
    return _lists(_D(tag, which, pair, metric), k)


@functools.lru_cache(maxsize=None)
def _thr(tag, pair, metric=EUCLIDEAN):
    """The real set's thresholds (test_radius_cpu.radius_thresholds: matrix entries): [0] the
    single-radius calls', the 5 % quantile; [1] the sweeps' three."""
    t = radius_thresholds(_D(tag, "real", pair, metric))
    return float(t[2]), np.array(t[1:], np.float32)


@functools.lru_cache(maxsize=None)
def _csr(tag, which, thr):
    """(count, offsets, idx, dist, class counts) of a set's queries at thr."""
    s = _set(tag, which)
    return radius_reference(s["tr"], s["te"], thr, EUCLIDEAN, labels=s["labels"], C=C, D=_D(tag, which, "qt"))


@functools.lru_cache(maxsize=None)
def _self(tag, which):
    """(rows, D or None): the real self-join set is test_dbscan_cpu's (its restatements are shared
    with the feature tests), the decoy the same builder under another seed."""
    n, d = SELF_SHAPES[tag]
    if which == "real":
        return distances("dbscan", n, d, EUCLIDEAN)
    return dbscan_set(n, d, seed=1234), None


@functools.lru_cache(maxsize=None)
def _self_perm(tag):
    """The real self-join set renumbered: (permutation, its distance matrix).  Lists and trees of it
    have the real ones' sizes."""
    X, D = _self(tag, "real")
    p = np.random.default_rng(4).permutation(len(X))
    return p, np.ascontiguousarray(D[p][:, p])


@functools.lru_cache(maxsize=None)
def _lof_tables(tag, which):
    dist, idx = _topk(tag, which, "tt", LOF_K[1] + 1)
    return lof_reference(idx, dist, 0, LOF_K[0], LOF_K[1], EUCLIDEAN)


# ---------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------
class Case:
    """entry: the wrapper's name; ctx: a key of CONTEXTS; make(which) -> the host inputs ("real" or
    "decoy"); run(ctx, t, out, stream) -> {name: tensor or host array}, t the device inputs, out(shape,
    dtype) a guarded output; want() -> {name: host array} of the restatement (the primary outputs);
    pin(ref) an assertion on the reference instead, where no restatement fixes the bits; stats(st)
    asserts that the form under test ran."""

    def __init__(self, entry, ctx, make, run, want=None, pin=None, stats=None, tag=""):
        self.entry, self.ctx, self.make, self.run, self.want, self.pin, self.stats = entry, ctx, make, run, want, pin, stats
        self.id = "-".join(x for x in (ctx, entry, tag) if x)


CASES = []


def case(entry, ctx="dir", tag="", stats=None, pin=None):
    """Decorator of a function returning (make, run, want)."""
    def add(fn):
        make, run, want = fn()
        CASES.append(Case(entry, ctx, make, run, want, pin, stats, tag))
        return fn
    return add


def _pick(tag, *names, decoy="decoy"):
    return lambda which: {n: _set(tag, which if which == "real" else decoy)[n] for n in names}


def _i32():
    return _torch().int32


def _f32():
    return _torch().float32


def _bf16_filter(st):
    assert st["filter_operands"] == "bf16 rounded" and st["filter_element"] == "bf16", st


def _i8_filter(st):
    assert st["filter_operands"] == "bf16 rounded" and st["filter_element"] == "i8", st


def _mfma_radius(st):
    assert st["radius_form"] == "mfma", st


def _segments1(st):
    assert st["train_segments"] == 1, st


def _segments3(st):
    assert st["train_segments"] == 3, st


# --- top-k, vote, weighted vote, regression ---------------------------------------------
def _predict_case(tag, k, metric=EUCLIDEAN):
    d = SHAPES[tag][2]

    def run(ctx, t, out, stream):
        nq = t["test"].shape[0]
        pred, dist, idx = out((nq,), _i32()), out((nq, k), _f32()), out((nq, k), _i32())
        ctx.predict_device(t["train"], t["labels"], t["test"], k, C, pred, dist, idx, stream=stream, d=d)
        return dict(pred=pred, dist=dist, idx=idx)

    def want():
        dist, idx = _topk(tag, "real", "qt", k, metric)
        return dict(dist=dist, idx=idx, pred=vote_reference(idx, _set(tag, "real")["labels"], C))

    return _pick(tag, "train", "labels", "test"), run, want


case("predict_device", stats=_segments1)(lambda: _predict_case("dir", K))
case("predict_device", "dir3", "k5", stats=_segments3)(lambda: _predict_case("dir", 5))
case("predict_device", "dir3", "k70", stats=_segments3)(lambda: _predict_case("dir", 70))
case("predict_device", "bf", stats=_bf16_filter)(lambda: _predict_case("bf", K))
case("predict_device", "i8", stats=_i8_filter)(lambda: _predict_case("i8", 10))
case("predict_device", "man", stats=_segments1)(lambda: _predict_case("dir", K, MANHATTAN))


@case("shard_topk_device")
def _shard_topk():
    base = 100

    def run(ctx, t, out, stream):
        rec = out((t["test"].shape[0], 3, K), _i32())
        ctx.shard_topk_device(t["train"], t["labels"], t["test"], K, C, base, rec, stream=stream, d=SHAPES["dir"][2])
        return dict(rec=rec)

    def want():
        dist, idx = _topk("dir", "real", "qt", K)
        return dict(rec=np.stack([bits(dist).view(np.int32), idx + base, _set("dir", "real")["labels"][idx]], axis=1))

    return _pick("dir", "train", "labels", "test"), run, want


def _shard_lists(which):
    """rec int32 [2][nq][3][K]: the lists of the two halves of the train rows, as shard_topk_device writes them."""
    s, D = _set("dir", which), _D("dir", which, "qt")
    half = D.shape[1] // 2
    rec = []
    for lo, hi in ((0, half), (half, D.shape[1])):
        dist, idx = _lists(D[:, lo:hi], K)
        rec.append(np.stack([bits(dist).view(np.int32), idx + lo, s["labels"][idx + lo]], axis=1))
    return np.ascontiguousarray(np.stack(rec))


@case("merge_vote_device")
def _merge_vote():
    def run(ctx, t, out, stream):
        nq = t["rec"].shape[1]
        pred, dist, idx = out((nq,), _i32()), out((nq, K), _f32()), out((nq, K), _i32())
        ctx.merge_vote_device(t["rec"], K, C, pred, dist, idx, stream=stream)
        return dict(pred=pred, dist=dist, idx=idx)

    def want():
        pred, dist, idx = merge_lists_reference(_shard_lists("real"), K, C)
        return dict(pred=pred, dist=dist, idx=idx)

    return (lambda which: dict(rec=_shard_lists(which))), run, want


def _correct(pred_all, qlabels):
    return (pred_all == qlabels[None, :]).sum(axis=1).astype(np.int64)


def _sweep_case(tag, entry):
    d = SHAPES[tag][2]
    loo = entry == "loo_device"

    def run(ctx, t, out, stream):
        nq = t["train" if loo else "test"].shape[0]
        pa = out((K, nq), _i32())
        if loo:
            _, corr = ctx.loo_device(t["train"], t["labels"], K, C, pred_all=pa, stream=stream, d=d)
            return dict(pred_all=pa, correct=corr)
        dist, idx = out((nq, K), _f32()), out((nq, K), _i32())
        _, corr = ctx.sweep_device(t["train"], t["labels"], t["test"], K, C, query_labels=t["qlabels"], pred_all=pa,
                                   dist=dist, idx=idx, stream=stream, d=d)
        return dict(pred_all=pa, correct=corr, dist=dist, idx=idx)

    def want():
        s = _set(tag, "real")
        if loo:
            pa, few = sweep_reference(_topk(tag, "real", "tt", K + 1)[1], s["labels"], C, self_base=0)
            return dict(pred_all=pa, correct=_correct(pa, s["labels"])) if not few else None
        dist, idx = _topk(tag, "real", "qt", K)
        pa, _ = sweep_reference(idx, s["labels"], C)
        return dict(pred_all=pa, correct=_correct(pa, s["qlabels"]), dist=dist, idx=idx)

    return _pick(tag, *(("train", "labels") if loo else ("train", "labels", "test", "qlabels"))), run, want


case("sweep_device")(lambda: _sweep_case("dir", "sweep_device"))
case("sweep_device", "bf", stats=_bf16_filter)(lambda: _sweep_case("bf", "sweep_device"))
case("loo_device")(lambda: _sweep_case("dir", "loo_device"))


def _list_inputs(*names):
    """Inputs of a list consumer: the set's own top-K lists and the named side arrays."""
    def make(which):
        dist, idx = _topk("dir", which, "qt", K)
        return dict({n: _set("dir", which)[n] for n in names}, idx=idx, dist=dist)
    return make


@case("vote_sweep_device")
def _vote_sweep():
    def run(ctx, t, out, stream):
        pa = out((K, t["idx"].shape[0]), _i32())
        _, corr = ctx.vote_sweep_device(t["idx"], t["labels"], C, query_labels=t["qlabels"], pred_all=pa, stream=stream)
        return dict(pred_all=pa, correct=corr)

    def want():
        s = _set("dir", "real")
        pa, _ = sweep_reference(_topk("dir", "real", "qt", K)[1], s["labels"], C)
        return dict(pred_all=pa, correct=_correct(pa, s["qlabels"]))

    make = _list_inputs("labels", "qlabels")
    return (lambda which: {k: v for k, v in make(which).items() if k != "dist"}), run, want


def _weighted_case(entry):
    d = SHAPES["dir"][2]

    def run(ctx, t, out, stream):
        nq = t["idx" if entry == "vote_weighted_device" else "train" if entry == "loo_weighted_device" else "test"].shape[0]
        sc = out((nq, C), _f32())
        if entry == "predict_weighted_device":
            pred = out((nq,), _i32())
            ctx.predict_weighted_device(t["train"], t["labels"], t["test"], K, C, "distance", pred=pred, scores=sc,
                                        stream=stream, d=d)
            return dict(pred=pred, scores=sc)
        pa = out((K, nq), _i32())
        if entry == "sweep_weighted_device":
            _, corr, _ = ctx.sweep_weighted_device(t["train"], t["labels"], t["test"], K, C, "distance",
                                                   query_labels=t["qlabels"], pred_all=pa, scores=sc, stream=stream, d=d)
        elif entry == "loo_weighted_device":
            _, corr, _ = ctx.loo_weighted_device(t["train"], t["labels"], K, C, "distance", pred_all=pa, scores=sc,
                                                 stream=stream, d=d)
        else:
            _, corr, _ = ctx.vote_weighted_device(t["idx"], t["dist"], t["labels"], C, "distance",
                                                  query_labels=t["qlabels"], pred_all=pa, scores=sc, stream=stream)
        return dict(pred_all=pa, correct=corr, scores=sc)

    def want():
        s = _set("dir", "real")
        if entry == "loo_weighted_device":
            dist, idx = _topk("dir", "real", "tt", K + 1)
            pa, sc, few = weighted_reference(idx, dist, s["labels"], C, INV_DIST, self_base=0)
            return dict(pred_all=pa, scores=sc, correct=_correct(pa, s["labels"])) if not few else None
        dist, idx = _topk("dir", "real", "qt", K)
        pa, sc, _ = weighted_reference(idx, dist, s["labels"], C, INV_DIST)
        if entry == "predict_weighted_device":
            return dict(pred=pa[K - 1], scores=sc)
        return dict(pred_all=pa, scores=sc, correct=_correct(pa, s["qlabels"]))

    make = {"vote_weighted_device": _list_inputs("labels", "qlabels"), "loo_weighted_device": _pick("dir", "train", "labels"),
            "predict_weighted_device": _pick("dir", "train", "labels", "test")}.get(
                entry, _pick("dir", "train", "labels", "test", "qlabels"))
    return make, run, want


for _e in ("sweep_weighted_device", "loo_weighted_device", "predict_weighted_device", "vote_weighted_device"):
    case(_e)(functools.partial(_weighted_case, _e))


def _regress_case(entry):
    d = SHAPES["dir"][2]

    def run(ctx, t, out, stream):
        nq = t["idx" if entry == "regress_vote_device" else "train" if entry == "regress_loo_device" else "test"].shape[0]
        if entry == "regress_device":
            pred = out((nq,), _f32())
            ctx.regress_device(t["train"], t["targets"], t["test"], K, "distance", pred=pred, stream=stream, d=d)
            return dict(pred=pred)
        pa = out((K, nq), _f32())
        if entry == "regress_sweep_device":
            _, sse, sae = ctx.regress_sweep_device(t["train"], t["targets"], t["test"], K, "distance",
                                                   query_targets=t["qtargets"], pred_all=pa, stream=stream, d=d)
        elif entry == "regress_loo_device":
            _, sse, sae = ctx.regress_loo_device(t["train"], t["targets"], K, "distance", pred_all=pa, stream=stream, d=d)
        else:
            _, sse, sae = ctx.regress_vote_device(t["idx"], t["dist"], t["targets"], "distance",
                                                  query_targets=t["qtargets"], pred_all=pa, stream=stream)
        return dict(pred_all=pa, sse=sse, sae=sae)

    def want():
        s = _set("dir", "real")
        if entry == "regress_loo_device":
            dist, idx = _topk("dir", "real", "tt", K + 1)
            return dict(pred_all=regress_reference(idx, dist, s["targets"], INV_DIST, self_base=0)[0])
        dist, idx = _topk("dir", "real", "qt", K)
        pa = regress_reference(idx, dist, s["targets"], INV_DIST)[0]
        return dict(pred=pa[K - 1]) if entry == "regress_device" else dict(pred_all=pa)

    make = {"regress_vote_device": _list_inputs("targets", "qtargets"), "regress_loo_device": _pick("dir", "train", "targets"),
            "regress_device": _pick("dir", "train", "targets", "test")}.get(
                entry, _pick("dir", "train", "targets", "test", "qtargets"))
    return make, run, want


for _e in ("regress_sweep_device", "regress_loo_device", "regress_device", "regress_vote_device"):
    case(_e)(functools.partial(_regress_case, _e))


# --- local outlier factor ---------------------------------------------------------------
def _lof_case(entry, tag="dir"):
    k_lo, k_hi = LOF_K
    Kr = k_hi - k_lo + 1

    def rows(which):
        if tag == "dir":
            return _set("dir", which)["train"], SHAPES["dir"][2]
        return _pad4(_self(tag, which)[0]), SELF_SHAPES[tag][1]

    def tables():
        if tag == "dir":
            return _lof_tables("dir", "real")
        dist, idx = _lists(_self(tag, "real")[1], k_hi + 1)
        return lof_reference(idx, dist, 0, k_lo, k_hi, EUCLIDEAN)

    def run(ctx, t, out, stream):
        n, d = t["train"].shape[0], rows("real")[1]
        lof = out((Kr, n), _f32())
        if entry == "lof_device":
            ctx.lof_device(t["train"], k_lo, k_hi, lof=lof, stream=stream, d=d)
            return dict(lof=lof)
        kd, lrd = out((n, Kr), _f32()), out((n, Kr), _torch().float64)
        ctx.lof_fit_device(t["train"], k_lo, k_hi, lof=lof, kd=kd, lrd=lrd, stream=stream, d=d)
        return dict(kd=kd, lrd=lrd, lof=lof)

    def want():
        kd, lrd, lof, few = tables()
        assert not few
        return dict(lof=lof) if entry == "lof_device" else dict(kd=kd, lrd=lrd, lof=lof)

    return (lambda which: dict(train=rows(which)[0])), run, want


case("lof_fit_device")(lambda: _lof_case("lof_fit_device"))
case("lof_device")(lambda: _lof_case("lof_device"))
case("lof_device", "bf", stats=_bf16_filter)(lambda: _lof_case("lof_device", "s64"))


@case("lof_lists_device")
def _lof_lists():
    k_lo, k_hi = LOF_K
    Kr = k_hi - k_lo + 1

    def make(which):
        dist, idx = _topk("dir", which, "tt", k_hi + 1)
        return dict(idx=idx, dist=dist)

    def run(ctx, t, out, stream):
        n = t["idx"].shape[0]
        lof, kd, lrd = out((Kr, n), _f32()), out((n, Kr), _f32()), out((n, Kr), _torch().float64)
        ctx.lof_lists_device(t["idx"], t["dist"], k_lo, k_hi, self_base=0, kd=kd, lrd=lrd, lof=lof, stream=stream)
        return dict(kd=kd, lrd=lrd, lof=lof)

    def want():
        kd, lrd, lof, _ = _lof_tables("dir", "real")
        return dict(kd=kd, lrd=lrd, lof=lof)

    return make, run, want


@case("score_device")
def _lof_score():
    """LofModel.score_device: the train rows, the fitted tables and the queries are all inputs."""
    k_lo, k_hi = LOF_K

    def make(which):
        kd, lrd, _, _ = _lof_tables("dir", which)
        s = _set("dir", which)
        return dict(train=s["train"], kd=kd, lrd=lrd, test=s["test"])

    def run(ctx, t, out, stream):
        model = sys.modules["knn_amd"].LofModel(ctx, t["train"], SHAPES["dir"][2], k_lo, k_hi, t["kd"], t["lrd"])
        lof = out((k_hi - k_lo + 1, t["test"].shape[0]), _f32())
        model.score_device(t["test"], lof=lof, stream=stream)
        return dict(lof=lof)

    def want():
        kd, lrd, _, _ = _lof_tables("dir", "real")
        qdist, qidx = _topk("dir", "real", "qt", k_hi)
        return dict(lof=lof_novelty_reference(qidx, qdist, kd, lrd, k_lo, k_hi, EUCLIDEAN)[0])

    return make, run, want


# --- radius neighbours ------------------------------------------------------------------
def _count_case(tag, ctx_metric=EUCLIDEAN, fill=False):
    """radius_count_device with every output; fill=True: and radius_fill_device on its offsets."""
    d = SHAPES[tag][2]

    def run(ctx, t, out, stream):
        thr = _thr(tag, "qt", ctx_metric)[0]
        count, pred, correct, cc, off = ctx.radius_count_device(
            t["train"], t["labels"], t["test"], threshold=thr, num_classes=C, query_labels=t["qlabels"],
            outlier_label=OUTLIER, class_counts=True, offsets=True, stream=stream, d=d)
        res = dict(count=count, pred=pred, correct=correct, cc=cc, offsets=off)
        if fill:
            res["idx"], res["dist"] = ctx.radius_fill_device(t["train"], t["test"], off, threshold=thr, stream=stream, d=d)
        return res

    def want():
        s = _set(tag, "real")
        count, off, idx, dist, cc = radius_reference(s["tr"], s["te"], _thr(tag, "qt", ctx_metric)[0], ctx_metric,
                                                     labels=s["labels"], C=C, D=_D(tag, "real", "qt", ctx_metric))
        pred = count_vote_reference(cc, OUTLIER)
        res = dict(count=count, offsets=off, cc=cc, pred=pred, correct=np.array([(pred == s["qlabels"]).sum()], np.int64))
        if fill:
            res.update(idx=idx, dist=dist)
        return res

    return _pick(tag, "train", "labels", "test", "qlabels", decoy="perm" if fill else "decoy"), run, want


case("radius_count_device")(lambda: _count_case("dir"))
case("radius_count_device", "man")(lambda: _count_case("dir", MANHATTAN))
case("radius_count_device", "bf", "and_fill", stats=_mfma_radius)(lambda: _count_case("bf", fill=True))


def _real_lists():
    """The real set's CSR lists at the single threshold: (offsets, idx, dist)."""
    return _csr("dir", "real", _thr("dir", "qt")[0])[1:4]


@case("radius_fill_device")
def _radius_fill():
    def make(which):
        s = _set("dir", which if which == "real" else "perm")
        return dict(train=s["train"], test=s["test"], offsets=_real_lists()[0])

    def run(ctx, t, out, stream):
        idx, dist = ctx.radius_fill_device(t["train"], t["test"], t["offsets"], threshold=_thr("dir", "qt")[0],
                                           stream=stream, d=SHAPES["dir"][2])
        return dict(idx=idx, dist=dist)

    return make, run, lambda: dict(idx=_real_lists()[1], dist=_real_lists()[2])


@case("radius_neighbors_device")
def _radius_neighbors():
    def run(ctx, t, out, stream):
        off, idx, dist = ctx.radius_neighbors_device(t["train"], t["test"], threshold=_thr("dir", "qt")[0], stream=stream,
                                                     d=SHAPES["dir"][2])
        return dict(offsets=off, idx=idx, dist=dist)

    return _pick("dir", "train", "test", decoy="perm"), run, lambda: dict(zip(("offsets", "idx", "dist"), _real_lists()))


def _csr_inputs(*names):
    """Inputs of a CSR list consumer: the real offsets and indices in both sets (the structure stays),
    the decoy's distances the real ones in reverse order, the named side arrays the set's own."""
    def make(which):
        off, idx, dist = _real_lists()
        s = _set("dir", which)
        return dict({n: s[n] for n in names}, offsets=off, idx=idx, dist=dist if which == "real" else dist[::-1].copy())
    return make


@case("radius_vote_device")
def _radius_vote():
    def run(ctx, t, out, stream):
        pred, correct, sc = ctx.radius_vote_device(t["offsets"], t["idx"], t["dist"], t["labels"], C, "distance", OUTLIER,
                                                   query_labels=t["qlabels"], scores=True, stream=stream)
        return dict(pred=pred, correct=correct, scores=sc)

    def want():
        s = _set("dir", "real")
        pred, sc = radius_vote_reference(*_real_lists(), s["labels"], C, INV_DIST, EUCLIDEAN, OUTLIER)
        return dict(pred=pred, scores=sc, correct=np.array([(pred == s["qlabels"]).sum()], np.int64))

    return _csr_inputs("labels", "qlabels"), run, want


@case("radius_regress_vote_device")
def _radius_regress_vote():
    def run(ctx, t, out, stream):
        return dict(pred=ctx.radius_regress_vote_device(t["offsets"], t["idx"], t["dist"], t["targets"], "distance",
                                                        stream=stream))

    def want():
        return dict(pred=radius_regress_reference(*_real_lists(), _set("dir", "real")["targets"], INV_DIST, EUCLIDEAN))

    return _csr_inputs("targets"), run, want


def _radius_predict_case(weights):
    d = SHAPES["dir"][2]

    def run(ctx, t, out, stream):
        pred, sc, count, correct = ctx.radius_predict_device(
            t["train"], t["labels"], t["test"], threshold=_thr("dir", "qt")[0], num_classes=C, weights=weights,
            outlier_label=OUTLIER, query_labels=t["qlabels"], stream=stream, d=d)
        return dict(pred=pred, scores=sc, count=count, correct=correct)

    def want():
        s = _set("dir", "real")
        count, off, idx, dist, cc = _csr("dir", "real", _thr("dir", "qt")[0])
        if weights == "uniform":
            pred, sc = count_vote_reference(cc, OUTLIER), cc.astype(np.float32)
        else:
            pred, sc = radius_vote_reference(off, idx, dist, s["labels"], C, INV_DIST, EUCLIDEAN, OUTLIER)
        return dict(pred=pred, scores=sc, count=count, correct=np.array([(pred == s["qlabels"]).sum()], np.int64))

    return _pick("dir", "train", "labels", "test", "qlabels", decoy="decoy" if weights == "uniform" else "perm"), run, want


case("radius_predict_device", tag="uniform")(lambda: _radius_predict_case("uniform"))
case("radius_predict_device", tag="distance")(lambda: _radius_predict_case("distance"))


@case("radius_loo_device")
def _radius_loo():
    def run(ctx, t, out, stream):
        pred, sc, count, correct = ctx.radius_loo_device(t["train"], t["labels"], threshold=_thr("dir", "tt")[0],
                                                         num_classes=C, outlier_label=OUTLIER, stream=stream,
                                                         d=SHAPES["dir"][2])
        return dict(pred=pred, scores=sc, count=count, correct=correct)

    def want():
        s = _set("dir", "real")
        count, _, _, _, cc = radius_reference(s["tr"], s["tr"], _thr("dir", "tt")[0], EUCLIDEAN, self_base=0,
                                              labels=s["labels"], C=C, D=_D("dir", "real", "tt").copy())
        pred = count_vote_reference(cc, OUTLIER)
        return dict(pred=pred, scores=cc.astype(np.float32), count=count,
                    correct=np.array([(pred == s["labels"]).sum()], np.int64))

    return _pick("dir", "train", "labels"), run, want


@case("radius_regress_device")
def _radius_regress():
    def run(ctx, t, out, stream):
        pred, count = ctx.radius_regress_device(t["train"], t["targets"], t["test"], threshold=_thr("dir", "qt")[0],
                                                weights="distance", stream=stream, d=SHAPES["dir"][2])
        return dict(pred=pred, count=count)

    def want():
        count, off, idx, dist, _ = _csr("dir", "real", _thr("dir", "qt")[0])
        return dict(pred=radius_regress_reference(off, idx, dist, _set("dir", "real")["targets"], INV_DIST, EUCLIDEAN),
                    count=count)

    return _pick("dir", "train", "targets", "test", decoy="perm"), run, want


def _radius_sweep_case(entry):
    d = SHAPES["dir"][2]
    loo = entry == "radius_sweep_loo_device"

    def run(ctx, t, out, stream):
        thr = _thr("dir", "tt" if loo else "qt")[1]
        if loo:
            got = ctx.radius_sweep_loo_device(t["train"], t["labels"], thresholds=thr, num_classes=C, outlier_label=OUTLIER,
                                              class_counts=True, stream=stream, d=d)
        else:
            got = ctx.radius_sweep_device(t["train"], t["labels"], t["test"], thresholds=thr, num_classes=C,
                                          query_labels=t["qlabels"], outlier_label=OUTLIER, class_counts=True,
                                          stream=stream, d=d)
        return dict(zip(("count", "pred", "correct", "outliers", "cc"), got))

    def want():
        s = _set("dir", "real")
        pair = "tt" if loo else "qt"
        count, cc, pred, correct, outliers = radius_sweep_reference(
            _D("dir", "real", pair), _thr("dir", pair)[1], 0 if loo else None, s["labels"], C, OUTLIER,
            s["labels"] if loo else s["qlabels"])
        return dict(count=count, cc=cc, pred=pred, correct=correct, outliers=outliers)

    return _pick("dir", *(("train", "labels") if loo else ("train", "labels", "test", "qlabels"))), run, want


case("radius_sweep_device")(lambda: _radius_sweep_case("radius_sweep_device"))
case("radius_sweep_loo_device")(lambda: _radius_sweep_case("radius_sweep_loo_device"))


def _top_lists():
    """The real set's CSR lists at the sweep's last threshold."""
    return _csr("dir", "real", float(_thr("dir", "qt")[1][-1]))[1:4]


@case("radius_vote_sweep_device")
def _radius_vote_sweep():
    def make(which):
        off, idx, dist = _top_lists()
        s = _set("dir", which)
        return dict(offsets=off, idx=idx, dist=dist if which == "real" else dist[::-1].copy(), labels=s["labels"],
                    qlabels=s["qlabels"])

    def run(ctx, t, out, stream):
        pred, correct, sc = ctx.radius_vote_sweep_device(t["offsets"], t["idx"], t["dist"], t["labels"], C,
                                                         thresholds=_thr("dir", "qt")[1], weights="distance",
                                                         outlier_label=OUTLIER, query_labels=t["qlabels"], stream=stream)
        return dict(pred=pred, correct=correct, scores=sc)

    def want():
        s = _set("dir", "real")
        pred, sc = radius_vote_sweep_reference(*_top_lists(), s["labels"], C, INV_DIST, EUCLIDEAN, OUTLIER,
                                               _thr("dir", "qt")[1])
        return dict(pred=pred, scores=sc, correct=_correct(pred, s["qlabels"]))

    return make, run, want


def _radius_sweep_predict_case(weights):
    def run(ctx, t, out, stream):
        pred, sc, count, correct = ctx.radius_sweep_predict_device(
            t["train"], t["labels"], t["test"], thresholds=_thr("dir", "qt")[1], num_classes=C, weights=weights,
            outlier_label=OUTLIER, query_labels=t["qlabels"], stream=stream, d=SHAPES["dir"][2])
        return dict(pred=pred, scores=sc, count=count, correct=correct)

    def want():
        s = _set("dir", "real")
        thr = _thr("dir", "qt")[1]
        count, cc, pred, _, _ = radius_sweep_reference(_D("dir", "real", "qt"), thr, None, s["labels"], C, OUTLIER)
        sc = cc.astype(np.float32)
        if weights != "uniform":
            pred, sc = radius_vote_sweep_reference(*_top_lists(), s["labels"], C, INV_DIST, EUCLIDEAN, OUTLIER, thr)
        return dict(pred=pred, scores=sc, count=count, correct=_correct(pred, s["qlabels"]))

    return _pick("dir", "train", "labels", "test", "qlabels", decoy="decoy" if weights == "uniform" else "perm"), run, want


case("radius_sweep_predict_device", tag="uniform")(lambda: _radius_sweep_predict_case("uniform"))
case("radius_sweep_predict_device", tag="distance")(lambda: _radius_sweep_predict_case("distance"))


# --- DBSCAN and the spanning tree -------------------------------------------------------
def _self_rows(tag):
    return lambda which: dict(train=_pad4(_self(tag, which)[0]))


def _dbscan_case(tag):
    n, d = SELF_SHAPES[tag]

    def run(ctx, t, out, stream):
        _, thr, m, _ = dbscan_case(n, d, EUCLIDEAN, 1)
        labels, count = out((n,), _i32()), out((n,), _i32())
        _, _, summary = ctx.dbscan_device(t["train"], threshold=float(thr), min_samples=m, labels=labels, count=count,
                                          stream=stream, d=d)
        return dict(labels=labels, count=count, summary=summary)

    return _self_rows(tag), run, lambda: dict(zip(("labels", "count", "summary"), dbscan_case(n, d, EUCLIDEAN, 1)[3]))


case("dbscan_device")(lambda: _dbscan_case("s11"))
case("dbscan_device", "bf", stats=_mfma_radius)(lambda: _dbscan_case("s64"))


@case("dbscan_lists_device")
def _dbscan_lists():
    n, d = SELF_SHAPES["s11"]

    def make(which):
        _, thr, _, _ = dbscan_case(n, d, EUCLIDEAN, 1)
        D = _self("s11", "real")[1] if which == "real" else _self_perm("s11")[1]
        _, off, idx, _, _ = radius_reference(None, None, thr, EUCLIDEAN, D=D)
        return dict(offsets=off, idx=idx)

    def run(ctx, t, out, stream):
        labels, count = out((n,), _i32()), out((n,), _i32())
        _, _, summary = ctx.dbscan_lists_device(t["offsets"], t["idx"], min_samples=dbscan_case(n, d, EUCLIDEAN, 1)[2],
                                                labels=labels, count=count, stream=stream)
        return dict(labels=labels, count=count, summary=summary)

    return make, run, lambda: dict(zip(("labels", "count", "summary"), dbscan_case(n, d, EUCLIDEAN, 1)[3]))


def _dbscan_sweep_case(tag, name):
    n, d = SELF_SHAPES[tag]

    def run(ctx, t, out, stream):
        _, _, thr, m, _ = sweep_case(name)
        labels = out((len(thr), n), _i32())
        _, count, summary = ctx.dbscan_sweep_device(t["train"], thresholds=thr, min_samples=m, labels=labels, count=True,
                                                    stream=stream, d=d)
        return dict(labels=labels, count=count, summary=summary)

    return _self_rows(tag), run, lambda: dict(zip(("labels", "count", "summary"), sweep_case(name)[4][:3]))


case("dbscan_sweep_device")(lambda: _dbscan_sweep_case("s3", "set1000x3"))
case("dbscan_sweep_device", "bf", stats=_mfma_radius)(lambda: _dbscan_sweep_case("s64", "set4096x64"))

MST_M = 4


def _mst_case(tag):
    n, d = SELF_SHAPES[tag]

    def run(ctx, t, out, stream):
        w, a, b = out((n - 1,), _f32()), out((n - 1,), _i32()), out((n - 1,), _i32())
        w, a, b, core, summary = ctx.mst_device(t["train"], min_samples=MST_M, core=True, w=w, a=a, b=b, stream=stream, d=d)
        return dict(w=w, a=a, b=b, core=core, summary=summary)

    def want():
        w, a, b, core, summary = mst_case("dbscan", n, d, EUCLIDEAN, MST_M)[2]
        return dict(w=w, a=a, b=b, core=core, summary=(summary, slice(0, 2)))

    return _self_rows(tag), run, want


case("mst_device")(lambda: _mst_case("s11"))
case("mst_device", "bf", stats=_bf16_filter)(lambda: _mst_case("s64"))


@functools.lru_cache(maxsize=None)
def _tree(which):
    """(w, a, b, core) of the s11 set, or of the same rows renumbered (as many edges)."""
    n, d = SELF_SHAPES["s11"]
    ref = mst_case("dbscan", n, d, EUCLIDEAN, MST_M)[2] if which == "real" else mst_reference(_self_perm("s11")[1], MST_M)
    assert len(ref[0]) == n - 1
    return ref[:4]


@case("mst_cut_device")
def _mst_cut():
    n = SELF_SHAPES["s11"][0]

    def thr():
        return thresholds_of(_self("s11", "real")[1], Q4)

    def run(ctx, t, out, stream):
        labels = out((len(Q4), n), _i32())
        _, summary = ctx.mst_cut_device(t["w"], t["a"], t["b"], t["core"], thresholds=thr(), labels=labels, stream=stream)
        return dict(labels=labels, summary=summary)

    def want():
        labels, summary = mst_cut(*_tree("real"), thr(), n)
        return dict(labels=labels, summary=summary)

    return (lambda which: dict(zip(("w", "a", "b", "core"), _tree(which)))), run, want


# --- confusion matrix, generator, MFMA probes ---------------------------------------------
@case("confusion_matrix_device")
def _confusion():
    def make(which):
        r = np.random.default_rng(50 + (which != "real"))
        lab = r.integers(0, C, size=1000).astype(np.int32)
        return dict(pred=np.where(r.random(1000) < 0.7, lab, r.integers(0, C, size=1000)).astype(np.int32), labels=lab)

    def run(ctx, t, out, stream):
        cm = out((C, C), _i32())
        _, acc = ctx.confusion_matrix_device(t["pred"], t["labels"], C, cm=cm, stream=stream)
        return dict(cm=cm, acc=np.array([acc], np.float32))

    def want():
        x = make("real")
        cm = np.zeros((C, C), np.int32)
        np.add.at(cm, (x["labels"], x["pred"]), 1)              # [true][pred], main.cpp:87
        return dict(cm=cm, acc=np.array([np.float32(np.trace(cm)) / np.float32(1000)], np.float32))

    return make, run, want


GEN = dict(row0=7, d=11, kind=0, seed=9, stream_id=2, n=300)


@case("generate")
def _generate():
    """The call has outputs alone: the producer writes them first, the generator after it.  The
    buffer has 8 rows more than the call fills; they stay the producer's, so the decoy's reference
    differs.  (The pad column of the 12-word rows is the generator's: it writes zeros there.)"""
    def make(which):
        r = np.random.default_rng(60 + (which != "real"))
        return dict(feat=r.standard_normal((GEN["n"] + 8, 12)).astype(np.float32),
                    labels=r.integers(0, C, size=GEN["n"]).astype(np.int32))

    def run(ctx, t, out, stream):
        ctx.generate(t["feat"][:GEN["n"]], t["labels"], GEN["row0"], GEN["d"], GEN["kind"], GEN["seed"],
                     GEN["stream_id"], C, stream=stream)
        return dict(feat=t["feat"], labels=t["labels"])

    def want():
        f, lab = _FIX["oracle"].gen(GEN["seed"], GEN["stream_id"], GEN["row0"], GEN["n"], GEN["d"], ld=12,
                                    kind=GEN["kind"], C=C)
        return dict(feat=np.concatenate([f, make("real")["feat"][GEN["n"]:]]), labels=lab)

    return make, run, want


def _probe_operands(which, i8):
    r = np.random.default_rng(70 + (which != "real") + 2 * i8)
    if i8:
        return dict(a=r.integers(-128, 128, size=(32, 64)).astype(np.int8), b=r.integers(-128, 128, size=(32, 64)).astype(np.int8))
    u = r.uniform(-1, 1, (2, 32, 64)).astype(np.float32).view(np.uint32)
    return dict(a=(u[0] >> 16).astype(np.uint16).view(np.int16), b=(u[1] >> 16).astype(np.uint16).view(np.int16))


def _pin_bf16_probe(ref):
    """No restatement fixes the MFMA's bits: test_gpu_mfma_cert's bound against the exact sums."""
    x = _probe_operands("real", False)
    av, bv = ((x[n].view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64) for n in ("a", "b"))
    for i in range(32):
        for j in range(32):
            p = av[i] * bv[j]
            assert abs(float(ref["out"][i, j]) - math.fsum(p)) <= 2 * 2.0 ** -24 * 64 * math.fsum(np.abs(p)) + 64 * 2.0 ** -126


def _probe_case(i8):
    def run(ctx, t, out, stream):
        if i8:
            return dict(out=ctx.mfma_probe_i8(t["a"], t["b"], stream=stream))
        bf = _torch().bfloat16
        return dict(out=ctx.mfma_probe_bf16(t["a"].view(bf), t["b"].view(bf), stream=stream))

    def want():
        x = _probe_operands("real", True)
        return dict(out=(x["a"].astype(np.int64) @ x["b"].astype(np.int64).T).astype(np.int32))

    return (lambda which: _probe_operands(which, i8)), run, want if i8 else None


case("mfma_probe_bf16", pin=_pin_bf16_probe)(lambda: _probe_case(False))
case("mfma_probe_i8")(lambda: _probe_case(True))

CASE_IDS = [c.id for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


# ---------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------
class Outs:
    """The outputs a case pre-allocates: guard-filled, with GUARD_WORDS guard elements past each one's
    extent.  Without a plan (a reference call, on the default stream) a request is served on the spot
    and noted; with the noted plan every buffer is allocated and filled at once, during setup, and
    the requests are served from them in order -- so no guard fill is enqueued behind the delays."""

    def __init__(self, plan=None):
        self.plan = plan
        self.flat = [] if plan is None else [self._new(shape, dtype) for shape, dtype in plan]
        self.asked = []

    @staticmethod
    def _new(shape, dtype):
        n = int(np.prod(shape))
        return _torch().full((n + GUARD_WORDS,), GUARD, dtype=dtype, device=DEV), n

    def __call__(self, shape, dtype):
        shape = tuple(shape)
        self.asked.append((shape, dtype))
        if self.plan is None:
            self.flat.append(self._new(shape, dtype))
        else:
            assert self.plan[len(self.asked) - 1] == (shape, dtype), "other outputs than the reference call's"
        f, n = self.flat[len(self.asked) - 1]
        return f[:n].view(shape)

    def intact(self):
        return all(bool((f[n:] == GUARD).all()) for f, n in self.flat)


def _host(res):
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in res.items() if v is not None}


def _same(a, b):
    """Two result dicts hold the same names, dtypes, shapes and bits: the first name that differs, or None."""
    if sorted(a) != sorted(b):
        return f"names {sorted(a)} != {sorted(b)}"
    for k in a:
        if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or not np.array_equal(_ubits(a[k]), _ubits(b[k])):
            return k
    return None


class Env:
    def __init__(self, knn):
        self.knn = knn
        self.ctxs = {k: knn.Context(0, **kw) for k, kw in CONTEXTS.items()}
        self.refs = {}
        self.rate = self.T = self.longest = None
        self.s = self.x = None
        self.control = None

    def close(self):
        for c in self.ctxs.values():
            c.close()

    def sleep(self, ms=None):
        """A device-side wait of ms (default T) on torch's current stream."""
        _torch().cuda._sleep(int((self.T if ms is None else ms) * self.rate))

    def calibrate(self):
        torch = _torch()
        torch.cuda._sleep(1_000_000)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cycles = 20_000_000
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        torch.cuda.synchronize()
        self.rate = cycles / e0.elapsed_time(e1)

    def reference(self, case, inputs):
        """The case on the default stream with these inputs in fresh tensors: (host results, ms by
        events, the outputs it pre-allocated)."""
        torch = _torch()
        ctx = self.ctxs[case.ctx]
        t = {k: _dev(v) for k, v in inputs.items()}
        out = Outs()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        res = case.run(ctx, t, out, None)
        e1.record()
        torch.cuda.synchronize()
        assert out.intact(), "guard words"
        return _host(res), e0.elapsed_time(e1), out.asked

    def references(self):
        """Every case's decoy and real reference (the decoy first, so the timed real call does not
        pay for the first call's workspace); a case that fails keeps its exception for its tests."""
        for c in CASES:
            try:
                real, decoy = c.make("real"), c.make("decoy")
                assert sorted(real) == sorted(decoy) and all(
                    real[k].shape == decoy[k].shape and real[k].dtype == decoy[k].dtype for k in real), "decoy shapes"
                ref_decoy, _, _ = self.reference(c, decoy)
                ref_real, ms, plan = self.reference(c, real)
                st = self.ctxs[c.ctx].stats()
                self.refs[c.id] = (real, decoy, ref_real, ref_decoy, ms, st, plan)
            except Exception as e:  # noqa: BLE001 -- re-raised by the case's own tests
                self.refs[c.id] = e
        times = [r[4] for r in self.refs.values() if not isinstance(r, Exception)]
        self.longest = max(times) if times else 0.0
        self.T = min(200.0, max(20.0, 20.0 * self.longest))

    def get(self, case):
        r = self.refs[case.id]
        if isinstance(r, Exception):
            raise r
        return r

    def produce(self, buf, src):
        """The producer on torch's current stream: the wait, then the real inputs over the decoy."""
        self.sleep()
        for k in buf:
            buf[k].copy_(src[k])

    def pick_streams(self):
        """s: the first of 4 fresh side streams on which the control shows the decoy; x: the first of
        4 whose wait overlaps a wait on s."""
        torch = _torch()
        c = next(c for c in CASES if c.id == "dir-predict_device")
        real, decoy, ref_real, ref_decoy, _, _, plan = self.get(c)
        seen = []
        for cand in [torch.cuda.Stream() for _ in range(4)]:
            buf, src = {k: _dev(v) for k, v in decoy.items()}, {k: _dev(v) for k, v in real.items()}
            out = Outs(plan)
            torch.cuda.synchronize()
            with torch.cuda.stream(cand):
                self.produce(buf, src)
            got = _host(c.run(self.ctxs["dir"], buf, out, 0))  # 0: hip_stream = NULL, the context's own stream
            torch.cuda.synchronize()
            seen.append("decoy" if _same(got, ref_decoy) is None else "real" if _same(got, ref_real) is None else "neither")
            if seen[-1] == "decoy":
                self.s = cand
                break
        self.control = seen
        if self.s is None:
            return
        for cand in [torch.cuda.Stream() for _ in range(4)]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(self.s):
                self.sleep(20.0)
            with torch.cuda.stream(cand):
                self.sleep(20.0)
            torch.cuda.synchronize()
            if (time.perf_counter() - t0) * 1e3 < 32.0:
                self.x = cand
                break

    def variant(self, case, variant):
        torch = _torch()
        ctx = self.ctxs[case.ctx]
        real, decoy, ref_real, _, _, _, plan = self.get(case)
        buf, src = {k: _dev(v) for k, v in decoy.items()}, {k: _dev(v) for k, v in real.items()}
        out = Outs(plan)
        torch.cuda.synchronize()
        if variant == "current":
            with torch.cuda.stream(self.s):
                self.produce(buf, src)
                res = case.run(ctx, buf, out, None)
        elif variant == "explicit":
            with torch.cuda.stream(self.s):
                self.produce(buf, src)
            with torch.cuda.stream(self.x):
                # (1.5 T: s has drained by about T + T / 20, so whatever a wrapper enqueues on torch's
                # current stream lands after the call's results, not before them)
                self.sleep(1.5 * self.T)
                res = case.run(ctx, buf, out, self.s.cuda_stream)
        else:
            self.produce(buf, src)
            res = case.run(ctx, buf, out, None)
        torch.cuda.synchronize()
        return _host(res), out.intact(), ref_real


@pytest.fixture(scope="module")
def env(knn, oracle):
    _FIX.update(knn=knn, oracle=oracle)
    e = Env(knn)
    try:
        e.calibrate()
        e.references()
        e.pick_streams()
        print(f"[streams] _sleep rate {e.rate:.0f} cycles/ms, longest reference call {e.longest:.3f} ms, T = {e.T:.1f} ms, "
              f"control {e.control}")
        yield e
    finally:
        e.close()


@pytest.fixture(scope="module")
def streams(env):
    """The module fails, it does not skip, when no stream shows the race."""
    assert env.s is not None, (f"sensitivity control: none of 4 side streams showed the decoy ({env.control}); "
                               f"a misplaced enqueue would not be seen with T = {env.T:.1f} ms")
    assert env.x is not None, "no side stream whose wait overlaps a wait on s: the explicit variant would be blind"
    return env


# ---------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------
def test_table_covers_every_stream_wrapper(knn):
    """Every method of Context and LofModel with a stream= parameter has a row in the table."""
    have = {name for cls in (knn.Context, knn.LofModel) for name, fn in inspect.getmembers(cls, inspect.isfunction)
            if not name.startswith("_") and "stream" in inspect.signature(fn).parameters}
    assert have == {c.entry for c in CASES}, sorted(have ^ {c.entry for c in CASES})


def test_control_shows_the_decoy(streams):
    """A call that is not ordered after the producer reads the decoy: T is long enough to see a
    misplaced enqueue."""
    assert streams.control[-1] == "decoy" and "neither" not in streams.control, streams.control
    assert 20.0 <= streams.T <= 200.0


@pytest.mark.parametrize("cid", CASE_IDS)
def test_reference_equals_restatement(env, cid):
    c = CASES[CASE_IDS.index(cid)]
    real, decoy, ref_real, ref_decoy, _, st, _ = env.get(c)
    if c.stats is not None:
        c.stats(st)
    if c.pin is not None:
        c.pin(ref_real)
    want = (c.want() if c.want is not None else None) or {}
    assert c.pin is not None or want, "the restatement does not cover this input set"
    for name, w in want.items():
        g = ref_real[name]
        if isinstance(w, tuple):
            w, sl = w
            g = g[sl]
        assert g.dtype == w.dtype and g.shape == w.shape, f"{name}: {g.dtype} {g.shape} != {w.dtype} {w.shape}"
        assert np.array_equal(_nbits(g), _nbits(w)), name
    assert _same(ref_real, ref_decoy) is not None, "vacuous: the decoy's reference equals the real one"


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_stream_variant(streams, cid, variant):
    got, intact, ref = streams.variant(CASES[CASE_IDS.index(cid)], variant)
    diff = _same(got, ref)
    assert diff is None, f"{cid} [{variant}]: output {diff!r} differs from the default-stream reference"
    assert intact, f"{cid} [{variant}]: guard words past an output were written"


def test_cached_train_on_two_streams(knn, streams):
    """cache_train: the first call on s prepares the train operands behind the producer, the second,
    on another side stream, finds them and runs no train pass; both equal the reference."""
    torch = _torch()
    e = streams
    c = next(c for c in CASES if c.id == "bf-predict_device")
    real, decoy, ref_real, _, _, _, plan = e.get(c)
    ctx = knn.Context(0, algo="gemm_bf16", cache_train=True)
    try:
        buf, src = {k: _dev(v) for k, v in decoy.items()}, {k: _dev(v) for k, v in real.items()}
        out1, out2 = Outs(plan), Outs(plan)
        test2 = _dev(decoy["test"])
        torch.cuda.synchronize()
        with torch.cuda.stream(e.s):
            e.produce(buf, src)
            got1 = c.run(ctx, buf, out1, None)
        st1 = ctx.stats()
        with torch.cuda.stream(e.x):
            e.sleep()
            test2.copy_(src["test"])
            got2 = c.run(ctx, dict(buf, test=test2), out2, None)
        st2 = ctx.stats()
        torch.cuda.synchronize()
        assert not st1["train_operands_cached"] and st1["filter_operands"] == "bf16 rounded", st1
        assert st2["train_operands_cached"], st2
        assert _same(_host(got1), ref_real) is None and _same(_host(got2), ref_real) is None
        assert out1.intact() and out2.intact()
    finally:
        ctx.close()
