"""Python host mirror of the MI355X KNN path (ctypes over libknn_amd.so).

The product is the C ABI in ``include/knn_amd.h`` (plus the reference-compatible C++
API in ``include/knn_arff.hpp``); this module binds it for the tests and ``bench.py``.
Names follow the reference (srna99/KNN-using-p_threads-and-MPI):

* ``KNN(train, test, k)``                      main.cpp:25      -> int32 predictions
* ``KNN_range(train, test, k, start, end)``    mpi.cpp:26 / multi-thread.cpp:37
* ``computeConfusionMatrix(pred, labels, C)``  main.cpp:87
* ``computeAccuracy(cm, n)``                   main.cpp:102
* ``read_arff(path)``                          libarff ArffParser::parse (arff_parser.cpp:23)
* ``shard_range(n, world, rank)``              multi-thread.cpp:154-158 / mpi.cpp:141-170
* ``train_sharded_predict(...)``               train-sharded KNN over ranks:
  per-shard exact top-k -> all-to-all of neighbour lists -> merge + vote
* ``Context.sweep_device / loo_device / vote_sweep_device / sweep`` and ``best_k``: the
  predictions and correct counts for every k <= K from one top-K pass (no reference counterpart)
* ``Context.sweep_weighted_device / loo_weighted_device / vote_weighted_device /
  predict_weighted_device / sweep_weighted``, ``WEIGHTS`` and ``proba``: the same with the
  distance-weighted vote and per-class scores (no reference counterpart)
* ``METRICS``, ``Context(metric=...)``, ``Context.set_metric`` and ``Context.metric``: the distance a
  context computes -- "euclidean" (squared Euclidean, the reference's and the default), "manhattan"
  or "chebyshev"; every predict / top-k / sweep / weighted call of the context follows it (no
  reference counterpart; the rules are in ``knn_amd.h`` "Metrics").  Under the last two
  ``weights="distance"`` is 1 / D and ``"sqdist"`` is rejected.
* ``Context.regress_sweep_device / regress_loo_device / regress_device / regress_vote_device /
  regress_sweep``, ``best_k_error`` and ``read_arff_targets``: k-NN regression on float32 targets
  -- the prediction for every k <= K from the same lists, under the same weight kinds and metrics,
  with the per-k sums of squared and absolute errors (no reference counterpart; the rules are in
  ``knn_amd.h`` "Regression")
* ``Context.lof_device / lof_fit_device / lof_lists_device``, ``LofModel.score_device``, ``lof_max``
  and ``lof_outliers``: the local outlier factor of every train row for every k in [k_lo, k_hi]
  from one leave-one-out top-k pass, and novelty scores of queries against the fitted tables (no
  reference counterpart; the rules are in ``knn_amd.h`` "Local outlier factor")
* ``Context.dbscan_sweep_device`` and ``best_eps``: DBSCAN's labels, counts and summaries at every
  one of up to 32 radii from three distance passes -- row r is ``Context.dbscan_device`` at
  ``radii[r]`` (no reference counterpart; the rules are in ``knn_amd.h`` "DBSCAN sweep")

Features are fp32 or bf16.  Host bf16 arrays are numpy ``uint16`` holding bf16 bits
(``to_bf16_bits`` / ``bf16_bits_to_f32``); device tensors are ``torch.bfloat16``.

There is no CPU fallback: if ``libknn_amd.so`` is missing or no gfx950 device is
visible, calls raise ``KnnError``.
"""
import ctypes
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# KNN_AMD_LIB overrides the library (A/B runs of alternative builds)
LIB_PATH = os.environ.get("KNN_AMD_LIB") or os.path.join(_HERE, "libknn_amd.so")

KNN_OK, KNN_EINVAL, KNN_ENOMEM, KNN_EHIP, KNN_ERANGE, KNN_ENODEV, KNN_EIO, KNN_ERCCL = range(8)
STATUS_NAMES = {0: "KNN_OK", 1: "KNN_EINVAL", 2: "KNN_ENOMEM", 3: "KNN_EHIP", 4: "KNN_ERANGE",
                5: "KNN_ENODEV", 6: "KNN_EIO", 7: "KNN_ERCCL"}
KNN_COMM_ID_BYTES = 128
KNN_F32, KNN_BF16 = 0, 1
ALGOS = {"auto": 0, "direct": 1, "gemm": 2, "gemm_split": 3, "gemm_bf16": 4, "direct_scan": 5, "gemm_i8": 6}
# knn_weight: the vote's weight kinds ("distance" is sklearn's weights="distance")
WEIGHTS = {"uniform": 0, "distance": 1, "sqdist": 2}
# knn_metric: the distance a context computes ("euclidean" is the reference's squared Euclidean)
METRICS = {"euclidean": 0, "manhattan": 1, "chebyshev": 2}
FILTER_OPERANDS = {-1: None, 0: "f32", 1: "bf16", 2: "bf16x3 split", 3: "bf16 rounded"}
# knn_last_stats()[11]: the element the filter multiplied.  Under "bf16 rounded" (fp32 rows rounded
# once to a narrow MFMA operand, one product per fp32 product) it is "i8" when the int8 form ran
FILTER_ELEMENTS = {0: "bf16", 1: "i8"}
# knn_last_stats()[13]: the form of a radius pass ("unsafe": the direct form, because a row norm is
# NaN, inf or >= 2^125 and the MFMA form's certificate does not hold)
RADIUS_FORMS = {0: "direct", 1: "mfma", 2: "unsafe"}


class KnnError(RuntimeError):
    def __init__(self, status, msg=""):
        self.status = status
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")


KNN_OPT_CACHE_TRAIN = 1
KNN_OPT_CACHE_TRAIN_DEVICE = 2
# contexts holding a cached device train tensor: Context.generate invalidates every one whose
# tensor shares bytes with what it writes (a slice, a view, another context's call)
_caching_contexts = weakref.WeakSet()


def _byte_span(t):
    """[first, last) device byte addresses a strided tensor covers (empty: (p, p))."""
    p = t.data_ptr()
    if t.numel() == 0:
        return p, p
    hi = sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1
    return p, p + hi * t.element_size()


class knn_opts(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("algo", ctypes.c_int32),
                ("train_splits", ctypes.c_int32), ("profile", ctypes.c_int32), ("flags", ctypes.c_int32)]


class knn_dataset(ctypes.Structure):
    _fields_ = [("feat", ctypes.c_void_p), ("labels", ctypes.c_void_p), ("n", ctypes.c_int64),
                ("d", ctypes.c_int32), ("ld", ctypes.c_int32), ("dtype", ctypes.c_int32)]


_lib = None


def load_library(path=LIB_PATH):
    """Load libknn_amd.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise KnnError(KNN_ENODEV, f"{path} not built: run `make -C {_HERE}` "
                                   "(or __graft_entry__.build())")
    # The torch wheel bundles its own ROCm runtime whose libamdhip64 has the same SONAME
    # (libamdhip64.so.7) as /opt/rocm's.  Loading torch first makes this library bind to
    # that already-loaded runtime, so a process never holds two HIP/HSA runtimes (which
    # leaves whichever initialises second without a device).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    P, I32, I64, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    DS = ctypes.POINTER(knn_dataset)
    sig = {
        "knn_version": (I32, []),
        "knn_build_id": (ctypes.c_char_p, []),
        "knn_create": (I32, [ctypes.POINTER(P), ctypes.POINTER(knn_opts)]),
        "knn_destroy": (None, [P]),
        "knn_last_error": (ctypes.c_char_p, [P]),
        "knn_predict": (I32, [P, DS, DS, I32, I32, I64, I64, P, P, P]),
        "knn_predict_device": (I32, [P, DS, DS, I32, I32, P, P, P, P]),
        "knn_shard_topk_device": (I32, [P, DS, DS, I32, I32, I64, P, P]),
        "knn_merge_vote_device": (I32, [P, I32, I64, I32, I32, P, P, P, P, P]),
        "knn_vote_sweep_device": (I32, [P, I64, I32, I32, P, I64, P, I64, P, P, P, P]),
        "knn_sweep_device": (I32, [P, DS, DS, I32, I32, I64, P, P, P, P, P, P]),
        "knn_sweep": (I32, [P, DS, DS, I32, I32, I64, P, P, P]),
        "knn_vote_weighted_device": (I32, [P, I64, I32, I32, P, P, I64, P, I32, I64, P, P, P, P, P]),
        "knn_sweep_weighted_device": (I32, [P, DS, DS, I32, I32, I32, I64, P, P, P, P, P, P, P]),
        "knn_predict_weighted_device": (I32, [P, DS, DS, I32, I32, I32, P, P, P, P, P]),
        "knn_sweep_weighted": (I32, [P, DS, DS, I32, I32, I32, I64, P, P, P, P]),
        "knn_regress_vote_device": (I32, [P, I64, I32, P, P, I64, P, I32, I64, P, P, P, P, P]),
        "knn_regress_sweep_device": (I32, [P, DS, DS, P, I32, I32, I64, P, P, P, P, P, P, P]),
        "knn_regress_device": (I32, [P, DS, DS, P, I32, I32, P, P, P, P]),
        "knn_regress_sweep": (I32, [P, DS, DS, P, I32, I32, I64, P, P, P, P]),
        "knn_lof_fit_device": (I32, [P, DS, I32, I32, P, P, P, P, P, P]),
        "knn_lof_score_device": (I32, [P, DS, DS, I32, I32, P, P, P, P]),
        "knn_lof_lists_device": (I32, [P, I64, I32, P, P, I64, I64, I32, I32, P, P, P, P]),
        "knn_radius_count_device": (I32, [P, DS, DS, F, I32, I64, I32, P, P, P, P, P, P, P]),
        "knn_radius_fill_device": (I32, [P, DS, DS, F, I64, P, P, P, P]),
        "knn_radius_vote_device": (I32, [P, I64, I64, P, P, P, P, I32, I32, I32, P, P, P, P, P]),
        "knn_radius_regress_device": (I32, [P, I64, I64, P, P, P, P, I32, P, P]),
        "knn_radius_sweep_count_device": (I32, [P, DS, DS, P, I32, I32, I64, I32, P, I64, P, P, P, P, P, P]),
        "knn_radius_sweep_max_queries": (I64, [P, I32, I32]),
        "knn_radius_vote_sweep_device": (I32, [P, I64, I64, P, P, P, P, I32, I32, P, I32, I32, P, I64, P, P, P, P]),
        "knn_dbscan_device": (I32, [P, DS, F, I32, P, P, P, P]),
        "knn_dbscan_lists_device": (I32, [P, I64, P, P, I32, P, P, P, P]),
        "knn_dbscan_sweep_device": (I32, [P, DS, P, I32, I32, I64, P, P, P, P]),
        "knn_mst_device": (I32, [P, DS, I32, P, P, P, P, P, P]),
        "knn_mst_cut_device": (I32, [P, I64, I64, P, P, P, P, P, I32, I64, P, P, P]),
        "knn_arff_copy_targets": (I32, [P, P, I32, P]),
        "knn_stage_times": (I32, [P, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(F), I32]),
        "knn_last_stats": (I32, [P, ctypes.POINTER(I64), I32]),
        "knn_generate": (I32, [P, P, P, I64, I64, I32, I32, I32, I32, ctypes.c_uint64,
                               ctypes.c_uint32, I32, P]),
        "knn_mfma_probe_bf16": (I32, [P, P, P, I32, P, P]),
        "knn_mfma_probe_i8": (I32, [P, P, P, I32, P, P]),
        "knn_debug_set_i8_coarsen": (I32, [P, F]),
        "knn_set_generation": (I32, [P, ctypes.c_uint64]),
        "knn_set_metric": (I32, [P, I32]),
        "knn_get_metric": (I32, [P]),
        "knn_comm_unique_id": (I32, [P]),
        "knn_comm_create": (I32, [P, P, I32, I32, ctypes.POINTER(P)]),
        "knn_comm_destroy": (None, [P]),
        "knn_comm_count": (I32, [P, ctypes.POINTER(I32)]),
        "knn_comm_broken": (I32, [P, ctypes.POINTER(I32)]),
        "knn_comm_set_exchange": (I32, [P, I64, I32]),
        "knn_predict_train_sharded": (I32, [P, P, DS, I64, DS, I32, I32, P, P, P, P]),
        "knn_shard_range": (I32, [I64, I32, I32, ctypes.POINTER(I64), ctypes.POINTER(I64)]),
        "knn_shard_policy": (I32, [I64, I64, I32, I32, I32, I64, ctypes.POINTER(I32)]),
        "knn_radius_policy": (I32, [I32, I32, I32, I64, I64, I32, ctypes.POINTER(I32)]),
        "knn_filter_policy": (I32, [I32, I32, I32, I64, I64, I32, ctypes.POINTER(I32), ctypes.POINTER(I32)]),
        "knn_exchange_layout": (I32, [I64, I32, I32, I32, P, P, P, P]),
        "knn_alloc_pinned": (I32, [ctypes.c_size_t, ctypes.POINTER(P)]),
        "knn_free_pinned": (None, [P]),
        "knn_confusion_matrix": (I32, [P, P, I64, I32, P]),
        "knn_confusion_matrix_device": (I32, [P, P, P, I64, I32, P, P, P]),
        "knn_accuracy": (F, [P, I32, I64]),
        "knn_arff_open": (I32, [ctypes.c_char_p, ctypes.POINTER(P), ctypes.c_char_p, I32]),
        "knn_arff_shape": (None, [P, ctypes.POINTER(I64), ctypes.POINTER(I32), ctypes.POINTER(I32)]),
        "knn_arff_copy": (I32, [P, P, I32, P]),
        "knn_arff_close": (None, [P]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _opt_ptr(t):
    """An optional device tensor's address (None: NULL)."""
    return None if t is None else t.data_ptr()


def _self_base(self_base):
    """The C ABI's self_base: -1 without self-removal."""
    return -1 if self_base is None else self_base


def to_bf16_bits(x):
    """float32 array -> uint16 bf16 bits (round to nearest even; exact for bf16 values)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_bits_to_f32(b):
    """uint16 bf16 bits -> the exactly widened float32 values."""
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def _dataset(feat, labels=None):
    """numpy features (float32, or uint16 = bf16 bits) -> knn_dataset (+ arrays to keep alive)."""
    if isinstance(feat, np.ndarray) and feat.dtype == np.uint16:
        feat, dtype = np.ascontiguousarray(feat), KNN_BF16
    else:
        feat, dtype = np.ascontiguousarray(feat, dtype=np.float32), KNN_F32
    if feat.ndim != 2:
        raise KnnError(KNN_EINVAL, "features must be 2-D [n][d]")
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32)
    ds = knn_dataset(feat.ctypes.data, None if lab is None else lab.ctypes.data, feat.shape[0],
                     feat.shape[1], feat.shape[1], dtype)
    return ds, (feat, lab)  # keep the arrays alive


def _tensor_dtype(t):
    import torch
    if t.dtype == torch.bfloat16:
        return KNN_BF16
    if t.dtype == torch.float32:
        return KNN_F32
    raise KnnError(KNN_EINVAL, f"features must be float32 or bfloat16, got {t.dtype}")


def _check_tensor(t, name, dtype, n=None):
    """A device output/label tensor: contiguous, of the element type the C ABI reads."""
    import torch
    if t.dtype != dtype:
        raise KnnError(KNN_EINVAL, f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise KnnError(KNN_EINVAL, f"{name} must be contiguous")
    if n is not None and t.numel() < n:
        raise KnnError(KNN_EINVAL, f"{name} holds {t.numel()} elements, needs {n}")
    return t


def _device_dataset(feat, labels=None, d=None):
    """A [n][ld] device tensor (unit stride along features; ld = its row stride) and its
    int32 labels -> knn_dataset.  Views such as x[:, :64] of a wider tensor are accepted
    (ld = the parent's row stride); anything with non-unit feature stride is rejected."""
    import torch
    if feat.dim() != 2:
        raise KnnError(KNN_EINVAL, "features must be a 2-D [n][ld] tensor")
    if feat.shape[0] > 1 and feat.stride(1) != 1:
        raise KnnError(KNN_EINVAL, "features must have unit stride along the feature axis")
    # (one row: torch may report any stride(0) for it; a view of a wider table keeps the table's
    # pitch -- x[:1, :257] of 264-column rows is as aligned as x[:2, :257] -- anything shorter than
    # the row is not a pitch)
    ld = feat.stride(0) if feat.shape[0] > 1 or feat.stride(0) >= feat.shape[1] else feat.shape[1]
    d = feat.shape[1] if d is None else d
    if d > feat.shape[1]:
        raise KnnError(KNN_EINVAL, f"d={d} exceeds the tensor's {feat.shape[1]} columns")
    if labels is not None:
        _check_tensor(labels, "labels", torch.int32, feat.shape[0])
    return knn_dataset(feat.data_ptr(), _opt_ptr(labels), feat.shape[0], d,
                       ld, _tensor_dtype(feat))


def _stream_arg(stream, tensor):
    """The HIP stream a device call is enqueued on: the caller's, else torch's current stream
    of the tensor's device -- so the call is ordered after the torch work that produced its
    inputs (a copy, a dtype conversion, a clone) and before the torch work that reads its
    outputs, with no extra synchronisation."""
    if stream is None and tensor is not None and getattr(tensor, "is_cuda", False):
        import torch
        # (the raw handle: 0.08 us per call against 1.9 for a torch.cuda.Stream object, on a
        # ~0.1 ms config-L call; scripts/diag_call_overhead.py)
        raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        stream = raw(tensor.device.index) if raw is not None else torch.cuda.current_stream(tensor.device).cuda_stream
    return None if stream is None else ctypes.c_void_p(stream)


def _torch_on(stream, tensor):
    """The context a wrapper does its own torch work under (a zero fill, an .item() read-back, a
    dtype conversion, a temporary): torch's current stream becomes the call's stream= when one is
    given, so the result does not depend on what torch's current stream is or on what is pending
    there.  Without stream= the call runs on torch's current stream already."""
    import contextlib
    if stream is None or not getattr(tensor, "is_cuda", False):
        return contextlib.nullcontext()
    import torch
    dev = tensor.device
    # (handle 0 is the legacy null stream, torch's default stream)
    return torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev) if stream else torch.cuda.default_stream(dev))


def _outputs(nq, k, pred=None, dist=None, idx=None):
    """Type/shape checks of device outputs (pred int32 [nq], dist float32 / idx int32 [nq][k])."""
    import torch
    if pred is not None:
        _check_tensor(pred, "pred", torch.int32, nq)
    if dist is not None:
        _check_tensor(dist, "dist", torch.float32, nq * k)
    if idx is not None:
        _check_tensor(idx, "idx", torch.int32, nq * k)


def shard_range(n, world, rank):
    """Contiguous split with the remainder on the last worker (multi-thread.cpp:154-158,
    mpi.cpp:141-170): worker w < world-1 gets [w*(n//world), (w+1)*(n//world))."""
    per, left = divmod(n, world)
    start = rank * per
    return start, start + per + (left if rank == world - 1 else 0)


def rank_queries(n_query, world, rank, scaling):
    """Query rows [q0, q0+nq) a rank owns.  "strong": the reference's split of a fixed
    test set (shard_range).  "weak": every rank owns n_query rows of its own,
    rank r taking global rows [r*n_query, (r+1)*n_query)."""
    if scaling == "weak":
        return rank * n_query, n_query
    q0, q1 = shard_range(n_query, world, rank)
    return q0, q1 - q0


def gather_predictions(pred_local, q0, n_total, world, rank, group=None):
    """Rank 0 receives every rank's predictions at their global offsets -- the
    reference's MPI_Gatherv (mpi.cpp:177-186) -- over torch.distributed (any backend).
    Returns the full int32 vector on rank 0, None elsewhere."""
    import torch.distributed as dist
    pred_local = np.ascontiguousarray(pred_local, np.int32)
    parts = [None] * world if rank == 0 else None
    dist.gather_object((int(q0), pred_local), parts, dst=0, group=group)
    if rank != 0:
        return None
    out = np.full(n_total, -1, np.int32)
    for off, p in parts:
        out[off:off + len(p)] = p
    return out


def exchange_shard_lists(rec, n_query, world, rank, group=None):
    """The train-sharded exchange: every rank holds its shard's neighbour
    lists for ALL queries, rec [n_query][3][k]; rank r owns queries shard_range(n_query,
    world, r) (the reference's split, mpi.cpp:141-170).  One all-to-all (RCCL over xGMI on
    the GPU node; any torch.distributed backend works) hands each rank the lists of its
    own queries from every shard: returns [world][nq_r][3][k] (source rank order = shard
    order = global index order) and this rank's query range (q0, q1)."""
    import torch
    import torch.distributed as dist
    k3 = rec.shape[1] * rec.shape[2]
    spans = [shard_range(n_query, world, r) for r in range(world)]
    q0, q1 = spans[rank]
    send = [(b - a) * k3 for a, b in spans]          # to rank r: its query rows
    recv = [(q1 - q0) * k3] * world                   # from every rank: my query rows
    out = torch.empty((world, q1 - q0) + tuple(rec.shape[1:]), dtype=rec.dtype, device=rec.device)
    if world == 1:
        out[0].copy_(rec)
    else:
        dist.all_to_all_single(out.view(-1), rec.contiguous().view(-1), recv, send, group=group)
    return out, (q0, q1)


def train_sharded_predict(ctx, train_shard, labels_shard, idx_base, test, k, num_classes, world, rank,
                          group=None, dist_out=None, idx_out=None, stream=None):
    """KNN with the train set sharded over ranks: this rank's
    shard (global rows [idx_base, idx_base + n)) against every query -> exchange ->
    merge + vote for the queries this rank owns.  Returns (pred [nq_r] int32 device
    tensor, (q0, q1)).  Bit-identical to the reference's serial KNN over the whole set."""
    import torch
    nq = test.shape[0]
    if stream is None and test.is_cuda:
        # one stream for topk -> all-to-all -> merge (the collective is ordered on torch's
        # current stream, so the merge must be too)
        stream = torch.cuda.current_stream(test.device).cuda_stream
    rec = torch.empty((nq, 3, k), dtype=torch.int32, device=test.device)
    ctx.shard_topk_device(train_shard, labels_shard, test, k, num_classes, idx_base, rec, stream=stream)
    lists, (q0, q1) = exchange_shard_lists(rec, nq, world, rank, group)
    del rec
    pred = torch.empty(q1 - q0, dtype=torch.int32, device=test.device)
    ctx.merge_vote_device(lists, k, num_classes, pred, dist_out, idx_out, stream=stream)
    return pred, (q0, q1)


class Context:
    """One device, one HIP stream (knn_create / knn_destroy)."""

    def __init__(self, device=0, algo="auto", train_splits=0, profile=False, cache_train=False,
                 metric="euclidean"):
        self.lib = load_library()
        # metric: a key of METRICS (or its number), set_metric changes it between calls
        # profile: False/0 off, True/1 per-stage HIP events, 2 = also count filter candidates,
        # 3 = events around the dominant stages only (filter, rescore, ...: knn_amd.h)
        # cache_train: predict() keeps the device copy of train across calls (KNN_OPT_CACHE_TRAIN)
        # and the device calls keep the operands derived from the caller's train tensor
        # (KNN_OPT_CACHE_TRAIN_DEVICE): this wrapper bumps the generation on every write it can see
        opts = knn_opts(device, ALGOS[algo], train_splits, int(profile),
                        KNN_OPT_CACHE_TRAIN | KNN_OPT_CACHE_TRAIN_DEVICE if cache_train else 0)
        self.cache_train = bool(cache_train)
        # the arrays whose addresses key the library's train cache (knn_predict): held until
        # the next call replaces them, so no later array can be allocated at a cached address
        # (_dataset copies inputs of another dtype or layout into temporaries)
        self._train_key = None
        # device calls under cache_train: the train tensor whose filter operands the library
        # keeps (knn_predict_device / knn_shard_topk_device), and its torch version counter --
        # a different tensor or an in-place write bumps the library's generation, and holding
        # the tensor keeps its address from being reused while it is cached
        self._dev_train = None
        self._generation = 0
        self.device = int(device)
        h = ctypes.c_void_p()
        st = self.lib.knn_create(ctypes.byref(h), ctypes.byref(opts))
        if st != KNN_OK:
            raise KnnError(st, f"knn_create(device={device}) failed")
        self.h = h
        if _metric_kind(metric) != 0:
            try:
                self.set_metric(metric)
            except KnnError:
                self.close()
                raise

    def _check(self, st):
        if st != KNN_OK:
            raise KnnError(st, self.lib.knn_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.knn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def predict(self, train_feat, train_labels, test_feat, k, num_classes=None, q_begin=0,
                q_end=None, topk=False):
        """Host arrays in, host arrays out (knn_predict)."""
        tr, keep1 = _dataset(train_feat, train_labels)
        te, keep2 = _dataset(test_feat)
        if num_classes is None:
            num_classes = int(keep1[1].max()) + 1 if keep1[1].size else 1
        if q_end is None:
            q_end = te.n
        nq = q_end - q_begin
        pred = np.zeros(max(nq, 0), np.int32)
        dist = np.zeros((max(nq, 0), k), np.float32) if topk else None
        idx = np.zeros((max(nq, 0), k), np.int32) if topk else None
        if self.cache_train:
            self._train_key = keep1
        self._check(self.lib.knn_predict(self.h, ctypes.byref(tr), ctypes.byref(te), k, num_classes,
                                         q_begin, q_end, _ptr(pred), _ptr(dist), _ptr(idx)))
        return (pred, dist, idx) if topk else pred

    def _on_device(self, tensor):
        """The tensor lives on this context's device (a call on another device's stream fails
        inside HIP with an unhelpful error)."""
        if tensor is not None and getattr(tensor, "is_cuda", False) and tensor.device.index != self.device:
            raise KnnError(KNN_EINVAL, f"tensor on cuda:{tensor.device.index}, context on device {self.device}")

    def _stream(self, stream, tensor):
        """_stream_arg, after _on_device."""
        self._on_device(tensor)
        return _stream_arg(stream, tensor)

    def _note_train(self, train):
        """cache_train: bump the generation when the train tensor is another one or was written
        in place since the last device call (torch's version counter)."""
        if not self.cache_train:
            return
        key = (train.data_ptr(), tuple(train.shape), train._version)
        if self._dev_train is None or self._dev_train[0] is not train or self._dev_train[1] != key:
            self.set_generation(self._generation + 1)
            self._dev_train = (train, key)
            _caching_contexts.add(self)

    def _invalidate_overlap(self, span):
        """The cached train tensor shares bytes with [span): the next device call bumps the
        generation (the write did not go through torch, so its version counter did not move)."""
        if self._dev_train is not None:
            a, b = _byte_span(self._dev_train[0])
            if a < span[1] and span[0] < b:
                self._dev_train = None

    def predict_device(self, train, labels, test, k, num_classes, pred, dist=None, idx=None,
                       stream=None, d=None):
        """Device tensors (torch, on this context's device) in and out (knn_predict_device).
        train/test: [n][ld] float32 or bfloat16 (both the same) with unit stride along the
        features and 16-byte-aligned rows: a contiguous tensor, or a column view x[:, c0:c0 + d]
        of a wider one (ld = its row stride); d (optional) reads only the first d columns.
        labels/pred/idx int32, contiguous; dist float32, contiguous.
        With cache_train the train-side filter operands are kept across calls on the same,
        unmodified train tensor (rewrites through torch are seen; after writing it by other
        means call set_generation)."""
        self._on_device(train)
        self._note_train(train)
        tr = _device_dataset(train, labels, d)
        te = _device_dataset(test, None, d)
        _outputs(te.n, k, pred, dist, idx)
        self._check(self.lib.knn_predict_device(
            self.h, ctypes.byref(tr), ctypes.byref(te), k, num_classes, pred.data_ptr(),
            _opt_ptr(dist), _opt_ptr(idx),
            self._stream(stream, test)))

    def shard_topk_device(self, train, labels, test, k, num_classes, idx_base, rec, stream=None, d=None):
        """Exact k nearest rows of one train shard for every query (knn_shard_topk_device).
        rec: int32 device tensor [nq][3][k] <- (dist bits, idx_base + row, label), ascending."""
        self._on_device(train)
        self._note_train(train)
        tr = _device_dataset(train, labels, d)
        te = _device_dataset(test, None, d)
        if tuple(rec.shape) != (test.shape[0], 3, k):
            raise KnnError(KNN_EINVAL, f"rec must be [{test.shape[0]}, 3, {k}]")
        import torch
        _check_tensor(rec, "rec", torch.int32)
        self._check(self.lib.knn_shard_topk_device(
            self.h, ctypes.byref(tr), ctypes.byref(te), k, num_classes, idx_base, rec.data_ptr(),
            self._stream(stream, test)))

    def merge_vote_device(self, rec, k, num_classes, pred, dist=None, idx=None, stream=None):
        """Merge nsrc per-shard neighbour lists rec [nsrc][nq][3][k] and vote (knn_merge_vote_device)."""
        nsrc, nq = rec.shape[0], rec.shape[1]
        if tuple(rec.shape[2:]) != (3, k) or pred.shape[0] != nq:
            raise KnnError(KNN_EINVAL, "rec must be [nsrc][nq][3][k] and pred [nq]")
        import torch
        _check_tensor(rec, "rec", torch.int32)
        _outputs(nq, k, pred, dist, idx)
        self._check(self.lib.knn_merge_vote_device(
            self.h, nsrc, nq, k, num_classes, rec.data_ptr(), pred.data_ptr(),
            _opt_ptr(dist), _opt_ptr(idx),
            self._stream(stream, rec)))

    # what the sweep-shaped calls (the k-sweep, the weighted vote, regression) share
    def _datasets_arg(self, train, labels, test, d):
        """The train / test knn_datasets of a device call; the train tensor is on this device and
        noted for the cache."""
        self._on_device(train)
        self._note_train(train)
        return _device_dataset(train, labels, d), _device_dataset(test, None, d)

    def _lists_arg(self, idx, dist, kin, self_base):
        """Neighbour lists idx int32 [nq][stride] and, optional, dist float32 of the same shape
        and strides (the uniform kind reads no distances), of which the first kin entries per row
        are read (None: all): returns nq, stride, kin, kmax (kin, or kin - 1 with self_base)."""
        import torch
        self._on_device(idx)
        if idx.dim() != 2:
            raise KnnError(KNN_EINVAL, "idx must be a 2-D [nq][stride] tensor")
        _check_tensor(idx, "idx", torch.int32)
        if dist is not None:
            _check_tensor(dist, "dist", torch.float32)
            if tuple(dist.shape) != tuple(idx.shape) or dist.stride() != idx.stride():
                raise KnnError(KNN_EINVAL, "dist must have idx's shape and strides")
            self._on_device(dist)
        nq, stride = idx.shape
        kin = stride if kin is None else kin
        return nq, stride, kin, kin - (0 if self_base is None else 1)

    @staticmethod
    def _pred_all_arg(pred_all, kmax, nq, dtype, device):
        """The caller's pred_all [kmax][nq], or a new one."""
        import torch
        if pred_all is None:
            pred_all = torch.empty((max(kmax, 0), nq), dtype=dtype, device=device)
        return _check_tensor(pred_all, "pred_all", dtype, max(kmax, 0) * nq)

    @staticmethod
    def _accum(side, name, side_dtype, nq, kmax, dtype, n=1):
        """The n per-k accumulators [kmax] that go with the queries' side input (labels -> correct,
        targets -> sse, sae), on its device; n Nones without it."""
        import torch
        if side is None:
            return [None] * n
        _check_tensor(side, name, side_dtype, nq)
        return [torch.empty(max(kmax, 0), dtype=dtype, device=side.device) for _ in range(n)]

    def _host_class_args(self, train_feat, train_labels, test_feat, kmax, num_classes, query_labels):
        """sweep's and sweep_weighted's host arguments: (train, test, num_classes, pred_all, query
        labels, correct, the arrays the datasets point into: held by the caller over its call)."""
        tr, keep = _dataset(train_feat, train_labels)
        te, keep2 = _dataset(test_feat)
        if num_classes is None:
            num_classes = int(keep[1].max()) + 1 if keep[1].size else 1
        pred_all = np.zeros((max(kmax, 0), te.n), np.int32)
        ql = None if query_labels is None else np.ascontiguousarray(query_labels, dtype=np.int32)
        if ql is not None and ql.size < te.n:
            raise KnnError(KNN_EINVAL, f"query_labels holds {ql.size} elements, needs {te.n}")
        correct = None if ql is None else np.zeros(max(kmax, 0), np.int64)
        if self.cache_train:
            self._train_key = keep
        return tr, te, num_classes, pred_all, ql, correct, (keep, keep2)

    def sweep_device(self, train, labels, test, kmax, num_classes, query_labels=None, pred_all=None,
                     self_base=None, dist=None, idx=None, stream=None, d=None):
        """Predictions (and correct counts) for every k in 1..kmax from one top-kmax pass
        (knn_sweep_device).  Returns (pred_all int32 [kmax][nq], correct int64 [kmax] or None
        without query_labels) as device tensors; pred_all[k - 1] is predict_device's pred for k.
        self_base: query q is train row self_base + q and is left out of its own neighbours
        (test must be those train rows).  dist / idx (optional) receive the [nq][kmax] lists."""
        import torch
        tr, te = self._datasets_arg(train, labels, test, d)
        pred_all = self._pred_all_arg(pred_all, kmax, te.n, torch.int32, test.device)
        _outputs(te.n, kmax, None, dist, idx)
        correct, = self._accum(query_labels, "query_labels", torch.int32, te.n, kmax, torch.int64)
        self._check(self.lib.knn_sweep_device(
            self.h, ctypes.byref(tr), ctypes.byref(te), kmax, num_classes, _self_base(self_base),
            _opt_ptr(query_labels), pred_all.data_ptr(), _opt_ptr(correct), _opt_ptr(dist), _opt_ptr(idx),
            self._stream(stream, test)))
        return pred_all, correct

    def loo_device(self, train, labels, kmax, num_classes, pred_all=None, dist=None, idx=None, stream=None,
                   d=None):
        """Leave-one-out on the train set: sweep_device with the train tensor as the queries,
        every row left out of its own neighbours, scored against its own label."""
        return self.sweep_device(train, labels, train, kmax, num_classes, query_labels=labels, pred_all=pred_all,
                                 self_base=0, dist=dist, idx=idx, stream=stream, d=d)

    def vote_sweep_device(self, idx, train_labels, num_classes, query_labels=None, pred_all=None,
                          self_base=None, kin=None, stream=None):
        """The prefix votes alone (knn_vote_sweep_device) on neighbour lists idx int32
        [nq][stride] -- predict_device's idx, merge_vote_device's, ... -- of which the first kin
        entries per row are read (default: all).  train_labels is indexed by the lists' train
        rows.  Returns (pred_all [kmax][nq], correct or None); kmax = kin, or kin - 1 with
        self_base."""
        import torch
        nq, stride, kin, kmax = self._lists_arg(idx, None, kin, self_base)
        _check_tensor(train_labels, "train_labels", torch.int32)
        pred_all = self._pred_all_arg(pred_all, kmax, nq, torch.int32, idx.device)
        correct, = self._accum(query_labels, "query_labels", torch.int32, nq, kmax, torch.int64)
        self._check(self.lib.knn_vote_sweep_device(
            self.h, nq, kin, num_classes, idx.data_ptr(), stride, train_labels.data_ptr(),
            _self_base(self_base), _opt_ptr(query_labels), pred_all.data_ptr(), _opt_ptr(correct),
            self._stream(stream, idx)))
        return pred_all, correct

    def sweep(self, train_feat, train_labels, test_feat, kmax, num_classes=None, query_labels=None,
              self_base=None):
        """Host arrays in, host arrays out (knn_sweep; not pipelined): (pred_all int32
        [kmax][nq], correct int64 [kmax] or None without query_labels)."""
        tr, te, num_classes, pred_all, ql, correct, keep = self._host_class_args(
            train_feat, train_labels, test_feat, kmax, num_classes, query_labels)
        self._check(self.lib.knn_sweep(self.h, ctypes.byref(tr), ctypes.byref(te), kmax, num_classes,
                                       _self_base(self_base), _ptr(ql), _ptr(pred_all), _ptr(correct)))
        return pred_all, correct

    @staticmethod
    def _scores_arg(scores, nq, num_classes, device):
        """scores: True = allocate float32 [nq][C], a tensor = use it, False / None = none."""
        import torch
        if scores is None or scores is False:
            return None
        if scores is True:
            return torch.empty((nq, num_classes), dtype=torch.float32, device=device)
        return _check_tensor(scores, "scores", torch.float32, nq * num_classes)

    def sweep_weighted_device(self, train, labels, test, kmax, num_classes, weights="distance", query_labels=None,
                              pred_all=None, self_base=None, scores=True, dist=None, idx=None, stream=None,
                              d=None):
        """sweep_device with the weighted vote (knn_sweep_weighted_device).  weights: a key of
        WEIGHTS (or its number).  Returns (pred_all int32 [kmax][nq], correct int64 [kmax] or None
        without query_labels, scores float32 [nq][C] = each class's summed weight over the kmax
        neighbours, or None with scores=False); ``proba(scores)`` normalises them."""
        import torch
        tr, te = self._datasets_arg(train, labels, test, d)
        pred_all = self._pred_all_arg(pred_all, kmax, te.n, torch.int32, test.device)
        _outputs(te.n, kmax, None, dist, idx)
        scores = self._scores_arg(scores, te.n, num_classes, test.device)
        correct, = self._accum(query_labels, "query_labels", torch.int32, te.n, kmax, torch.int64)
        self._check(self.lib.knn_sweep_weighted_device(
            self.h, ctypes.byref(tr), ctypes.byref(te), kmax, num_classes, _weight_kind(weights),
            _self_base(self_base), _opt_ptr(query_labels), pred_all.data_ptr(), _opt_ptr(correct), _opt_ptr(scores),
            _opt_ptr(dist), _opt_ptr(idx), self._stream(stream, test)))
        return pred_all, correct, scores

    def loo_weighted_device(self, train, labels, kmax, num_classes, weights="distance", pred_all=None, scores=True,
                            dist=None, idx=None, stream=None, d=None):
        """Leave-one-out on the train set with the weighted vote (loo_device's sibling)."""
        return self.sweep_weighted_device(train, labels, train, kmax, num_classes, weights, query_labels=labels,
                                          pred_all=pred_all, self_base=0, scores=scores, dist=dist, idx=idx,
                                          stream=stream, d=d)

    def predict_weighted_device(self, train, labels, test, k, num_classes, weights="distance", pred=None,
                                scores=True, dist=None, idx=None, stream=None, d=None):
        """The weighted vote for one k (knn_predict_weighted_device): returns (pred int32 [nq],
        scores float32 [nq][C] or None).  dist / idx (optional) receive the [nq][k] lists."""
        import torch
        tr, te = self._datasets_arg(train, labels, test, d)
        if pred is None:
            pred = torch.empty(te.n, dtype=torch.int32, device=test.device)
        _outputs(te.n, k, pred, dist, idx)
        scores = self._scores_arg(scores, te.n, num_classes, test.device)
        self._check(self.lib.knn_predict_weighted_device(
            self.h, ctypes.byref(tr), ctypes.byref(te), k, num_classes, _weight_kind(weights), pred.data_ptr(),
            _opt_ptr(scores), _opt_ptr(dist), _opt_ptr(idx), self._stream(stream, test)))
        return pred, scores

    def vote_weighted_device(self, idx, dist, train_labels, num_classes, weights="distance", query_labels=None,
                             pred_all=None, self_base=None, kin=None, scores=True, stream=None):
        """The weighted prefix votes alone (knn_vote_weighted_device) on neighbour lists idx int32
        / dist float32 [nq][stride] (same shape and strides) of which the first kin entries per
        row are read (default: all).  Returns (pred_all [kmax][nq], correct or None, scores or
        None); kmax = kin, or kin - 1 with self_base."""
        import torch
        nq, stride, kin, kmax = self._lists_arg(idx, dist, kin, self_base)
        _check_tensor(train_labels, "train_labels", torch.int32)
        pred_all = self._pred_all_arg(pred_all, kmax, nq, torch.int32, idx.device)
        scores = self._scores_arg(scores, nq, num_classes, idx.device)
        correct, = self._accum(query_labels, "query_labels", torch.int32, nq, kmax, torch.int64)
        self._check(self.lib.knn_vote_weighted_device(
            self.h, nq, kin, num_classes, idx.data_ptr(), _opt_ptr(dist), stride, train_labels.data_ptr(),
            _weight_kind(weights), _self_base(self_base), _opt_ptr(query_labels), pred_all.data_ptr(),
            _opt_ptr(correct), _opt_ptr(scores), self._stream(stream, idx)))
        return pred_all, correct, scores

    def sweep_weighted(self, train_feat, train_labels, test_feat, kmax, num_classes=None, weights="distance",
                       query_labels=None, self_base=None, scores=True):
        """Host arrays in, host arrays out (knn_sweep_weighted; not pipelined): (pred_all int32
        [kmax][nq], correct int64 [kmax] or None without query_labels, scores float32 [nq][C] or
        None with scores=False)."""
        tr, te, num_classes, pred_all, ql, correct, keep = self._host_class_args(
            train_feat, train_labels, test_feat, kmax, num_classes, query_labels)
        sc = np.zeros((te.n, max(num_classes, 0)), np.float32) if scores else None
        self._check(self.lib.knn_sweep_weighted(self.h, ctypes.byref(tr), ctypes.byref(te), kmax, num_classes,
                                                _weight_kind(weights), _self_base(self_base),
                                                _ptr(ql), _ptr(pred_all), _ptr(correct), _ptr(sc)))
        return pred_all, correct, sc

    def regress_sweep_device(self, train, targets, test, kmax, weights="uniform", query_targets=None,
                             pred_all=None, self_base=None, dist=None, idx=None, stream=None, d=None):
        """k-NN regression for every k in 1..kmax from one top-kmax pass (knn_regress_sweep_device).
        targets: float32 [n_train].  Returns (pred_all float32 [kmax][nq], sse, sae float64 [kmax]
        = the sums of squared / absolute errors against query_targets, or None, None without
        them); pred_all[k - 1] is regress_device's pred for k.  self_base, dist, idx as
        sweep_device."""
        import torch
        tr, te = self._datasets_arg(train, None, test, d)
        _check_tensor(targets, "targets", torch.float32, tr.n)
        pred_all = self._pred_all_arg(pred_all, kmax, te.n, torch.float32, test.device)
        _outputs(te.n, kmax, None, dist, idx)
        sse, sae = self._accum(query_targets, "query_targets", torch.float32, te.n, kmax, torch.float64, 2)
        self._check(self.lib.knn_regress_sweep_device(
            self.h, ctypes.byref(tr), ctypes.byref(te), targets.data_ptr(), kmax, _weight_kind(weights),
            _self_base(self_base), _opt_ptr(query_targets), pred_all.data_ptr(), _opt_ptr(sse), _opt_ptr(sae),
            _opt_ptr(dist), _opt_ptr(idx), self._stream(stream, test)))
        return pred_all, sse, sae

    def regress_loo_device(self, train, targets, kmax, weights="uniform", pred_all=None, dist=None, idx=None,
                           stream=None, d=None):
        """Leave-one-out regression on the train set: every row predicted from the others and
        scored against its own target (loo_device's sibling)."""
        return self.regress_sweep_device(train, targets, train, kmax, weights, query_targets=targets,
                                         pred_all=pred_all, self_base=0, dist=dist, idx=idx, stream=stream, d=d)

    def regress_device(self, train, targets, test, k, weights="uniform", pred=None, dist=None, idx=None,
                       stream=None, d=None):
        """The regression for one k (knn_regress_device): returns pred float32 [nq].  dist / idx
        (optional) receive the [nq][k] lists."""
        import torch
        tr, te = self._datasets_arg(train, None, test, d)
        _check_tensor(targets, "targets", torch.float32, tr.n)
        if pred is None:
            pred = torch.empty(te.n, dtype=torch.float32, device=test.device)
        _check_tensor(pred, "pred", torch.float32, te.n)
        _outputs(te.n, k, None, dist, idx)
        self._check(self.lib.knn_regress_device(
            self.h, ctypes.byref(tr), ctypes.byref(te), targets.data_ptr(), k, _weight_kind(weights),
            pred.data_ptr(), _opt_ptr(dist), _opt_ptr(idx), self._stream(stream, test)))
        return pred

    def regress_vote_device(self, idx, dist, train_targets, weights="uniform", query_targets=None, pred_all=None,
                            self_base=None, kin=None, stream=None):
        """The regression alone (knn_regress_vote_device) on neighbour lists idx int32 / dist
        float32 [nq][stride] (dist may be None with "uniform") of which the first kin entries per
        row are read (default: all).  train_targets is indexed by the lists' train rows.  Returns
        (pred_all [kmax][nq], sse, sae or None, None); kmax = kin, or kin - 1 with self_base."""
        import torch
        nq, stride, kin, kmax = self._lists_arg(idx, dist, kin, self_base)
        _check_tensor(train_targets, "train_targets", torch.float32)
        pred_all = self._pred_all_arg(pred_all, kmax, nq, torch.float32, idx.device)
        sse, sae = self._accum(query_targets, "query_targets", torch.float32, nq, kmax, torch.float64, 2)
        self._check(self.lib.knn_regress_vote_device(
            self.h, nq, kin, idx.data_ptr(), _opt_ptr(dist), stride, train_targets.data_ptr(),
            _weight_kind(weights), _self_base(self_base), _opt_ptr(query_targets), pred_all.data_ptr(),
            _opt_ptr(sse), _opt_ptr(sae), self._stream(stream, idx)))
        return pred_all, sse, sae

    def regress_sweep(self, train_feat, train_targets, test_feat, kmax, weights="uniform", query_targets=None,
                      self_base=None):
        """Host arrays in, host arrays out (knn_regress_sweep; not pipelined): (pred_all float32
        [kmax][nq], sse, sae float64 [kmax] or None, None without query_targets)."""
        tr, keep1 = _dataset(train_feat)
        te, keep2 = _dataset(test_feat)
        tt = _host_targets(train_targets, "train_targets", tr.n)
        qt = None if query_targets is None else _host_targets(query_targets, "query_targets", te.n)
        pred_all = np.zeros((max(kmax, 0), te.n), np.float32)
        sse = None if qt is None else np.zeros(max(kmax, 0), np.float64)
        sae = None if qt is None else np.zeros(max(kmax, 0), np.float64)
        if self.cache_train:
            self._train_key = keep1
        self._check(self.lib.knn_regress_sweep(self.h, ctypes.byref(tr), ctypes.byref(te), _ptr(tt), kmax,
                                               _weight_kind(weights), _self_base(self_base),
                                               _ptr(qt), _ptr(pred_all), _ptr(sse), _ptr(sae)))
        return pred_all, sse, sae

    # local outlier factor (knn_amd.h "Local outlier factor")
    @staticmethod
    def _lof_out(out, name, shape, dtype, device):
        """An optional LOF output: True = allocate, a tensor = use it, False / None = none."""
        import torch
        if out is None or out is False:
            return None
        if out is True:
            return torch.empty(shape, dtype=dtype, device=device)
        return _check_tensor(out, name, dtype, shape[0] * shape[1])

    def lof_fit_device(self, train, k_lo, k_hi=None, lof=False, dist=None, idx=None, stream=None, d=None, kd=None,
                       lrd=None):
        """Fit the local outlier factor on the train rows for every k in [k_lo, k_hi] (k_hi=None: the
        single k = k_lo) from one leave-one-out top-(k_hi + 1) pass (knn_lof_fit_device).  Returns a
        LofModel holding kd float32 [n][Kr], lrd float64 [n][Kr], the range and the train tensor;
        with lof=True (or a float32 [Kr][n] tensor) also model.lof, the train rows' own scores.
        dist / idx (optional, [n][k_hi + 1]) receive the lists before self-removal, which
        lof_lists_device takes with self_base=0.  A KnnError(KNN_ERANGE) (k_hi > n - 1) is raised
        after the outputs are written: pass tensors (kd, lrd, lof) to read them."""
        import torch
        k_hi = k_lo if k_hi is None else k_hi
        Kr = max(k_hi - k_lo + 1, 0)
        self._on_device(train)
        self._note_train(train)
        tr = _device_dataset(train, None, d)
        _outputs(tr.n, k_hi + 1, None, dist, idx)
        kd = self._lof_out(True if kd is None else kd, "kd", (tr.n, Kr), torch.float32, train.device)
        lrd = self._lof_out(True if lrd is None else lrd, "lrd", (tr.n, Kr), torch.float64, train.device)
        lof = self._lof_out(lof, "lof", (Kr, tr.n), torch.float32, train.device)
        model = LofModel(self, train, d, k_lo, k_hi, kd, lrd, lof)
        self._check(self.lib.knn_lof_fit_device(
            self.h, ctypes.byref(tr), k_lo, k_hi, kd.data_ptr(), lrd.data_ptr(), _opt_ptr(lof), _opt_ptr(dist),
            _opt_ptr(idx), self._stream(stream, train)))
        return model

    def lof_device(self, train, k_lo, k_hi=None, lof=None, dist=None, idx=None, stream=None, d=None):
        """The local outlier factor of every train row for every k in [k_lo, k_hi] (k_hi=None: the
        single k = k_lo): lof float32 [Kr][n], row k - k_lo for k (knn_lof_fit_device with the scores
        alone).  ``lof_max`` takes the per-row maximum over the range, ``lof_outliers`` the rows
        above a threshold.  lof, dist, idx as lof_fit_device."""
        import torch
        k_hi = k_lo if k_hi is None else k_hi
        self._on_device(train)
        self._note_train(train)
        tr = _device_dataset(train, None, d)
        _outputs(tr.n, k_hi + 1, None, dist, idx)
        lof = self._lof_out(True if lof is None else lof, "lof", (max(k_hi - k_lo + 1, 0), tr.n), torch.float32,
                            train.device)
        self._check(self.lib.knn_lof_fit_device(
            self.h, ctypes.byref(tr), k_lo, k_hi, None, None, lof.data_ptr(), _opt_ptr(dist), _opt_ptr(idx),
            self._stream(stream, train)))
        return lof

    def lof_lists_device(self, idx, dist, k_lo, k_hi=None, self_base=None, kd=None, lrd=None, lof=True, stream=None):
        """The LOF kernels alone (knn_lof_lists_device) on lists idx int32 / dist float32 [n][stride]
        the caller holds, list i belonging to row i of the n rows the indices name: the first
        k_hi + 1 entries of a row with self_base=0 (row i is removed from its list), the first k_hi
        with self_base=None (already removed: loo_device's lists).  kd float32 [n][Kr] / lrd float64
        [n][Kr] (True or a tensor) are filled when asked for.  Returns (lof float32 [Kr][n] or None,
        kd or None, lrd or None)."""
        import torch
        k_hi = k_lo if k_hi is None else k_hi
        Kr = max(k_hi - k_lo + 1, 0)
        n, stride, kin, _ = self._lists_arg(idx, dist, k_hi + (0 if self_base is None else 1), self_base)
        if dist is None:
            raise KnnError(KNN_EINVAL, "lof: dist is needed")
        kd = self._lof_out(kd, "kd", (n, Kr), torch.float32, idx.device)
        lrd = self._lof_out(lrd, "lrd", (n, Kr), torch.float64, idx.device)
        lof = self._lof_out(lof, "lof", (Kr, n), torch.float32, idx.device)
        self._check(self.lib.knn_lof_lists_device(
            self.h, n, kin, idx.data_ptr(), dist.data_ptr(), stride, _self_base(self_base), k_lo, k_hi, _opt_ptr(kd),
            _opt_ptr(lrd), _opt_ptr(lof), self._stream(stream, idx)))
        return lof, kd, lrd

    # radius neighbours (knn_amd.h "Radius neighbours")
    def _threshold(self, radius, threshold):
        """The binary32 threshold of a radius call: exactly one of radius= (float32(r) * float32(r)
        under the Euclidean metric, whose distances are squared; float32(r) otherwise) and
        threshold= (passed as it is, in the units of the reported distance)."""
        if (radius is None) == (threshold is None):
            raise KnnError(KNN_EINVAL, "give exactly one of radius= and threshold=")
        if threshold is not None:
            return float(np.float32(threshold))
        r = np.float32(radius)
        if r < 0:
            raise KnnError(KNN_EINVAL, f"radius must be >= 0, got {radius}")
        with np.errstate(over="ignore"):
            return float(r * r if self.metric == "euclidean" else r)

    def radius_count_device(self, train, labels, test, radius=None, threshold=None, num_classes=None,
                            query_labels=None, self_base=None, outlier_label=-1, class_counts=False, offsets=False,
                            stream=None, d=None):
        """How many train rows lie within the radius of each query, and their uniform vote
        (knn_radius_count_device; one distance pass, no lists).  labels and num_classes may be None
        when no class output is wanted.  Returns (count int32 [nq], pred int32 [nq] or None without
        labels, correct int64 [1] or None without query_labels, class_counts int32 [nq][C] or None,
        offsets int64 [nq + 1] or None).  A query with no neighbour predicts outlier_label."""
        import torch
        thr = self._threshold(radius, threshold)
        tr, te = self._datasets_arg(train, labels, test, d)
        dev = test.device
        voting = labels is not None
        if (voting or class_counts) and (labels is None or num_classes is None):
            raise KnnError(KNN_EINVAL, "class outputs need labels and num_classes")
        with _torch_on(stream, test):
            count = torch.empty(te.n, dtype=torch.int32, device=dev)
            pred = torch.empty(te.n, dtype=torch.int32, device=dev) if voting else None
            correct = None
            if query_labels is not None:
                if not voting:
                    raise KnnError(KNN_EINVAL, "query_labels need labels and num_classes")
                _check_tensor(query_labels, "query_labels", torch.int32, te.n)
                correct = torch.zeros(1, dtype=torch.int64, device=dev)
            cc = torch.empty((te.n, num_classes), dtype=torch.int32, device=dev) if class_counts else None
            off = torch.empty(te.n + 1, dtype=torch.int64, device=dev) if offsets else None
            self._check(self.lib.knn_radius_count_device(
                self.h, ctypes.byref(tr), ctypes.byref(te), thr, num_classes or 0, _self_base(self_base), outlier_label,
                _opt_ptr(query_labels), count.data_ptr(), _opt_ptr(cc), _opt_ptr(pred), _opt_ptr(correct), _opt_ptr(off),
                self._stream(stream, test)))
            return count, pred, correct, cc, off

    def radius_fill_device(self, train, test, offsets, radius=None, threshold=None, self_base=None,
                           return_distance=True, stream=None, d=None):
        """The lists that go with a count call's offsets (knn_radius_fill_device): the same train,
        test, threshold, self_base and metric.  Reads offsets[-1] (one synchronisation) to size
        idx int32 [total] and dist float32 [total] (None with return_distance=False)."""
        import torch
        thr = self._threshold(radius, threshold)
        tr, te = self._datasets_arg(train, None, test, d)
        _check_tensor(offsets, "offsets", torch.int64, te.n + 1)
        with _torch_on(stream, test):
            total = int(offsets[te.n].item())
            # (at least one element: an empty tensor has no address to hand to the library)
            idx = torch.empty(max(total, 1), dtype=torch.int32, device=test.device)
            dist = torch.empty(max(total, 1), dtype=torch.float32, device=test.device) if return_distance else None
            self._check(self.lib.knn_radius_fill_device(
                self.h, ctypes.byref(tr), ctypes.byref(te), thr, _self_base(self_base), offsets.data_ptr(),
                idx.data_ptr(), _opt_ptr(dist), self._stream(stream, test)))
            return idx[:total], None if dist is None else dist[:total]

    def radius_neighbors_device(self, train, test, radius=None, threshold=None, self_base=None, return_distance=True,
                                stream=None, d=None):
        """sklearn's radius_neighbors as CSR lists: (offsets int64 [nq + 1], idx int32 [total], dist
        float32 [total] or None).  Query q's neighbours are idx[offsets[q]:offsets[q + 1]], in
        ascending train index -- NOT sorted by distance.  Runs the count pass, one .item() on
        offsets[-1], then the fill pass."""
        _, _, _, _, off = self.radius_count_device(train, None, test, radius, threshold, self_base=self_base,
                                                   offsets=True, stream=stream, d=d)
        idx, dist = self.radius_fill_device(train, test, off, radius, threshold, self_base, return_distance,
                                            stream, d)
        return off, idx, dist

    def radius_vote_device(self, offsets, idx, dist, train_labels, num_classes, weights="uniform", outlier_label=-1,
                           query_labels=None, scores=True, stream=None):
        """The weighted vote alone on CSR lists the caller holds (knn_radius_vote_device; dist may
        be None with "uniform").  Returns (pred int32 [nq], correct int64 [1] or None, scores
        float32 [nq][C] or None)."""
        import torch
        self._on_device(idx)
        nq = offsets.numel() - 1
        _check_tensor(offsets, "offsets", torch.int64, 1)
        _check_tensor(idx, "idx", torch.int32)
        if dist is not None:
            _check_tensor(dist, "dist", torch.float32, idx.numel())
        _check_tensor(train_labels, "train_labels", torch.int32)
        with _torch_on(stream, idx):
            pred = torch.empty(nq, dtype=torch.int32, device=idx.device)
            scores = self._scores_arg(scores, nq, num_classes, idx.device)
            correct = None
            if query_labels is not None:
                _check_tensor(query_labels, "query_labels", torch.int32, nq)
                correct = torch.zeros(1, dtype=torch.int64, device=idx.device)
            self._check(self.lib.knn_radius_vote_device(
                self.h, nq, train_labels.numel(), offsets.data_ptr(), idx.data_ptr(), _opt_ptr(dist),
                train_labels.data_ptr(), num_classes, _weight_kind(weights), outlier_label, _opt_ptr(query_labels),
                pred.data_ptr(), _opt_ptr(correct), _opt_ptr(scores), self._stream(stream, idx)))
            return pred, correct, scores

    def radius_regress_vote_device(self, offsets, idx, dist, train_targets, weights="uniform", stream=None):
        """The regression alone on CSR lists the caller holds (knn_radius_regress_device): pred
        float32 [nq], NaN for a query with no neighbour."""
        import torch
        self._on_device(idx)
        nq = offsets.numel() - 1
        _check_tensor(offsets, "offsets", torch.int64, 1)
        _check_tensor(idx, "idx", torch.int32)
        if dist is not None:
            _check_tensor(dist, "dist", torch.float32, idx.numel())
        _check_tensor(train_targets, "train_targets", torch.float32)
        pred = torch.empty(nq, dtype=torch.float32, device=idx.device)
        self._check(self.lib.knn_radius_regress_device(
            self.h, nq, train_targets.numel(), offsets.data_ptr(), idx.data_ptr(), _opt_ptr(dist),
            train_targets.data_ptr(), _weight_kind(weights), pred.data_ptr(), self._stream(stream, idx)))
        return pred

    def radius_predict_device(self, train, labels, test, radius=None, threshold=None, num_classes=None,
                              weights="uniform", outlier_label=-1, query_labels=None, self_base=None, scores=True,
                              stream=None, d=None):
        """RadiusNeighborsClassifier.predict: returns (pred int32 [nq], scores float32 [nq][C] or
        None with scores=False, count int32 [nq]); with query_labels a fourth element, correct int64
        [1].  "uniform" takes the count pass alone (no lists are built; the scores are the class
        counts as floats); the weighted kinds run count, fill and the vote on the lists."""
        import torch
        with _torch_on(stream, test):
            if _weight_kind(weights) == WEIGHTS["uniform"]:
                count, pred, correct, cc, _ = self.radius_count_device(
                    train, labels, test, radius, threshold, num_classes, query_labels, self_base, outlier_label,
                    class_counts=bool(scores), stream=stream, d=d)
                sc = cc.to(torch.float32) if cc is not None else None
            else:
                count, _, _, _, off = self.radius_count_device(train, None, test, radius, threshold,
                                                               self_base=self_base, offsets=True, stream=stream, d=d)
                idx, dist = self.radius_fill_device(train, test, off, radius, threshold, self_base, True, stream, d)
                pred, correct, sc = self.radius_vote_device(off, idx, dist, labels, num_classes, weights, outlier_label,
                                                            query_labels, scores, stream)
            return (pred, sc, count) if query_labels is None else (pred, sc, count, correct)

    def radius_loo_device(self, train, labels, radius=None, threshold=None, num_classes=None, weights="uniform",
                          outlier_label=-1, scores=True, stream=None, d=None):
        """Leave-one-out on the train set: every row predicted from the other rows within the
        radius and scored against its own label.  Returns (pred, scores or None, count, correct)."""
        return self.radius_predict_device(train, labels, train, radius, threshold, num_classes, weights,
                                          outlier_label, query_labels=labels, self_base=0, scores=scores,
                                          stream=stream, d=d)

    # DBSCAN (knn_amd.h "DBSCAN")
    def _dbscan_out(self, n, labels, count, dev):
        """labels int32 [n] (the caller's, or new), count int32 [n] or None, summary int64 [4]."""
        import torch
        if labels is None:
            labels = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
        else:
            _check_tensor(labels, "labels", torch.int32, n)
        if count is True:
            count = torch.empty(max(n, 1), dtype=torch.int32, device=dev)[:n]
        elif count is False or count is None:
            count = None
        else:
            _check_tensor(count, "count", torch.int32, n)
        return labels, count, torch.zeros(4, dtype=torch.int64, device=dev)

    def dbscan_device(self, train, radius=None, threshold=None, min_samples=5, labels=None, count=False, stream=None,
                      d=None):
        """sklearn.cluster.DBSCAN's labels of the train rows under the context's metric
        (knn_dbscan_device): three distance passes over the rows against themselves, no neighbour
        lists.  Exactly one of radius= and threshold= (as the radius calls); a row is a core row when
        at least min_samples rows, itself included, lie within the threshold.  Returns (labels int32
        [n]: clusters 0, 1, ... in ascending order of their smallest row, a border row the smallest
        cluster number among its core neighbours, -1 noise; count int32 [n] or None with count=False;
        summary int64 [4] = clusters, core rows, border rows, noise rows).  labels / count may be
        tensors to fill."""
        thr = self._threshold(radius, threshold)
        if int(min_samples) != min_samples:
            raise KnnError(KNN_EINVAL, f"min_samples must be an integer, got {min_samples!r}")
        self._on_device(train)
        self._note_train(train)
        tr = _device_dataset(train, None, d)
        with _torch_on(stream, train):
            labels, count, summary = self._dbscan_out(tr.n, labels, count, train.device)
            self._check(self.lib.knn_dbscan_device(
                self.h, ctypes.byref(tr), thr, int(min_samples), labels.data_ptr(), _opt_ptr(count), summary.data_ptr(),
                self._stream(stream, train)))
            return labels, count, summary

    def dbscan_lists_device(self, offsets, idx, min_samples=5, labels=None, count=False, stream=None):
        """The same clustering on CSR lists the caller holds (knn_dbscan_lists_device): offsets int64
        [n + 1] and idx int32 of a self-join whose lists hold the row itself
        (radius_neighbors_device(train, train, ...)), or lists concatenated from train shards.
        Returns (labels, count or None, summary) as dbscan_device."""
        import torch
        self._on_device(idx)
        _check_tensor(offsets, "offsets", torch.int64, 1)
        _check_tensor(idx, "idx", torch.int32)
        if int(min_samples) != min_samples:
            raise KnnError(KNN_EINVAL, f"min_samples must be an integer, got {min_samples!r}")
        n = offsets.numel() - 1
        with _torch_on(stream, idx):
            labels, count, summary = self._dbscan_out(n, labels, count, idx.device)
            # (at least one element: an empty tensor has no address to hand to the library)
            ip = idx if idx.numel() else torch.zeros(1, dtype=torch.int32, device=idx.device)
            self._check(self.lib.knn_dbscan_lists_device(
                self.h, n, offsets.data_ptr(), ip.data_ptr(), int(min_samples), labels.data_ptr(), _opt_ptr(count),
                summary.data_ptr(), self._stream(stream, idx)))
            return labels, count, summary

    def dbscan_sweep_device(self, train, radii=None, thresholds=None, min_samples=5, labels=None, count=False,
                            stream=None, d=None):
        """dbscan_device at every one of R <= 32 non-decreasing radii from three distance passes,
        whatever R is (knn_dbscan_sweep_device).  Exactly one of radii= and thresholds= (as the
        radius sweep).  Returns (labels int32 [R][n], count int32 [R][n] or None with count=False,
        summary int64 [R][4]); row r holds the very bits dbscan_device returns at radii[r] on this
        context.  labels may be an int32 tensor [R][ld] with ld >= n to fill: the columns past n
        are not touched, and count=True then has the same pitch."""
        import torch
        thr = self._thresholds(radii, thresholds)
        R = int(thr.size)
        if int(min_samples) != min_samples:
            raise KnnError(KNN_EINVAL, f"min_samples must be an integer, got {min_samples!r}")
        self._on_device(train)
        self._note_train(train)
        tr = _device_dataset(train, None, d)
        n, dev, rows = tr.n, train.device, max(R, 1)
        ld = n
        if labels is None:
            labels = torch.empty((rows, max(n, 1)), dtype=torch.int32, device=dev)[:, :n]
            ld = max(n, 1)
        else:
            if labels.dtype != torch.int32 or labels.dim() != 2 or labels.shape[0] < rows or labels.stride(1) != 1:
                raise KnnError(KNN_EINVAL, "labels must be an int32 tensor [R][ld] with unit column stride")
            self._on_device(labels)
            ld = labels.stride(0) if labels.shape[0] > 1 else max(labels.shape[1], 1)
            if labels.shape[1] < n:
                ld = labels.shape[1]  # (the library refuses ld_out < n)
        with _torch_on(stream, train):
            cnt = torch.empty((rows, max(ld, 1)), dtype=torch.int32, device=dev) if count else None
            summary = torch.zeros((rows, 4), dtype=torch.int64, device=dev)
            self._check(self.lib.knn_dbscan_sweep_device(
                self.h, ctypes.byref(tr), thr.ctypes.data_as(ctypes.c_void_p), R, int(min_samples), ld, labels.data_ptr(),
                _opt_ptr(cnt), summary.data_ptr(), self._stream(stream, train)))
            return labels, (None if cnt is None else cnt[:, :n]), summary

    # the mutual-reachability spanning tree (knn_amd.h "Spanning tree")
    def mst_device(self, train, min_samples=5, core=False, w=None, a=None, b=None, stream=None, d=None):
        """The minimum spanning tree of the mutual-reachability graph of the train rows under the
        context's metric (knn_mst_device): w = max(c(a), c(b), D(a, b)), c the min_samples-th smallest
        distance of a row (itself included), edges strictly ordered by (w, a, b).  Returns (w float32
        [E], a int32 [E], b int32 [E] with a < b, ascending by that order; core float32 [n] or None
        with core=False; summary int64 [4] = edges E, components n - E, rounds, rows sent through
        distance passes).  E = n - 1 when every pair of rows has a finite distance.  All in the units
        of the reported distance (squared under the Euclidean metric).  w / a / b may be tensors of at
        least n - 1 elements to fill: the entries past E are left as they were."""
        import torch
        if int(min_samples) != min_samples:
            raise KnnError(KNN_EINVAL, f"min_samples must be an integer, got {min_samples!r}")
        self._on_device(train)
        self._note_train(train)
        tr = _device_dataset(train, None, d)
        n, dev = tr.n, train.device
        m = max(n - 1, 1)
        with _torch_on(stream, train):
            w = torch.empty(m, dtype=torch.float32, device=dev) if w is None else _check_tensor(w, "w", torch.float32, m)
            a = torch.empty(m, dtype=torch.int32, device=dev) if a is None else _check_tensor(a, "a", torch.int32, m)
            b = torch.empty(m, dtype=torch.int32, device=dev) if b is None else _check_tensor(b, "b", torch.int32, m)
            c = torch.empty(max(n, 1), dtype=torch.float32, device=dev)[:n] if core else None
            summary = torch.zeros(4, dtype=torch.int64, device=dev)
            self._check(self.lib.knn_mst_device(
                self.h, ctypes.byref(tr), int(min_samples), w.data_ptr(), a.data_ptr(), b.data_ptr(), _opt_ptr(c),
                summary.data_ptr(), self._stream(stream, train)))
            E = int(summary[0].item())
            return w[:E], a[:E], b[:E], c, summary

    def mst_cut_device(self, w, a, b, core, radii=None, thresholds=None, labels=None, stream=None):
        """DBSCAN* at every one of R <= 32 non-decreasing radii from a tree mst_device returned, with no
        distance pass (knn_mst_cut_device).  Exactly one of radii= and thresholds= (as the radius
        sweep).  core is mst_device(..., core=True)'s; it gives n.  Returns (labels int32 [R][n]: a
        core row's cluster, numbered 0, 1, ... by ascending smallest row, -1 for every other row --
        border rows are not assigned; summary int64 [R][3] = clusters, core rows, other rows).
        labels may be an int32 tensor [R][ld] with ld >= n to fill."""
        import torch
        thr = self._thresholds(radii, thresholds)
        R = int(thr.size)
        self._on_device(core)
        _check_tensor(core, "core", torch.float32)
        n, dev, rows = core.numel(), core.device, max(R, 1)
        E = w.numel()
        _check_tensor(w, "w", torch.float32)
        _check_tensor(a, "a", torch.int32, E)
        _check_tensor(b, "b", torch.int32, E)
        ld = n
        if labels is None:
            labels = torch.empty((rows, max(n, 1)), dtype=torch.int32, device=dev)[:, :n]
            ld = max(n, 1)
        else:
            if labels.dtype != torch.int32 or labels.dim() != 2 or labels.shape[0] < rows or labels.stride(1) != 1:
                raise KnnError(KNN_EINVAL, "labels must be an int32 tensor [R][ld] with unit column stride")
            self._on_device(labels)
            ld = labels.stride(0) if labels.shape[0] > 1 else max(labels.shape[1], 1)
            if labels.shape[1] < n:
                ld = labels.shape[1]  # (the library refuses ld_out < n)
        with _torch_on(stream, core):
            summary = torch.zeros((rows, 3), dtype=torch.int64, device=dev)
            # (at least one element: an empty tensor has no address to hand to the library)
            one = lambda t: t if t.numel() else torch.zeros(1, dtype=t.dtype, device=dev)
            self._check(self.lib.knn_mst_cut_device(
                self.h, n, E, one(w).data_ptr(), one(a).data_ptr(), one(b).data_ptr(), one(core).data_ptr(),
                thr.ctypes.data_as(ctypes.c_void_p), R, ld, labels.data_ptr(), summary.data_ptr(),
                self._stream(stream, core)))
            return labels, summary

    # radius sweep (knn_amd.h "Radius sweep")
    def _thresholds(self, radii, thresholds):
        """The binary32 thresholds of a sweep: exactly one of radii= (each float32(r) * float32(r)
        under the Euclidean metric, float32(r) otherwise) and thresholds= (passed as they are).
        The library checks their number, range and order."""
        if (radii is None) == (thresholds is None):
            raise KnnError(KNN_EINVAL, "give exactly one of radii= and thresholds=")
        if thresholds is not None:
            return np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(-1))
        r = np.asarray(radii, dtype=np.float32).reshape(-1)
        if (r < 0).any():
            raise KnnError(KNN_EINVAL, f"radii must be >= 0, got {radii}")
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(r * r if self.metric == "euclidean" else r)

    def radius_sweep_device(self, train, labels, test, radii=None, thresholds=None, num_classes=None,
                            query_labels=None, self_base=None, outlier_label=-1, class_counts=False, query_block=None,
                            stream=None, d=None):
        """The counts and the uniform vote of every one of R <= 32 non-decreasing radii from one
        distance pass (knn_radius_sweep_count_device).  Returns (count int32 [R][nq], pred int32
        [R][nq] or None without labels, correct int64 [R] or None without query_labels, outliers
        int64 [R] = the queries with no neighbour[, class_counts int32 [R][nq][C] with
        class_counts=True]); row r is radius_count_device at radii[r].  The queries are walked in
        blocks of query_block, or of the most the library's workspace takes; every block writes
        its columns of the outputs and adds into correct / outliers."""
        import torch
        thr = self._thresholds(radii, thresholds)
        R = int(thr.size)
        tr, te = self._datasets_arg(train, labels, test, d)
        dev = test.device
        nq = te.n
        voting = labels is not None
        if (voting or class_counts) and (labels is None or num_classes is None):
            raise KnnError(KNN_EINVAL, "class outputs need labels and num_classes")
        if query_labels is not None:
            if not voting:
                raise KnnError(KNN_EINVAL, "query_labels need labels and num_classes")
            _check_tensor(query_labels, "query_labels", torch.int32, nq)
        C = num_classes if voting else 0
        rows = max(R, 1)
        with _torch_on(stream, test):
            count = torch.empty((rows, nq), dtype=torch.int32, device=dev)
            pred = torch.empty((rows, nq), dtype=torch.int32, device=dev) if voting else None
            correct = torch.zeros(rows, dtype=torch.int64, device=dev) if query_labels is not None else None
            outliers = torch.zeros(rows, dtype=torch.int64, device=dev)
            cc = torch.empty((rows, nq, num_classes), dtype=torch.int32, device=dev) if class_counts else None
            if query_block is None:
                query_block = int(self.lib.knn_radius_sweep_max_queries(self.h, R, C)) if 1 <= R <= 32 else max(nq, 1)
            if query_block < 1:
                raise KnnError(KNN_EINVAL, f"query_block must be >= 1, got {query_block}")
            st = self._stream(stream, test)
            thr_p = thr.ctypes.data_as(ctypes.c_void_p)
            q0 = 0
            while True:  # (nq = 0: one call, for the library's checks)
                n = min(query_block, nq - q0)
                # (an empty tensor has no address)
                tq = knn_dataset((te.feat or 0) + q0 * te.ld * (2 if te.dtype == KNN_BF16 else 4), None, n, te.d, te.ld,
                                 te.dtype)
                self._check(self.lib.knn_radius_sweep_count_device(
                    self.h, ctypes.byref(tr), ctypes.byref(tq), thr_p, R, C,
                    -1 if self_base is None else self_base + q0, outlier_label,
                    None if query_labels is None or nq == 0 else query_labels.data_ptr() + 4 * q0, nq,
                    count.data_ptr() + 4 * q0, None if cc is None else cc.data_ptr() + 4 * q0 * num_classes,
                    None if pred is None else pred.data_ptr() + 4 * q0, _opt_ptr(correct) if nq else None,
                    outliers.data_ptr(), st))
                q0 += n
                if q0 >= nq:
                    break
            out = (count, pred, correct, outliers)
            return out + (cc,) if class_counts else out

    def radius_sweep_loo_device(self, train, labels, radii=None, thresholds=None, num_classes=None,
                                outlier_label=-1, class_counts=False, query_block=None, stream=None, d=None):
        """Leave-one-out for every radius: every train row voted on by the other rows within each
        radius and scored against its own label (radius_sweep_device with self_base=0)."""
        return self.radius_sweep_device(train, labels, train, radii, thresholds, num_classes, query_labels=labels,
                                        self_base=0, outlier_label=outlier_label, class_counts=class_counts,
                                        query_block=query_block, stream=stream, d=d)

    def radius_vote_sweep_device(self, offsets, idx, dist, train_labels, num_classes, radii=None, thresholds=None,
                                 weights="uniform", outlier_label=-1, query_labels=None, scores=True, stream=None):
        """The weighted vote of every radius on CSR lists the caller holds, filled at any threshold
        >= the last one (knn_radius_vote_sweep_device): row r is radius_vote_device on the entries
        with dist <= thresholds[r].  Returns (pred int32 [R][nq], correct int64 [R] or None, scores
        float32 [R][nq][C] or None)."""
        import torch
        self._on_device(idx)
        thr = self._thresholds(radii, thresholds)
        R = int(thr.size)
        nq = offsets.numel() - 1
        _check_tensor(offsets, "offsets", torch.int64, 1)
        _check_tensor(idx, "idx", torch.int32)
        if dist is None:
            raise KnnError(KNN_EINVAL, "the vote sweep reads the distances under every kind of weights")
        _check_tensor(dist, "dist", torch.float32, idx.numel())
        _check_tensor(train_labels, "train_labels", torch.int32)
        rows = max(R, 1)
        with _torch_on(stream, idx):
            pred = torch.empty((rows, nq), dtype=torch.int32, device=idx.device)
            sc = torch.empty((rows, nq, num_classes), dtype=torch.float32, device=idx.device) if scores else None
            correct = None
            if query_labels is not None:
                _check_tensor(query_labels, "query_labels", torch.int32, nq)
                correct = torch.zeros(rows, dtype=torch.int64, device=idx.device)
            self._check(self.lib.knn_radius_vote_sweep_device(
                self.h, nq, train_labels.numel(), offsets.data_ptr(), idx.data_ptr(), dist.data_ptr(),
                train_labels.data_ptr(), num_classes, _weight_kind(weights), thr.ctypes.data_as(ctypes.c_void_p), R,
                outlier_label, _opt_ptr(query_labels), nq, pred.data_ptr(), _opt_ptr(correct), _opt_ptr(sc),
                self._stream(stream, idx)))
            return pred, correct, sc

    def radius_sweep_predict_device(self, train, labels, test, radii=None, thresholds=None, num_classes=None,
                                    weights="uniform", outlier_label=-1, query_labels=None, self_base=None,
                                    scores=True, stream=None, d=None):
        """radius_predict_device for every radius: returns (pred int32 [R][nq], scores float32
        [R][nq][C] or None, count int32 [R][nq]); with query_labels a fourth element, correct int64
        [R].  "uniform" takes the count sweep alone (no lists; the scores are the class counts as
        floats); the weighted kinds build the lists once, at the last threshold, and run the vote
        sweep on them."""
        import torch
        thr = self._thresholds(radii, thresholds)
        with _torch_on(stream, test):
            if _weight_kind(weights) == WEIGHTS["uniform"]:
                out = self.radius_sweep_device(train, labels, test, None, thr, num_classes, query_labels, self_base,
                                               outlier_label, class_counts=bool(scores), stream=stream, d=d)
                count, pred, correct = out[0], out[1], out[2]
                sc = out[4].to(torch.float32) if scores else None
            else:
                if not 1 <= thr.size <= 32:
                    raise KnnError(KNN_EINVAL, f"{thr.size} thresholds outside [1, 32]")
                top = float(thr[-1])
                off, idx, dist = self.radius_neighbors_device(train, test, threshold=top, self_base=self_base,
                                                              stream=stream, d=d)
                pred, correct, sc = self.radius_vote_sweep_device(off, idx, dist, labels, num_classes, None, thr, weights,
                                                                  outlier_label, query_labels, scores, stream)
                # count[r][q]: the entries of q's list within thr[r]
                nq = off.numel() - 1
                seg = torch.repeat_interleave(torch.arange(nq, device=idx.device), (off[1:] - off[:-1]))
                t = torch.from_numpy(thr).to(idx.device)
                count = torch.zeros((thr.size, nq), dtype=torch.int32, device=idx.device)
                if idx.numel():
                    inside = (dist[None, :] <= t[:, None]).to(torch.int32)
                    count.index_add_(1, seg, inside)
            return (pred, sc, count) if query_labels is None else (pred, sc, count, correct)

    def radius_regress_device(self, train, targets, test, radius=None, threshold=None, weights="uniform",
                              self_base=None, stream=None, d=None):
        """RadiusNeighborsRegressor.predict: the weighted mean of the targets of the train rows
        within the radius, NaN where there is none.  Returns (pred float32 [nq], count int32 [nq])."""
        import torch
        _check_tensor(targets, "targets", torch.float32, train.shape[0])
        count, _, _, _, off = self.radius_count_device(train, None, test, radius, threshold, self_base=self_base,
                                                       offsets=True, stream=stream, d=d)
        need_dist = _weight_kind(weights) != WEIGHTS["uniform"]
        idx, dist = self.radius_fill_device(train, test, off, radius, threshold, self_base, need_dist, stream, d)
        return self.radius_regress_vote_device(off, idx, dist, targets, weights, stream), count

    def generate(self, feat, labels, row0, d, kind, seed, stream_id, num_classes, dtype=None,
                 stream=None):
        """Fill a device tensor [n][ld] (and labels) with the synthetic rows of SURVEY.md 8d.
        kind 0 / 1: uniform fp32 grid / bf16-exact values; 2 / 3: the same clustered (the row's
        class centroid + noise: labels carry signal).  A bfloat16 tensor receives bf16 bits
        (kinds 1 and 3: bf16-exact values)."""
        dtype = _tensor_dtype(feat) if dtype is None else dtype
        self._check(self.lib.knn_generate(
            self.h, feat.data_ptr(), _opt_ptr(labels), row0,
            feat.shape[0], d, feat.shape[1], dtype, kind, seed, stream_id, num_classes,
            self._stream(stream, feat)))
        # written behind torch's back: every context caching a train tensor that shares bytes with
        # feat (feat itself, a slice or view of it, a tensor feat is a view of) bumps its
        # generation at its next call
        span = _byte_span(feat)
        for c in list(_caching_contexts):
            c._invalidate_overlap(span)

    def confusion_matrix_device(self, pred, labels, num_classes, cm=None, stream=None):
        """computeConfusionMatrix / computeAccuracy (main.cpp:87-112) on device tensors:
        returns (cm int32 [C][C] device tensor, accuracy as the reference's float)."""
        import torch
        _check_tensor(pred, "pred", torch.int32)
        _check_tensor(labels, "labels", torch.int32, pred.shape[0])
        with _torch_on(stream, pred):
            if cm is None:
                cm = torch.empty((num_classes, num_classes), dtype=torch.int32, device=pred.device)
            corr = torch.zeros(1, dtype=torch.int64, device=pred.device)
            self._check(self.lib.knn_confusion_matrix_device(
                self.h, pred.data_ptr(), labels.data_ptr(), pred.shape[0], num_classes, cm.data_ptr(),
                corr.data_ptr(), self._stream(stream, pred)))
            n = pred.shape[0]
            return cm, float(np.float32(int(corr.item())) / np.float32(n)) if n else float("nan")

    def mfma_probe_bf16(self, a, b, stream=None):
        """The bf16 filter's MFMA chain on device operands a, b: [32][K] torch.bfloat16
        (K % 16 == 0) -> float32 [32][32] = a @ b.T as v_mfma_f32_32x32x16_bf16 sums it."""
        import torch
        if a.shape != b.shape or a.dim() != 2 or a.shape[0] != 32 or a.dtype != torch.bfloat16:
            raise KnnError(KNN_EINVAL, "a, b must be [32][K] bfloat16")
        with _torch_on(stream, a):
            a, b = a.contiguous(), b.contiguous()
            out = torch.empty((32, 32), dtype=torch.float32, device=a.device)
            self._check(self.lib.knn_mfma_probe_bf16(self.h, a.data_ptr(), b.data_ptr(), a.shape[1], out.data_ptr(),
                                                     self._stream(stream, a)))
            return out

    def mfma_probe_i8(self, a, b, stream=None):
        """The int8 filter's MFMA chain on device operands a, b: [32][K] torch.int8 (K % 32 == 0)
        -> int32 [32][32] = a @ b.T as v_mfma_i32_32x32x32_i8 sums it."""
        import torch
        if a.shape != b.shape or a.dim() != 2 or a.shape[0] != 32 or a.dtype != torch.int8 or b.dtype != torch.int8:
            raise KnnError(KNN_EINVAL, "a, b must be [32][K] int8")
        with _torch_on(stream, a):
            a, b = a.contiguous(), b.contiguous()
            out = torch.empty((32, 32), dtype=torch.int32, device=a.device)
            self._check(self.lib.knn_mfma_probe_i8(self.h, a.data_ptr(), b.data_ptr(), a.shape[1], out.data_ptr(),
                                                   self._stream(stream, a)))
            return out

    def _set_i8_coarsen(self, mul):
        """Test hook: the int8 filter's quantisation step times mul (1 <= mul <= 8) from now on."""
        self._check(self.lib.knn_debug_set_i8_coarsen(self.h, float(mul)))

    def set_generation(self, generation):
        """Invalidate cached train uploads and train-side filter operands (knn_set_generation)."""
        self._check(self.lib.knn_set_generation(self.h, generation))
        self._generation = int(generation)

    def set_metric(self, metric):
        """The distance of every later call on this context (knn_set_metric): a key of METRICS or
        its number.  KnnError(KNN_EINVAL) for an unknown metric, and for a non-Euclidean one on a
        context whose algo is a GEMM form or "direct_scan"."""
        self._check(self.lib.knn_set_metric(self.h, _metric_kind(metric)))

    @property
    def metric(self):
        """The context's metric as a key of METRICS (knn_get_metric)."""
        m = self.lib.knn_get_metric(self.h)
        return next(name for name, v in METRICS.items() if v == m)

    def stage_times(self):
        names = (ctypes.c_char_p * 256)()
        ms = (ctypes.c_float * 256)()
        n = self.lib.knn_stage_times(self.h, names, ms, 256)
        out = {}
        for i in range(n):
            key = names[i].decode()
            out[key] = out.get(key, 0.0) + ms[i]
        return out

    def stats(self):
        v = (ctypes.c_int64 * 22)()
        self.lib.knn_last_stats(self.h, v, 22)
        return {"candidates": v[0], "fallback_queries": v[1], "train_segments": v[2],
                "filter_operands": FILTER_OPERANDS.get(v[3], v[3]), "rerun_split": bool(v[4]),
                "fused_norm": bool(v[5]), "h2d_train_bytes": v[6], "h2d_query_bytes": v[7],
                "train_operands_cached": bool(v[8]), "filter_mfma": v[9],
                "queries_per_wave": v[10],
                "filter_element": FILTER_ELEMENTS.get(v[11], v[11]) if v[3] in (1, 2, 3) else None,
                "parked_passes": v[12], "radius_form": RADIUS_FORMS.get(v[13], v[13]),
                "radius_exact_pairs": v[14], "filter_width": v[15], "filter_chunks": v[16],
                "seeded_queries": v[17], "dbscan_border_queries": v[18], "dbscan_unions": v[19],
                "mst_rounds": v[20], "mst_pass_rows": v[21]}

    def last_seed(self, nq):
        """Test hook (knn_debug_last_seed): the thresholds the int8 filter's seed pass published in the
        last pass of the last call, one float32 per query (+inf: none).  profile = 2 contexts only;
        an empty array when that pass ran no seed."""
        out = np.full(nq, np.inf, dtype=np.float32)
        fn = self.lib.knn_debug_last_seed  # (a test hook: not in load_library's table)
        fn.restype, fn.argtypes = ctypes.c_longlong, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong]
        n = fn(self.h, out.ctypes.data, nq)
        if n < 0:
            raise KnnError(KNN_EINVAL, "knn_debug_last_seed")
        return out[:n]


def comm_unique_id():
    """knn_comm_unique_id: 128 bytes to hand to every rank (the caller's bootstrap)."""
    lib = load_library()
    buf = ctypes.create_string_buffer(KNN_COMM_ID_BYTES)
    st = lib.knn_comm_unique_id(buf)
    if st != KNN_OK:
        raise KnnError(st, "knn_comm_unique_id")
    return buf.raw


def build_id():
    """(id baked into the loaded libknn_amd.so, id of the sources beside it): equal when the
    library was built from this tree (build_id.py)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("knn_amd_build_id", os.path.join(_HERE, "build_id.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return load_library().knn_build_id().decode(), mod.compute()


def shard_range_c(n, world, rank):
    """knn_shard_range (the C ABI's copy of shard_range, used by knn_predict_train_sharded)."""
    lib = load_library()
    a, b = ctypes.c_int64(), ctypes.c_int64()
    st = lib.knn_shard_range(n, world, rank, ctypes.byref(a), ctypes.byref(b))
    if st != KNN_OK:
        raise KnnError(st, "knn_shard_range")
    return a.value, b.value


def shard_policy(n_train, n_query, d, dtype, world, hbm_bytes=0):
    """knn_shard_policy: "test" (queries split, train replicated) or "train" (train split,
    per-shard top-k exchanged and merged) for a world-GPU run.  dtype: "f32" or "bf16"."""
    lib = load_library()
    p = ctypes.c_int32()
    st = lib.knn_shard_policy(n_train, n_query, d, KNN_BF16 if dtype == "bf16" else KNN_F32, world, hbm_bytes,
                              ctypes.byref(p))
    if st != KNN_OK:
        raise KnnError(st, "knn_shard_policy")
    return "train" if p.value == 1 else "test"


def radius_policy(metric, dtype, d, n_train, n_query, algo="auto"):
    """knn_radius_policy: "direct" or "mfma", the form a radius pass of n_query queries against
    n_train rows takes on a context of that metric and algo.  dtype: "f32" or "bf16"."""
    lib = load_library()
    f = ctypes.c_int32()
    st = lib.knn_radius_policy(_metric_kind(metric), KNN_BF16 if dtype == "bf16" else KNN_F32, d, n_train, n_query,
                               ALGOS[algo] if isinstance(algo, str) else int(algo), ctypes.byref(f))
    if st != KNN_OK:
        raise KnnError(st, "knn_radius_policy")
    return RADIUS_FORMS[f.value]


FILTER_FORMS = {0: "direct", 1: "fused", 2: "filter", 3: "wide"}


def filter_policy(dtype, d, k, n_train, n_query, algo="auto"):
    """knn_filter_policy: (form, operand_width) of a top-k pass of n_query queries of d features
    against n_train rows at this k on a context of that algo (squared Euclidean, no train_splits).
    form: "direct", "fused" (k_gemm_fused), "filter" (k_gemm_filter) or "wide"; operand_width: the
    filter's operand row width in features, 0 for "direct".  dtype: "f32" or "bf16"."""
    lib = load_library()
    f, w = ctypes.c_int32(), ctypes.c_int32()
    st = lib.knn_filter_policy(KNN_BF16 if dtype == "bf16" else KNN_F32, d, k, n_train, n_query,
                               ALGOS[algo] if isinstance(algo, str) else int(algo), ctypes.byref(f), ctypes.byref(w))
    if st != KNN_OK:
        raise KnnError(st, "knn_filter_policy")
    return FILTER_FORMS[f.value], w.value


def exchange_layout(nq, k, world, rank):
    """knn_exchange_layout: (send_off, send_cnt, recv_off, recv_cnt) int32-element arrays of
    the train-sharded all-to-all of rank `rank`."""
    lib = load_library()
    arrs = [np.zeros(world, np.int64) for _ in range(4)]
    st = lib.knn_exchange_layout(nq, k, world, rank, *[_ptr(a) for a in arrs])
    if st != KNN_OK:
        raise KnnError(st, "knn_exchange_layout")
    return tuple(arrs)


class Comm:
    """An RCCL communicator bound to a context (knn_comm_create; collective over nranks)."""

    def __init__(self, ctx, uid, nranks, rank):
        self.lib = ctx.lib
        self.ctx = ctx
        self.nranks, self.rank = nranks, rank
        h = ctypes.c_void_p()
        st = self.lib.knn_comm_create(ctx.h, ctypes.create_string_buffer(bytes(uid), KNN_COMM_ID_BYTES), nranks,
                                      rank, ctypes.byref(h))
        if st != KNN_OK:
            raise KnnError(st, f"knn_comm_create(nranks={nranks}, rank={rank})")
        self.h = h

    def predict_train_sharded(self, shard, labels, idx_base, test, k, num_classes, pred, dist=None, idx=None,
                              stream=None, d=None):
        """knn_predict_train_sharded: this rank's train shard (global rows [idx_base, ...)) and
        every query in, the owned queries' (shard_range) predictions out."""
        self.ctx._on_device(shard)
        self.ctx._note_train(shard)
        tr = _device_dataset(shard, labels, d)
        te = _device_dataset(test, None, d)
        q0, q1 = shard_range(te.n, self.nranks, self.rank)
        _outputs(q1 - q0, k, pred, dist, idx)
        st = self.lib.knn_predict_train_sharded(
            self.ctx.h, self.h, ctypes.byref(tr), idx_base, ctypes.byref(te), k, num_classes, pred.data_ptr(),
            _opt_ptr(dist), _opt_ptr(idx),
            self.ctx._stream(stream, test))
        if st != KNN_OK:
            raise KnnError(st, self.lib.knn_last_error(self.ctx.h).decode())
        return q0, q1

    def count(self):
        """The number of ranks the RCCL communicator spans (knn_comm_count: ncclCommCount)."""
        n = ctypes.c_int32()
        st = self.lib.knn_comm_count(self.h, ctypes.byref(n))
        if st != KNN_OK:
            raise KnnError(st, "knn_comm_count")
        return n.value

    def set_exchange(self, chunk_elems=0, self_via_rccl=False):
        """knn_comm_set_exchange: RCCL messages of at most chunk_elems int32 (0: the default,
        256 MiB); self_via_rccl sends the rank's own block through the RCCL loop too (a one-rank
        communicator then runs the multi-rank exchange's offsets and counts)."""
        st = self.lib.knn_comm_set_exchange(self.h, int(chunk_elems), 1 if self_via_rccl else 0)
        if st != KNN_OK:
            raise KnnError(st, "knn_comm_set_exchange")

    def broken(self):
        """True once a collective failed and the communicator was aborted (knn_comm_broken)."""
        b = ctypes.c_int32()
        st = self.lib.knn_comm_broken(self.h, ctypes.byref(b))
        if st != KNN_OK:
            raise KnnError(st, "knn_comm_broken")
        return bool(b.value)

    def close(self):
        if getattr(self, "h", None):
            self.lib.knn_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PinnedArray:
    """A numpy array over page-locked host memory (knn_alloc_pinned / knn_free_pinned)."""

    def __init__(self, shape, dtype):
        self.lib = load_library()
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        p = ctypes.c_void_p()
        st = self.lib.knn_alloc_pinned(max(nbytes, 1), ctypes.byref(p))
        if st != KNN_OK:
            raise KnnError(st, f"knn_alloc_pinned({nbytes})")
        self.ptr = p
        buf = (ctypes.c_char * max(nbytes, 1)).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if getattr(self, "ptr", None):
            self.array = None
            self.lib.knn_free_pinned(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def read_arff(path):
    """Parse a NUMERIC ARFF file -> (features float32 [n][d], labels int32 [n], num_classes)."""
    lib = load_library()
    h = ctypes.c_void_p()
    err = ctypes.create_string_buffer(512)
    st = lib.knn_arff_open(os.fsencode(path), ctypes.byref(h), err, 512)
    if st != KNN_OK:
        raise KnnError(st, err.value.decode())
    try:
        n, na, C = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        lib.knn_arff_shape(h, ctypes.byref(n), ctypes.byref(na), ctypes.byref(C))
        d = na.value - 1
        feat = np.zeros((n.value, max(d, 0)), np.float32)
        labels = np.zeros(n.value, np.int32)
        st = lib.knn_arff_copy(h, _ptr(feat), max(d, 0), _ptr(labels))
        if st != KNN_OK:
            raise KnnError(st, "non-numeric or missing value in " + str(path))
        return feat, labels, C.value
    finally:
        lib.knn_arff_close(h)


def read_arff_targets(path):
    """(features float32 [n][d], targets float32 [n]): read_arff with the last attribute kept as
    a float, not truncated to a class (any finite value, negative or fractional)."""
    lib = load_library()
    h = ctypes.c_void_p()
    err = ctypes.create_string_buffer(512)
    st = lib.knn_arff_open(os.fsencode(path), ctypes.byref(h), err, len(err))
    if st != KNN_OK:
        raise KnnError(st, err.value.decode(errors="replace"))
    try:
        n, na, C = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        lib.knn_arff_shape(h, ctypes.byref(n), ctypes.byref(na), ctypes.byref(C))
        d = na.value - 1
        feat = np.zeros((n.value, d), np.float32)
        targets = np.zeros(n.value, np.float32)
        st = lib.knn_arff_copy_targets(h, _ptr(feat), d, _ptr(targets))
        if st != KNN_OK:
            raise KnnError(st, "non-numeric or missing value in " + str(path))
        return feat, targets
    finally:
        lib.knn_arff_close(h)


def KNN(train, test, k, ctx=None):
    """main.cpp:25 -- train = (features, labels), test = features or (features, labels).
    k <= 0 gives all-zero predictions like the reference."""
    tf, tl = train
    qf = test[0] if isinstance(test, tuple) else test
    if k <= 0:
        return np.zeros(len(qf), np.int32)
    return (ctx or default_context()).predict(tf, tl, qf, k, int(np.max(tl)) + 1)


def KNN_range(train, test, k, start, end, ctx=None):
    """mpi.cpp:26 -- predictions for test rows [start, end)."""
    tf, tl = train
    qf = test[0] if isinstance(test, tuple) else test
    if k <= 0:
        return np.zeros(end - start, np.int32)
    return (ctx or default_context()).predict(tf, tl, qf, k, int(np.max(tl)) + 1, start, end)


def best_k(correct):
    """The k a sweep's correct counts choose: the smallest k among those with the most correct
    (correct[k - 1] belongs to k; a numpy array, a list or a tensor)."""
    c = correct.cpu().numpy() if hasattr(correct, "cpu") else np.asarray(correct)
    if c.ndim != 1 or c.size == 0:
        raise KnnError(KNN_EINVAL, "correct must be a non-empty 1-D array")
    return int(np.argmax(c)) + 1  # argmax returns the first maximum


def best_radius(correct):
    """The index r a radius sweep's correct counts choose: the smallest index among those with the
    most correct (the radii are non-decreasing, so it is the smallest such radius)."""
    c = correct.cpu().numpy() if hasattr(correct, "cpu") else np.asarray(correct)
    if c.ndim != 1 or c.size == 0:
        raise KnnError(KNN_EINVAL, "correct must be a non-empty 1-D array")
    return int(np.argmax(c))  # argmax returns the first maximum


def best_k_error(err):
    """The smallest k with the least error in a regression's sse or sae [kmax] (numpy array or
    tensor); NaN entries (a prefix that reached a missing entry, a non-finite target) are ignored.
    KnnError when every entry is NaN."""
    e = np.asarray(err.cpu() if hasattr(err, "cpu") else err, dtype=np.float64)
    ok = ~np.isnan(e)
    if not ok.any():
        raise KnnError(KNN_EINVAL, "best_k_error: every entry is NaN")
    at = np.flatnonzero(ok)
    return int(at[np.argmin(e[at])]) + 1  # argmin returns the first minimum


class LofModel:
    """A fitted local outlier factor (Context.lof_fit_device): the train tensor (and the d it was
    read with), the range [k_lo, k_hi], kd float32 [n][Kr] and lrd float64 [n][Kr] of the train
    rows, and lof float32 [Kr][n], their own scores, when the fit was asked for them."""

    def __init__(self, ctx, train, d, k_lo, k_hi, kd, lrd, lof=None):
        self.ctx, self.train, self.d = ctx, train, d
        self.k_lo, self.k_hi = k_lo, k_hi
        self.kd, self.lrd, self.lof = kd, lrd, lof

    def score_device(self, test, lof=None, stream=None):
        """Novelty scores of queries that are not train rows (knn_lof_score_device): lof float32
        [Kr][nq] from each query's plain top-k_hi list against the train rows and the fitted
        tables.  A query equal to a train row keeps that row, at distance 0."""
        import torch
        c = self.ctx
        tr, te = c._datasets_arg(self.train, None, test, self.d)
        Kr = max(self.k_hi - self.k_lo + 1, 0)
        lof = c._lof_out(True if lof is None else lof, "lof", (Kr, te.n), torch.float32, test.device)
        c._check(c.lib.knn_lof_score_device(
            c.h, ctypes.byref(tr), ctypes.byref(te), self.k_lo, self.k_hi, self.kd.data_ptr(), self.lrd.data_ptr(),
            lof.data_ptr(), c._stream(stream, test)))
        return lof


def lof_max(lof):
    """The per-row maximum of lof [Kr][n] over the range of k (the LOF paper's rule for choosing
    MinPts): [n], a tensor for a tensor, else a numpy array.  NaN entries (a k the row has too few
    neighbours for) are ignored; a row that is NaN for every k stays NaN."""
    if hasattr(lof, "cpu"):
        import torch
        nan = torch.isnan(lof)
        m = torch.where(nan, torch.full_like(lof, float("-inf")), lof).max(dim=0).values
        return torch.where(nan.all(dim=0), torch.full_like(m, float("nan")), m)
    a = np.asarray(lof, np.float32)
    return np.fmax.reduce(a, axis=0)


def lof_outliers(scores, threshold=1.5):
    """The row indices (ascending, int64) whose score [n] -- a row of lof, or lof_max -- is above
    threshold; NaN scores are never above it."""
    if hasattr(scores, "cpu"):
        import torch
        return torch.nonzero(scores > threshold).reshape(-1)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(np.asarray(scores) > threshold).astype(np.int64)


def dbscan_sizes(labels):
    """The cluster sizes of DBSCAN labels [n] (noise, -1, is not counted): int64 [clusters], entry c
    the rows of cluster c; a tensor for a tensor, else a numpy array."""
    if hasattr(labels, "cpu"):
        import torch
        lab = labels.reshape(-1).to(torch.int64)
        return torch.bincount(lab[lab >= 0])
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    return np.bincount(lab[lab >= 0]).astype(np.int64)


def mst_linkage(w, a, b, n):
    """scipy's linkage matrix Z float64 [n - 1][4] of a spanning tree (host arrays or tensors, in
    mst_device's order): the edges merged in order, heights w, scipy's cluster ids (a leaf is its
    row, merge j makes cluster n + j) and sizes, the smaller id first.  Defined only for a connected
    tree: ValueError unless there are n - 1 edges that join all n rows."""
    host = lambda x: x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    w, a, b = host(w).astype(np.float64), host(a).astype(np.int64), host(b).astype(np.int64)
    n = int(n)
    if n < 1 or not (w.shape == a.shape == b.shape == (n - 1,)):
        raise ValueError(f"a connected tree of {n} rows has {n - 1} edges, got {w.shape[0] if w.ndim else w.shape}")
    parent = np.arange(n, dtype=np.int64)
    cid = np.arange(n, dtype=np.int64)   # a root's scipy cluster id
    size = np.ones(n, dtype=np.int64)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    Z = np.empty((n - 1, 4), dtype=np.float64)
    for j in range(n - 1):
        if not (0 <= a[j] < n and 0 <= b[j] < n):
            raise ValueError(f"edge {j} names a row outside [0, {n})")
        ra, rb = find(a[j]), find(b[j])
        if ra == rb:
            raise ValueError(f"edge {j} closes a cycle: not a tree")
        Z[j] = (min(cid[ra], cid[rb]), max(cid[ra], cid[rb]), w[j], size[ra] + size[rb])
        parent[rb] = ra
        size[ra] += size[rb]
        cid[ra] = n + j
    return Z


def best_eps(summary):
    """The index of the row of a DBSCAN sweep's summary [R][4] (clusters, core, border, noise; a
    tensor or an array) to look at first: among the rows with the MOST CLUSTERS the one with the
    FEWEST NOISE ROWS, and the smallest index when several rows tie on both.  A host helper: a
    tensor is copied to the host."""
    s = summary.cpu().numpy() if hasattr(summary, "cpu") else np.asarray(summary)
    s = s.reshape(-1, 4).astype(np.int64)
    if s.shape[0] == 0:
        raise KnnError(KNN_EINVAL, "best_eps: the summary has no rows")
    top = s[:, 0] == s[:, 0].max()
    noise = np.where(top, s[:, 3], np.iinfo(np.int64).max)
    return int(np.argmin(noise))  # (argmin: the first of equal values)


def _host_targets(t, name, n):
    """A host target array: float32 and contiguous as it stands -- no silent cast."""
    if not isinstance(t, np.ndarray) or t.dtype != np.float32:
        raise KnnError(KNN_EINVAL, f"{name} must be a float32 numpy array, got {getattr(t, 'dtype', type(t))}")
    if not t.flags["C_CONTIGUOUS"]:
        raise KnnError(KNN_EINVAL, f"{name} must be contiguous")
    if t.size < n:
        raise KnnError(KNN_EINVAL, f"{name} holds {t.size} elements, needs {n}")
    return t


def _weight_kind(weights):
    """A key of WEIGHTS, or a knn_weight number (passed on: the library rejects unknown ones)."""
    if isinstance(weights, str):
        if weights not in WEIGHTS:
            raise KnnError(KNN_EINVAL, f"weights must be one of {sorted(WEIGHTS)}, got {weights!r}")
        return WEIGHTS[weights]
    return int(weights)


def _metric_kind(metric):
    """A key of METRICS, or a knn_metric number (passed on: the library rejects unknown ones)."""
    if isinstance(metric, str):
        if metric not in METRICS:
            raise KnnError(KNN_EINVAL, f"metric must be one of {sorted(METRICS)}, got {metric!r}")
        return METRICS[metric]
    return int(metric)


def proba(scores):
    """Class probabilities from a weighted vote's scores [nq][C] (numpy array or tensor):
    scores / scores.sum(1), as sklearn's predict_proba.  Rows that sum to 0 (too few neighbours)
    or hold inf give nan."""
    if hasattr(scores, "cpu"):
        return scores / scores.sum(dim=1, keepdim=True)
    s = np.asarray(scores, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return s / s.sum(axis=1, keepdims=True)


def computeConfusionMatrix(predictions, labels, num_classes):
    """main.cpp:87 -- [true][pred] counts, C x C int32."""
    lib = load_library()
    p = np.ascontiguousarray(predictions, np.int32)
    lab = np.ascontiguousarray(labels, np.int32)
    cm = np.zeros((num_classes, num_classes), np.int32)
    st = lib.knn_confusion_matrix(_ptr(p), _ptr(lab), len(p), num_classes, _ptr(cm))
    if st != KNN_OK:
        raise KnnError(st, "label or prediction outside [0, num_classes)")
    return cm


def computeAccuracy(cm, n):
    """main.cpp:102 -- trace / n as float32."""
    lib = load_library()
    cm = np.ascontiguousarray(cm, np.int32)
    return float(np.float32(lib.knn_accuracy(_ptr(cm), cm.shape[0], n)))
