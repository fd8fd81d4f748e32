#!/usr/bin/env python3
"""Times the Manhattan and Chebyshev direct form (k_metric_tile) against the Euclidean direct form
it was modelled on (DESIGN.md "Metrics"), on one box in one process, with HIP events, every shape
warmed up, the three metrics alternating call by call, the median of --reps calls each:

  (a) 262,144 x 64 fp32 train rows (generator kind 0), 16,384 queries, k = 10, algo = "direct":
      the Euclidean pass is k_direct_tile there, the same skeleton.  From profile = 1 contexts:
      the "direct_tile" / "metric_tile" stage (and "merge_vote") per metric, the ratio
      metric_tile / direct_tile, and s = (max - min) / median of the Euclidean repeats, the
      spread a ratio has to exceed to mean anything.
  (b) the `large` ARFF pair, k = 5, whole predict_device call on device buffers, algo = "auto":
      Euclidean runs the short-row kernel k_direct_rows there, which the metrics do not have.

One JSON line.

  python scripts/time_metric.py [--reps 7] [--n-train 262144] [--n-query 16384]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "knn-using-p_threads-and-mpi_amd")
DATA = os.path.join(REPO, "tests", "data")
METRICS = ("euclidean", "manhattan", "chebyshev")


def load_pkg():
    spec = importlib.util.spec_from_file_location("knn_amd", os.path.join(PKG, "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["knn_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(ctxs, call, reps, warm=2):
    """reps rounds of one call per metric, in turn: {metric: {"call_ms": [...], stage: [...]}}."""
    out = {m: {"call_ms": []} for m in METRICS}
    for r in range(warm + reps):
        for m in METRICS:
            ms = timed(lambda: call(ctxs[m]))
            if r < warm:
                continue
            out[m]["call_ms"].append(ms)
            for name, v in ctxs[m].stage_times().items():
                out[m].setdefault(name, []).append(v)
    return out


def summary(runs):
    return {m: {k: round(statistics.median(v), 4) for k, v in r.items()} for m, r in runs.items()}


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n-train", type=int, default=262_144)
    ap.add_argument("--n-query", type=int, default=16_384)
    a = ap.parse_args()
    knn = load_pkg()
    dev = torch.device("cuda", 0)
    res = {"reps": a.reps}

    # (a) the tile kernels side by side
    nt, nq, d, C, k = a.n_train, a.n_query, 64, 10, 10
    ctxs = {m: knn.Context(0, algo="direct", profile=1, metric=m) for m in METRICS}
    tr = torch.empty((nt, d), dtype=torch.float32, device=dev)
    tl = torch.empty(nt, dtype=torch.int32, device=dev)
    te = torch.empty((nq, d), dtype=torch.float32, device=dev)
    ctxs["euclidean"].generate(tr, tl, 0, d, 0, 1, 0, C)
    ctxs["euclidean"].generate(te, None, 0, d, 0, 1, 1, C)
    pred = torch.empty(nq, dtype=torch.int32, device=dev)
    runs = alternate(ctxs, lambda c: c.predict_device(tr, tl, te, k, C, pred), a.reps)
    stage = {"euclidean": "direct_tile", "manhattan": "metric_tile", "chebyshev": "metric_tile"}
    for m in METRICS:
        assert stage[m] in runs[m], (m, sorted(runs[m]))
    base = statistics.median(runs["euclidean"]["direct_tile"])
    res["a"] = {"n_train": nt, "n_query": nq, "d": d, "k": k, "median_ms": summary(runs),
                "segments": {m: ctxs[m].stats()["train_segments"] for m in METRICS},
                "s_euclidean_direct_tile": round(spread(runs["euclidean"]["direct_tile"]), 4),
                "spread_metric_tile": {m: round(spread(runs[m]["metric_tile"]), 4) for m in METRICS[1:]},
                "metric_tile_over_direct_tile": {
                    m: round(statistics.median(runs[m]["metric_tile"]) / base, 4) for m in METRICS[1:]}}
    for c in ctxs.values():
        c.close()

    # (b) the large ARFF pair, whole call (report only)
    tf, tlab, Ctr = knn.read_arff(os.path.join(DATA, "large-train.arff"))
    qf, _, _ = knn.read_arff(os.path.join(DATA, "large-test.arff"))
    dd = tf.shape[1]
    pad = lambda x: np.pad(x, ((0, 0), (0, -x.shape[1] % 4)))   # device rows are 16-byte aligned
    tr, te = torch.from_numpy(pad(tf)).to(dev), torch.from_numpy(pad(qf)).to(dev)
    tl = torch.from_numpy(tlab).to(dev)
    pred = torch.empty(len(qf), dtype=torch.int32, device=dev)
    ctxs = {m: knn.Context(0, metric=m) for m in METRICS}
    runs = alternate(ctxs, lambda c: c.predict_device(tr, tl, te, 5, Ctr, pred, d=dd), max(a.reps, 21), warm=5)
    base = statistics.median(runs["euclidean"]["call_ms"])
    res["b"] = {"n_train": len(tf), "n_query": len(qf), "d": dd, "k": 5, "median_ms": summary(runs),
                "s_euclidean_call": round(spread(runs["euclidean"]["call_ms"]), 4),
                "call_over_euclidean": {m: round(statistics.median(runs[m]["call_ms"]) / base, 3) for m in METRICS[1:]}}
    for c in ctxs.values():
        c.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
