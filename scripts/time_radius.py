#!/usr/bin/env python3
"""Times the radius-neighbour pass (k_radius_tile, DESIGN.md "Radius neighbours") against the
top-k tile kernel of the same metric, on one box in one process, with HIP events / profile = 1
stages, every call warmed up, the calls alternating round by round, the median of --reps each.

Shape: DESIGN.md "Metrics" (a) -- 262,144 x 64 fp32 train rows (generator kind 0), 16,384 queries.
Thresholds, per metric, from the top-k export of predict_device on a 256-query sample: the median
10th-neighbour distance ("sparse", about 10 neighbours per query) and the median 1,024th ("dense").

  yardstick       predict_device k = 10, algo = "direct": the "direct_tile" (Euclidean) or
                  "metric_tile" stage, and s = (max - min) / median of its repeats
  the one bar     sparse "radius_count" stage (count + pred + correct) <= (1 + s) x the yardstick
  report only     the count pass without class outputs, the dense count pass, the fill pass sparse
                  and dense, radius_vote / radius_regress on the dense lists ("distance" weights),
                  the whole weighted radius_predict_device call, and the `large` ARFF pair at
                  threshold 0 (each test row's exact copies: about 7 neighbours per query)

One JSON line.

  python scripts/time_radius.py [--reps 7] [--n-train 262144] [--n-query 16384]
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
YARDSTICK = {"euclidean": "direct_tile", "manhattan": "metric_tile", "chebyshev": "metric_tile"}


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


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def med(v):
    return round(statistics.median(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n-train", type=int, default=262_144)
    ap.add_argument("--n-query", type=int, default=16_384)
    a = ap.parse_args()
    knn = load_pkg()
    dev = torch.device("cuda", 0)
    nt, nq, d, C = a.n_train, a.n_query, 64, 10
    ctxs = {m: knn.Context(0, algo="direct", profile=1, metric=m) for m in METRICS}
    tr = torch.empty((nt, d), dtype=torch.float32, device=dev)
    tl = torch.empty(nt, dtype=torch.int32, device=dev)
    te = torch.empty((nq, d), dtype=torch.float32, device=dev)
    ql = torch.empty(nq, dtype=torch.int32, device=dev)
    ctxs["euclidean"].generate(tr, tl, 0, d, 0, 1, 0, C)
    ctxs["euclidean"].generate(te, ql, 0, d, 0, 1, 1, C)
    y = torch.randn(nt, dtype=torch.float32, device=dev)
    pred = torch.empty(nq, dtype=torch.int32, device=dev)

    # thresholds from the top-k export on a query sample
    thr = {}
    ns, kd = min(256, nq), min(1024, nt)
    for m in METRICS:
        sp = torch.empty(ns, dtype=torch.int32, device=dev)
        sd = torch.empty((ns, kd), dtype=torch.float32, device=dev)
        si = torch.empty((ns, kd), dtype=torch.int32, device=dev)
        ctxs[m].predict_device(tr, tl, te[:ns], kd, C, sp, sd, si)
        thr[m] = {"sparse": float(sd[:, min(9, kd - 1)].median().item()), "dense": float(sd[:, kd - 1].median().item())}

    lists = {}     # (metric, density) -> (offsets, idx, dist), built once (also the warm-up of the fill)
    mean_neighbours = {}
    for m in METRICS:
        for dens in ("sparse", "dense"):
            lists[m, dens] = ctxs[m].radius_neighbors_device(tr, te, threshold=thr[m][dens])
            mean_neighbours[f"{m}_{dens}"] = round(lists[m, dens][1].numel() / nq, 2)

    segments = {}
    for m in METRICS:
        ctxs[m].radius_count_device(tr, tl, te, threshold=thr[m]["sparse"], num_classes=C)
        segments[m] = ctxs[m].stats()["train_segments"]

    def stage(c, name):
        return c.stage_times()[name]

    calls = {
        "yardstick": lambda m, c: (c.predict_device(tr, tl, te, 10, C, pred), stage(c, YARDSTICK[m]))[1],
        "count_sparse": lambda m, c: (c.radius_count_device(tr, tl, te, threshold=thr[m]["sparse"], num_classes=C,
                                                            query_labels=ql), stage(c, "radius_count"))[1],
        "count_sparse_no_classes": lambda m, c: (c.radius_count_device(tr, None, te, threshold=thr[m]["sparse"]),
                                                 stage(c, "radius_count"))[1],
        "count_dense": lambda m, c: (c.radius_count_device(tr, tl, te, threshold=thr[m]["dense"], num_classes=C,
                                                           query_labels=ql), stage(c, "radius_count"))[1],
        "fill_sparse": lambda m, c: (c.radius_fill_device(tr, te, lists[m, "sparse"][0], threshold=thr[m]["sparse"]),
                                     stage(c, "radius_fill"))[1],
        "fill_dense": lambda m, c: (c.radius_fill_device(tr, te, lists[m, "dense"][0], threshold=thr[m]["dense"]),
                                    stage(c, "radius_fill"))[1],
        "vote_dense": lambda m, c: (c.radius_vote_device(*lists[m, "dense"], tl, C, "distance"),
                                    stage(c, "radius_vote"))[1],
        "regress_dense": lambda m, c: (c.radius_regress_vote_device(*lists[m, "dense"], y, "distance"),
                                       stage(c, "radius_regress"))[1],
        "predict_weighted_sparse_call": lambda m, c: timed(lambda: c.radius_predict_device(
            tr, tl, te, threshold=thr[m]["sparse"], num_classes=C, weights="distance")),
        "predict_weighted_dense_call": lambda m, c: timed(lambda: c.radius_predict_device(
            tr, tl, te, threshold=thr[m]["dense"], num_classes=C, weights="distance")),
    }
    runs = {m: {n: [] for n in calls} for m in METRICS}
    warm = 2
    for r in range(warm + a.reps):
        for name, fn in calls.items():
            for m in METRICS:
                ms = fn(m, ctxs[m])
                if r >= warm:
                    runs[m][name].append(ms)
    res = {"reps": a.reps, "n_train": nt, "n_query": nq, "d": d, "thresholds": thr, "mean_neighbours": mean_neighbours,
           "segments": segments,
           "median_ms": {m: {n: med(v) for n, v in runs[m].items()} for m in METRICS}, "bar": {}}
    for m in METRICS:
        s = spread(runs[m]["yardstick"])
        ratio = statistics.median(runs[m]["count_sparse"]) / statistics.median(runs[m]["yardstick"])
        res["bar"][m] = {"s": round(s, 4), "count_sparse_over_yardstick": round(ratio, 4),
                         "spread_count_sparse": round(spread(runs[m]["count_sparse"]), 4), "met": ratio <= 1 + s}
    for c in ctxs.values():
        c.close()

    # the large ARFF pair, whole calls (report only)
    tf, tlab, Ctr = knn.read_arff(os.path.join(DATA, "large-train.arff"))
    qf, _, _ = knn.read_arff(os.path.join(DATA, "large-test.arff"))
    dd = tf.shape[1]
    pad = lambda x: np.pad(x, ((0, 0), (0, -x.shape[1] % 4)))   # device rows are 16-byte aligned
    atr, ate = torch.from_numpy(pad(tf)).to(dev), torch.from_numpy(pad(qf)).to(dev)
    atl = torch.from_numpy(tlab).to(dev)
    apred = torch.empty(len(qf), dtype=torch.int32, device=dev)
    ctx = knn.Context(0)
    arff = {"topk5_call": [], "radius_uniform_call": [], "radius_weighted_call": []}
    for r in range(5 + max(a.reps, 21)):
        t = {"topk5_call": timed(lambda: ctx.predict_device(atr, atl, ate, 5, Ctr, apred, d=dd)),
             "radius_uniform_call": timed(lambda: ctx.radius_predict_device(atr, atl, ate, threshold=0.0, num_classes=Ctr,
                                                                            scores=False, d=dd)),
             "radius_weighted_call": timed(lambda: ctx.radius_predict_device(atr, atl, ate, threshold=0.0, num_classes=Ctr,
                                                                             weights="distance", d=dd))}
        if r >= 5:
            for n, v in t.items():
                arff[n].append(v)
    count = ctx.radius_count_device(atr, None, ate, threshold=0.0, d=dd)[0]
    arff_segments = ctx.stats()["train_segments"]
    res["large_arff"] = {"n_train": len(tf), "n_query": len(qf), "d": dd, "threshold": 0.0,
                         "mean_neighbours": round(float(count.float().mean().item()), 2),
                         "segments": arff_segments, "median_ms": {n: med(v) for n, v in arff.items()}}
    ctx.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
