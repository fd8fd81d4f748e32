#!/usr/bin/env python3
"""Times the k-sweep against what it replaces (DESIGN.md "k-sweep"), with HIP events, the
median of --reps warm calls each:

  sweep      one sweep_device(kmax) call: predictions and correct counts for every k <= kmax
  predict    one predict_device(k = kmax) call
  loop       the loop of kmax predict_device calls, k = 1..kmax (the way to the same curve
             without the sweep)

and, from a profile = 1 context, the stage times of one sweep call ("vote_sweep" beside the
distance pass's own stages).  Workloads: the `large` ARFF pair of tests/data, and bench.py's
config A shape (1,000,000 x 128 fp32 train rows, 100,000 queries).  One JSON line each.

  python scripts/time_sweep.py [--workload large|A|both] [--kmax 32] [--reps 5]
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


def load_pkg():
    spec = importlib.util.spec_from_file_location("knn_amd", os.path.join(PKG, "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["knn_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def median_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def workload(knn, name, dev):
    if name == "large":
        tf, tl, C = knn.read_arff(os.path.join(REPO, "tests", "data", "large-train.arff"))
        qf, ql, _ = knn.read_arff(os.path.join(REPO, "tests", "data", "large-test.arff"))
        d = tf.shape[1]
        pad = lambda x: np.pad(x, ((0, 0), (0, -x.shape[1] % 4)))  # 16-byte device rows
        return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (pad(tf), tl, pad(qf), ql)] + [C, d]
    nt, nq, d, C = 1_000_000, 100_000, 128, 10
    ctx = knn.Context(0)
    tr = torch.empty((nt, d), dtype=torch.float32, device=dev)
    tl = torch.empty(nt, dtype=torch.int32, device=dev)
    te = torch.empty((nq, d), dtype=torch.float32, device=dev)
    ql = torch.empty(nq, dtype=torch.int32, device=dev)
    ctx.generate(tr, tl, 0, d, 0, 1, 0, C)
    ctx.generate(te, ql, 0, d, 0, 1, 1, C)
    ctx.close()
    return [tr, tl, te, ql, C, d]


def run(knn, name, kmax, reps):
    dev = torch.device("cuda", 0)
    tr, tl, te, ql, C, d = workload(knn, name, dev)
    nq = te.shape[0]
    ctx = knn.Context(0)
    pred = torch.empty(nq, dtype=torch.int32, device=dev)
    pred_all = torch.empty((kmax, nq), dtype=torch.int32, device=dev)
    sweep = lambda: ctx.sweep_device(tr, tl, te, kmax, C, query_labels=ql, pred_all=pred_all, d=d)
    predict = lambda: ctx.predict_device(tr, tl, te, kmax, C, pred, d=d)

    def loop():
        for k in range(1, kmax + 1):
            ctx.predict_device(tr, tl, te, k, C, pred, d=d)

    res = {"workload": name, "n_train": tr.shape[0], "n_query": nq, "d": d, "kmax": kmax, "reps": reps,
           "sweep_ms": median_ms(sweep, reps), "predict_kmax_ms": median_ms(predict, reps),
           "loop_1_to_kmax_ms": median_ms(loop, reps, warm=1)}
    # the sweep's last row is the single call's answer
    _, corr = sweep()
    predict()
    assert torch.equal(pred_all[kmax - 1], pred)
    res["best_k"] = knn.best_k(corr)
    ctx.close()
    pctx = knn.Context(0, profile=1)
    for _ in range(3):
        pctx.sweep_device(tr, tl, te, kmax, C, query_labels=ql, pred_all=pred_all, d=d)
    res["sweep_stages_ms"] = {k: round(v, 4) for k, v in pctx.stage_times().items()}
    pctx.close()
    for k in ("sweep_ms", "predict_kmax_ms", "loop_1_to_kmax_ms"):
        res[k] = round(res[k], 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="both", choices=["large", "A", "both"])
    ap.add_argument("--kmax", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    knn = load_pkg()
    for w in (["large", "A"] if a.workload == "both" else [a.workload]):
        run(knn, w, a.kmax, a.reps)


if __name__ == "__main__":
    main()
