#!/usr/bin/env python3
"""Times the weighted vote against the uniform k-sweep it extends (DESIGN.md "Weighted vote"),
on one box in one run, with HIP events, the median of --reps warm calls each:

  sweep              one sweep_device(kmax) call (k_vote_sweep, unchanged)
  weighted[kind]     one sweep_weighted_device(kmax) call for each of uniform / distance /
                     sqdist, without and with the per-class scores

and, from a profile = 1 context, the stage times of one call of each: "vote_sweep" and
"vote_weighted" beside the distance pass's own stages.  Workload: bench.py's config A shape
(1,000,000 x 128 fp32 train rows, 100,000 queries), K = 32.  One JSON line.

  python scripts/time_weighted.py [--kmax 32] [--reps 5] [--n-train 1000000] [--n-query 100000]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kmax", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-train", type=int, default=1_000_000)
    ap.add_argument("--n-query", type=int, default=100_000)
    a = ap.parse_args()
    knn = load_pkg()
    dev = torch.device("cuda", 0)
    nt, nq, d, C, kmax = a.n_train, a.n_query, 128, 10, a.kmax
    ctx = knn.Context(0)
    tr = torch.empty((nt, d), dtype=torch.float32, device=dev)
    tl = torch.empty(nt, dtype=torch.int32, device=dev)
    te = torch.empty((nq, d), dtype=torch.float32, device=dev)
    ql = torch.empty(nq, dtype=torch.int32, device=dev)
    ctx.generate(tr, tl, 0, d, 0, 1, 0, C)
    ctx.generate(te, ql, 0, d, 0, 1, 1, C)
    pred_all = torch.empty((kmax, nq), dtype=torch.int32, device=dev)
    scores = torch.empty((nq, C), dtype=torch.float32, device=dev)
    res = {"n_train": nt, "n_query": nq, "d": d, "kmax": kmax, "reps": a.reps}
    res["sweep_ms"] = median_ms(lambda: ctx.sweep_device(tr, tl, te, kmax, C, query_labels=ql, pred_all=pred_all), a.reps)
    old, old_corr = ctx.sweep_device(tr, tl, te, kmax, C, query_labels=ql)
    for kind in knn.WEIGHTS:
        res[f"weighted_{kind}_ms"] = median_ms(
            lambda: ctx.sweep_weighted_device(tr, tl, te, kmax, C, kind, query_labels=ql, pred_all=pred_all,
                                              scores=False), a.reps)
        res[f"weighted_{kind}_scores_ms"] = median_ms(
            lambda: ctx.sweep_weighted_device(tr, tl, te, kmax, C, kind, query_labels=ql, pred_all=pred_all,
                                              scores=scores), a.reps)
        _, corr, _ = ctx.sweep_weighted_device(tr, tl, te, kmax, C, kind, query_labels=ql, pred_all=pred_all,
                                               scores=scores)
        res[f"best_k_{kind}"] = knn.best_k(corr)
        res[f"differs_from_uniform_{kind}"] = round(float((pred_all != old).float().mean().item()), 4)
        if kind == "uniform":   # the uniform kind is the existing vote
            assert torch.equal(pred_all, old) and torch.equal(corr, old_corr)
    ctx.close()
    pctx = knn.Context(0, profile=1)
    for _ in range(3):
        pctx.sweep_device(tr, tl, te, kmax, C, query_labels=ql, pred_all=pred_all)
    st = pctx.stage_times()
    res["sweep_stages_ms"] = {k: round(v, 4) for k, v in st.items()}
    pass_ms = sum(v for k, v in st.items() if k != "vote_sweep")
    res["vote_sweep_ms"] = round(st["vote_sweep"], 4)
    for kind in knn.WEIGHTS:
        for with_scores in (False, True):
            for _ in range(3):
                pctx.sweep_weighted_device(tr, tl, te, kmax, C, kind, query_labels=ql, pred_all=pred_all,
                                           scores=scores if with_scores else False)
            v = pctx.stage_times()["vote_weighted"]
            key = f"vote_weighted_{kind}{'_scores' if with_scores else ''}"
            res[f"{key}_ms"] = round(v, 4)
            res[f"{key}_over_vote_sweep"] = round(v / st["vote_sweep"], 2)
            res[f"{key}_over_pass"] = round(v / pass_ms, 4)
    pctx.close()
    for k, v in res.items():
        if k.endswith("_ms") and isinstance(v, float):
            res[k] = round(v, 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
