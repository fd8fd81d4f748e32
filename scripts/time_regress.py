#!/usr/bin/env python3
"""Times k-NN regression against the weighted vote it sits beside (DESIGN.md "Regression"), on
one box in one run, on the same tensors, with HIP events, the median of --reps warm calls each:

  weighted[kind]     one sweep_weighted_device(kmax) call (predictions + correct counts, no scores)
  regress[kind]      one regress_sweep_device(kmax) call (predictions + sse + sae), and the same
                     without the query targets (predictions only: no partials, no reduce)

and, from a profile = 1 context, the "vote_weighted" and "regress" stage times of one call of
each.  Two workloads: bench.py's config A shape (1,000,000 x 128 fp32 train rows, 100,000
queries) at K = 32, and K = 1024 on 16,384 x 16 train rows and 4,096 queries.  One JSON line each.

  python scripts/time_regress.py [--reps 5] [--skip-a]
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
KINDS = ("uniform", "distance")


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


def run(knn, name, nt, nq, d, kmax, reps):
    dev = torch.device("cuda", 0)
    C = 10
    ctx = knn.Context(0)
    tr = torch.empty((nt, d), dtype=torch.float32, device=dev)
    tl = torch.empty(nt, dtype=torch.int32, device=dev)
    te = torch.empty((nq, d), dtype=torch.float32, device=dev)
    ql = torch.empty(nq, dtype=torch.int32, device=dev)
    ctx.generate(tr, tl, 0, d, 0, 1, 0, C)
    ctx.generate(te, ql, 0, d, 0, 1, 1, C)
    g = torch.Generator(device=dev).manual_seed(1)
    y = torch.randn(nt, generator=g, device=dev) * 100
    qy = torch.randn(nq, generator=g, device=dev) * 100
    pred_i = torch.empty((kmax, nq), dtype=torch.int32, device=dev)
    pred_f = torch.empty((kmax, nq), dtype=torch.float32, device=dev)
    res = {"workload": name, "n_train": nt, "n_query": nq, "d": d, "kmax": kmax, "reps": reps}
    for kind in KINDS:
        res[f"weighted_{kind}_ms"] = median_ms(
            lambda: ctx.sweep_weighted_device(tr, tl, te, kmax, C, kind, query_labels=ql, pred_all=pred_i,
                                              scores=False), reps)
        res[f"regress_{kind}_ms"] = median_ms(
            lambda: ctx.regress_sweep_device(tr, y, te, kmax, kind, query_targets=qy, pred_all=pred_f), reps)
        res[f"regress_{kind}_pred_only_ms"] = median_ms(
            lambda: ctx.regress_sweep_device(tr, y, te, kmax, kind, pred_all=pred_f), reps)
        _, sse, sae = ctx.regress_sweep_device(tr, y, te, kmax, kind, query_targets=qy, pred_all=pred_f)
        res[f"best_k_sse_{kind}"] = knn.best_k_error(sse)
        res[f"best_k_sae_{kind}"] = knn.best_k_error(sae)
    ctx.close()
    pctx = knn.Context(0, profile=1)
    for kind in KINDS:
        for _ in range(3):
            pctx.sweep_weighted_device(tr, tl, te, kmax, C, kind, query_labels=ql, pred_all=pred_i, scores=False)
        st = pctx.stage_times()
        vw = st["vote_weighted"]
        res[f"pass_{kind}_ms"] = round(sum(v for k, v in st.items() if k != "vote_weighted"), 4)
        res[f"vote_weighted_{kind}_ms"] = round(vw, 4)
        for with_sums in (True, False):
            for _ in range(3):
                pctx.regress_sweep_device(tr, y, te, kmax, kind, query_targets=qy if with_sums else None,
                                          pred_all=pred_f)
            v = pctx.stage_times()["regress"]
            key = f"regress_stage_{kind}{'' if with_sums else '_pred_only'}"
            res[f"{key}_ms"] = round(v, 4)
            res[f"{key}_over_vote_weighted"] = round(v / vw, 2)
    pctx.close()
    for k, v in res.items():
        if k.endswith("_ms") and isinstance(v, float):
            res[k] = round(v, 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-a", action="store_true", help="only the small K = 1024 workload")
    a = ap.parse_args()
    knn = load_pkg()
    if not a.skip_a:
        run(knn, "A shape, K = 32", 1_000_000, 100_000, 128, 32, a.reps)
    run(knn, "K = 1024", 16_384, 4_096, 16, 1024, a.reps)


if __name__ == "__main__":
    main()
