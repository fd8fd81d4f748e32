#!/usr/bin/env python3
"""Times DBSCAN (DESIGN.md "DBSCAN") against what a user ran before it existed: the self-join
radius_neighbors_device(train, train), whose lists any clustering elsewhere would need first.  One
box, one process, every call warmed up, the calls alternating round by round, the median of --reps.

Rows: fp32, generator kind 0, --n-train x d.  The threshold is the median 10th-neighbour distance of
a 256-row sample ("sparse"); min_samples = 5.  A direct context (algo="direct") and an MFMA context
(algo="gemm_bf16"); on the latter d = 128 as well.

  yardstick  radius_neighbors_device(train, train) and its "radius_fill" stage, the parent's code, in
             the same process; s = (max - min) / median of the yardstick's repeats
  bar (a)    stage "dbscan_link" <= (1 + s) x stage "radius_fill" of the self-join at the same threshold
  bar (b)    the whole dbscan_device call <= (1 + s) x (the whole radius_neighbors_device call
             + b x its "radius_fill" stage), b = dbscan_border_queries / n
  report     the dense threshold (median 1,024th neighbour), the three metrics, clustered rows
             (generator kind 2), dbscan_unions, the four stages, the cluster structure found

One JSON line, also written to --out.

  python scripts/time_dbscan.py [--reps 7] [--n-train 262144] [--out profiles/dbscan.json] [--no-report]
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
STAGES = ("radius_count", "dbscan_link", "dbscan_border", "dbscan_labels")
MIN_SAMPLES = 5


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dbscan.json"))
    ap.add_argument("--no-report", action="store_true", help="the bars alone")
    a = ap.parse_args()
    knn = load_pkg()
    dev = torch.device("cuda", 0)
    n, C = a.n_train, 10
    gen = knn.Context(0, algo="direct")

    def rows(d, kind=0):
        tr = torch.empty((n, d), dtype=torch.float32, device=dev)
        tl = torch.empty(n, dtype=torch.int32, device=dev)
        gen.generate(tr, tl, 0, d, kind, 1, 0, C)
        return tr, tl

    def thresholds(ctx, tr, tl):
        ns, kd = min(256, n), min(1024, n)
        sp = torch.empty(ns, dtype=torch.int32, device=dev)
        sd = torch.empty((ns, kd), dtype=torch.float32, device=dev)
        si = torch.empty((ns, kd), dtype=torch.int32, device=dev)
        ctx.predict_device(tr, tl, tr[:ns], kd, C, sp, sd, si)
        return {"sparse": float(sd[:, min(9, kd - 1)].median().item()), "dense": float(sd[:, kd - 1].median().item())}

    def one(ctx, tr, thr):
        """One profiled DBSCAN call: stages, counters, structure."""
        ms = timed(lambda: ctx.dbscan_device(tr, threshold=thr, min_samples=MIN_SAMPLES))
        _, _, summary = ctx.dbscan_device(tr, threshold=thr, min_samples=MIN_SAMPLES)
        st, sg = ctx.stats(), ctx.stage_times()
        print(f"report call: {ms:.1f} ms", file=sys.stderr, flush=True)
        return {"call_ms": round(ms, 3), "stages_ms": {k: round(v, 4) for k, v in sg.items()},
                "summary": dict(zip(("clusters", "core", "border", "noise"), summary.cpu().tolist())),
                "border_queries": st["dbscan_border_queries"], "unions": st["dbscan_unions"],
                "segments": st["train_segments"], "form": st["radius_form"]}

    def bars(algo, d, tr, thr):
        prof, plain = knn.Context(0, algo=algo, profile=1), knn.Context(0, algo=algo)
        stage = {k: [] for k in STAGES + ("radius_fill",)}
        call = {"dbscan": [], "radius_neighbors": []}
        warm = 2
        for r in range(warm + a.reps):
            prof.dbscan_device(tr, threshold=thr, min_samples=MIN_SAMPLES)
            sg = prof.stage_times()
            nb = prof.stats()["dbscan_border_queries"]
            form = prof.stats()["radius_form"]
            prof.radius_neighbors_device(tr, tr, threshold=thr)
            fill = prof.stage_times()["radius_fill"]
            t_db = timed(lambda: plain.dbscan_device(tr, threshold=thr, min_samples=MIN_SAMPLES))
            t_rn = timed(lambda: plain.radius_neighbors_device(tr, tr, threshold=thr))
            if r >= warm:
                for k in STAGES:
                    stage[k].append(sg[k])
                stage["radius_fill"].append(fill)
                call["dbscan"].append(t_db)
                call["radius_neighbors"].append(t_rn)
        b = nb / n
        s_fill, s_call = spread(stage["radius_fill"]), spread(call["radius_neighbors"])
        link, fill = statistics.median(stage["dbscan_link"]), statistics.median(stage["radius_fill"])
        db, rn = statistics.median(call["dbscan"]), statistics.median(call["radius_neighbors"])
        out = {"algo": algo, "form": form, "d": d, "threshold": thr, "border_fraction": round(b, 5),
               "median_stage_ms": {k: med(v) for k, v in stage.items()}, "median_call_ms": {k: med(v) for k, v in call.items()},
               "bar_a": {"s": round(s_fill, 4), "dbscan_link_ms": round(link, 4), "radius_fill_ms": round(fill, 4),
                         "met": link <= (1 + s_fill) * fill},
               "bar_b": {"s": round(s_call, 4), "dbscan_call_ms": round(db, 4),
                         "yardstick_ms": round(rn + b * fill, 4), "met": db <= (1 + s_call) * (rn + b * fill)}}
        prof.close()
        plain.close()
        print(f"bars {algo} d={d}: done", file=sys.stderr, flush=True)
        return out

    res = {"reps": a.reps, "n_train": n, "min_samples": MIN_SAMPLES, "bars": [], "report": {}}
    for d, algos in ((64, ("direct", "gemm_bf16")), (128, ("gemm_bf16",))):
        tr, tl = rows(d)
        thr = thresholds(gen, tr, tl)
        for algo in algos:
            res["bars"].append(bars(algo, d, tr, thr["sparse"]))
        if d == 64 and not a.no_report:
            rep = res["report"]
            for algo in ("direct", "gemm_bf16"):
                c = knn.Context(0, algo=algo, profile=2)
                rep[f"{algo}_sparse"] = one(c, tr, thr["sparse"])
                rep[f"{algo}_dense"] = one(c, tr, thr["dense"])
                c.radius_neighbors_device(tr, tr, threshold=thr["dense"], return_distance=False)
                rep[f"{algo}_dense"]["radius_fill_ms"] = round(c.stage_times()["radius_fill"], 4)
                c.close()
            for metric in ("manhattan", "chebyshev"):
                c = knn.Context(0, algo="direct", profile=2, metric=metric)
                rep[metric] = one(c, tr, thresholds(c, tr, tl)["sparse"])
                c.close()
            ctr, ctl = rows(64, kind=2)
            cthr = thresholds(gen, ctr, ctl)["sparse"]
            for algo in ("direct", "gemm_bf16"):
                c = knn.Context(0, algo=algo, profile=2)
                rep[f"{algo}_clustered"] = one(c, ctr, cthr)
                c.close()
            del ctr, ctl
        del tr, tl
    gen.close()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
