#!/usr/bin/env python3
"""Times the DBSCAN eps sweep (DESIGN.md "DBSCAN sweep") against what it replaces: one dbscan_device
call per radius.  One box, one process, every call warmed up, the calls alternating round by round,
the median of --reps, HIP events around whole calls.

Rows: fp32, generator kind 0, --n-train x d; min_samples = 5.  R thresholds equally spaced in rank
between the median 5th- and the median 64th-neighbour distance of a 256-row sample (the range a
k-distance plot points at).  Cases: the direct form at d = 64, the MFMA form (algo="gemm_bf16") at
d = 64 and d = 128.

  yardstick     the R dbscan_device calls of the PARENT commit's library in the same process
                (--parent-pkg: a directory with that commit's __init__.py and libknn_amd.so), whole
                calls summed round by round; s = (max - min) / median of the sums
  the bar       per case: the whole dbscan_sweep_device call is faster than that sum by more than 3 s
  report only   the sweep's stages, radius_exact_pairs of the sweep against the single calls' sum,
                dbscan_unions, the same table at --thresholds-wide (fewer repeats: --reps-wide), and the
                single-radius dbscan_device call of this library against the parent's (the same
                kernels: equal within the parent's spread)

One JSON line, also written to --out.  Without --parent-pkg the yardstick is this library's own
single calls and the result says so ("parent": false).

  python scripts/time_dbscan_sweep.py [--reps 7] [--thresholds 8] [--thresholds-wide 32] [--reps-wide 3]
                                      [--n-train 262144] [--parent-pkg DIR] [--cases direct64,mfma64,mfma128]
                                      [--out profiles/dbscan_sweep.json]
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
CASES = {"direct64": ("direct", 64), "mfma64": ("gemm_bf16", 64), "mfma128": ("gemm_bf16", 128)}
MIN_SAMPLES = 5


def load_pkg(pkg_dir, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg_dir, "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
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


def alternate(calls, reps, warm):
    """calls: name -> fn() returning ms, run one after the other round by round.  {name: [ms]}"""
    runs = {n: [] for n in calls}
    for r in range(warm + reps):
        for name, fn in calls.items():
            ms = fn()
            if r >= warm:
                runs[name].append(ms)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--thresholds", type=int, default=8)
    ap.add_argument("--thresholds-wide", type=int, default=32)
    ap.add_argument("--reps-wide", type=int, default=3)
    ap.add_argument("--n-train", type=int, default=262_144)
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dbscan_sweep.json"))
    a = ap.parse_args()
    knn = load_pkg(PKG, "knn_amd")
    old = load_pkg(a.parent_pkg, "knn_amd_parent") if a.parent_pkg else knn  # (each binds the library beside it)
    dev = torch.device("cuda", 0)
    n, C = a.n_train, 10
    res = {"reps": a.reps, "reps_wide": a.reps_wide, "n_train": n, "min_samples": MIN_SAMPLES, "parent": bool(a.parent_pkg),
           "build_id": knn.load_library().knn_build_id().decode(),
           "parent_build_id": old.load_library().knn_build_id().decode(), "cases": {}}

    for case in a.cases.split(","):
        algo, d = CASES[case]
        new_c, old_c = knn.Context(0, algo=algo), old.Context(0, algo=algo)  # whole calls: no events inside
        new_x, old_x = knn.Context(0, algo=algo, profile=2), old.Context(0, algo=algo, profile=2)
        tr = torch.empty((n, d), dtype=torch.float32, device=dev)
        tl = torch.empty(n, dtype=torch.int32, device=dev)
        new_c.generate(tr, tl, 0, d, 0, 1, 0, C)
        ns, kd = min(256, n), min(65, n)  # (the row itself is its own first neighbour)
        sp = torch.empty(ns, dtype=torch.int32, device=dev)
        sd = torch.empty((ns, kd), dtype=torch.float32, device=dev)
        si = torch.empty((ns, kd), dtype=torch.int32, device=dev)
        new_c.predict_device(tr, tl, tr[:ns], kd, C, sp, sd, si)
        out = {"algo": algo, "d": d, "tables": {}}

        for R, reps, warm in ((a.thresholds, a.reps, 2), (a.thresholds_wide, a.reps_wide, 1)):
            if R < 1 or reps < 1:
                continue
            ranks = np.round(np.linspace(min(5, kd - 1), kd - 1, R)).astype(np.int64)
            thr = np.sort(np.float32([sd[:, int(k)].median().item() for k in ranks]))

            def singles(c):
                return [c.dbscan_device(tr, threshold=float(t), min_samples=MIN_SAMPLES, count=True) for t in thr]

            # the same answers first
            labels, count, summary = new_c.dbscan_sweep_device(tr, thresholds=thr, min_samples=MIN_SAMPLES, count=True)
            form = new_c.stats()["radius_form"]
            for r, (l1, c1, s1) in enumerate(singles(old_c)):
                assert torch.equal(labels[r], l1) and torch.equal(count[r], c1) and torch.equal(summary[r], s1), (case, r)
            assert old_c.stats()["radius_form"] == form
            mid = float(thr[len(thr) // 2])
            calls = {
                "sweep_call": lambda: timed(lambda: new_c.dbscan_sweep_device(tr, thresholds=thr, min_samples=MIN_SAMPLES)),
                "parent_singles_sum": lambda: timed(lambda: [old_c.dbscan_device(tr, threshold=float(t),
                                                                                 min_samples=MIN_SAMPLES) for t in thr]),
                "single_call": lambda: timed(lambda: new_c.dbscan_device(tr, threshold=mid, min_samples=MIN_SAMPLES)),
                "parent_single_call": lambda: timed(lambda: old_c.dbscan_device(tr, threshold=mid, min_samples=MIN_SAMPLES)),
            }
            runs = alternate(calls, reps, warm)
            s = spread(runs["parent_singles_sum"])
            m_sum, m_sw = statistics.median(runs["parent_singles_sum"]), statistics.median(runs["sweep_call"])
            m_one, m_pone = statistics.median(runs["single_call"]), statistics.median(runs["parent_single_call"])
            # one profiled call each: stages, exact evaluations, hooks
            new_x.dbscan_sweep_device(tr, thresholds=thr, min_samples=MIN_SAMPLES)
            st, sg = new_x.stats(), new_x.stage_times()
            ex_single = un_single = 0
            for t in thr:
                old_x.dbscan_device(tr, threshold=float(t), min_samples=MIN_SAMPLES)
                ex_single += old_x.stats()["radius_exact_pairs"]
                un_single += old_x.stats()["dbscan_unions"]
            out["tables"][f"R{R}"] = {
                "form": form, "thresholds": [float(t) for t in thr], "reps": reps,
                "summary": summary.cpu().tolist(),
                "median_ms": {k: med(v) for k, v in runs.items()},
                "spread": {k: round(spread(v), 4) for k, v in runs.items()},
                "bar": {"s": round(s, 4), "parent_singles_sum_ms": round(m_sum, 4), "sweep_ms": round(m_sw, 4),
                        "speedup": round(m_sum / m_sw, 3), "met": m_sw < m_sum * (1 - 3 * s)},
                "stages_ms": {k: round(v, 4) for k, v in sg.items()},
                "exact_pairs": {"sweep": st["radius_exact_pairs"], "singles_sum": ex_single},
                "unions": {"sweep": st["dbscan_unions"], "singles_sum": un_single},
                "border_queries": st["dbscan_border_queries"], "segments": st["train_segments"],
                "single_call_equal": abs(m_one - m_pone) <= spread(runs["parent_single_call"]) * m_pone,
            }
            print(f"{case} R={R}: sweep {m_sw:.2f} ms, singles {m_sum:.2f} ms", file=sys.stderr, flush=True)
        res["cases"][case] = out
        for c in (new_c, old_c, new_x, old_x):
            c.close()
        del tr, tl

    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
