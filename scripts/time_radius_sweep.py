#!/usr/bin/env python3
"""Times the radius sweep against the single-threshold calls it replaces (DESIGN.md "Radius sweep"),
on one box in one process, every call warmed up, the calls alternating round by round, the median of
--reps each.

Rows: fp32, generator kind 0, --n-train x --n-query.  Thresholds: R = --thresholds values equally
spaced in rank between the median 10th-neighbour distance ("sparse") and the median 1,024th
("dense") of a 256-query top-k export of predict_device.

Cases: the direct form at d = 64 (a context with algo="direct") under the Euclidean and the
Manhattan metric, the MFMA form (algo="gemm_bf16") at d = 64 and d = 128.

  yardstick     the R radius_count_device calls (count, pred, correct) of the PARENT commit's library
                in the same process (--parent-pkg: a directory with that commit's __init__.py and
                libknn_amd.so), whole calls summed round by round; s = (max - min) / median of the sums
  the bar       per case: the whole radius_sweep_device call (count, pred, correct, outliers) is
                faster than that sum by more than 3 s
  report only   the sweep against ONE single-threshold call at thr[R - 1] (the price of the R - 1
                extra thresholds); radius_exact_pairs of the sweep against the single call's
                (profile = 2); the vote sweep on lists held at thr[R - 1] against R radius_vote_device
                calls on pre-filtered sub-lists; the single-threshold "radius_count" stage of this
                library against the parent's (the same kernels: equal within the parent's spread)

One JSON line.  Without --parent-pkg the yardstick is this library's own single calls and the
result says so ("parent": false).

  python scripts/time_radius_sweep.py [--reps 7] [--thresholds 8] [--n-train 262144] [--n-query 16384]
                                      [--parent-pkg DIR] [--cases direct64,manhattan64,mfma64,mfma128]
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
CASES = {"direct64": ("direct", "euclidean", 64), "manhattan64": ("direct", "manhattan", 64),
         "mfma64": ("gemm_bf16", "euclidean", 64), "mfma128": ("gemm_bf16", "euclidean", 128)}


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


def alternate(calls, reps, warm=2):
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
    ap.add_argument("--n-train", type=int, default=262_144)
    ap.add_argument("--n-query", type=int, default=16_384)
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    knn = load_pkg(PKG, "knn_amd")
    old = load_pkg(a.parent_pkg, "knn_amd_parent") if a.parent_pkg else knn
    dev = torch.device("cuda", 0)
    C, R = 10, a.thresholds
    nt, nq = a.n_train, a.n_query
    res = {"reps": a.reps, "R": R, "n_train": nt, "n_query": nq, "parent": bool(a.parent_pkg),
           "build_id": knn.load_library().knn_build_id().decode(),
           "parent_build_id": old.load_library().knn_build_id().decode(), "cases": {}}

    for case in a.cases.split(","):
        algo, metric, d = CASES[case]
        new_c = knn.Context(0, algo=algo, metric=metric)             # whole calls: no events inside
        old_c = old.Context(0, algo=algo, metric=metric)
        new_p = knn.Context(0, algo=algo, metric=metric, profile=1)  # the stages
        old_p = old.Context(0, algo=algo, metric=metric, profile=1)
        new_x = knn.Context(0, algo=algo, metric=metric, profile=2)  # the exact evaluations
        tr = torch.empty((nt, d), dtype=torch.float32, device=dev)
        tl = torch.empty(nt, dtype=torch.int32, device=dev)
        te = torch.empty((nq, d), dtype=torch.float32, device=dev)
        ql = torch.empty(nq, dtype=torch.int32, device=dev)
        new_c.generate(tr, tl, 0, d, 0, 1, 0, C)
        new_c.generate(te, ql, 0, d, 0, 1, 1, C)
        # thresholds: equally spaced in rank between the 10th and the 1,024th neighbour
        ns, kd = min(256, nq), min(1024, nt)
        sp = torch.empty(ns, dtype=torch.int32, device=dev)
        sd = torch.empty((ns, kd), dtype=torch.float32, device=dev)
        si = torch.empty((ns, kd), dtype=torch.int32, device=dev)
        new_c.predict_device(tr, tl, te[:ns], kd, C, sp, sd, si)
        ranks = np.unique(np.round(np.linspace(min(9, kd - 1), kd - 1, R)).astype(np.int64))
        thr = np.sort(np.float32([sd[:, int(k)].median().item() for k in ranks]))
        top = float(thr[-1])

        def singles(c):
            return [c.radius_count_device(tr, tl, te, threshold=float(t), num_classes=C, query_labels=ql) for t in thr]

        # the same answers first
        sw = new_c.radius_sweep_device(tr, tl, te, thresholds=thr, num_classes=C, query_labels=ql)
        form = new_c.stats()["radius_form"]
        ref = singles(old_c)
        for r in range(len(thr)):
            assert torch.equal(sw[0][r], ref[r][0]) and torch.equal(sw[1][r], ref[r][1]), (case, r)
            assert int(sw[2][r]) == int(ref[r][2][0]), (case, r)
        assert old_c.stats()["radius_form"] == form
        off, idx, dist = new_c.radius_neighbors_device(tr, te, threshold=top)
        seg = torch.repeat_interleave(torch.arange(nq, device=dev), off[1:] - off[:-1])
        subs = []
        for t in thr:
            keep = dist <= float(t)
            so = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
            so[1:] = torch.cumsum(torch.bincount(seg[keep], minlength=nq), 0)
            # (at least one element: an empty tensor has no address to hand to the library)
            pad_i, pad_d = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)
            subs.append((so, torch.cat([idx[keep], pad_i]), torch.cat([dist[keep], pad_d])))
        vs = new_c.radius_vote_sweep_device(off, idx, dist, tl, C, thresholds=thr, weights="distance", query_labels=ql)
        for r, (so, si_, sd_) in enumerate(subs):
            vp, vc, vsc = new_c.radius_vote_device(so, si_, sd_, tl, C, "distance", -1, ql)
            assert torch.equal(vs[0][r], vp) and torch.equal(vs[2][r].view(torch.int32), vsc.view(torch.int32)), (case, r)

        calls = {
            "sweep_call": lambda: timed(lambda: new_c.radius_sweep_device(tr, tl, te, thresholds=thr, num_classes=C,
                                                                          query_labels=ql)),
            "parent_singles_sum": lambda: timed(lambda: singles(old_c)),
            "single_top_call": lambda: timed(lambda: new_c.radius_count_device(tr, tl, te, threshold=top, num_classes=C,
                                                                               query_labels=ql)),
            "parent_single_top_call": lambda: timed(lambda: old_c.radius_count_device(tr, tl, te, threshold=top,
                                                                                     num_classes=C, query_labels=ql)),
            "count_stage_top": lambda: (new_p.radius_count_device(tr, tl, te, threshold=top, num_classes=C,
                                                                  query_labels=ql),
                                        new_p.stage_times().get("radius_count", 0.0))[1],
            "parent_count_stage_top": lambda: (old_p.radius_count_device(tr, tl, te, threshold=top, num_classes=C,
                                                                         query_labels=ql),
                                               old_p.stage_times().get("radius_count", 0.0))[1],
            "sweep_stage": lambda: (new_p.radius_sweep_device(tr, tl, te, thresholds=thr, num_classes=C, query_labels=ql),
                                    new_p.stage_times().get("radius_sweep", 0.0))[1],
            "vote_sweep_call": lambda: timed(lambda: new_c.radius_vote_sweep_device(
                off, idx, dist, tl, C, thresholds=thr, weights="distance", query_labels=ql)),
            "filtered_votes_sum": lambda: timed(lambda: [new_c.radius_vote_device(so, si_, sd_, tl, C, "distance", -1, ql)
                                                         for so, si_, sd_ in subs]),
        }
        runs = alternate(calls, a.reps)
        s = spread(runs["parent_singles_sum"])
        m_sum, m_sw = statistics.median(runs["parent_singles_sum"]), statistics.median(runs["sweep_call"])
        new_x.radius_sweep_device(tr, tl, te, thresholds=thr, num_classes=C, query_labels=ql)
        ex_sweep = new_x.stats()["radius_exact_pairs"]
        new_x.radius_count_device(tr, tl, te, threshold=top, num_classes=C, query_labels=ql)
        ex_single = new_x.stats()["radius_exact_pairs"]
        res["cases"][case] = {
            "algo": algo, "metric": metric, "d": d, "form": form, "segments": new_c.stats()["train_segments"],
            "thresholds": [float(t) for t in thr],
            "mean_neighbours": [round(float(sw[0][r].sum().item()) / nq, 2) for r in range(len(thr))],
            "median_ms": {n: med(v) for n, v in runs.items()},
            "spread": {n: round(spread(v), 4) for n, v in runs.items()},
            "bar": {"s": round(s, 4), "parent_singles_sum_ms": round(m_sum, 4), "sweep_ms": round(m_sw, 4),
                    "speedup": round(m_sum / m_sw, 3), "met": m_sw < m_sum * (1 - 3 * s)},
            "sweep_over_single_top": round(m_sw / statistics.median(runs["single_top_call"]), 3),
            "exact_pairs": {"sweep": ex_sweep, "single_top": ex_single, "pairs": nt * nq},
            "count_stage_equal": abs(statistics.median(runs["count_stage_top"]) -
                                     statistics.median(runs["parent_count_stage_top"])) <=
            spread(runs["parent_count_stage_top"]) * statistics.median(runs["parent_count_stage_top"]),
        }
        for c in (new_c, old_c, new_p, old_p, new_x):
            c.close()
        del tr, tl, te, ql, off, idx, dist, subs, seg
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
