#!/usr/bin/env python3
"""Times the mutual-reachability spanning tree (DESIGN.md "Spanning tree").  One box, one process, every
call warmed up, the forms alternating round by round, the median of --reps, HIP events around whole
calls.

Rows: fp32, generator kind 0, --n-train x d for every d of --dims; direct contexts; min_samples = 5.

  forms         mst          mst_device as the library ships it
                mst_lists    the list shortcut on, lists of max(min_samples, 16) entries
                mst_nolists  KNN_MST_LISTS=0: every row through every pass -- yardstick (a)
                mst_L0 / mst_L32   the shortcut with lists of min_samples / max(min_samples, 32) entries
                sweep32      dbscan_sweep_device at 32 radii on the same context -- (b), recorded, no bar
                cut32        mst_cut_device at the same 32 thresholds on the finished tree
  the bar       the shortcut is the default only if mst_lists beats mst_nolists by more than three of
                mst_nolists' spreads, s = (max - min) / median
  report only   every stage of one profiled call per form, rounds, rows sent through passes (the sum
                and the mean per round), the ratio mst / sweep32
  the same bits every mst form returns the same (w, a, b, core); the cut equals the sweep's labels on
                its core rows -- asserted before anything is timed

The 32 thresholds are equally spaced in rank between the median 5th- and the median 64th-neighbour
distance of a 256-row sample (time_dbscan_sweep.py's).  One JSON line, also written to --out.

  python scripts/time_mst.py [--reps 7] [--n-train 262144] [--dims 64,128] [--out profiles/mst.json]
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
MIN_SAMPLES = 5
# form -> the test hooks its context is created under
FORMS = {"mst": {}, "mst_lists": {"KNN_MST_LISTS": "1", "KNN_MST_LIST_L": "16"}, "mst_nolists": {"KNN_MST_LISTS": "0"},
         "mst_L0": {"KNN_MST_LISTS": "1", "KNN_MST_LIST_L": "0"}, "mst_L32": {"KNN_MST_LISTS": "1", "KNN_MST_LIST_L": "32"}}


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


def context(knn, hooks, **kw):
    """A direct context created under the given test hooks (the library reads them at knn_create)."""
    old = {k: os.environ.get(k) for k in ("KNN_MST_LISTS", "KNN_MST_LIST_L")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(hooks)
    try:
        return knn.Context(0, algo="direct", **kw)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--n-train", type=int, default=262_144)
    ap.add_argument("--dims", default="64,128")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mst.json"))
    a = ap.parse_args()
    knn = load_pkg(PKG, "knn_amd")
    dev = torch.device("cuda", 0)
    n, C, R = a.n_train, 10, 32
    res = {"reps": a.reps, "n_train": n, "min_samples": MIN_SAMPLES,
           "build_id": knn.load_library().knn_build_id().decode(), "cases": {}}

    for d in [int(v) for v in a.dims.split(",")]:
        plain = {f: context(knn, h) for f, h in FORMS.items()}           # whole calls: no events inside
        prof = {f: context(knn, h, profile=1) for f, h in FORMS.items()}
        tr = torch.empty((n, d), dtype=torch.float32, device=dev)
        tl = torch.empty(n, dtype=torch.int32, device=dev)
        plain["mst"].generate(tr, tl, 0, d, 0, 1, 0, C)
        ns, kd = min(256, n), min(65, n)  # (the row itself is its own first neighbour)
        sp = torch.empty(ns, dtype=torch.int32, device=dev)
        sd = torch.empty((ns, kd), dtype=torch.float32, device=dev)
        si = torch.empty((ns, kd), dtype=torch.int32, device=dev)
        plain["mst"].predict_device(tr, tl, tr[:ns], kd, C, sp, sd, si)
        ranks = np.round(np.linspace(min(5, kd - 1), kd - 1, R)).astype(np.int64)
        thr = np.sort(np.float32([sd[:, int(k)].median().item() for k in ranks]))

        # the same bits first
        trees = {f: c.mst_device(tr, min_samples=MIN_SAMPLES, core=True) for f, c in plain.items()}
        for f, t in trees.items():
            for x, y in zip(t[:4], trees["mst"][:4]):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (d, f)
            assert t[4][:2].tolist() == trees["mst"][4][:2].tolist(), (d, f)
        w, ea, eb, core, summary = trees["mst"]
        ctx = plain["mst"]
        labels, count, ssum = ctx.dbscan_sweep_device(tr, thresholds=thr, min_samples=MIN_SAMPLES, count=True)
        cut, csum = ctx.mst_cut_device(w, ea, eb, core, thresholds=thr)
        assert torch.equal(cut, torch.where(count >= MIN_SAMPLES, labels, torch.full_like(labels, -1))), d
        assert torch.equal(csum[:, :2], ssum[:, :2]), d
        del labels, count, cut, trees

        calls = {f: (lambda c=c: timed(lambda: c.mst_device(tr, min_samples=MIN_SAMPLES, core=True))) for f, c in plain.items()}
        calls["sweep32"] = lambda: timed(lambda: ctx.dbscan_sweep_device(tr, thresholds=thr, min_samples=MIN_SAMPLES))
        calls["cut32"] = lambda: timed(lambda: ctx.mst_cut_device(w, ea, eb, core, thresholds=thr))
        runs = {f: [] for f in calls}
        for r in range(a.warm + a.reps):
            for f, fn in calls.items():
                ms = fn()
                if r >= a.warm:
                    runs[f].append(ms)
            print(f"d={d} round {r}: " + ", ".join(f"{f} {v[-1]:.1f}" for f, v in runs.items() if v), file=sys.stderr, flush=True)
        med = {f: statistics.median(v) for f, v in runs.items()}
        s = spread(runs["mst_nolists"])
        # one profiled call each: stages, rounds, rows sent through passes
        forms = {}
        for f, c in prof.items():
            c.mst_device(tr, min_samples=MIN_SAMPLES)
            st, sg = c.stats(), c.stage_times()
            forms[f] = {"stages_ms": {k: round(v, 4) for k, v in sg.items()}, "rounds": st["mst_rounds"],
                        "pass_rows": st["mst_pass_rows"], "pass_rows_per_round": round(st["mst_pass_rows"] / max(st["mst_rounds"], 1), 1),
                        "segments": st["train_segments"]}
        res["cases"][f"d{d}"] = {
            "d": d, "summary": summary.cpu().tolist(), "thresholds": [float(t) for t in thr],
            "median_ms": {f: round(v, 4) for f, v in med.items()},
            "spread": {f: round(spread(v), 4) for f, v in runs.items()},
            "bar": {"s": round(s, 4), "nolists_ms": round(med["mst_nolists"], 4), "lists_ms": round(med["mst_lists"], 4),
                    "speedup": round(med["mst_nolists"] / med["mst_lists"], 3),
                    "met": med["mst_lists"] < med["mst_nolists"] * (1 - 3 * s)},
            "list_length": {"L0_ms": round(med["mst_L0"], 4), "L16_ms": round(med["mst_lists"], 4), "L32_ms": round(med["mst_L32"], 4)},
            "mst_over_sweep32": round(med["mst"] / med["sweep32"], 3),
            "forms": forms,
        }
        for c in list(plain.values()) + list(prof.values()):
            c.close()
        del tr, tl, w, ea, eb, core

    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
