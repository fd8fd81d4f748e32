#!/usr/bin/env python3
"""Times the local outlier factor (DESIGN.md "Local outlier factor") on one box in one process, with
HIP events, the median of --reps warm calls each:

  call        one lof_device(train, k_lo, k_hi) call: the leave-one-out top-(k_hi + 1) pass of the
              train rows against themselves, then k_lof_compact, k_lof_lrd, k_lof_score
  stages      from a profile = 1 context, per call: the three "lof" stages in launch order
              (compact, lrd, score) and the top-(k_hi + 1) pass (every other stage of the call)

Workload: 262,144 x 64 fp32 rows, the single k = 20 and the range 10..32.  The question it answers:
do the LOF stages stay a small fraction of the pass?  One JSON object, printed and written to --out.

  python scripts/time_lof.py [--reps 7] [--rows 262144] [--out profiles/lof.json]
"""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "knn-using-p_threads-and-mpi_amd")
RANGES = ((20, 20), (10, 32))
KERNELS = ("compact", "lrd", "score")


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


def stages(ctx):
    """The last call's stages in launch order: [(name, ms)] (Context.stage_times adds up equal names)."""
    names = (ctypes.c_char_p * 256)()
    ms = (ctypes.c_float * 256)()
    n = ctx.lib.knn_stage_times(ctx.h, names, ms, 256)
    return [(names[i].decode(), ms[i]) for i in range(n)]


def run(knn, n, d, k_lo, k_hi, reps):
    dev = torch.device("cuda", 0)
    ctx = knn.Context(0)
    tr = torch.empty((n, d), dtype=torch.float32, device=dev)
    lab = torch.empty(n, dtype=torch.int32, device=dev)
    ctx.generate(tr, lab, 0, d, 0, 1, 0, 10)
    Kr = k_hi - k_lo + 1
    lof = torch.empty((Kr, n), dtype=torch.float32, device=dev)
    res = {"n": n, "d": d, "k_lo": k_lo, "k_hi": k_hi, "reps": reps}
    res["call_ms"] = median_ms(lambda: ctx.lof_device(tr, k_lo, k_hi, lof=lof), reps)
    st = ctx.stats()
    res["filter_operands"], res["filter_width"] = st["filter_operands"], st["filter_width"]
    m = knn.lof_max(lof)
    res["rows_above_1.5"] = int(knn.lof_outliers(m).numel())
    res["largest_lof"] = float(m.max())
    ctx.close()
    pctx = knn.Context(0, profile=1)
    for _ in range(2):
        pctx.lof_device(tr, k_lo, k_hi, lof=lof)
    per = {name: [] for name in KERNELS}
    passes, totals = [], []
    for _ in range(reps):
        pctx.lof_device(tr, k_lo, k_hi, lof=lof)
        s = stages(pctx)
        lofs = [ms for name, ms in s if name == "lof"]
        assert len(lofs) == 3, s
        for name, ms in zip(KERNELS, lofs):
            per[name].append(ms)
        totals.append(sum(lofs))
        passes.append(sum(ms for name, ms in s if name != "lof"))
    pctx.close()
    for name in KERNELS:
        res[f"lof_{name}_ms"] = statistics.median(per[name])
    res["lof_stages_ms"] = statistics.median(totals)
    res["pass_ms"] = statistics.median(passes)
    res["lof_over_pass"] = res["lof_stages_ms"] / res["pass_ms"]
    for k, v in res.items():
        if isinstance(v, float):
            res[k] = round(v, 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=262_144)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lof.json"))
    a = ap.parse_args()
    knn = load_pkg()
    out = {"script": "scripts/time_lof.py", "device": torch.cuda.get_device_name(0),
           "workloads": [run(knn, a.rows, 64, k_lo, k_hi, a.reps) for k_lo, k_hi in RANGES]}
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
