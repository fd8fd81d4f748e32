#!/usr/bin/env python3
"""Times top-k calls at row widths between and beyond the filter's tile widths against a baseline
build of the library (DESIGN.md "Any row width", "Measured").

The baseline is another build of the package (--parent-pkg: the directory that holds its
__init__.py and libknn_amd.so, e.g. the parent commit built in a scratch checkout): there a
gemm_bf16 or AUTO context at a width outside 64 / 128 / 256 runs the direct form, so the same call
on the baseline is the yardstick.  Baseline and new run alternately, each shape in a fresh process;
every shape is warmed up; times are HIP-event medians of --reps calls.

  main table   --n-train x --n-query fp32 rows (generator kind 0), k = 10, algo = gemm_bf16, d in --dims:
               the whole predict_device call of both builds, the new build's "gemm_filter" stage
               (a second context with profile = 1) and that stage as a fraction of the bf16 dense
               roof (2 nt nq dp FLOP at --roof-pflops)
  spread       (max - min) / median of the baseline's repeats, per shape
  the bar      at a new width the new call is faster than the baseline's by more than three times
               the baseline's spread; at 64 / 128 / 256 the two are equal within that spread
  --auto-edge  32,768 x 32,768, k = 10, AUTO contexts, d = 96 and 768: the same bar

One JSON line per shape and a summary line.

  python scripts/time_wide_rows.py --parent-pkg DIR [--reps 7] [--dims 96,100,...] [--auto-edge] [--out FILE]
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "knn-using-p_threads-and-mpi_amd")
OLD_WIDTHS = (64, 128, 256)
DIMS = (64, 96, 100, 128, 192, 200, 256, 384, 512, 768, 1024, 1536)


def child(a):
    import torch
    spec = importlib.util.spec_from_file_location("knn_amd", os.path.join(a.pkg, "__init__.py"))
    knn = importlib.util.module_from_spec(spec)
    sys.modules["knn_amd"] = knn
    spec.loader.exec_module(knn)
    dev = "cuda:0"
    d, nt, nq, k, C = a.d, a.n_train, a.n_query, 10, 10
    ld = (d + 3) // 4 * 4
    ctx = knn.Context(0, algo=a.algo)
    train = torch.empty((nt, ld), dtype=torch.float32, device=dev)
    test = torch.empty((nq, ld), dtype=torch.float32, device=dev)
    labels = torch.empty(nt, dtype=torch.int32, device=dev)
    ctx.generate(train, labels, 0, d, 0, 1, 0, C)
    ctx.generate(test, None, 0, d, 0, 1, 1, C)
    pred = torch.empty(nq, dtype=torch.int32, device=dev)
    dist = torch.empty((nq, k), dtype=torch.float32, device=dev)
    idx = torch.empty((nq, k), dtype=torch.int32, device=dev)

    def call(c):
        c.predict_device(train[:, :d], labels, test[:, :d], k, C, pred, dist, idx)

    def timed(c):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call(c)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(2):
        call(ctx)
    torch.cuda.synchronize()
    ms = [timed(ctx) for _ in range(a.reps)]
    st = ctx.stats()
    ctx.close()
    out = {"d": d, "ms": statistics.median(ms), "spread": (max(ms) - min(ms)) / statistics.median(ms),
           "filter_operands": st.get("filter_operands"), "fallback_queries": st.get("fallback_queries"),
           "filter_width": st.get("filter_width", None), "checksum": int(idx.sum().item())}
    if st.get("filter_operands") is not None:
        pctx = knn.Context(0, algo=a.algo, profile=1)
        call(pctx)
        torch.cuda.synchronize()
        fs = []
        for _ in range(a.reps):
            call(pctx)
            torch.cuda.synchronize()
            fs.append(pctx.stage_times().get("gemm_filter", 0.0))
        pctx.close()
        out["filter_ms"] = statistics.median(fs)
    print("RESULT " + json.dumps(out), flush=True)


def run_child(pkg, d, a, algo, nt, nq):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--pkg", pkg, "--d", str(d), "--algo", algo,
           "--n-train", str(nt), "--n-query", str(nq), "--reps", str(a.reps)]
    env = dict(os.environ, KNN_AMD_LIB=os.path.join(pkg, "libknn_amd.so"))
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=a.child_timeout)
    if p.returncode != 0:
        # a failed child ends the measurement: nothing more is started on the device
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        raise SystemExit(f"child failed (rc={p.returncode}) at d={d} pkg={pkg}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def shape(a, d, algo, nt, nq, what):
    old = run_child(a.parent_pkg, d, a, algo, nt, nq)
    new = run_child(PKG, d, a, algo, nt, nq)
    s = old["spread"]
    row = {"table": what, "d": d, "algo": algo, "n_train": nt, "n_query": nq, "parent_ms": old["ms"], "parent_spread": s,
           "new_ms": new["ms"], "new_spread": new["spread"], "ratio": old["ms"] / new["ms"],
           "parent_operands": old["filter_operands"], "new_operands": new["filter_operands"],
           "new_width": new["filter_width"], "new_fallback": new["fallback_queries"],
           "same_checksum": old["checksum"] == new["checksum"]}
    if "filter_ms" in new:
        dp = new["filter_width"] or d
        row["new_filter_ms"] = new["filter_ms"]
        row["filter_of_roof"] = (2.0 * nt * nq * dp / (a.roof_pflops * 1e15)) / (new["filter_ms"] * 1e-3)
    if d in OLD_WIDTHS and what == "main":
        row["bar"] = "equal within the parent's spread"
        row["met"] = abs(new["ms"] - old["ms"]) <= s * old["ms"]
    else:
        row["bar"] = "faster by more than 3x the parent's spread"
        row["met"] = old["ms"] - new["ms"] > 3.0 * s * old["ms"]
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-pkg")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dims", default=",".join(str(d) for d in DIMS))
    ap.add_argument("--n-train", type=int, default=262_144)
    ap.add_argument("--n-query", type=int, default=16_384)
    ap.add_argument("--auto-edge", action="store_true")
    ap.add_argument("--roof-pflops", type=float, default=2.5)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--pkg")
    ap.add_argument("--d", type=int)
    ap.add_argument("--algo", default="gemm_bf16")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_pkg:
        ap.error("--parent-pkg is needed")
    rows = [shape(a, int(d), "gemm_bf16", a.n_train, a.n_query, "main") for d in a.dims.split(",") if d]
    if a.auto_edge:
        rows += [shape(a, d, "auto", 32_768, 32_768, "auto_edge") for d in (96, 768)]
    summary = {"summary": True, "all_met": all(r["met"] for r in rows), "not_met": [(r["table"], r["d"]) for r in rows if not r["met"]]}
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"rows": rows, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
