#!/usr/bin/env python3
"""Times the two forms of the radius distance pass against each other (DESIGN.md "Radius
neighbours", "The MFMA form"): the direct form (k_radius_tile, a context with algo="direct") and the
MFMA-filtered form (k_radius_gemm, algo="gemm_bf16"), on one box in one process, every call warmed
up, the two forms alternating round by round, the median of --reps each.

Rows: fp32, generator kind 0.  Thresholds as in time_radius.py, from the top-k export of
predict_device on a 256-query sample: the median 10th-neighbour distance ("sparse") and the median
1,024th ("dense").

  yardstick     the direct form in the same process, s = (max - min) / median of its repeats
  the bar       per d in --dims, on --n-train x --n-query: the sparse "radius_count" stage of the MFMA
                form is faster than the direct form's by more than s, and so is the whole
                radius_count_device call on a context without cache_train (operand build included)
  the floors    whole radius_count_device calls, MFMA uncached and cached against direct, at
                16,384 rows x {1, 256, 16,384} queries and 65,536 x 256
  report only   the dense count, the fill sparse and dense, the whole weighted
                radius_predict_device call, the stages "radius_norms" / "radius_operands", and with
                --config-a one sparse count call of each form on 1M x 128 against 100k queries

One JSON line.

  python scripts/time_radius_mfma.py [--reps 7] [--dims 64,128,256] [--n-train 262144] [--n-query 16384] [--config-a]
                                     [--floors 16384x1,16384x256,...] [--floors-only]
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
FORMS = ("direct", "mfma")
FLOOR_SHAPES = ((16_384, 1), (16_384, 256), (16_384, 16_384), (65_536, 256))


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


def alternate(calls, ctxs, reps, warm=2):
    """calls: name -> fn(ctx) returning ms; ctxs: label -> context.  {label: {name: [ms]}}"""
    runs = {f: {n: [] for n in calls} for f in ctxs}
    for r in range(warm + reps):
        for name, fn in calls.items():
            for f, c in ctxs.items():
                ms = fn(c)
                if r >= warm:
                    runs[f][name].append(ms)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dims", default="64,128,256")
    ap.add_argument("--n-train", type=int, default=262_144)
    ap.add_argument("--n-query", type=int, default=16_384)
    ap.add_argument("--config-a", action="store_true")
    ap.add_argument("--floors", default=",".join(f"{n}x{q}" for n, q in FLOOR_SHAPES),
                    help="rows x queries of the whole-call floor measurements")
    ap.add_argument("--floors-only", action="store_true", help="skip the bar and the report: the floors alone")
    a = ap.parse_args()
    floor_shapes = [tuple(int(v) for v in s.split("x")) for s in a.floors.split(",") if s]
    knn = load_pkg()
    dev = torch.device("cuda", 0)
    C = 10
    ctxs = {"direct": knn.Context(0, algo="direct", profile=1), "mfma": knn.Context(0, algo="gemm_bf16", profile=1)}
    # whole calls: no events inside the call; the cached context keeps the train-side operands
    plain = {"direct": knn.Context(0, algo="direct"), "mfma": knn.Context(0, algo="gemm_bf16"),
             "mfma_cached": knn.Context(0, algo="gemm_bf16", cache_train=True)}
    res = {"reps": a.reps, "n_train": a.n_train, "n_query": a.n_query, "dims": {}, "floors": {}}

    def rows(nt, nq, d):
        tr = torch.empty((nt, d), dtype=torch.float32, device=dev)
        tl = torch.empty(nt, dtype=torch.int32, device=dev)
        te = torch.empty((nq, d), dtype=torch.float32, device=dev)
        ql = torch.empty(nq, dtype=torch.int32, device=dev)
        ctxs["direct"].generate(tr, tl, 0, d, 0, 1, 0, C)
        ctxs["direct"].generate(te, ql, 0, d, 0, 1, 1, C)
        return tr, tl, te, ql

    def thresholds(tr, tl, te):
        ns, kd = min(256, len(te)), min(1024, len(tr))
        sp = torch.empty(ns, dtype=torch.int32, device=dev)
        sd = torch.empty((ns, kd), dtype=torch.float32, device=dev)
        si = torch.empty((ns, kd), dtype=torch.int32, device=dev)
        ctxs["direct"].predict_device(tr, tl, te[:ns], kd, C, sp, sd, si)
        return {"sparse": float(sd[:, min(9, kd - 1)].median().item()), "dense": float(sd[:, kd - 1].median().item())}

    def stage(c, name):
        return c.stage_times().get(name, 0.0)

    for d in (int(x) for x in a.dims.split(",")):
        nt, nq = a.n_train, a.n_query
        tr, tl, te, ql = rows(nt, nq, d)
        thr = thresholds(tr, tl, te)

        def bars():
            lists, info = {}, {}
            for dens in ("sparse", "dense"):
                for f in FORMS:
                    lists[f, dens] = ctxs[f].radius_neighbors_device(tr, te, threshold=thr[dens])
                    info[f"{f}_{dens}_segments"] = ctxs[f].stats()["train_segments"]
                assert torch.equal(lists["direct", dens][0], lists["mfma", dens][0])
                assert torch.equal(lists["direct", dens][1], lists["mfma", dens][1])
                assert torch.equal(lists["direct", dens][2].view(torch.int32), lists["mfma", dens][2].view(torch.int32))
                info[f"{dens}_mean_neighbours"] = round(lists["direct", dens][1].numel() / nq, 2)
            assert ctxs["mfma"].stats()["radius_form"] == "mfma" and ctxs["direct"].stats()["radius_form"] == "direct"
            f_of = {id(c): f for f, c in ctxs.items()}
            calls = {
                "count_sparse": lambda c: (c.radius_count_device(tr, tl, te, threshold=thr["sparse"], num_classes=C,
                                                                 query_labels=ql), stage(c, "radius_count"))[1],
                "count_dense": lambda c: (c.radius_count_device(tr, tl, te, threshold=thr["dense"], num_classes=C,
                                                                query_labels=ql), stage(c, "radius_count"))[1],
                "fill_sparse": lambda c: (c.radius_fill_device(tr, te, lists[f_of[id(c)], "sparse"][0], threshold=thr["sparse"]),
                                          stage(c, "radius_fill"))[1],
                "fill_dense": lambda c: (c.radius_fill_device(tr, te, lists[f_of[id(c)], "dense"][0], threshold=thr["dense"]),
                                         stage(c, "radius_fill"))[1],
                "norms_stage": lambda c: (c.radius_count_device(tr, None, te, threshold=thr["sparse"]),
                                          stage(c, "radius_norms"))[1],
                "operands_stage": lambda c: (c.radius_count_device(tr, None, te, threshold=thr["sparse"]),
                                             stage(c, "radius_operands"))[1],
            }
            runs = alternate(calls, ctxs, a.reps)
            whole = {
                "count_sparse_call": lambda c: timed(lambda: c.radius_count_device(tr, tl, te, threshold=thr["sparse"],
                                                                                   num_classes=C, query_labels=ql)),
                "predict_weighted_sparse_call": lambda c: timed(lambda: c.radius_predict_device(
                    tr, tl, te, threshold=thr["sparse"], num_classes=C, weights="distance")),
                "predict_weighted_dense_call": lambda c: timed(lambda: c.radius_predict_device(
                    tr, tl, te, threshold=thr["dense"], num_classes=C, weights="distance")),
            }
            wruns = alternate(whole, plain, a.reps)
            out = {"thresholds": thr, **info,
                   "median_ms": {f: {n: med(v) for n, v in runs[f].items()} for f in ctxs},
                   "median_call_ms": {f: {n: med(v) for n, v in wruns[f].items()} for f in plain}, "bar": {}}
            for name, rr, direct, mfma in (("count_sparse_stage", runs, "direct", "mfma"),
                                           ("count_sparse_call_uncached", wruns, "direct", "mfma")):
                key = "count_sparse" if rr is runs else "count_sparse_call"
                s = spread(rr[direct][key])
                md, mm = statistics.median(rr[direct][key]), statistics.median(rr[mfma][key])
                out["bar"][name] = {"s": round(s, 4), "direct_ms": round(md, 4), "mfma_ms": round(mm, 4),
                                    "speedup": round(md / mm, 3), "met": mm < md * (1 - s)}
            return out

        if not a.floors_only:
            res["dims"][str(d)] = bars()

        if d in (64, 128):
            fl = {}
            for fnt, fnq in floor_shapes:
                ftr, ftl, fte = tr[:fnt], tl[:fnt], te[:fnq]
                fthr = thresholds(ftr, ftl, fte if fnq >= 256 else te[:256])["sparse"]
                fr = alternate({"call": lambda c: timed(lambda: c.radius_count_device(ftr, ftl, fte, threshold=fthr,
                                                                                      num_classes=C))}, plain, a.reps)
                s = spread(fr["direct"]["call"])
                md = statistics.median(fr["direct"]["call"])
                fl[f"{fnt}x{fnq}"] = {"s": round(s, 4), **{f: med(fr[f]["call"]) for f in plain},
                                      "mfma_not_slower": statistics.median(fr["mfma"]["call"]) <= md * (1 + s),
                                      "mfma_cached_not_slower": statistics.median(fr["mfma_cached"]["call"]) <= md * (1 + s)}
            res["floors"][str(d)] = fl
        del tr, tl, te, ql

    if a.config_a:
        tr, tl, te, ql = rows(1_000_000, 100_000, 128)
        thr = thresholds(tr, tl, te)["sparse"]
        ca = {}
        for f in ("mfma", "direct"):
            ctxs[f].radius_count_device(tr, tl, te[:4096], threshold=thr, num_classes=C)    # warm-up on a slice
            ms = timed(lambda: ctxs[f].radius_count_device(tr, tl, te, threshold=thr, num_classes=C, query_labels=ql))
            ca[f] = {"call_ms": round(ms, 3), "radius_count_ms": round(stage(ctxs[f], "radius_count"), 3),
                     "segments": ctxs[f].stats()["train_segments"]}
        res["config_a"] = {"n_train": 1_000_000, "n_query": 100_000, "d": 128, "threshold": thr, **ca}

    for c in list(ctxs.values()) + list(plain.values()):
        c.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
