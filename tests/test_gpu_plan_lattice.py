"""Every top-k filter kernel instance at both ends of its k range and at its size edges, on the GPU.

The cases are tests/test_plan_lattice_cpu.py's lattice(): for every operand class (fp32 `gemm`,
`gemm_split`, `gemm_bf16` on fp32 rows, `gemm` on bf16 rows, `gemm_i8`), row width and test hook
(KNN_FUSED_QG, KNN_FUSED_HEAPS, KNN_FUSED_PARK) the first and the last k of every range over which
the library's own plan functions keep one plan, and k = 129, where the filter hands over to the
direct form.  One test function per plan range.  Each (plan, k) runs on a star of sizes (star()):
nt = k (every row is a neighbour, in order), nt within one row of the 32- and 64-row tiles and of
their pairs, quads and octets, a piece with fewer rows than k (train_splits = 3 and 8), and nq
within one row of the plan's query block -- all prefixes of one generated 1,025 x 513 set per
(d, dtype), plain ("gen") and with exact copies of rows across tile edges and queries that are
train rows ("dups").

Every call asserts indices, distance bits and predictions equal to the C oracle's (one oracle call
per train prefix; a smaller k and fewer queries are prefixes of its lists,
test_plan_lattice_cpu.py::test_reference_prefixes), and that the intended path ran: the operands,
the element, the fused form, the queries per wave, the operand width and the segments from the
stats against the lattice's plan and knn_filter_policy.  On the plain rows no query may take the
exact fallback (fallback_queries == 0, rerun_split false: a filter that drops a neighbour or
overflows would otherwise hide behind the exact scan) -- with eight forced pieces a lane half sees
at most 96 rows, below its 128-entry sub-slice, so this is a condition, not a tolerance.  On the
int8 class (profile = 2) the seed pass is run both ways: no finite seed below the oracle's k-th
distance, none at all below the first train size knn_debug_seed_tiles samples, one per query from
there up.  No GPU result is ever the yardstick.
"""
import contextlib
import os

import numpy as np
import pytest

from test_plan_lattice_cpu import (C, K_LAST, NQ_MAX, NT_MAX, SEED, WIDE_D, WIDE_K, WIDE_NQ, WIDE_NT, base_rows, expected,
                                   group_id, lattice, prefix_rows, reference, seed_tiles, split_sizes, star, wide_plan)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GROUPS = lattice()
KINDS = ("gen", "dups")
OPERANDS = {"fp32": "f32", "split": "bf16x3 split", "rounded": "bf16 rounded", "bf16": "bf16", "int8": "bf16 rounded"}
HOOK_ENV = {"qg": "KNN_FUSED_QG", "heaps": "KNN_FUSED_HEAPS", "park": "KNN_FUSED_PARK", "seed": "KNN_FUSED_SEED"}
_base, _sets, _ctx = {}, {}, {}


@contextlib.contextmanager
def _hook_env(hooks):
    """The hooks' environment for one knn_create (which snapshots it), then the caller's again."""
    old = {v: os.environ.get(v) for v in HOOK_ENV.values()}
    try:
        for name, var in HOOK_ENV.items():
            os.environ.pop(var, None)
            val = hooks.get(name)
            if val is not None and not (name == "heaps" and not val):   # (KNN_FUSED_HEAPS counts when set)
                os.environ[var] = str(val)
        yield
    finally:
        for var, val in old.items():
            os.environ.pop(var, None)
            if val is not None:
                os.environ[var] = val


def _context(knn, algo, hooks, splits=0, profile=0):
    """One context per (algo, hooks, train_splits) for the whole module."""
    key = (algo, tuple(sorted(hooks.items())), splits, profile)
    if key not in _ctx:
        with _hook_env(hooks):
            _ctx[key] = knn.Context(0, algo=algo, train_splits=splits, profile=profile)
    return _ctx[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()
    _sets.clear()
    _base.clear()


def _set(oracle, d, bf16, kind, nt):
    """(train, labels, queries) of one train prefix on the device, the labels on the host and the
    oracle's lists for all 513 queries; built once."""
    import torch
    key = (d, bf16, kind, nt)
    if key not in _sets:
        if (d, bf16) not in _base:
            _base[d, bf16] = base_rows(oracle, d, bf16)
        tr, tl, te = prefix_rows(_base[d, bf16], nt, kind == "dups")
        dt = torch.bfloat16 if bf16 else torch.float32
        pitch = -(-d // 8) * 8      # (16-byte rows; the calls pass the true d, so the pad columns are never read)

        def dev(x):
            t = torch.zeros((len(x), pitch), dtype=dt)
            t[:, :d] = torch.from_numpy(np.ascontiguousarray(x))
            return t.to(DEV)

        _sets[key] = (dev(tr), torch.from_numpy(np.ascontiguousarray(tl)).to(DEV), dev(te), tl,
                      reference(oracle, tr, tl, te))
    return _sets[key]


def _run(ctx, s, k, nq, d, views=False):
    """views: the rows as column views [:, :d] of the padded tables (a one-row view included) instead
    of the tables with the true d."""
    import torch
    pred = torch.empty(nq, dtype=torch.int32, device=DEV)
    dist = torch.empty((nq, k), dtype=torch.float32, device=DEV)
    idx = torch.empty((nq, k), dtype=torch.int32, device=DEV)
    if views:
        ctx.predict_device(s[0][:, :d], s[1], s[2][:nq, :d], k, C, pred, dist, idx)
    else:
        ctx.predict_device(s[0], s[1], s[2][:nq], k, C, pred, dist, idx, d=d)
    return pred.cpu().numpy(), dist.cpu().numpy().view(np.uint32), idx.cpu().numpy()


def _same(got, want, what):
    assert np.array_equal(got[2], want[2]), f"{what}: indices"
    assert np.array_equal(got[1], want[1]), f"{what}: distance bits"
    assert np.array_equal(got[0], want[0]), f"{what}: predictions"


def _path(knn, g, c, nt, nq, st, kind, splits, what):
    """The stats of the call against the lattice's plan and the library's policy at this size."""
    form, width = knn.filter_policy(g["dtype"], g["d"], c["k"], nt, nq, g["algo"])
    assert form == c["form"], (what, form)
    if form == "direct":
        assert st["filter_operands"] is None and st["filter_element"] is None and not st["fused_norm"], (what, st)
        assert st["filter_width"] == 0 and st["filter_chunks"] == 0 and st["queries_per_wave"] == 0, (what, st)
        assert st["fallback_queries"] == 0 and not st["rerun_split"], (what, st)
        return
    assert st["filter_operands"] == OPERANDS[g["name"]], (what, st)
    assert st["filter_element"] == (None if g["name"] == "fp32" else "i8" if c["i8"] else "bf16"), (what, st)
    assert st["fused_norm"] == (form == "fused"), (what, st)
    assert st["queries_per_wave"] == (32 * c["qg"] if form == "fused" else 0), (what, st)
    assert st["filter_width"] == width == g["d"] and st["filter_chunks"] == 1, (what, st)
    assert st["train_segments"] == (min(8, splits) if splits else st["train_segments"]) >= 1, (what, st)
    if kind == "gen":
        assert st["fallback_queries"] == 0 and not st["rerun_split"], (what, st)


def _num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("g", GROUPS, ids=group_id)
def test_plan_range(knn, oracle, g):
    d, bf16 = g["d"], g["dtype"] == "bf16"
    calls = 0
    for c in g["cases"]:
        k = c["k"]
        i8 = bool(c["i8"])
        hooks = dict(g["hooks"])
        if not c["qg"]:
            hooks = {}            # (no fused kernel at this k: the hooks have nothing to force)
        sizes = [(nt, nq, 0) for nt, nq in star(k, c["bm"], c["extra_nt"])]
        sizes += [(nt, nq, sp) for sp in (3, 8) for nt, nq in split_sizes(k, c["bm"])]
        for kind in KINDS:
            for nt, nq, splits in sizes:
                s = _set(oracle, d, bf16, kind, nt)
                want = expected(s[4], s[3], k, nq)
                if k == nt:
                    assert np.array_equal(np.sort(want[2], axis=1), np.tile(np.arange(nt, dtype=np.int32), (nq, 1)))
                for seed in ((1, 0) if i8 else (None,)):
                    h = dict(hooks, seed=seed) if i8 else hooks
                    ctx = _context(knn, g["algo"], h, splits, 2 if i8 else 0)
                    what = f"{group_id(g)} k={k} {kind} nt={nt} nq={nq} splits={splits} seed={seed}"
                    got = _run(ctx, s, k, nq, d)
                    st = ctx.stats()
                    calls += 1
                    _same(got, want, what)
                    _path(knn, g, c, nt, nq, st, kind, splits, what)
                    if not i8:
                        assert st["seeded_queries"] == 0, (what, st)
                        continue
                    if hooks.get("park") == 0:
                        assert st["parked_passes"] == 0, (what, st)
                    sd = ctx.last_seed(nq)
                    if seed == 1 and seed_tiles(nt, c["bn"], nq, _num_cus()) > 0:
                        kth = want[1].view(np.float32)[:, k - 1]
                        assert len(sd) == nq and not np.isnan(sd).any(), what
                        assert (sd[np.isfinite(sd)] >= kth[np.isfinite(sd)]).all(), what
                        assert st["seeded_queries"] == nq == int(np.isfinite(sd).sum()), (what, st)
                    else:
                        assert st["seeded_queries"] == 0 and len(sd) == 0, (what, st)
    print(f"{group_id(g)}: {calls} calls")


@pytest.mark.parametrize("d", WIDE_D)
def test_wide_edges(knn, oracle, d):
    """k_gemm_wide (rows wider than 256 features, chunks of 128): its 256-row groups and 256-query
    blocks from one row below to one row above, one group and three, k on both sides of the list
    register classes and k = nt."""
    w = wide_plan(128)
    assert w["bm"] == 256 and w["group_rows"] == 256           # (the shapes below are their edges)
    ctx = _context(knn, "gemm_bf16", {})
    calls = 0
    for kind in KINDS:
        for k in WIDE_K:
            for nt in sorted({k, *WIDE_NT}):
                if nt < k:
                    continue
                s = _set(oracle, d, False, kind, nt)
                for nq in WIDE_NQ:
                    what = f"wide d={d} k={k} {kind} nt={nt} nq={nq}"
                    _same(_run(ctx, s, k, nq, d, views=kind == "dups"), expected(s[4], s[3], k, nq), what)
                    st = ctx.stats()
                    calls += 1
                    assert knn.filter_policy("f32", d, k, nt, nq, "gemm_bf16") == ("wide", -(-d // 128) * 128), what
                    assert st["filter_operands"] == "bf16 rounded" and st["filter_element"] == "bf16", (what, st)
                    assert not st["fused_norm"] and st["queries_per_wave"] == 0 and st["train_segments"] >= 1, (what, st)
                    assert st["filter_width"] == -(-d // 128) * 128 and st["filter_chunks"] == -(-d // 128), (what, st)
                    if kind == "gen":
                        assert st["fallback_queries"] == 0 and not st["rerun_split"], (what, st)
    print(f"wide d={d}: {calls} calls")


def test_lattice_shape():
    """What this file ran: no case dropped on the way from the lattice (the CPU file checks the
    lattice itself)."""
    assert len({group_id(g) for g in GROUPS}) == len(GROUPS) > 0
    assert all(g["cases"] and all(c["k"] in (g["lo"], g["hi"]) for c in g["cases"]) for g in GROUPS)
    assert any(c["k"] == K_LAST for g in GROUPS for c in g["cases"])
    assert NT_MAX == 1025 and NQ_MAX == 513 and SEED > 0
