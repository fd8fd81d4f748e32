"""The lattice of top-k kernel instances: every k at which the library changes the kernel it runs.

No GPU.  The library picks a top-k kernel by plan rules: knn_fused_plan (k_gemm_fused),
knn_gemm_filter_plan (k_gemm_filter), knn_wide_plan (k_gemm_wide) and knn_list_regs (the list
registers of k_rescore, k_direct_tile, k_exact_scan and k_merge_vote).  lattice() walks k = 1..129
through the library's own host views of those rules -- knn_fused_debug_plan,
knn_debug_gemm_filter_plan, knn_debug_wide_plan, knn_filter_policy, knn_debug_seed_tiles and the
text of knn_list_regs -- for every operand class, row width and test hook, records each maximal k
range with one plan, and emits both ends of every range: a switch at a | a + 1 yields both values,
and 128 | 129 is where the filter hands over to the direct form.  tests/test_gpu_plan_lattice.py
runs every emitted (plan, k) on the GPU against the oracle; nothing here restates a rule, so a
changed rule moves the cases with it -- and fails test_ranges_are_the_documented_ones, whose table
is DESIGN.md's.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import PKG_DIR, load_pkg
from test_metric_cpu import vote_reference

C = 10
SEED = 71
NT_MAX, NQ_MAX = 1025, 513
K_LAST = 129                      # one past the filter's largest k: the direct form
ELEM_F32, ELEM_BF16, ELEM_SPLIT = 0, 1, 2
FUSED_FIELDS = ("nw", "qg", "rg", "minw", "nbuf", "bm", "lds", "kr", "ls", "i8", "has_kernel")
FILTER_FIELDS = ("nw", "qg", "rg", "minw", "nbuf", "bm", "lds")

# operand classes: (name, data type, context algo, row widths, the element k_gemm_filter multiplies)
CLASSES = (
    ("fp32", "f32", "gemm", (32, 64, 128), ELEM_F32),
    ("split", "f32", "gemm_split", (32, 64, 128), ELEM_SPLIT),
    ("rounded", "f32", "gemm_bf16", (64, 128, 256), ELEM_BF16),
    ("bf16", "bf16", "gemm", (64, 128, 256), ELEM_BF16),
    # the int8 plan exists at d = 128, k <= 32 (knn_fused_plan); a larger k runs the bf16 operands
    ("int8", "f32", "gemm_i8", (128,), ELEM_BF16),
)
# the star of sizes every (plan, k) runs on: both sides of the 32- and 64-row tiles and of their
# pairs, quads and octets, a partial last group, and the whole set
NT_STAR = (33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 1025)
# k_gemm_wide (rows wider than 256 features): the issue's shapes, edges of its groups and blocks
WIDE_D = (257, 384, 385)
WIDE_K = (1, 64, 65, 128)
WIDE_NT = (255, 256, 257, 513)
WIDE_NQ = (1, 255, 256, 257)


def _lib():
    lib = load_pkg().load_library()
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    lib.knn_fused_debug_plan.argtypes = [I, I, LL, I, I, I, I, I, P]
    lib.knn_fused_debug_plan.restype = I
    lib.knn_debug_gemm_filter_plan.argtypes = [I, I, I, P]
    lib.knn_debug_gemm_filter_plan.restype = I
    lib.knn_debug_wide_plan.argtypes = [I, P]
    lib.knn_debug_wide_plan.restype = I
    lib.knn_debug_seed_tiles.argtypes = [LL, I, LL, I, P, I, P]
    lib.knn_debug_seed_tiles.restype = I
    return lib


def fused_plan(d, k, qg, heaps, i8):
    """knn_fused_debug_plan with the hooks forced (the plan then depends on nothing else)."""
    out = np.zeros(len(FUSED_FIELDS), np.int64)
    assert _lib().knn_fused_debug_plan(d, k, NQ_MAX, 256, qg, heaps, 1, i8, out.ctypes.data) == 0
    return dict(zip(FUSED_FIELDS, out.tolist()))


def filter_plan(elem, row_bytes, k):
    out = np.zeros(len(FILTER_FIELDS), np.int64)
    assert _lib().knn_debug_gemm_filter_plan(elem, row_bytes, k, out.ctypes.data) == 0
    return dict(zip(FILTER_FIELDS, out.tolist()))


def wide_plan(k):
    out = np.zeros(len(FILTER_FIELDS) + 1, np.int64)
    assert _lib().knn_debug_wide_plan(k, out.ctypes.data) == 0
    return dict(zip(FILTER_FIELDS + ("group_rows",), out.tolist()))


def seed_tiles(nt, bn, nq=NQ_MAX, num_cus=256):
    """How many tile blocks of bn rows the seed pass samples of nt train rows."""
    return _lib().knn_debug_seed_tiles(nt, bn, nq, num_cus, None, 0, None)


def first_seeded(bn):
    """The smallest train set the seed pass samples (knn_seed_sample), tile blocks of bn rows."""
    return next(nt for nt in range(1, 4096) if seed_tiles(nt, bn) > 0)


def list_classes():
    """The k classes of knn_list_regs (list registers of 64 entries), from its text: the function
    is inline in knn_kernels.h and every launcher switches on it."""
    with open(os.path.join(PKG_DIR, "csrc", "knn_kernels.h")) as f:
        m = re.search(r"inline int knn_list_regs\(int k\) \{ return (.*?); \}", f.read())
    assert m, "knn_list_regs changed its form: restate list_classes()"
    steps = re.findall(r"k <= (\d+) \? (\d+)", m.group(1))
    last = int(re.search(r": (\d+)$", m.group(1)).group(1))
    assert steps and all(int(kk) == 64 * int(r) for kk, r in steps), m.group(1)
    return tuple(int(kk) for kk, _ in steps) + (64 * last,)


def list_regs(k):
    return next(i for i, top in enumerate(list_classes()) if k <= top)


def hooks_of(name, d):
    """Every setting of the test hooks that can change the plan of (class, d): KNN_FUSED_QG (the
    queries per wave), KNN_FUSED_HEAPS (d = 256) and, on the int8 class, KNN_FUSED_PARK."""
    if name in ("fp32", "split"):
        return [{}]
    return [{"qg": qg, "heaps": heaps, **({"park": park} if name == "int8" else {})}
            for qg in (1, 2) for heaps in ((0, 1) if d == 256 else (0,))
            for park in ((1, 0) if name == "int8" else (None,))]


def plan_of(name, d, k, hooks):
    """What runs for (class, d, k) under the hooks, from the library: a hashable plan (without its
    LDS bytes, which grow with k inside one shape) and the details of this k."""
    knn = load_pkg()
    _, dtype, algo, _, elem = next(c for c in CLASSES if c[0] == name)
    form, width = knn.filter_policy(dtype, d, k, NT_MAX, NQ_MAX, algo)
    regs = list_regs(k)
    if form == "direct":
        return ("direct", regs), {"form": form, "bm": 0, "lds": 0, "qg": 0, "i8": 0, "bn": 0}
    assert width == d
    if hooks:
        f = fused_plan(d, k, hooks["qg"], hooks["heaps"], 1) if name == "int8" else {"nw": 0}
        if f["nw"] == 0:
            f = fused_plan(d, k, hooks["qg"], hooks["heaps"], 0)
        assert (f["nw"] > 0) == (form == "fused"), (name, d, k, hooks, form, f)
        if f["nw"] > 0:
            park = hooks.get("park") if f["i8"] else None
            plan = ("fused",) + tuple(f[n] for n in ("nw", "qg", "rg", "minw", "nbuf", "bm", "kr", "ls", "i8")) + (park, regs)
            return plan, {"form": form, "bm": f["bm"], "lds": f["lds"], "qg": f["qg"], "i8": f["i8"],
                          "bn": 32 * f["rg"], "has_kernel": f["has_kernel"]}
    assert form == "filter"
    row_bytes = 4 * d if name in ("fp32", "split") else 2 * d
    f = filter_plan(elem, row_bytes, k)
    plan = ("filter", row_bytes) + tuple(f[n] for n in ("nw", "qg", "rg", "minw", "nbuf", "bm")) + (regs,)
    return plan, {"form": form, "bm": f["bm"], "lds": f["lds"], "qg": 0, "i8": 0, "bn": 32 * f["rg"]}


def walk(name, d, hooks):
    """[(lo, hi, plan, {k: details})]: the maximal k ranges of one plan over k = 1..129."""
    runs = []
    for k in range(1, K_LAST + 1):
        plan, info = plan_of(name, d, k, hooks)
        if runs and runs[-1][2] == plan:
            runs[-1][1] = k
            runs[-1][3][k] = info
        else:
            runs.append([k, k, plan, {k: info}])
    return [tuple(r) for r in runs]


def star(k, bm, extra_nt=()):
    """The (nt, nq) a lattice case runs on: a star, not the cross -- nt over the tile and group
    edges (and k itself: every row is a neighbour) at two query counts, nq over the block edges at
    two train sizes."""
    bm = bm or 256
    out = [(nt, nq) for nt in sorted({k, *NT_STAR, *extra_nt}) if nt >= k for nq in (33, bm + 1)]
    out += [(nt, nq) for nq in sorted({1, 31, 32, 33, bm - 1, bm, bm + 1, NQ_MAX}) if nq <= NQ_MAX
            for nt in (max(k, 257), NT_MAX)]
    return list(dict.fromkeys(out))


def split_sizes(k, bm):
    """The two sizes of a plan that also run with forced train_splits (3 and 8 pieces: at 257 rows
    a piece holds 64 rows or none, fewer than k from k = 65 up)."""
    return [(max(k, 257), 33), (NT_MAX, (bm or 256) + 1)]


def lattice():
    """The cases of tests/test_gpu_plan_lattice.py, grouped by plan range: a list of dicts
    {name, dtype, algo, d, hooks, lo, hi, plan, cases: [{k, form, bm, qg, i8, bn, extra_nt}]}.  A
    (class, d, plan, k) that several hook settings reach runs under the first of them."""
    seen, groups = set(), []
    for name, dtype, algo, ds, _ in CLASSES:
        for d in ds:
            for hooks in hooks_of(name, d):
                for lo, hi, plan, info in walk(name, d, hooks):
                    cases = []
                    for k in dict.fromkeys((lo, hi)):
                        if (name, d, plan, k) in seen:
                            continue
                        seen.add((name, d, plan, k))
                        c = dict(info[k], k=k, extra_nt=())
                        if c["i8"]:
                            # both sides of the seed pass's first sampled size
                            first = first_seeded(c["bn"])
                            c["extra_nt"] = (first - 1, first)
                        cases.append(c)
                    if cases:
                        groups.append({"name": name, "dtype": dtype, "algo": algo, "d": d, "hooks": hooks, "lo": lo,
                                       "hi": hi, "plan": plan, "cases": cases})
    return groups


def group_id(g):
    h = "".join(f"-{n}{v}" for n, v in g["hooks"].items())
    return f"{g['name']}-d{g['d']}{h}-k{g['lo']}_{g['hi']}"


# -----------------------------------------------------------------------------------------
# the data of the GPU lattice (shared, so the CPU test below pins the reference's properties)
# -----------------------------------------------------------------------------------------
def base_rows(oracle, d, bf16):
    """The generated set of one (d, dtype): 1,025 train rows, their labels and 513 queries (kind 1:
    every value is exact in bf16, so the oracle runs on the widened floats)."""
    tr, tl = oracle.gen(SEED + d, 0, 0, NT_MAX, d, kind=1 if bf16 else 0, C=C)
    te, _ = oracle.gen(SEED + d, 1, 0, NQ_MAX, d, kind=1 if bf16 else 0, C=C)
    return tr, tl, te


def prefix_rows(base, nt, dups):
    """(train, labels, test) of the prefix of nt rows.  dups: exact copies across tile edges --
    rows 31..33 and 63..65 are rows 0..5, the last three rows are the first three, and every fourth
    query is a train row."""
    tr, tl, te = base
    tr, tl = tr[:nt], tl[:nt]
    if not dups:
        return tr, tl, te
    tr, te = tr.copy(), te.copy()
    for dst, src in ((31, 0), (63, 3)):
        n = max(0, min(3, nt - dst))
        tr[dst:dst + n] = tr[src:src + n]
    if nt >= 6:
        tr[nt - 3:] = tr[:3]
    q4 = np.arange(0, len(te), 4)
    te[q4] = tr[(7 * q4 + 1) % nt]
    return tr, tl, te


def reference(oracle, tr, tl, te, kmax=K_LAST):
    """One oracle call at min(nt, kmax) neighbours for every query: (dist bits, idx).  The lists of
    a smaller k and of the first nq queries are prefixes of these (test_reference_prefixes)."""
    kk = min(len(tr), kmax)
    bad, _, dist, idx = oracle.knn(tr, tl, te, kk, C)
    assert bad == 0
    return dist.view(np.uint32), idx


def votes(idx, labels, num_classes=C):
    """vote_reference (test_metric_cpu.py: bincount argmax, ties to the smallest label) for all
    lists in one bincount -- the lattice votes on some ten thousand lists; test_votes_restatement
    pins it to vote_reference."""
    idx = np.asarray(idx)
    nq = len(idx)
    lab = labels[idx].astype(np.int64) + num_classes * np.arange(nq, dtype=np.int64)[:, None]
    counts = np.bincount(lab.ravel(), minlength=nq * num_classes).reshape(nq, num_classes)
    return np.argmax(counts, axis=1).astype(np.int32)


def expected(ref, tl, k, nq):
    """(pred, dist bits, idx) of the first nq queries at k neighbours, from reference()'s lists."""
    dist, idx = ref[0][:nq, :k], ref[1][:nq, :k]
    return votes(idx, tl), dist, idx


# -----------------------------------------------------------------------------------------
# tests
# -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def groups():
    return lattice()


def test_hooks_answer_like_their_rules(knn):
    lib = _lib()
    out = np.zeros(8, np.int64)
    for bad in ((-1, 256, 10), (4, 256, 10), (0, 100, 10), (0, 256, 0)):
        assert lib.knn_debug_gemm_filter_plan(*bad, out.ctypes.data) == -1
    assert lib.knn_debug_gemm_filter_plan(0, 256, 10, None) == -1
    assert lib.knn_debug_wide_plan(0, out.ctypes.data) == -1 and lib.knn_debug_wide_plan(10, None) == -1
    # the hooks stay out of the public header
    with open(os.path.join(os.path.dirname(PKG_DIR), "include", "knn_amd.h")) as f:
        src = f.read()
    assert "knn_debug_gemm_filter_plan" not in src and "knn_debug_wide_plan" not in src
    for k in (1, 64, 65, 128):
        w = wide_plan(k)
        # the GPU file's wide shapes are the edges of these two numbers
        assert (w["nw"], w["qg"], w["rg"], w["bm"], w["group_rows"]) == (8, 1, 1, 256, 256) and w["lds"] <= 160 * 1024
    # the rounded operands run the bf16 kernel: one plan (elem 3 = ELEM_ROUND)
    for k in (1, 90, 128):
        assert filter_plan(3, 512, k) == filter_plan(ELEM_BF16, 512, k)
    # wherever the policy sends a size to k_gemm_filter its plan fits the LDS, blocks hold 32 queries
    # per wave and the tile is 32 or 64 rows
    for name, dtype, algo, ds, elem in CLASSES:
        for d in ds:
            for k in range(1, 129):
                if knn.filter_policy(dtype, d, k, NT_MAX, NQ_MAX, algo)[0] == "filter":
                    f = filter_plan(elem, 4 * d if name in ("fp32", "split") else 2 * d, k)
                    assert f["lds"] <= 160 * 1024 and f["bm"] == 32 * f["nw"] and f["rg"] in (1, 2) and f["nbuf"] == 2, f


def test_votes_restatement():
    rng = np.random.default_rng(5)
    for nq, nt, k, classes in ((1, 1, 1, 10), (33, 7, 7, 3), (257, 1000, 129, 10), (9, 4096, 1024, 10), (40, 50, 2, 10)):
        labels = rng.integers(0, classes, size=nt).astype(np.int32)
        idx = np.array([rng.permutation(nt)[:k] for _ in range(nq)], np.int32)
        got = votes(idx, labels, classes)
        assert got.dtype == np.int32 and np.array_equal(got, vote_reference(idx, labels, classes))
    # ties go to the smallest label
    assert votes(np.array([[0, 1, 2, 3]]), np.array([7, 2, 7, 2], np.int32)).tolist() == [2]


def test_one_row_view_keeps_its_pitch(knn):
    """The lattice runs one query (nq = 1) and one train row (k = nt = 1) of d = 257 floats: a
    one-row column view of padded rows has the table's pitch, like a view of two rows -- it was
    given the view's width (257 floats: not 16-byte rows) and refused.  A one-row tensor whose
    stride is shorter than its row keeps the row's width."""
    import torch
    table = torch.zeros((4, 264), dtype=torch.float32)
    for n in (1, 2, 4):
        ds = knn._device_dataset(table[:n, :257])
        assert (ds.n, ds.d, ds.ld) == (n, 257, 264)
    assert knn._device_dataset(table[:1]).ld == 264 and knn._device_dataset(table[:1], d=257).d == 257
    odd = torch.zeros(264, dtype=torch.float32).as_strided((1, 264), (1, 1))
    assert knn._device_dataset(odd).ld == 264


def test_list_classes():
    assert list_classes() == (64, 128, 256, 512, 1024)
    assert [list_regs(k) for k in (1, 64, 65, 128, 129, 1024)] == [0, 0, 1, 1, 2, 4]


def test_ranges_cover_and_have_both_ends(groups):
    """Every plan the walk finds -- under every hook setting -- has a lattice case at each end of
    its range; the ranges are contiguous and cover 1..128, then the direct form at 129; every fused
    plan has its kernel."""
    have = {(g["name"], g["d"], g["plan"], c["k"]) for g in groups for c in g["cases"]}
    assert len(have) == sum(len(g["cases"]) for g in groups)
    plans = set()
    for name, _, _, ds, _ in CLASSES:
        for d in ds:
            for hooks in hooks_of(name, d):
                runs = walk(name, d, hooks)
                assert runs[0][0] == 1 and runs[-1][:2] == (K_LAST, K_LAST) and runs[-1][2][0] == "direct"
                assert runs[-2][1] == 128 and runs[-2][2][0] != "direct"
                for a, b in zip(runs, runs[1:]):
                    assert b[0] == a[1] + 1
                for lo, hi, plan, info in runs:
                    plans.add((name, d, plan))
                    assert (name, d, plan, lo) in have and (name, d, plan, hi) in have, (name, d, hooks, lo, hi, plan)
                    if plan[0] == "fused":
                        assert all(i["has_kernel"] == 1 for i in info.values()), (name, d, hooks, lo, hi)
                    assert all(i["lds"] <= 160 * 1024 for i in info.values())
    assert {p for p in plans} == {(g["name"], g["d"], g["plan"]) for g in groups}
    print(f"{len(groups)} plan ranges, {len(have)} (plan, k) cases, "
          f"{sum(len(star(c['k'], c['bm'], c['extra_nt'])) for g in groups for c in g['cases'])} star sizes")


def _describe(plan):
    if plan[0] == "direct":
        return "direct form"
    if plan[0] == "fused":
        nw, qg, rg, _, nbuf, _, kr, ls, i8, park, regs = plan[1:]
        return (f"k_gemm_fused (nw {nw}, qg {qg}, rg {rg}, nbuf {nbuf}, kr {kr}"
                f"{', list exchange' if ls else ''}{', int8' if i8 else ''}"
                f"{'' if park is None else f', park {park}'}), list regs {regs + 1}")
    rb, nw, qg, rg, minw, nbuf, _, regs = plan[1:]
    return f"k_gemm_filter ({rb}-byte rows, nw {nw}, qg {qg}, rg {rg}, minw {minw}, nbuf {nbuf}), list regs {regs + 1}"


# DESIGN.md "Testing": the ranges the library reports, as (class, d, hooks) -> the last k of every
# range.  A rule that changes fails here first; correct both tables from this test's output.
DOCUMENTED = {
    # k_gemm_filter on the caller's fp32 rows / their [hi | lo] split: (class, d)
    ("fp32", 32): (64, 117, 128, 129),
    ("fp32", 64): (64, 85, 128, 129),
    ("fp32", 128): (21, 64, 128, 129),
    ("split", 32): (64, 117, 128, 129),
    ("split", 64): (64, 121, 128, 129),
    ("split", 128): (64, 89, 121, 128, 129),
    # the bf16 operands: (class, d, KNN_FUSED_QG, KNN_FUSED_HEAPS)
    **{(name, 64, qg, 0): (16, 32, 64, 113, 128, 129) for name in ("rounded", "bf16") for qg in (1, 2)},
    **{(name, 128, qg, 0): (16, 32, 64, 81, 117, 128, 129) for name in ("rounded", "bf16") for qg in (1, 2)},
    **{(name, 256, qg, 0): (16, 32, 64, 104, 121, 128, 129) for name in ("rounded", "bf16") for qg in (1, 2)},
    **{(name, 256, qg, 1): (16, 32, 64, 85, 121, 128, 129) for name in ("rounded", "bf16") for qg in (1, 2)},
    # the int8 operands (k <= 32), the bf16 ones above: (class, d, KNN_FUSED_QG, KNN_FUSED_HEAPS, KNN_FUSED_PARK)
    **{("int8", 128, qg, 0, park): (16, 32, 64, 81, 117, 128, 129) for qg in (1, 2) for park in (0, 1)},
}


def test_ranges_are_the_documented_ones():
    got = {}
    for name, _, _, ds, _ in CLASSES:
        for d in ds:
            for hooks in hooks_of(name, d):
                runs = walk(name, d, hooks)
                key = (name, d) + tuple(hooks.values())
                got[key] = tuple(hi for _, hi, _, _ in runs)
                print(f"{name} d={d} {hooks or ''}")
                for lo, hi, plan, info in runs:
                    print(f"    k {lo:3d}..{hi:3d}  {_describe(plan)}, LDS {info[lo]['lds']}..{info[hi]['lds']}")
    print(f"seed pass: first sampled train size {first_seeded(64)} (64-row tile blocks), {first_seeded(32)} (32-row)")
    assert got == DOCUMENTED


def test_star_sizes():
    for k, bm in ((1, 128), (33, 256), (128, 512), (129, 0)):
        s = star(k, bm, (448, 449) if k == 1 else ())
        bm = bm or 256
        assert len(s) == len(set(s)) and all(nt >= k and 1 <= nq <= NQ_MAX and nt <= NT_MAX for nt, nq in s)
        nts, nqs = {nt for nt, _ in s}, {nq for _, nq in s}
        assert k in nts and NT_MAX in nts and {n for n in NT_STAR if n >= k} <= nts
        assert {1, 31, 32, 33, bm - 1, bm, bm + 1} <= nqs | {n for n in (bm, bm + 1) if n > NQ_MAX}
        assert all((nt, nq) in s for nt, nq in split_sizes(k, bm))
        if k == 1:
            assert {448, 449} <= nts
    # the seed pass's first sampled sizes lie inside the star's range, above the 300-row size
    assert 300 < first_seeded(64) < first_seeded(32) < 511
    assert seed_tiles(first_seeded(64) - 1, 64) == 0 and seed_tiles(first_seeded(32) - 1, 32) == 0


@pytest.mark.parametrize("d,bf16", [(32, False), (64, True)])
def test_reference_prefixes(oracle, d, bf16):
    """The GPU file calls the oracle once per train prefix, at min(nt, 129) neighbours and all 513
    queries: a smaller k is a prefix of those lists, fewer queries a prefix of those rows, and the
    vote restatement on the prefix is the oracle's own prediction."""
    base = base_rows(oracle, d, bf16)
    if bf16:
        u = base[0].view(np.uint32)
        assert not (u & 0xFFFF).any()                      # exact in bf16
    for nt, dups in ((300, False), (66, True), (5, True)):
        tr, tl, te = prefix_rows(base, nt, dups)
        if dups:
            assert nt < 34 or np.array_equal(tr[31:34], tr[0:3])
            assert nt < 6 or np.array_equal(tr[nt - 3:], tr[:3])
            assert all((te[q] == tr).all(axis=1).any() for q in range(0, NQ_MAX, 4))
        ref = reference(oracle, tr, tl, te)
        assert ref[0].shape == (NQ_MAX, min(nt, K_LAST))
        for k, nq in ((1, 1), (min(nt, 17), 33), (min(nt, 128), 513), (nt if nt < K_LAST else 65, 257)):
            bad, pred, dist, idx = oracle.knn(tr, tl, te[:nq], k, C)
            assert bad == 0
            epred, edist, eidx = expected(ref, tl, k, nq)
            assert np.array_equal(idx, eidx) and np.array_equal(dist.view(np.uint32), edist) and np.array_equal(pred, epred)
