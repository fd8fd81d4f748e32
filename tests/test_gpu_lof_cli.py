"""The CLI's --lof[=KLO] flag (KNN_lof): one line per k in [KLO, K] with the count of train rows
whose local outlier factor is above --lof-threshold=T and the largest LOF with its row, equal to
Context.lof_device on the same file; and its refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA, PKG_DIR
from test_gpu_lof import _rows_dev
from test_regress_cpu import fbits

pytestmark = pytest.mark.gpu

EXE = os.path.join(PKG_DIR, "knn_cli")
LINE = re.compile(r"^The (\d+)-NN local outlier factor of (\d+) train instances required \d+ ms CPU time\. "
                  r"(\d+) rows above (\S+), largest (\S+) at row (-?\d+)$")


def _run(k, flags, tmp_path):
    out = tmp_path / "lof.txt"
    # (the test path is not read: it names no file)
    r = subprocess.run([EXE, f"{DATA}/small-train.arff", f"{DATA}/no-such-test.arff", str(k), *flags],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, KNN_CLI_PRED_OUT=str(out)))
    assert r.returncode == 0, r.stderr
    lines = [LINE.match(l) for l in r.stdout.strip().split("\n")]
    assert all(lines), r.stdout
    scores = np.array([row.split() for row in out.read_text().strip().split("\n")], np.float32)
    return [m.groups() for m in lines], scores


@pytest.mark.parametrize("k,flags,k_lo,thr,metric", [
    (7, ("--lof=3",), 3, 1.5, "euclidean"),
    (5, ("--lof",), 5, 1.5, "euclidean"),
    (6, ("--lof=2", "--lof-threshold=1.1", "--metric=manhattan"), 2, 1.1, "manhattan"),
])
def test_lof_lines_equal_python(knn, tmp_path, k, flags, k_lo, thr, metric):
    tf, _, _ = knn.read_arff(os.path.join(DATA, "small-train.arff"))
    c = knn.Context(0, metric=metric)
    try:
        lof = c.lof_device(_rows_dev(tf), k_lo, k).cpu().numpy()
    finally:
        c.close()
    lines, scores = _run(k, flags, tmp_path)
    assert np.array_equal(fbits(scores), fbits(lof))                 # (%.9g round-trips binary32)
    assert [int(g[0]) for g in lines] == list(range(k_lo, k + 1))
    counts = []
    for g, row in zip(lines, lof):
        assert int(g[1]) == len(tf) and float(g[3]) == thr
        assert int(g[2]) == int((row > np.float32(thr)).sum())
        assert int(g[5]) == int(np.argmax(row)) and g[4] == f"{row.max():.4f}"
        counts.append(int(g[2]))
    assert np.isfinite(lof).all() and 0 < max(counts) < len(tf)


def test_lof_refusals():
    base = [EXE, f"{DATA}/small-train.arff", f"{DATA}/small-test.arff", "5"]
    for flags in (["--lof", "--regress"], ["--lof", "--radius=1"], ["--lof", "--radii=0.5,1"],
                  ["--lof", "--weights=distance"], ["--lof", "--weights=uniform"], ["--lof", "--sweep"],
                  ["--lof", "--sweep=loo"], ["--lof=0"], ["--lof=6"], ["--lof=abc"], ["--lof=2x"], ["--lof="],
                  ["--lof", "--lof-threshold=abc"], ["--lof-threshold=1.5"]):
        r = subprocess.run(base + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--lof" in r.stderr and r.stdout == "", (flags, r.returncode, r.stderr)
    r = subprocess.run(base[:3] + ["256", "--lof"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--lof" in r.stderr and r.stdout == ""
