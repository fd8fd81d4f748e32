"""The CLI's --mst[=M] [--mst-cuts=R1,R2,...] flag (KNN_mst, KNN_mst_cut) on a synthetic ARFF pair the
test writes: the tree's line and one DBSCAN* line per cut against test_mst_cpu's restatement, the
dumped labels against it and against --dbscan='s labels on the core rows; every refusal exits 1."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR
from test_dbscan_cpu import EUCLIDEAN, MANHATTAN, dbscan_set
from test_metric_cpu import metric_distances
from test_mst_cpu import mst_cut, mst_reference

EXE = os.path.join(PKG_DIR, "knn_cli")
TREE = re.compile(r"^The mutual-reachability spanning tree \(min_samples (\d+)\) of (\S+) has (\d+) edges in (\d+) "
                  r"components, longest (\S+)$")
CUT = re.compile(r"^The radius-(\S+) DBSCAN\* \(min_samples (\d+)\) of (\S+) found (\d+) clusters: (\d+) core rows, "
                 r"(\d+) other rows \(border rows are not assigned\)$")
CUTS = ("0.25", "0.5", "0.5", "1", "3")


def _write_arff(path, X):
    with open(path, "w") as f:
        f.write("@relation r\n" + "".join(f"@attribute a{i} numeric\n" for i in range(X.shape[1])))
        f.write("@attribute class numeric\n@data\n")
        for row in X:
            f.write(",".join("%.9g" % v for v in row) + ",0\n")


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """(train path, test path, rows): 300 lattice rows in three features, so the tree has ties
    everywhere; the test file holds other rows and is never read."""
    d = tmp_path_factory.mktemp("mst_cli")
    X = dbscan_set(300, 3)
    _write_arff(d / "train.arff", X)
    _write_arff(d / "test.arff", dbscan_set(20, 3, seed=99))
    return str(d / "train.arff"), str(d / "test.arff"), X


def _cli(pair, flags, out=None):
    env = dict(os.environ)
    env.pop("KNN_AMD_METRIC", None)
    if out is not None:
        env["KNN_CLI_PRED_OUT"] = str(out)
    return subprocess.run([EXE, pair[0], pair[1], "5", *flags], capture_output=True, text=True, timeout=120, env=env)


@pytest.mark.gpu
@pytest.mark.parametrize("m,metric,extra", [(5, EUCLIDEAN, ()), (3, MANHATTAN, ("--metric=manhattan",))])
def test_report_lines(pair, tmp_path, m, metric, extra):
    X = pair[2]
    n = len(X)
    D = metric_distances(X, X, metric)
    w, a, b, core, summary = mst_reference(D, m)
    radii = np.array([float(c) for c in CUTS], np.float32)
    thr = radii * radii if metric == EUCLIDEAN else radii
    ref_labels, ref_summary = mst_cut(w, a, b, core, thr, n)
    out = tmp_path / "labels.txt"
    run = _cli(pair, [f"--mst={m}" if m != 5 else "--mst", "--mst-cuts=" + ",".join(CUTS), *extra], out)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().split("\n")
    assert len(lines) == 1 + len(CUTS)
    t = TREE.match(lines[0])
    longest = np.sqrt(w[-1]) if metric == EUCLIDEAN else w[-1]
    assert t and t.groups() == (str(m), pair[0], str(n - 1), "1", "%g" % float(np.float32(longest))), lines[0]
    labels = [np.array(row.split(), np.int32) for row in out.read_text().strip().split("\n")]
    for r, cut in enumerate(CUTS):
        c = CUT.match(lines[1 + r])
        assert c and c.groups() == (cut, str(m), pair[0], *[str(v) for v in ref_summary[r]]), lines[1 + r]
        assert np.array_equal(labels[r], ref_labels[r]), cut
        # --dbscan= at the same radius: the same clusters and core rows, the same labels on the core rows
        one = tmp_path / f"one{r}.txt"
        d = _cli(pair, [f"--dbscan={cut}", f"--min-samples={m}", *extra], one)
        assert d.returncode == 0, d.stderr
        found = re.search(r"found (\d+) clusters: (\d+) core,", d.stdout)
        assert found and found.groups() == (str(ref_summary[r, 0]), str(ref_summary[r, 1])), d.stdout
        dl = np.array(one.read_text().split(), np.int32)
        assert np.array_equal(labels[r][labels[r] >= 0], dl[labels[r] >= 0])
    assert ref_summary[:, 0].max() >= 3 and len({tuple(s) for s in ref_summary.tolist()}) >= 3  # the cuts differ
    # the tree alone
    alone = _cli(pair, [f"--mst={m}", *extra])
    assert alone.returncode == 0 and alone.stdout.strip() == lines[0]


# the CLI refuses a bad --mst before it creates a context: no GPU is needed
@pytest.mark.parametrize("extra", [
    ["--mst=0"], ["--mst=257"], ["--mst=x"], ["--mst="], ["--mst=3.5"], ["--mst-cuts=1,2"], ["--mst", "--mst-cuts="],
    ["--mst", "--mst-cuts=2,1"], ["--mst", "--mst-cuts=1,x"], ["--mst", "--mst-cuts=-1"], ["--mst", "--mst-cuts=nan"],
    ["--mst", "--mst-cuts=" + ",".join(["1"] * 33)], ["--mst", "--min-samples=3"], ["--mst", "--dbscan=1"],
    ["--mst", "--dbscan-radii=1,2"], ["--mst", "--lof"], ["--mst", "--lof-threshold=2"], ["--mst", "--sweep"],
    ["--mst", "--sweep=loo"], ["--mst", "--regress"], ["--mst", "--radius=2"], ["--mst", "--radii=1,2"],
    ["--mst", "--weights=distance"], ["--mst", "--outlier=3"]])
def test_cli_refuses(pair, extra):
    r = _cli(pair, extra)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    assert "usage: --mst[=M]" in r.stderr and r.stdout == ""
