"""The CLI's --dbscan=R [--min-samples=M] flag (KNN_dbscan): one line with the clusters and the
core, border and noise rows of the train file, equal to Context.dbscan_device on the same file (and
to test_dbscan_cpu's restatement); and its refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA, PKG_DIR
from test_dbscan_cpu import METRICS, dbscan_reference
from test_gpu_dbscan import _rows_dev
from test_metric_cpu import metric_distances

pytestmark = pytest.mark.gpu

EXE = os.path.join(PKG_DIR, "knn_cli")
LINE = re.compile(r"^The radius-(\S+) DBSCAN \(min_samples (\d+)\) of (\S+) found (\d+) clusters: (\d+) core, (\d+) border, "
                  r"(\d+) noise rows$")


@pytest.mark.parametrize("flags,radius,m,metric", [
    (("--dbscan=12.5",), 12.5, 5, 0),
    (("--dbscan=15", "--min-samples=3"), 15.0, 3, 0),
    (("--min-samples=5", "--dbscan=20", "--metric=manhattan"), 20.0, 5, 1),
    (("--dbscan=8", "--metric=chebyshev"), 8.0, 5, 2),
])
def test_dbscan_line_equals_python(knn, tmp_path, flags, radius, m, metric):
    train = os.path.join(DATA, "small-train.arff")
    tf, _, _ = knn.read_arff(train)
    r = np.float32(radius)
    ref = dbscan_reference(metric_distances(tf, tf, metric), r * r if metric == 0 else r, m)
    assert ref[2][0] >= 10 and ref[2][1] >= 100 and ref[2][3] >= 100
    c = knn.Context(0, metric=METRICS[metric])
    try:
        labels, _, summary = c.dbscan_device(_rows_dev(tf), radius=radius, min_samples=m)
        labels, summary = labels.cpu().numpy(), summary.cpu().numpy()
    finally:
        c.close()
    assert np.array_equal(labels, ref[0]) and np.array_equal(summary, ref[2])
    out = tmp_path / "labels.txt"
    # (K and the test path keep their positions and are not read: the path names no file)
    run = subprocess.run([EXE, train, f"{DATA}/no-such-test.arff", "5", *flags], capture_output=True, text=True,
                         timeout=120, env=dict(os.environ, KNN_CLI_PRED_OUT=str(out)))
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().split("\n")
    g = LINE.match(lines[0])
    assert len(lines) == 1 and g, run.stdout
    assert float(g.group(1)) == radius and int(g.group(2)) == m and g.group(3) == train
    assert [int(g.group(i)) for i in (4, 5, 6, 7)] == summary.tolist()
    assert np.array_equal(np.array(out.read_text().split(), np.int32), labels)


def test_dbscan_refusals():
    base = [EXE, f"{DATA}/small-train.arff", f"{DATA}/small-test.arff", "5"]
    for flags in (["--dbscan=1", "--regress"], ["--dbscan=1", "--radius=1"], ["--dbscan=1", "--radii=0.5,1"],
                  ["--dbscan=1", "--weights=distance"], ["--dbscan=1", "--weights=uniform"], ["--dbscan=1", "--sweep"],
                  ["--dbscan=1", "--sweep=loo"], ["--dbscan=1", "--lof"], ["--dbscan=1", "--lof=2"],
                  ["--dbscan=1", "--outlier=2"], ["--dbscan=-0.5"], ["--dbscan=abc"], ["--dbscan=2x"], ["--dbscan="],
                  ["--dbscan=nan"], ["--dbscan=1", "--min-samples=0"], ["--dbscan=1", "--min-samples=-3"],
                  ["--dbscan=1", "--min-samples=2.5"], ["--dbscan=1", "--min-samples="], ["--min-samples=4"]):
        r = subprocess.run(base + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--dbscan" in r.stderr and r.stdout == "", (flags, r.returncode, r.stderr)
