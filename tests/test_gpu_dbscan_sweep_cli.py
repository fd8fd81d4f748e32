"""The CLI's --dbscan-radii=R1,R2,... [--min-samples=M] flag (KNN_dbscan_sweep): --dbscan='s line
once per radius, each equal -- line and labels -- to what --dbscan= prints at that radius."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA, PKG_DIR
from test_gpu_dbscan_cli import LINE

pytestmark = pytest.mark.gpu

EXE = os.path.join(PKG_DIR, "knn_cli")


def _cli(flags, out):
    train = os.path.join(DATA, "small-train.arff")
    # (K and the test path keep their positions and are not read: the path names no file)
    run = subprocess.run([EXE, train, f"{DATA}/no-such-test.arff", "5", *flags], capture_output=True, text=True,
                         timeout=120, env=dict(os.environ, KNN_CLI_PRED_OUT=str(out)))
    assert run.returncode == 0, run.stderr
    return run.stdout.strip().split("\n"), out.read_text().strip().split("\n")


@pytest.mark.parametrize("radii,extra", [
    (("8", "12.5", "12.5", "15", "20"), ("--min-samples=3",)),
    (("6", "8", "20", "40"), ("--metric=manhattan",)),
])
def test_sweep_lines_equal_single_radius_lines(tmp_path, radii, extra):
    lines, labels = _cli(["--dbscan-radii=" + ",".join(radii), *extra], tmp_path / "sweep.txt")
    assert len(lines) == len(radii) == len(labels)
    clusters = []
    for r, radius in enumerate(radii):
        one, lab = _cli([f"--dbscan={radius}", *extra], tmp_path / f"one{r}.txt")
        assert len(one) == 1 and LINE.match(one[0]) and lines[r] == one[0], (radius, lines[r], one)
        assert np.array_equal(np.array(labels[r].split(), np.int32), np.array(lab, np.int32)), radius
        clusters.append(int(LINE.match(one[0]).group(4)))
    assert max(clusters) >= 10 and len(set(clusters)) >= 3  # the radii give different clusterings
