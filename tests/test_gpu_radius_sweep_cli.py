"""The CLI's --radii= flag (KNN_radius_sweep / KNN_radius_sweep_loo): the radius classifier's line
once per radius, equal to the --radius= lines of the same radii one by one, and its refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DATA, PKG_DIR

EXE = os.path.join(PKG_DIR, "knn_cli")
RADII = ["3", "0.5", "2", "2", "1"]                                  # unsorted, one doubled
TIME = re.compile(r"required \d+ ms")


def _run(flags, tmp_path, name):
    out = tmp_path / name
    r = subprocess.run([EXE, f"{DATA}/medium-train.arff", f"{DATA}/medium-test.arff", "5", "--outlier=-3", *flags],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, KNN_CLI_PRED_OUT=str(out)))
    assert r.returncode == 0, r.stderr
    return [TIME.sub("required N ms", l) for l in r.stdout.strip().split("\n")], out.read_text()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [(), ("--metric=manhattan", "--weights=distance"), ("--weights=sqdist",),
                                   ("--sweep=loo",)])
def test_radii_lines_equal_radius_lines(tmp_path, flags):
    lines, preds = _run([f"--radii={','.join(RADII)}", *flags], tmp_path, "sweep.txt")
    order = sorted(RADII, key=float)
    assert len(lines) == len(order)
    rows = preds.strip().split("\n")
    seen = set()
    for r, line, row in zip(order, lines, rows):
        single, spred = _run([f"--radius={r}", *flags], tmp_path, "single.txt")
        assert [line] == single, (r, flags)
        assert np.array_equal(np.array(row.split(), np.int32), np.array(spred.split(), np.int32)), (r, flags)
        seen.add(line)
    assert len(seen) >= 3                                            # the radii tell the rows apart


def test_radii_refusals():
    base = [EXE, f"{DATA}/small-train.arff", f"{DATA}/small-test.arff", "5"]
    many = ",".join(["1"] * 33)
    for flags in (["--radii=0.5,1", "--regress"], ["--radii=0.5,1", "--radius=1"], ["--radii=0.5,1", "--sweep"],
                  [f"--radii={many}"], ["--radii=abc"], ["--radii=1,-1"], ["--radii=0.5x"], ["--radii="],
                  ["--radii=1,,2"], ["--radii=1,"], ["--radii=nan"]):
        r = subprocess.run(base + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "radii" in r.stderr and r.stdout == "", (flags, r.returncode, r.stderr)
