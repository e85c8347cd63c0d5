"""GPU: tools/run_sequence.py --save-map / --load-map — the map of a synthetic drive written as .npy files, imported by a second run and used to
localise the same sweeps without updating it."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_save_map_then_localize_against_the_loaded_map(tmp_path):
    kio = importlib.import_module("vloam_amd.kitti_io")
    n = 4
    drive = ["--synthetic", str(n), "--azimuth", "256", "--mapping-skip-frame", "1"]
    tool = [sys.executable, os.path.join(ROOT, "tools", "run_sequence.py")]
    r = subprocess.run(tool + drive + ["--out", str(tmp_path / "a"), "--save-map", str(tmp_path / "map")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    corner, surf = np.load(tmp_path / "map" / "corner.npy"), np.load(tmp_path / "map" / "surf.npy")
    assert corner.dtype == surf.dtype == np.float32 and corner.shape[1] == surf.shape[1] == 4 and corner.shape[0] > 1000 and surf.shape[0] > 500
    pose = [float(v) for v in open(tmp_path / "map" / "start_pose.txt").read().split()]
    mo = kio.read_trajectory(tmp_path / "a" / "MO0.txt")
    assert len(pose) == 7 and abs(np.linalg.norm(pose[:4]) - 1.0) < 1e-9 and mo.shape == (n, 4, 4)
    # the same sweeps against the imported map, from the map's origin: one row per sweep, every one solved, the map untouched
    r = subprocess.run(tool + drive + ["--out", str(tmp_path / "b"), "--load-map", str(tmp_path / "map"), "--start-pose", "0 0 0 1 0 0 0", "--localize-only"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"imported (\d+) corner / (\d+) surf map points", r.stdout)
    assert m and 0 < int(m.group(1)) <= corner.shape[0] and 0 < int(m.group(2)) <= surf.shape[0], r.stdout   # (a centroid on a voxel face may merge with its neighbour: tests/test_gpu_voxel_faces.py keys such points)
    m = re.search(r"localised (\d+) sweeps against the imported map \((\d+) solved\)", r.stdout)
    assert m and int(m.group(1)) == n and int(m.group(2)) == n, r.stdout
    loc = kio.read_trajectory(tmp_path / "b" / "LOC0.txt")
    assert loc.shape == (n, 4, 4) and not (tmp_path / "b" / "MO0.txt").exists()
    assert np.isfinite(loc).all()
