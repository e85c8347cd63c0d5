"""-m gpu: tools/run_sequence.py --merge-map — two short synthetic drives become one map.  The first run saves its map (--save-map); the second
maps another drive and folds the first run's map into its own under a known --merge-pose before it saves.  The saved map must be the model's
merge (tests/map_merge_model.py) of the first map into what the second run saves without the merge, bit for bit, and the result record must
stand in the metrics file.  These maps were not built to keep off voxel faces, so the model keys with the device's own f32 arithmetic
(voxel_key_model.voxel_index)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import map_merge_model as mm
from voxel_key_model import CEN0, voxel_index

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF = (0.4, 0.8)   # the tool's default handle: mapping_line_resolution / mapping_plane_resolution


def test_two_drives_one_map(tmp_path):
    tool = [sys.executable, os.path.join(ROOT, "tools", "run_sequence.py"), "--azimuth", "512"]
    d1, d2, d2m, dry = (str(tmp_path / n) for n in ("map1", "map2", "map2_merged", "map2_dry"))
    pose = list(mm.quat_yaw_roll(10.0, 1.0)) + [3.0, -2.0, 0.1]
    arg = " ".join("%.17g" % v for v in pose)

    def run(*args):
        r = subprocess.run(tool + list(args), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    run("--synthetic", "3", "--out", str(tmp_path / "o1"), "--save-map", d1)
    run("--synthetic", "4", "--out", str(tmp_path / "o2"), "--save-map", d2)
    metrics = str(tmp_path / "m.jsonl")
    out = run("--synthetic", "4", "--out", str(tmp_path / "o3"), "--merge-map", d1, "--merge-pose", arg, "--save-map", d2m, "--metrics", metrics)
    assert "merged " + d1 in out
    rec = json.loads(open(metrics).read().splitlines()[-1])["map_merge"]
    assert rec["apply"] is True and rec["pose"] == pose
    for k, name in enumerate(("corner.npy", "surf.npy")):
        first, own, got = (np.load(os.path.join(d, name)) for d in (d1, d2, d2m))
        assert first.shape[0] > 300 and own.shape[0] > first.shape[0]
        want = mm.merge(own, first, LEAF[k], cen=CEN0, q=pose[:4], t=pose[4:], index=voxel_index)
        assert got.shape == want["cloud"].shape and got.tobytes() == want["cloud"].tobytes(), name
        for f, v in want["res"].items():
            assert rec[f][k] == v, (name, f, rec[f], v)
        assert rec["n_hit_points"][k] > 0 and rec["n_new_points"][k] > 0 and rec["n_skipped_raw"][k] == 0
    # the trajectories are those of the run that did not merge, and a dry run saves the un-merged map
    for name in ("LO0.txt", "MO0.txt"):
        assert open(str(tmp_path / "o2" / name)).read() == open(str(tmp_path / "o3" / name)).read(), name
    out = run("--synthetic", "4", "--out", str(tmp_path / "o4"), "--merge-map", d1, "--merge-pose", arg, "--merge-dry-run", "--save-map", dry)
    assert "would merge " + d1 in out
    for name in ("corner.npy", "surf.npy"):
        assert np.load(os.path.join(dry, name)).tobytes() == np.load(os.path.join(d2, name)).tobytes(), name
