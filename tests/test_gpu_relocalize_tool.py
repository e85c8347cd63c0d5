"""GPU: tools/run_sequence.py --relocalize — the map of a synthetic drive saved, then the same sweeps localised against the loaded map from a
start pose that is 1.5 m, -1.0 m and 8 degrees of yaw off: the first sweep is relocalised on a grid around that pose, the rest follow from it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_STEP_T, HALF_STEP_YAW = 0.25, float(np.deg2rad(1.25))   # half a step of the grid below


def rows_of(path):
    return [json.loads(line) for line in open(path)]


def apart(a, b):
    """(metres, radians) between two poses (q xyzw, t)."""
    a, b = np.array(a), np.array(b)
    return float(np.linalg.norm(a[4:] - b[4:])), 2.0 * float(np.arccos(min(1.0, abs(np.dot(a[:4], b[:4])) / (np.linalg.norm(a[:4]) * np.linalg.norm(b[:4])))))


@pytest.mark.gpu
def test_relocalize_the_first_sweep_then_follow(tmp_path):
    n = 4
    drive = ["--synthetic", str(n), "--azimuth", "256", "--mapping-skip-frame", "1"]
    tool = [sys.executable, os.path.join(ROOT, "tools", "run_sequence.py")]
    run = lambda extra: subprocess.run(tool + drive + extra, capture_output=True, text=True, timeout=600)
    r = run(["--out", str(tmp_path / "a"), "--save-map", str(tmp_path / "map")])
    assert r.returncode == 0, r.stdout + r.stderr
    load = ["--load-map", str(tmp_path / "map"), "--localize-only"]
    # the exact start pose: sweep 0 was taken at the map's origin
    r = run(["--out", str(tmp_path / "b"), "--metrics", str(tmp_path / "b.jsonl"), "--start-pose", "0 0 0 1 0 0 0"] + load)
    assert r.returncode == 0, r.stdout + r.stderr
    exact = rows_of(tmp_path / "b.jsonl")
    assert len(exact) == n and all(row["flags"] & 1 for row in exact) and "relocalize" not in exact[0]
    # ... and one that is off by more than the scan-to-map association forgives
    a = np.deg2rad(8.0) / 2.0
    off = "0 0 %.17g %.17g 1.5 -1.0 0" % (np.sin(a), np.cos(a))
    r = run(["--out", str(tmp_path / "c"), "--metrics", str(tmp_path / "c.jsonl"), "--start-pose", off, "--relocalize", "2 0.5 10 2.5 4"] + load)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "relocalised sweep 0: candidate" in r.stdout and "localised %d sweeps against the imported map (%d solved)" % (n, n) in r.stdout, r.stdout
    got = rows_of(tmp_path / "c.jsonl")
    assert len(got) == n and all("relocalize" not in row for row in got[1:])
    blk = got[0]["relocalize"]
    assert blk["n_candidates"] == 9 * 9 * 9 and blk["n_refined"] == 4 and 0 <= blk["best"] < 4 and blk["candidate"] == blk["candidates"][blk["best"]]
    for key in ("coarse", "fine"):
        assert sorted(blk[key]) == ["n_hit", "n_used", "sum_d2_q24"] and sum(blk[key]["n_hit"]) > 0.5 * sum(blk[key]["n_used"]), blk[key]
    assert blk["refined_pose"] == got[0]["loc_pose"] and len(blk["guess"]) == 7
    # the grid point nearest the truth is (1, 6, 1): the winner is it or a direct neighbour
    ix, iy, iyaw = blk["candidate"] % 9, (blk["candidate"] // 9) % 9, blk["candidate"] // 81
    assert abs(ix - 1) <= 1 and abs(iy - 6) <= 1 and abs(iyaw - 1) <= 1, blk["candidate"]
    for k in range(n):   # the first row within half a grid step of the run that knew the start pose; the rows behind it follow from it
        dt, da = apart(got[k]["loc_pose"], exact[k]["loc_pose"])
        print("sweep %d: %.4f m, %.3f degrees from the run with the exact start pose" % (k, dt, np.rad2deg(da)))
        assert got[k]["flags"] & 1 and np.isfinite(got[k]["loc_pose"]).all()
        assert dt <= HALF_STEP_T and da <= HALF_STEP_YAW, (k, dt, da)
    assert os.path.exists(tmp_path / "c" / "LOC0.txt") and not os.path.exists(tmp_path / "c" / "MO0.txt")
    # without --localize-only the option is refused, and the message says what to do instead
    r = run(["--out", str(tmp_path / "d"), "--load-map", str(tmp_path / "map"), "--relocalize", "2 0.5 10 2.5"])
    assert r.returncode != 0 and "--localize-only" in r.stderr and "--load-map DIR --start-pose" in r.stderr, r.stderr
