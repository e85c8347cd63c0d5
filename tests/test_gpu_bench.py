"""-m gpu: the single-GPU bench line as a plain run prints it (no --full: the headline and nothing else) and --dump-outputs DIR — what the
timed path computed in its last step, written as .npy; two runs with the same arguments write the same arrays, and the dumped poses are the
CPU oracle's for the same synthetic sweeps."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

MAP_WARMUP, WARMUP, STEPS = 6, 2, 3
DUMPED = ["cornerPointsLessSharp", "cornerPointsSharp", "laserCloud", "laserCloudMap", "laserCloudRegistered", "surfPointsFlat",
          "surfPointsLessFlat", "trajectory"]
FULL_ONLY = {"roofline", "kernels", "reference_timers", "cpu_baseline", "parity_vs_oracle", "configs1", "batched", "latency", "sustained",
             "host_input", "configs3", "configs3_from_images"}


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--map-warmup", str(MAP_WARMUP), "--synth-procs", "2", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs(tmp_path, synth, orc):
    runs = [_plain_run(tmp_path / name) for name in ("a", "b")]
    for d in runs:
        assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["n_gpus"] == 1 and d["unit"] == "scans/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f32 points / f64 poses+residuals" and d["config"]["map_warmup_sweeps"] == MAP_WARMUP
        assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-9 * d["value"]
        assert not FULL_ONLY & set(d), FULL_ONLY & set(d)
    got = {}
    for name in DUMPED:
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.ndim == 2 and a.shape[0] > 0, name
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), name   # same arguments, same outputs, bit for bit
        got[name] = a
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == [n + ".npy" for n in DUMPED]
    c = runs[0]["counts_last_sweep"]
    assert got["laserCloud"].shape == (c["N2"], 4) and got["cornerPointsLessSharp"].shape == (c["n_lessSharp"], 4)
    assert got["surfPointsLessFlat"].shape == (c["n_lessFlat"], 4)
    # the dumped poses of the timed sweeps are the oracle's for the bench's own sequence (rank 0's seeds, every sweep from the first)
    multi = importlib.import_module("vloam_amd.multi")
    T = MAP_WARMUP + WARMUP + STEPS
    seq = synth.SynthSequence(n_rings=64, n_azimuth=2048, n_sweeps=T, **multi.rank_sequence_seeds(0))
    o = orc.Oracle(scan_line=64, with_mapping=True)
    traj = got["trajectory"]
    assert traj.shape == (STEPS, 14) and traj.dtype == np.float64
    for k in range(T):
        assert o.process(seq.sweep(k)) == 0
        if k < MAP_WARMUP + WARMUP:
            continue
        row = traj[k - MAP_WARMUP - WARMUP]
        qw, tw, _, _ = o.lo_pose()
        qm, tm = o.map_published_pose()
        assert np.linalg.norm(row[4:7] - tw) < 1e-6 and min(np.linalg.norm(row[0:4] - qw), np.linalg.norm(row[0:4] + qw)) < 1e-6, k
        assert np.linalg.norm(row[11:14] - tm) < 1e-6 and min(np.linalg.norm(row[7:11] - qm), np.linalg.norm(row[7:11] + qm)) < 1e-6, k
