"""-m gpu: the stream plan of a handle (csrc/stream_plan.h) under the runtime's default pool of 4 hardware queues and under 16.  With 4 the
stage streams are created at three priority levels (one hardware-queue pool each), with 16 all at normal priority; the results must not
notice.  Every run is a child process of its own with GPU_MAX_HW_QUEUES set explicitly (the runtime reads it once, when it initialises):
  - 40 sweeps of 64 x 2048 with mapping, as device pointers, stage by stage, from host memory only (the copy stream is created by the first
    vloam_process_scan) and host / device mixed;
  - a batch of 4 sessions (different sequences).
Trajectory, whole map and feature clouds are bit-identical between the two budgets and between the entry points."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_SWEEPS, N_BATCH_SWEEPS, B = 40, 16, 4


def _results(h):
    h.sync()
    out = {"traj": h.trajectory().copy(), "map": h.get_map().view(np.uint32).copy()}
    for w in (0, 2, 4, 7, 8):
        out["feat%d" % w] = h.features(w).view(np.uint32).copy()
    return out


def _child(inp, out_path):
    """Runs in a fresh process (GPU_MAX_HW_QUEUES set by the parent)."""
    sys.path.insert(0, HERE)
    import conftest
    vl = conftest.load_pkg()
    import torch
    data = np.load(inp)
    sweeps, small = data["sweeps"], data["small"]
    n_pts = sweeps.shape[1]
    dev = torch.from_numpy(sweeps).cuda()
    stride = n_pts * 16
    res = {}

    def handle(**kw):
        return vl.Handle(0, with_mapping=1, max_points=max(n_pts, 1024), max_frames=N_SWEEPS + 8, **kw)

    h = handle()
    for k in range(N_SWEEPS):
        h.process_scan_device(dev.data_ptr() + k * stride, n_pts)
    for key, v in _results(h).items():
        res["device_" + key] = v
    h.close()

    h = handle()
    for k in range(N_SWEEPS):
        h.reset_frame()
        h.scan_registration(sweeps[k])
        h.laser_odometry()
        h.laser_mapping()
    for key, v in _results(h).items():
        res["stagewise_" + key] = v
    h.close()

    h = handle()   # host memory from the first call on: the copy stream is opened by this handle's first deferred host sweep
    for k in range(N_SWEEPS):
        h.process_scan(sweeps[k])
    for key, v in _results(h).items():
        res["host_" + key] = v
    h.close()

    h = handle()
    for k in range(N_SWEEPS):
        if k % 3 == 1:
            h.process_scan_device(dev.data_ptr() + k * stride, n_pts)
        else:
            h.process_scan(sweeps[k])
    for key, v in _results(h).items():
        res["mixed_" + key] = v
    h.close()

    # a batch of B sessions
    ds = torch.from_numpy(small).cuda()
    ns = small.shape[2]
    hb = vl.Handle(0, n_sessions=B, with_mapping=1)
    for k in range(N_BATCH_SWEEPS):
        hb.batch_process_scan_device([ds[b, k].data_ptr() for b in range(B)], [ns] * B)
    hb.sync()
    for b in range(B):
        hb.select(b)
        res["batch%d_traj" % b] = hb.trajectory().copy()
        res["batch%d_map" % b] = hb.get_map().view(np.uint32).copy()
    hb.close()
    np.savez(out_path, **res)


@pytest.fixture(scope="module")
def runs(synth, tmp_path_factory):
    d = tmp_path_factory.mktemp("queue_budget")
    seq = synth.SynthSequence(n_rings=64, n_azimuth=2048, n_sweeps=N_SWEEPS + 1)
    sweeps = np.stack([seq.sweep(k) for k in range(N_SWEEPS)])
    small = []
    for b in range(B):
        sq = synth.SynthSequence(n_rings=64, n_azimuth=512, n_sweeps=N_BATCH_SWEEPS + 1, seed_scene=300 + 7 * b, seed_traj=301 + 7 * b, seed_noise=302 + 7 * b)
        small.append(np.stack([sq.sweep(k) for k in range(N_BATCH_SWEEPS)]))
    inp = str(d / "in.npz")
    np.savez(inp, sweeps=sweeps, small=np.stack(small))
    out = {}
    for q in (4, 16):
        path = str(d / ("q%d.npz" % q))
        env = dict(os.environ, GPU_MAX_HW_QUEUES=str(q))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), inp, path], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, "GPU_MAX_HW_QUEUES=%d: child exited with %d\n%s\n%s" % (q, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
        out[q] = (dict(np.load(path)), r.stderr)
    return out


def test_the_plan_follows_the_budget(runs):
    # 4 queues: the pooled plan (said once per process); 16: every stream at normal priority, nothing said
    assert "priority pools" in runs[4][1]
    assert "priority pools" not in runs[16][1]


@pytest.mark.parametrize("path", ["device", "stagewise", "host", "mixed"])
def test_sweeps_are_bit_identical_across_budgets_and_entry_points(runs, path):
    ref = runs[16][0]
    assert np.isfinite(ref["device_traj"]).all() and ref["device_map"].shape[0] > 1000
    for q in (4, 16):
        r = runs[q][0]
        for key in ("traj", "map", "feat0", "feat2", "feat4", "feat7", "feat8"):
            a, b = r["%s_%s" % (path, key)], ref["device_" + key]
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), "GPU_MAX_HW_QUEUES=%d %s: %s differs" % (q, path, key)


def test_batch_of_four_sessions_under_four_queues(runs):
    r4, r16 = runs[4][0], runs[16][0]
    for b in range(B):
        assert np.isfinite(r4["batch%d_traj" % b]).all() and r4["batch%d_map" % b].shape[0] > 100
        for key in ("traj", "map"):
            a, other = r4["batch%d_%s" % (b, key)], r16["batch%d_%s" % (b, key)]
            assert a.shape == other.shape and np.array_equal(a.view(np.uint8), other.view(np.uint8)), "session %d: %s" % (b, key)
    assert not np.array_equal(r4["batch0_traj"], r4["batch1_traj"]), "the sessions are different sequences"


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
