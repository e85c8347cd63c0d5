"""-m gpu: the opt-in long ring tier (vloam_config::max_ring_points > 4096, k_sr_ring_long) against the unmodified CPU oracle.

A default handle refuses scan lines of more than 4 096 points (test_gpu_scan_registration.py); a handle created with max_ring_points = N
processes lines of up to N points bit for bit like the reference, whose rings grow by push_back (scan_registration.cpp:266)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_scan_registration import FAR_RING, assert_grid_too_fine, check_cloud, far_stretch_cloud
from test_gpu_batch import same_poses
from test_gpu_launch_configs import LAUNCH, assert_map, assert_poses, oracle_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATURES = [(1, "sharp"), (2, "lessSharp"), (3, "flat"), (4, "lessFlat")]


def lines_over_4096(o):
    return np.count_nonzero(np.bincount(o.cloud(0)[:, 3].astype(np.int64), minlength=64) > 4096)


def check_features(h, o, what):
    check_cloud(h.features(0), o.cloud(0), "laserCloud " + what)
    for which, name in FEATURES:
        check_cloud(h.features(which), o.cloud(which), "%s %s" % (name, what))


def check_stagewise(h, o, cloud, what):
    """Every array of the parity hooks (debug = 1) and the five clouds, all four floats."""
    h.reset_frame()
    h.scan_registration(cloud)
    assert o.scan_registration(cloud) == 0
    d = h.sr_debug()
    check_features(h, o, what)
    start, end = o.sr_ints(3), o.sr_ints(4)
    cur_o, sort_o, lab_o, pick_o = o.sr_curvature(), o.sr_ints(0), o.sr_ints(2), o.sr_ints(1)
    for r in range(start.shape[0]):
        if end[r] - start[r] < 6:
            continue
        s, e = start[r], end[r]
        assert np.array_equal(d["curvature"][s:e].view(np.uint32), cur_o[s:e].view(np.uint32)), "%s: curvature ring %d" % (what, r)
        assert np.array_equal(d["sort"][s:e], sort_o[s:e]), "%s: sort order ring %d" % (what, r)
        assert np.array_equal(d["label"][s:e], lab_o[s:e]), "%s: labels ring %d" % (what, r)
        assert np.array_equal(d["picked"][s - 5:e + 6], pick_o[s - 5:e + 6]), "%s: picked ring %d" % (what, r)
    assert np.array_equal(d["sharpInd"], o.sr_ints(5)) and np.array_equal(d["lessSharpInd"], o.sr_ints(6)) and np.array_equal(d["flatInd"], o.sr_ints(7))


@pytest.mark.parametrize("n_az", [4300, 6250])
def test_long_rings_stage_by_stage(vl, orc, synth, n_az):
    h = vl.Handle(0, max_ring_points=8192, max_points=400000, debug=1, with_mapping=0)
    seq = synth.SynthSequence(n_rings=64, n_azimuth=n_az, n_sweeps=3)
    for k in (0, 2):
        o = orc.Oracle(with_mapping=False)
        check_stagewise(h, o, seq.sweep(k), "64 x %d sweep %d" % (n_az, k))
        assert lines_over_4096(o) > 10


def one_ring(n, radius=20.0, el_deg=-10.43, noise=0.0, seed=0):
    """A single scan line of n points (beam 35 of the HDL-64E table)."""
    az = -2 * np.pi * np.arange(n) / n
    rad = radius + noise * np.random.default_rng(seed).standard_normal(n)
    el = np.deg2rad(el_deg)
    c = np.zeros((n, 4), dtype=np.float32)
    c[:, 0], c[:, 1], c[:, 2] = rad * np.cos(el) * np.cos(az), rad * np.cos(el) * np.sin(az), rad * np.sin(el)
    return c


def test_ring_of_exactly_the_capacity_and_one_more(vl, orc):
    h = vl.Handle(0, max_ring_points=8192, debug=1, with_mapping=0)
    cloud = one_ring(8192, noise=0.05)
    o = orc.Oracle(with_mapping=False)
    check_stagewise(h, o, cloud, "8 192-point ring")
    assert o.cloud(0).shape[0] == 8192
    with pytest.raises(vl.VloamError) as ei:
        h.reset_frame()
        h.scan_registration(one_ring(8193, noise=0.05))
        h.laser_odometry()   # (the stage that reads the sweep's error word)
    assert ei.value.status == vl.ERR_CAPACITY and "8192" in str(ei.value)


def test_ring_of_exactly_the_long_tier_limit_and_one_more(vl, orc):
    """The top of the opt-in tier: a ring of exactly 16 384 points goes through (stage-wise against the oracle), one of 16 385 is refused."""
    h = vl.Handle(0, max_ring_points=16384, debug=1, with_mapping=0)
    cloud = one_ring(16384, noise=0.05)
    o = orc.Oracle(with_mapping=False)
    check_stagewise(h, o, cloud, "16 384-point ring")
    assert o.cloud(0).shape[0] == 16384
    with pytest.raises(vl.VloamError) as ei:
        h.reset_frame()
        h.scan_registration(one_ring(16385, noise=0.05))
        h.laser_odometry()   # (the stage that reads the sweep's error word)
    assert ei.value.status == vl.ERR_CAPACITY and "16384" in str(ei.value)


def test_voxel_grid_too_fine_for_a_long_ring_passes_its_candidates_through(vl, orc, synth):
    """The same guard of the per-ring VoxelGrid(0.2) in the long tier: the far-stretch cloud with 4 097 returns on its far ring, on a handle
    of the smallest ring capacity above 4 096."""
    cloud = far_stretch_cloud(synth, n_far_ring=4097)
    h = vl.Handle(0, scan_line=16, max_ring_points=4097, debug=1, with_mapping=0)
    h.reset_frame()
    h.scan_registration(cloud)
    o = orc.Oracle(scan_line=16, with_mapping=False)
    assert o.scan_registration(cloud) == 0
    assert np.bincount(o.cloud(0)[:, 3].astype(np.int64))[FAR_RING] == 4097
    assert_grid_too_fine(o, FAR_RING)
    check_features(h, o, "far stretch on a 4 097-point ring")


def test_long_rings_with_a_voxel_for_almost_every_point(vl, orc, synth):
    """Returns from 120 m lie 0.1 m apart at 7 500 columns and from 400 m 0.33 m: nearly every lessFlat point is a voxel of its own."""
    n_az = 7500
    el = np.deg2rad(synth.beam_elevations_deg(64))[:, None]
    az = (-2 * np.pi * np.arange(n_az) / n_az)[None, :]
    rad = 400.0 + 0.01 * np.random.default_rng(3).standard_normal((64, n_az))
    cloud = np.zeros((64, n_az, 4), dtype=np.float32)
    cloud[..., 0] = rad * np.cos(el) * np.cos(az)
    cloud[..., 1] = rad * np.cos(el) * np.sin(az)
    cloud[..., 2] = rad * np.sin(el)
    cloud = cloud.transpose(1, 0, 2).reshape(-1, 4).copy()
    h = vl.Handle(0, max_ring_points=8192, max_points=64 * n_az, debug=1, with_mapping=0)
    o = orc.Oracle(with_mapping=False)
    check_stagewise(h, o, cloud, "400 m rings")
    per_ring = np.bincount(o.cloud(4)[:, 3].astype(np.int64))
    assert per_ring.max() > 7000, per_ring.max()


def test_rings_jump_without_warning_while_streaming(vl, orc, synth):
    """~2 000-point rings, then ~6 000 from sweep 6 on, through vloam_process_scan: the host runs ahead of the kernels, so the first long
    sweeps reach the long tier's catch-all workgroup; every sweep is processed and the last one's features equal the oracle's."""
    plan = [2000] * 6 + [6000] * 4
    clouds = [synth.SynthSequence(n_rings=64, n_azimuth=n_az, n_sweeps=k + 1).sweep(k) for k, n_az in enumerate(plan)]
    h = vl.Handle(0, max_ring_points=8192, max_points=400000, with_mapping=0)
    for c in clouds:
        h.process_scan(c)
    h.sync()
    o = orc.Oracle(with_mapping=False)
    assert o.scan_registration(clouds[-1]) == 0
    assert lines_over_4096(o) > 10
    check_features(h, o, "last sweep")


def run_oracle(o, clouds):
    rows = []
    for c in clouds:
        assert o.process(c) == 0
        qw, tw, _, _ = o.lo_pose()
        qm, tm = o.map_published_pose()
        rows.append(np.concatenate([qw, tw, qm, tm]))
    return np.array(rows)


def test_hdl64e_drive_through_the_whole_pipeline(vl, orc, synth):
    seq = synth.SynthSequence(n_sweeps=31, sensor="hdl64e")
    clouds = [seq.sweep(k) for k in range(30)]
    with pytest.raises(vl.VloamError) as ei:   # a default handle still refuses the first sweep
        hd = vl.Handle(0, with_mapping=0)
        hd.scan_registration(clouds[0])
        hd.laser_odometry()
    assert ei.value.status == vl.ERR_CAPACITY and "4096" in str(ei.value)
    h = vl.Handle(0, max_ring_points=8192, with_mapping=1)
    for c in clouds:
        h.process_scan(c)
    h.sync()
    o = orc.Oracle(with_mapping=True)
    ref = run_oracle(o, clouds)
    assert lines_over_4096(o) >= 2
    assert_poses(h.trajectory(), ref, "hdl64e")
    assert_map(h, o, "hdl64e")


def test_hdl32_at_5hz(vl, orc, synth):
    """scan_line 32 at 4 500 firings per revolution (an HDL-32E at 5 Hz) with the HDL-32 launch file's parameters."""
    p = LAUNCH["HDL_32"][2]
    seq = synth.SynthSequence(n_rings=32, n_azimuth=4500, n_sweeps=17, speed=4.0)
    clouds = [seq.sweep(k) for k in range(16)]
    h = vl.Handle(0, scan_line=32, max_ring_points=8192, with_mapping=1, **p)
    for c in clouds:
        h.process_scan(c)
    h.sync()
    o = oracle_for(orc, "HDL_32")
    ref = run_oracle(o, clouds)
    assert lines_over_4096(o) >= 4
    assert_poses(h.trajectory(), ref, "HDL-32 at 5 Hz")
    assert_map(h, o, "HDL-32 at 5 Hz")


def test_batch_of_long_ring_sequences(vl, orc, synth):
    """Three sessions with different long-ring sequences: each session's clouds equal its single-session run bit for bit, its poses equal
    that run's to the solvers' round-off and the oracle's within the launch-config tolerance."""
    seqs = [synth.SynthSequence(n_rings=64, n_azimuth=4300, n_sweeps=7),
            synth.SynthSequence(n_sweeps=7, sensor="hdl64e"),
            synth.SynthSequence(n_rings=64, n_azimuth=6250, n_sweeps=7, seed_traj=7)]
    clouds = [[s.sweep(k) for k in range(6)] for s in seqs]
    hb = vl.Handle(0, n_sessions=3, max_ring_points=8192, max_points=400000, with_mapping=1)
    for k in range(6):
        hb.batch_process_scan([clouds[b][k] for b in range(3)])
    hb.sync()
    for b in range(3):
        hs = vl.Handle(0, max_ring_points=8192, max_points=400000, with_mapping=1)
        for c in clouds[b]:
            hs.process_scan(c)
        hs.sync()
        hb.select(b)
        assert same_poses(hb.trajectory(), hs.trajectory()), "session %d" % b   # (solver round-off, as in test_gpu_batch.py)
        for which in range(5):
            assert np.array_equal(hb.features(which).view(np.uint32), hs.features(which).view(np.uint32)), "session %d cloud %d" % (b, which)
        ref = run_oracle(orc.Oracle(with_mapping=True), clouds[b])
        assert_poses(hb.trajectory(), ref, "session %d" % b)
        hs.close()


def test_run_sequence_tool_with_the_hdl64e_model(vl, synth, tmp_path):
    import importlib
    kio = importlib.import_module("vloam_amd.kitti_io")
    out = tmp_path / "res"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_sequence.py"), "--synthetic", "8", "--sensor", "hdl64e",
                        "--max-ring-points", "8192", "--out", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lo, mo = kio.read_trajectory(out / "LO0.txt"), kio.read_trajectory(out / "MO0.txt")
    # the same sweeps through the library in this process, written the same way
    seq = synth.SynthSequence(n_rings=64, n_sweeps=9, sensor="hdl64e")
    loam = vl.LidarOdometryMapping(device=0, mapping_skip_frame=2, max_ring_points=8192)
    tf = kio.VloamTF(kio.make_T([0, 0, 0.0074, 0.99997], [0.81, -0.32, 0.80]), kio.make_T([0.5, -0.5, 0.5, -0.5], [1.08, -0.32, 0.72]))
    ref = tmp_path / "lib"
    os.makedirs(ref)
    lo_rows, mo_rows = [], []
    for k in range(8):
        loam.reset()
        loam.scanRegistrationIO(seq.sweep(k))
        loam.laserOdometryIO()
        loam.laserMappingIO()
        lo, lm = loam.laser_odometry, loam.laser_mapping
        tf.LO2CamPrior(lo.q_last_curr, lo.t_last_curr)
        lo_rows.append(tf.LO2Cam0StartFrame(lo.q_w_curr, lo.t_w_curr, k))
        mo_rows.append(tf.MO2Cam0StartFrame(lm.q_w_curr, lm.t_w_curr, k))
    kio.write_trajectory(ref / "LO0.txt", lo_rows)
    kio.write_trajectory(ref / "MO0.txt", mo_rows)
    assert (out / "LO0.txt").read_text() == (ref / "LO0.txt").read_text()
    assert (out / "MO0.txt").read_text() == (ref / "MO0.txt").read_text()
