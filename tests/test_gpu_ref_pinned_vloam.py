"""-m gpu: vloam_process_frame against the recorded output of the REFERENCE'S OWN coupled frame loop (tests/golden/ref_vloam_*.npz, written
by tests/golden/make_golden.py from oracle/_ref/libref_vloam.so — vloam_tf.cpp and lidar_odometry_mapping.cpp compiled unmodified over the
VO and LiDAR halves; tests/test_ref_vloam.py re-checks the recordings wherever the reference exists).  Reads only the recordings.

Per frame on a debug handle.  Bit for bit: the VO rows (kind, depth0, observations), both counters, the bucket maps of the current and the
previous frame, the factor sets of both odometry rounds, and x_in of both rounds against vo_result()["prior_q/t"] (combined mode).  To
POSE_TOL of tests/test_gpu_vloam.py (x (k + 1) for accumulated poses; that file's frame-1 allowance of 2e-7 / 1e-6 is NOT used: the device
is within 2e-10 of the recording at frame 1): prior_q/t against velo_last_VOT_velo_curr, vo_trajectory() against world_VOT_base_last,
trajectory() against world_LOT_base_last / world_MOT_base_last.  To SOLVE_TOL of tests/test_gpu_vo.py: the VO solve, frame 1 included.

Batch: a batched handle has ONE sensor rig — vloam_set_extrinsics and vloam_vo_set_calib write every session (capi_frame.cpp) — so scenarios A
and D, whose rigs differ, cannot be two sessions of one handle.  Each runs as one session of a two-session vloam_batch_process_frame under
its own rig, next to a session fed the other scenario's sweeps and matches, A in slot 0 and D in slot 1, and is held to its recording.

Live: where oracle/_ref/libref_vloam.so travelled with the tree, scenario D at 64 x 512 against the library itself.

The degenerate recording: the frames the reference gates (NaN velo_last_VOT_velo_curr, world_VOT_base_last kept) are the frames the
device flags VLOAM_SWEEP_VO_DEGENERATE and at which vloam_sync reports VLOAM_ERR_INVALID, as include/vloam_hip/c_api.h documents (never
before the first such frame); in combined mode the poses are NaN where the reference's are, in detached mode the LO / map poses stay the
recorded finite ones.  The combined session ends where the reference's does: before the first mapped frame after the NaN.
"""
import os

import numpy as np
import pytest

import ref_vloam_cases as cases

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-8      # tests/test_gpu_vloam.py
SOLVE_TOL = 1e-8     # tests/test_gpu_vo.py
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["combined", "detached", "extrinsics"]
TF = {n: i for i, n in enumerate(("imu_T_velo", "imu_T_cam0", "base_T_imu", "base_T_cam0", "velo_T_cam0", "world_VOT_base_last", "base_last_VOT_base_curr",
                                  "cam0_curr_VOT_cam0_last", "velo_last_VOT_velo_curr"))}
TF.update(world_LOT_base_last=12, world_MOT_base_last=18)


def load(name):
    return np.load(os.path.join(HERE, "golden", "ref_vloam_%s.npz" % name))


def qdist(a, b):
    return min(np.linalg.norm(a - b), np.linalg.norm(a + b))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def pose_err(q, t, row12, kio):
    """A device pose (q xyzw, t) against a recorded transform (basis row-major, origin)."""
    T = kio.make_T(q, t)
    return float(max(np.max(np.abs(T[:3, :3].reshape(-1) - row12[:9])), np.max(np.abs(T[:3, 3] - row12[9:]))))


def make(vl, z, prefix="", **kw):
    o = cases.opts_of(z, prefix)
    h = vl.Handle(0, scan_line=o["scan_line"], mapping_skip_frame=o["mapping_skip_frame"], detach_VO_LO=o["detach_VO_LO"], reset_VO_to_identity=o["reset_VO_to_identity"],
                  remove_VO_outlier=o["remove_VO_outlier"], with_mapping=1, **kw)
    h.vo_set_calib(z["cam_T_velo"], z["rect0_T_cam"], z["P_rect0"])
    h.set_extrinsics(z[prefix + "base_T_cam0"], z[prefix + "velo_T_cam0"])
    return h, o


def check_frame(h, z, k, o, kio, w, prefix="", maxima=None):
    pre = "%sf%d_" % (prefix, k)
    tfs = z[pre + "tfs"]
    r = h.vo_result()
    tol1 = POSE_TOL     # frame 1 too: measured on the device 2.5e-16 (solve) and 4.7e-11 (prior) there, so test_gpu_vloam.py's 2e-7 allowance is not needed
    m = cases.matches_of(z, k)
    if k > 0:
        n = m[0].shape[0]
        d = h.vo_debug(n)
        for name, kk in (("cur", k), ("prev", k - 1)):
            want = cases.dense(z, "f%d_" % kk)
            assert np.array_equal(d[name][3], want[3]), "%s: bucket_count of the %s map" % (w, name)
            for a in range(3):
                assert same_bits(d[name][a], want[a]), "%s: bucket array %d of the %s map" % (w, a, name)
        assert np.array_equal(d["match_rows"][:, 0], z[pre + "vo_kind"]), "%s: kinds" % w
        assert same_bits(d["match_rows"][:, 1], z[pre + "vo_depth0"]), "%s: depth0" % w
        assert np.array_equal(d["match_rows"][:, 2:], z[pre + "vo_obs"]), "%s: observations" % w
        assert (r["counter32"], r["counter22"]) == tuple(int(v) for v in z[pre + "vo_counters"]), "%s: counters" % w
        x = z[pre + "vo_x"]
        e = max(np.linalg.norm(r["angles"] - x[6:9]), np.linalg.norm(r["t"] - x[9:12]))
        print("%s: VO solve differs by %.3e" % (w, e))
        assert e < SOLVE_TOL, "%s: the VO solve" % w
    prior = z[pre + "prior"]
    if np.any(np.isnan(prior)):
        return False
    e = max(qdist(r["prior_q"], prior[:4]), np.linalg.norm(r["prior_t"] - prior[4:]))
    print("%s: velo_last_VOT_velo_curr differs by %.3e" % (w, e))
    assert e < (1e-15 if k == 0 else tol1), "%s: velo_last_VOT_velo_curr" % w
    for outer in range(2 if k > 0 else 0):
        dbg = h.lo_debug(outer)
        assert np.array_equal(dbg["corner"], z["%slo%d_corner" % (pre, outer)]), "%s round %d: corner factors" % (w, outer)
        assert np.array_equal(dbg["plane"], z["%slo%d_plane" % (pre, outer)]), "%s round %d: plane factors" % (w, outer)
        x_in = dbg["rec"]["x_in"]
        if not o["detach_VO_LO"]:
            assert np.array_equal(x_in[:4], r["prior_q"]) and np.array_equal(x_in[4:], r["prior_t"]), "%s round %d: starts from the prior" % (w, outer)
        x = z["%slo%d_x" % (pre, outer)]
        assert qdist(x_in[:4], x[:4]) < tol1 and np.linalg.norm(x_in[4:] - x[4:7]) < tol1, "%s round %d: x_in" % (w, outer)
    return True


def check_poses(h, z, k, kio, w, prefix=""):
    pre = "%sf%d_" % (prefix, k)
    tfs = z[pre + "tfs"]
    tol = POSE_TOL * (k + 1)
    tj, vj = h.trajectory()[k], h.vo_trajectory()[k]
    for name, q, t in (("world_VOT_base_last", vj[0:4], vj[4:7]), ("world_LOT_base_last", tj[0:4], tj[4:7]), ("world_MOT_base_last", tj[7:11], tj[11:14])):
        want = tfs[TF[name]]
        if np.any(np.isnan(want)):
            assert np.any(np.isnan(np.concatenate([q, t]))), "%s: the reference's %s is NaN, the device's is %s %s" % (w, name, q, t)
            continue
        e = pose_err(q, t, want, kio)
        print("%s: %s differs by %.3e" % (w, name, e))
        assert e < tol, "%s: %s" % (w, name)


@pytest.fixture(scope="module")
def kio(vl):
    from vloam_amd import kitti_io
    return kitti_io


@pytest.mark.parametrize("name", NAMES)
def test_process_frame_against_the_recorded_reference(vl, kio, name):
    z = load(name)
    h, o = make(vl, z, debug=1)
    for k in range(int(z["n_run"])):
        w = "%s frame %d" % (name, k)
        h.process_frame(cases.cloud_of(z, k), *cases.matches_of(z, k))
        h.sync()
        assert check_frame(h, z, k, o, kio, w)
        check_poses(h, z, k, kio, w)
    # the trajectory files: rows formed the way tools/run_sequence.py forms them equal the reference's bytes
    tf = kio.VloamTF(*[kio.make_T(s[:4], s[4:]) for s in z["statics"]])
    want = [cases.rows_per_frame(z, which) for which in range(3)]
    tj, vj = h.trajectory(), h.vo_trajectory()
    for k in range(int(z["n_run"])):
        if not (o["start_frame"] <= k <= o["end_frame"]):
            assert all(want[which][k] == "" for which in range(3))
            continue
        c = k - o["start_frame"]
        tf.world_VOT_base_last = kio.make_T(vj[k, 0:4], vj[k, 4:7])
        got = [kio.format_pose_row(tf.VO2Cam0StartFrame(c)), kio.format_pose_row(tf.LO2Cam0StartFrame(tj[k, 0:4], tj[k, 4:7], c)),
               kio.format_pose_row(tf.MO2Cam0StartFrame(tj[k, 7:11], tj[k, 11:14], c))]
        for which in range(3):
            assert got[which] == want[which][k], "%s frame %d file %d:\ndevice    %r\nreference %r" % (name, k, which, got[which], want[which][k])
    h.close()


def test_streamed_frames_give_the_bytes_of_the_per_frame_run(vl):
    z = load("combined")
    out = []
    for sync in (True, False):
        h, _ = make(vl, z)
        for k in range(int(z["n_run"])):
            h.process_frame(cases.cloud_of(z, k), *cases.matches_of(z, k))
            if sync:
                h.sync()
        h.sync()
        out.append((h.trajectory().copy(), h.vo_trajectory().copy()))
        h.close()
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()


@pytest.mark.parametrize("prefix", ["", "d_"], ids=["combined", "detached"])
def test_degenerate_frames_behave_as_recorded(vl, kio, prefix):
    z = load("degenerate")
    h, o = make(vl, z, prefix, debug=1, sweep_log=1)
    n = int(z[prefix + "n_run"])
    gated = []
    for k in range(n):
        w = "degenerate%s frame %d" % (prefix, k)
        status = int(z["%sf%d_status" % (prefix, k)])
        if status != 0:      # the reference cannot map this frame (NaN position -> int, laser_mapping.cpp:207): nothing recorded to hold the device to
            break
        h.process_frame(cases.cloud_of(z, k), *cases.matches_of(z, k))
        nan_ref = bool(np.any(np.isnan(z["%sf%d_prior" % (prefix, k)])))
        gated.append(nan_ref)
        try:      # c_api.h: after a VO solve with a zero rotation angle vloam_sync reports VLOAM_ERR_INVALID — and nowhere else
            h.sync()
            raised = False
        except vl.VloamError as e:
            assert e.status == vl.ERR_INVALID and any(gated), "%s: vloam_sync reported %d" % (w, e.status)
            raised = True
        if nan_ref:
            assert raised, "%s: the reference gated this frame, vloam_sync reported nothing" % w
        flags = int(h.sweep_log(k, 1)[0]["error_bits"])
        assert bool(flags & vl.SWEEP_VO_DEGENERATE) == nan_ref, "%s: VLOAM_SWEEP_VO_DEGENERATE is %d, the reference's gate says %s" % (w, flags, nan_ref)
        finite = check_frame(h, z, k, o, kio, w, prefix)
        assert finite == (not nan_ref)
        check_poses(h, z, k, kio, w, prefix)
    assert any(gated)
    h.close()


@pytest.mark.parametrize("name,slot", [("combined", 0), ("extrinsics", 1)])
def test_two_session_batch_against_the_recorded_reference(vl, kio, name, slot):
    """See the module docstring: the checked session carries its own scenario's rig; its neighbour is fed the other scenario's inputs."""
    z, other = load(name), load("extrinsics" if name == "combined" else "combined")
    o = cases.opts_of(z)
    h = vl.Handle(0, n_sessions=2, scan_line=o["scan_line"], mapping_skip_frame=o["mapping_skip_frame"], detach_VO_LO=o["detach_VO_LO"],
                  reset_VO_to_identity=o["reset_VO_to_identity"], remove_VO_outlier=o["remove_VO_outlier"], with_mapping=1)
    h.vo_set_calib(z["cam_T_velo"], z["rect0_T_cam"], z["P_rect0"])
    h.set_extrinsics(z["base_T_cam0"], z["velo_T_cam0"])
    n = int(z["n_run"])
    for k in range(n):
        mine, theirs = (cases.cloud_of(z, k), cases.matches_of(z, k)), (cases.cloud_of(other, k), cases.matches_of(other, k))
        pair = [mine, theirs] if slot == 0 else [theirs, mine]
        h.batch_process_frame([p[0] for p in pair], [p[1] for p in pair])
        h.sync()
        h.select(slot)
        w = "batch, %s in slot %d, frame %d" % (name, slot, k)
        r = h.vo_result()
        if k > 0:
            x = z["f%d_vo_x" % k]
            assert (r["counter32"], r["counter22"]) == tuple(int(v) for v in z["f%d_vo_counters" % k]), "%s: counters" % w
            assert max(np.linalg.norm(r["angles"] - x[6:9]), np.linalg.norm(r["t"] - x[9:12])) < SOLVE_TOL, "%s: the VO solve" % w
        prior = z["f%d_prior" % k]
        assert qdist(r["prior_q"], prior[:4]) < POSE_TOL and np.linalg.norm(r["prior_t"] - prior[4:]) < POSE_TOL, "%s: velo_last_VOT_velo_curr" % w
        check_poses(h, z, k, kio, w)
    h.select(1 - slot)
    assert np.all(np.isfinite(h.trajectory())) and not np.array_equal(h.trajectory()[n - 1][:7], z["f%d_lo_pose" % (n - 1)]), "the neighbour ran its own sequence"
    h.close()


def test_scenario_d_at_64x512_live_against_the_reference_binary(vl, kio):
    import ref
    if not os.path.exists(os.path.join(ref.REF_OUT, ref.VLOAM_LIB)):
        pytest.skip("oracle/_ref/libref_vloam.so (the reference's coupled frame loop, compiled where the reference exists) did not travel with this tree")
    sc = cases.extrinsics_scenario(n_az=512, n=4, n_match=1400)
    o = sc["opts"]
    r = cases.new_session(ref, sc, o)
    h = vl.Handle(0, detach_VO_LO=0, with_mapping=1, debug=1)
    h.vo_set_calib(*sc["calib"])
    for k, c in enumerate(sc["frames"]):
        w = "D 64 x 512 live, frame %d" % k
        m = sc["matches"][k] if sc["matches"][k] is not None else (None, None)
        assert r.frame(c, *m) == 0
        tfs = r.tfs()
        if k == 0:
            h.set_extrinsics(cases.T4(tfs[TF["base_T_cam0"]]), cases.T4(tfs[TF["velo_T_cam0"]]))
        h.process_frame(c, *m)
        h.sync()
        res = h.vo_result()
        if k > 0:
            v = r.vo(m[0].shape[0])
            d = h.vo_debug(m[0].shape[0])
            assert np.array_equal(d["match_rows"][:, 0], v["match_rows"][:, 0]) and same_bits(d["match_rows"][:, 1], v["match_rows"][:, 1]), "%s: VO rows" % w
            assert np.array_equal(d["match_rows"][:, 2:], v["match_rows"][:, 2:7]), "%s: observations" % w
            assert (res["counter32"], res["counter22"]) == (v["counter32"], v["counter22"]) and v["counter32"] > 10, "%s: counters" % w
            e = max(np.linalg.norm(res["angles"] - v["x_out"][:3]), np.linalg.norm(res["t"] - v["x_out"][3:]))
            print("%s: VO solve differs by %.3e" % (w, e))
            assert e < SOLVE_TOL, "%s: the VO solve" % w
        pq, pt = r.tf_rotation(8), tfs[8, 9:]
        assert qdist(res["prior_q"], pq) < POSE_TOL and np.linalg.norm(res["prior_t"] - pt) < POSE_TOL, "%s: velo_last_VOT_velo_curr" % w
        tol = POSE_TOL * (k + 1)
        tj, vj = h.trajectory()[k], h.vo_trajectory()[k]
        for name, q, t in (("world_VOT_base_last", vj[0:4], vj[4:7]), ("world_LOT_base_last", tj[0:4], tj[4:7]), ("world_MOT_base_last", tj[7:11], tj[11:14])):
            e = pose_err(q, t, tfs[TF[name]], kio)
            print("%s: %s differs by %.3e" % (w, name, e))
            assert e < tol, "%s: %s" % (w, name)
    h.close()
