"""-m gpu: the HIP visual-odometry stack (csrc/vo_kernels.hip) through the C ABI against the output of the REFERENCE'S OWN
point_cloud_util.cpp / visual_odometry.cpp::solveNlsAll — not against the oracle.

Reads only the committed recordings tests/golden/ref_vo_*.npz (written by tests/golden/make_golden.py from oracle/_ref/libref_vo.so, the
reference's files compiled unmodified; tests/test_ref_visual_odometry.py re-checks them wherever the reference exists; layout:
tests/ref_vo_cases.py).  Through vo_set_calib / vo_process_point_cloud / vo_solve / vo_debug, bit for bit: the bucket maps of both
ping-pong slots, per match the kind, depth0 and the observations; exact: both counters; the solve to the 1e-8 of tests/test_gpu_vo.py.
The ABI takes integer pixel pairs and the initial angle-axis, so a run is replayed from the pairs the reference derived from its keypoints
and from the parameters its ceres::Solve started from (both recorded); entries the optical-flow status ruled out never reach the ABI.
Behind the reference's text the minimizer and the 3 x 3 QR are the oracle's restatements.
"""
import glob
import os

import numpy as np
import pytest

import ref_vo_cases as cases

pytestmark = pytest.mark.gpu

SOLVE_TOL = 1e-8     # tests/test_gpu_vo.py
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "ref_vo_*.npz")))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def cloud_of(z, k):
    c = np.zeros((z["f%d_cloud" % k].shape[0], 4), dtype=np.float32)
    c[:, :3] = z["f%d_cloud" % k]
    return c


def check_maps(d, z, k, w):
    for name, k_rec in (("cur", k), ("prev", k - 1)):
        if k_rec < 0:
            continue
        want = cases.dense(z, k_rec)
        assert np.array_equal(d[name][3], want[3]), "%s: bucket_count of the %s map" % (w, name)
        for a in range(3):
            assert same_bits(d[name][a], want[a]), "%s: bucket array %d of the %s map" % (w, a, name)


def check_rows(got, rows, w):
    assert np.array_equal(got[:, 0], rows[:, 0]), "%s: kinds" % w
    assert same_bits(got[:, 1], rows[:, 1]), "%s: depth0" % w
    assert np.array_equal(got[:, 2:], rows[:, 2:7]), "%s: observations" % w


def test_the_recordings_are_all_here():
    assert [os.path.basename(p)[:-4] for p in GOLDEN] == ["ref_vo_64x256_3frames", "ref_vo_64x256_perturbed", "ref_vo_edges", "ref_vo_match_loop"]


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_device_stagewise_against_the_reference_binarys_recorded_output(vl, path):
    z = np.load(path)
    calib = (z["cam_T_velo"], z["rect0_T_cam"], z["P_rect0"])
    n_pts = max(z["f%d_cloud" % k].shape[0] for k in range(int(z["n_frames"])))
    for si in range(int(z["n_sessions"])):
        remove, reset, flow = (int(v) for v in z["s%d_opts" % si])
        h = vl.Handle(0, with_mapping=0, debug=1, remove_VO_outlier=remove, reset_VO_to_identity=reset, max_points=max(n_pts, 1024))
        h.vo_set_calib(*calib)
        runs = set(int(v) for v in z["s%d_run_frames" % si])
        for k in range(int(z["n_frames"])):
            w = "%s session %d frame %d" % (os.path.basename(path)[:-4], si, k)
            h.vo_process_point_cloud(cloud_of(z, k))
            if k not in runs:
                continue
            pre = "s%d_r%d_" % (si, k)
            rows = z[pre + "rows"]
            rows = rows[rows[:, 0] != -1]
            x_in, x_out, cnt = z[pre + "x_in"], z[pre + "x_out"], z[pre + "counters"]
            aa, t, c32, c22 = h.vo_solve(rows[:, 7:9].astype(np.int32), rows[:, 9:11].astype(np.int32), x_in[:3], x_in[3:])
            d = h.vo_debug(rows.shape[0])
            check_maps(d, z, k, w)
            check_rows(d["match_rows"], rows, w)
            assert (c32, c22) == (int(cnt[0]), int(cnt[1])), "%s: counters" % w
            print("%s: %d + %d factors, |d angles| %.2e |d t| %.2e" % (w, c32, c22, np.linalg.norm(aa - x_out[:3]), np.linalg.norm(t - x_out[3:])))
            assert np.linalg.norm(aa - x_out[:3]) < SOLVE_TOL and np.linalg.norm(t - x_out[3:]) < SOLVE_TOL, "%s: the solve" % w
        h.close()


def test_process_frame_gives_the_rows_of_the_stagewise_calls(vl, synth):
    """The coupled path once: vloam_process_frame on the three-frame case leaves the recorded VO rows, counters and bucket maps — the
    same the stage-wise calls give — and, with reset_VO_to_identity, the recorded solve."""
    z = np.load(os.path.join(HERE, "golden", "ref_vo_64x256_3frames.npz"))
    base_T_cam0, velo_T_cam0 = synth.kitti_like_extrinsics()
    h = vl.Handle(0, with_mapping=0, debug=1, remove_VO_outlier=100, reset_VO_to_identity=1)
    h.vo_set_calib(z["cam_T_velo"], z["rect0_T_cam"], z["P_rect0"])
    h.set_extrinsics(base_T_cam0, velo_T_cam0)
    for k in range(int(z["n_frames"])):
        w = "process_frame, frame %d" % k
        if k == 0:
            h.process_frame(cloud_of(z, k))
            continue
        rows, x_out, cnt = z["s0_r%d_rows" % k], z["s0_r%d_x_out" % k], z["s0_r%d_counters" % k]
        assert np.all(rows[:, 0] != -1)
        h.process_frame(cloud_of(z, k), rows[:, 7:9].astype(np.int32), rows[:, 9:11].astype(np.int32))
        h.sync()
        d = h.vo_debug(rows.shape[0])
        check_maps(d, z, k, w)
        check_rows(d["match_rows"], rows, w)
        r = h.vo_result()
        assert (r["counter32"], r["counter22"]) == (int(cnt[0]), int(cnt[1])), "%s: counters" % w
        assert np.linalg.norm(r["angles"] - x_out[:3]) < SOLVE_TOL and np.linalg.norm(r["t"] - x_out[3:]) < SOLVE_TOL, "%s: the solve" % w
    h.close()
