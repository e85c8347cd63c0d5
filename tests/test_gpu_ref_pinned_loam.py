"""-m gpu: HIP laser odometry and mapping through the C ABI against the output of the REFERENCE'S OWN laser_odometry.cpp / laser_mapping.cpp
— not against the oracle.

Always: the committed recordings tests/golden/ref_lo_*.npz / ref_map_*.npz (written by tests/golden/make_golden.py from
oracle/_ref/libref_loam.so, the reference's files compiled unmodified; tests/test_ref_laser_odometry.py regenerates and re-checks them
wherever the reference exists).  Stage-wise on a debug handle: per outer round the correspondence indices (exact), the raw residuals at the
initial point (RESID_TOL), the parameters in and out; the world pose; the hand-over clouds and skip frames; for the mapping whether it
optimised, the stack sizes, per round the factors' stack points (bit for bit), line points (up to the eigenvector's sign) and planes,
residuals, poses; the published pose; the points per cube of the whole window; the published map.  Then the same sweeps once through
vloam_process_scan (VO priors included): trajectory and map.  Tolerances: tests/test_gpu_laser_odometry.py's.

Additionally, when oracle/_ref/libref_loam.so travelled with the tree: a 64 x 2048 sequence, the hdl64e drive and a window roll live
against the library.  Behind the reference's text the minimizer, kd-tree, eigen-solver and QR are the oracle's restatements.
"""
import glob
import os

import numpy as np
import pytest

import ref_cases

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-8
RESID_TOL = 1e-9
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "ref_lo_*.npz")) + glob.glob(os.path.join(HERE, "golden", "ref_map_*.npz")))
N_CUBES = 21 * 21 * 11


def qdist(a, b):
    return min(np.linalg.norm(a - b), np.linalg.norm(a + b))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check_lo_round(h, outer, corner, plane, res0, x, w):
    d = h.lo_debug(outer)
    assert np.array_equal(d["corner"], corner), "%s: corner correspondences" % w
    assert np.array_equal(d["plane"], plane), "%s: plane correspondences" % w
    rec = d["rec"]
    assert rec["n_factors"] == corner.shape[0] + plane.shape[0]
    r_dev = np.concatenate([d["resid"][:, d["corner_slots"]].T.reshape(-1), d["resid"][0, d["plane_slots"]]])
    assert r_dev.shape == res0.shape
    print("%s: max |residual difference| %.3e" % (w, np.max(np.abs(r_dev - res0), initial=0)))
    assert np.max(np.abs(r_dev - res0), initial=0) < RESID_TOL, w
    assert qdist(rec["x_in"][:4], x[0:4]) < POSE_TOL and np.linalg.norm(rec["x_in"][4:] - x[4:7]) < POSE_TOL, "%s: parameters in" % w
    assert qdist(rec["x_out"][:4], x[7:11]) < POSE_TOL and np.linalg.norm(rec["x_out"][4:] - x[11:14]) < POSE_TOL, "%s: parameters out" % w


def check_map_round(h, z, k, outer, w):
    d = h.map_debug(outer)
    ne = int(z["map%d_%d_ne" % (k, outer)])
    curr, cab, spl = z["map%d_%d_curr" % (k, outer)], z["map%d_%d_cab" % (k, outer)], z["map%d_%d_spl" % (k, outer)]
    x, res0 = z["map%d_%d_x" % (k, outer)], z["map%d_%d_res0" % (k, outer)]
    assert (d["corner_idx"].size, d["surf_idx"].size) == (ne, curr.shape[0] - ne), "%s: %d / %d factors, the reference %d / %d" % (
        w, d["corner_idx"].size, d["surf_idx"].size, ne, curr.shape[0] - ne)
    assert same_bits(h.features(7)[d["corner_idx"], :3], curr[:ne]), "%s: corner factors' stack points" % w
    assert same_bits(h.features(8)[d["surf_idx"], :3], curr[ne:]), "%s: plane factors' stack points" % w
    da, db, oa, ob = d["corner_ab"][:, :3], d["corner_ab"][:, 3:], cab[:, :3], cab[:, 3:]
    e1 = np.maximum(np.abs(da - oa).max(axis=1, initial=0), np.abs(db - ob).max(axis=1, initial=0))
    e2 = np.maximum(np.abs(da - ob).max(axis=1, initial=0), np.abs(db - oa).max(axis=1, initial=0))
    assert np.max(np.minimum(e1, e2), initial=0) < 1e-9, "%s: line points" % w
    assert np.max(np.abs(d["surf_plane"] - spl), initial=0) < 1e-9, "%s: planes" % w
    # raw residuals at the initial point; an edge residual changes sign with the eigenvector's (a <-> b), so edges compare per factor up to sign
    re_dev = d["resid"][:, d["corner_slots"]].T
    re_ref = res0[:3 * ne].reshape(-1, 3)
    de = np.minimum(np.abs(re_dev - re_ref).max(axis=1, initial=0), np.abs(re_dev + re_ref).max(axis=1, initial=0))
    dp = np.abs(d["resid"][0, d["surf_slots"]] - res0[3 * ne:])
    print("%s: max |residual difference| edges %.3e planes %.3e" % (w, np.max(de, initial=0), np.max(dp, initial=0)))
    assert np.max(de, initial=0) < RESID_TOL and np.max(dp, initial=0) < RESID_TOL, w
    rec = d["rec"]
    assert rec["n_factors"] == curr.shape[0]
    assert qdist(rec["x_in"][:4], x[0:4]) < POSE_TOL * (k + 1) and np.linalg.norm(rec["x_in"][4:] - x[4:7]) < POSE_TOL * (k + 1), "%s: pose before" % w
    assert qdist(rec["x_out"][:4], x[7:11]) < POSE_TOL * (k + 1) and np.linalg.norm(rec["x_out"][4:] - x[11:14]) < POSE_TOL * (k + 1), "%s: pose after" % w


def run_stagewise(vl, z, name):
    p = ref_cases.loam_golden_params(z)
    n, mapping = int(z["n_sweeps"]), bool(z["with_mapping"])
    h = vl.Handle(0, scan_line=p["scan_line"], minimum_range=p["minimum_range"], mapping_line_resolution=p["line_res"], mapping_plane_resolution=p["plane_res"],
                  mapping_skip_frame=p["mapping_skip_frame"], detach_VO_LO=int(p["detach_vo_lo"]), debug=1, with_mapping=int(mapping))
    last_counts = None
    for k in range(n):
        w = "%s sweep %d" % (name, k)
        h.reset_frame()
        if int(z["has_prior"]):
            h.set_lo_prior(z["prior_%d" % k][:4], z["prior_%d" % k][4:])
        h.scan_registration(ref_cases.loam_golden_sweep(z, k))
        qw, tw, ql, tl = h.laser_odometry()
        rounds = int(z["lo%d_n" % k])
        assert rounds == (0 if k == 0 else 2)
        for outer in range(rounds):
            check_lo_round(h, outer, z["lo%d_%d_corner" % (k, outer)], z["lo%d_%d_plane" % (k, outer)], z["lo%d_%d_res0" % (k, outer)], z["lo%d_%d_x" % (k, outer)],
                           "%s round %d" % (w, outer))
        pose = z["lo%d_pose" % k]
        assert qdist(qw, pose[:4]) < POSE_TOL * (k + 1) and np.linalg.norm(tw - pose[4:]) < POSE_TOL * (k + 1), "%s world pose" % w
        if rounds:
            x = z["lo%d_1_x" % k]
            assert qdist(ql, x[7:11]) < POSE_TOL and np.linalg.norm(tl - x[11:14]) < POSE_TOL, "%s f2f pose" % w
        # LaserOdometry::output's skip_frame: frameCount % mapping_skip_frame after the increment of solveLO (laser_odometry.cpp:535, :618)
        # (the handle counts a sweep once its last stage is done: without mapping that was the odometry, with it the mapping is still to come)
        skip = (h.frame_count() + int(mapping)) % p["mapping_skip_frame"] != 0
        assert skip == bool(int(z["lo%d_skip" % k])), "%s skip_frame: the device's frame count is %d" % (w, h.frame_count())
        if not mapping:
            assert same_bits(h.features(5), z["lo%d_c2" % k]) and same_bits(h.features(6), z["lo%d_c4" % k]), "%s laserCloudCornerLast / SurfLast" % w
            assert same_bits(h.features(0), ref_cases.loam_golden_full(z, k)), "%s laserCloudFullRes" % w
            continue
        # the hand-over clouds are the sweep's own less-sharp / less-flat clouds (laser_odometry.cpp:511-517), which tests/test_gpu_ref_pinned.py
        # pins to the reference; the mapping recordings do not repeat them (file size)
        assert same_bits(h.features(5), h.features(2)) and same_bits(h.features(6), h.features(4)), "%s laserCloudCornerLast / SurfLast" % w
        qm, tm = h.laser_mapping()
        pub = z["map%d_pub" % k]
        assert qdist(qm, pub[:4]) < POSE_TOL * (k + 1) and np.linalg.norm(tm - pub[4:]) < POSE_TOL * (k + 1), "%s published map pose" % w
        if skip:     # LaserMapping::input keeps nothing and solveMapping does not run: the map is what the last mapped sweep left
            if last_counts is not None:
                assert np.array_equal(h.debug_raw(2, 66, np.int32).reshape(2, N_CUBES), last_counts), "%s: a skipped sweep changed the map" % w
            continue
        st = h.map_state()
        solves = int(z["map%d_n" % k])
        assert st["do_optimize"] == (1 if solves == 2 else 0), "%s: optimised %d, the reference solved %d times" % (w, st["do_optimize"], solves)
        assert (st["n_corner_stack"], st["n_surf_stack"]) == tuple(int(v) for v in z["map%d_stacks" % k]), "%s stack sizes" % w
        for outer in range(solves):
            check_map_round(h, z, k, outer, "%s map round %d" % (w, outer))
        last_counts = z["map%d_counts" % k]
        assert np.array_equal(h.debug_raw(2, 66, np.int32).reshape(2, N_CUBES), last_counts), "%s points per cube" % w
    return h


def check_map_cloud(got, want, what):
    """Same points in the same order, intensities bit for bit; a coordinate is f32(q p + t) of f64 poses that agree to POSE_TOL, so it is the
    same float or its neighbour (the rule of tests/test_gpu_laser_mapping.py for the registered cloud)."""
    assert got.shape == want.shape and got.shape[0] > 100, "%s: %s vs %s points" % (what, got.shape, want.shape)
    g, w = np.ascontiguousarray(got[:, :4]), np.ascontiguousarray(want[:, :4])
    assert np.array_equal(g[:, 3].view(np.uint32), w[:, 3].view(np.uint32)), "%s intensities" % what
    ulp = np.abs(g[:, :3].view(np.int32).astype(np.int64) - w[:, :3].view(np.int32).astype(np.int64))
    print("%s: %d of %d coordinates not bit-equal (max %d ulp)" % (what, int(np.count_nonzero(ulp)), ulp.size, int(ulp.max())))
    assert ulp.max() <= 1 and np.mean(ulp == 0) > 0.999, what


def test_the_recordings_are_all_here():
    assert sorted(os.path.basename(p)[:-4] for p in GOLDEN) == sorted(ref_cases.loam_golden_cases())


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_device_stagewise_against_the_reference_binarys_recorded_output(vl, path):
    z = np.load(path)
    h = run_stagewise(vl, z, os.path.basename(path)[:-4])
    if bool(z["with_mapping"]):
        h.sync()
        check_map_cloud(h.get_map(), z["map_cloud"], "/laser_cloud_map")
    h.close()


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_device_process_scan_against_the_reference_binarys_recorded_output(vl, path):
    """The same sweeps through vloam_process_scan (no host sync between the stages): trajectory and map.  A recorded VO prior is set before
    each sweep (vloam_set_lo_prior holds for the next sweep's odometry), so the warm-start overwrite of both outer rounds is checked on this
    path too: without it the poses of ref_lo_16x256_prior_skip2 are off by the prior's centimetres."""
    z = np.load(path)
    p = ref_cases.loam_golden_params(z)
    n, mapping = int(z["n_sweeps"]), bool(z["with_mapping"])
    h = vl.Handle(0, scan_line=p["scan_line"], minimum_range=p["minimum_range"], mapping_line_resolution=p["line_res"], mapping_plane_resolution=p["plane_res"],
                  mapping_skip_frame=p["mapping_skip_frame"], detach_VO_LO=int(p["detach_vo_lo"]), with_mapping=int(mapping))
    for k in range(n):
        if int(z["has_prior"]):
            h.set_lo_prior(z["prior_%d" % k][:4], z["prior_%d" % k][4:])
        h.process_scan(ref_cases.loam_golden_sweep(z, k))
    h.sync()
    t = h.trajectory()
    assert t.shape == (n, 14)
    for k in range(n):
        pose = z["lo%d_pose" % k]
        assert qdist(t[k, :4], pose[:4]) < POSE_TOL * (k + 1) and np.linalg.norm(t[k, 4:7] - pose[4:]) < POSE_TOL * (k + 1), "sweep %d world pose" % k
        if mapping:
            pub = z["map%d_pub" % k]
            assert qdist(t[k, 7:11], pub[:4]) < POSE_TOL * (k + 1) and np.linalg.norm(t[k, 11:14] - pub[4:]) < POSE_TOL * (k + 1), "sweep %d map pose" % k
    if mapping:
        check_map_cloud(h.get_map(), z["map_cloud"], "/laser_cloud_map")
    h.close()


def test_class_mirror_hands_over_the_references_skip_frame(vl):
    """LaserOdometry.output() / LaserMapping.input() of the package's mirror of the reference's classes, mapping_skip_frame = 2: the
    skip_frame flag of every sweep is the recorded one (sweeps 0, 2, 4 skipped), input() accepts it, and the poses follow the recording."""
    z = np.load(os.path.join(HERE, "golden", "ref_map_16x256_skip2.npz"))
    p = ref_cases.loam_golden_params(z)
    loam = vl.LidarOdometryMapping(0, scan_line=p["scan_line"], mapping_skip_frame=p["mapping_skip_frame"], with_mapping=1)
    flags = []
    for k in range(int(z["n_sweeps"])):
        loam.reset()
        loam.scanRegistrationIO(ref_cases.loam_golden_sweep(z, k))
        loam.laserOdometryIO()
        q, t, corner, surf, full, skip = loam.laser_odometry.output()
        flags.append(bool(skip))
        assert bool(skip) == bool(int(z["lo%d_skip" % k])), "sweep %d skip_frame" % k
        loam.laser_mapping.input(corner, surf, full, q, t, skip)
        qm, tm = loam.laserMappingIO()
        pub = z["map%d_pub" % k]
        assert qdist(qm, pub[:4]) < POSE_TOL * (k + 1) and np.linalg.norm(tm - pub[4:]) < POSE_TOL * (k + 1), "sweep %d published map pose" % k
    assert flags == [True, False] * (len(flags) // 2)
    loam.hd.close()


def _live():
    import ref
    return ref if os.path.exists(os.path.join(ref.REF_OUT, ref.LOAM_LIB)) else None


@pytest.mark.parametrize("name", ["64x2048", "hdl64e", "roll"])
def test_device_against_the_reference_binary_live(vl, name):
    ref = _live()
    if ref is None:
        pytest.skip("oracle/_ref/libref_loam.so (the reference's laser_odometry.cpp / laser_mapping.cpp, compiled where the reference exists) did not travel with this tree")
    walk = None
    if name == "roll":     # the first leg of branch_cases.six_way_walk: the window rolls along -x
        import branch_cases
        walk = branch_cases.six_way_walk()[:12]
        sweeps = ref_cases.synth_sequence(64, 2048, len(walk))
    else:
        sweeps = ref_cases.synth_sequence(64, 2048, 3) if name == "64x2048" else ref_cases.synth_sequence(64, None, 3, sensor="hdl64e")
    kw = dict(max_ring_points=8192) if name == "hdl64e" else {}
    h = vl.Handle(0, with_mapping=1, max_points=max(max(c.shape[0] for c in sweeps), 1024), **kw)
    r = ref.Loam()
    for k, c in enumerate(sweeps):
        w = "%s sweep %d (live)" % (name, k)
        assert r.stage_sr(c) == 0 and r.stage_lo() == 0
        h.reset_frame()
        h.scan_registration(c)
        qw, tw, _, _ = h.laser_odometry()
        rq, rt = r.lo_pose()
        assert qdist(qw, rq) < POSE_TOL * (k + 1) and np.linalg.norm(tw - rt) < POSE_TOL * (k + 1), "%s world pose" % w
        if walk is not None:   # both sides are handed the same pose: the reference's odometry plus the walk
            h.set_mapping_input(q_wodom_curr=rq, t_wodom_curr=rt + walk[k])
            assert r.stage_map(q=rq, t=rt + walk[k]) == 0
        else:
            assert r.stage_map() == 0
        qm, tm = h.laser_mapping()
        pq, pt = r.published_pose(1)
        assert qdist(qm, pq) < POSE_TOL * (k + 1) and np.linalg.norm(tm - pt) < POSE_TOL * (k + 1), "%s map pose" % w
        assert h.map_state()["do_optimize"] == (1 if r.num_solves(r.MAPPING) == 2 else 0), w
        assert np.array_equal(h.debug_raw(2, 66, np.int32).reshape(2, N_CUBES), r.map_cube_counts()), "%s points per cube" % w
    if walk is not None:
        assert h.map_state()["cen"][0] > 10, "440 m along -x: the window must have rolled (laser_mapping.cpp:218-247)"
    h.close()
