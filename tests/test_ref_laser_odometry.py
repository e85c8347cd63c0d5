"""CPU: the oracle's laser odometry against the REFERENCE'S OWN laser_odometry.cpp, compiled unmodified (oracle/_ref/libref_loam.so through
oracle/ref.py; stand-in headers in oracle/ref_shim/), chained behind its own scan_registration.cpp as lidar_odometry_mapping.cpp:96-150
chains them.

Compared per sweep: the number of ceres::Solve calls (the two outer rounds); per round the residual blocks in AddResidualBlock order —
corner factors first, plane factors after, their counts, the correspondence index triples recovered from the functors' points (matched bit
for bit against the sweep's own clouds) against o.lo_corr(), the raw residuals at the initial point, the parameters in and out —;
q_w_curr / t_w_curr as output() hands them over; the three hand-over clouds bit for bit and in order; skip_frame.

Tolerances are the project's (tests/test_gpu_laser_odometry.py): RESID_TOL, POSE_TOL (x frame index for the accumulated pose).  Integers,
flags and f32 clouds are exact.

What is pinned: control flow, constants (NEARBY_SCAN, DISTANCE_SQ_THRESHOLD), the adjacent-line walks, the warm-start overwrite, the pose
composition, the skip-frame hand-over.  What is NOT: the minimizer and the kd-tree behind the reference are the oracle's own restatements
(oracle/ref_bridge.cpp, ref_shim/pcl/kdtree/kdtree_flann.h) — Ceres and FLANN do not exist on the build machine.

Skips: only when neither the reference checkout nor a built oracle/_ref/ exists.
"""
import numpy as np
import pytest

import ref_cases

import ref

pytestmark = pytest.mark.skipif(not ref.available(), reason=ref.SKIP_REASON)

POSE_TOL = 1e-8
RESID_TOL = 1e-9


def qdist(a, b):
    return min(np.linalg.norm(np.asarray(a) - np.asarray(b)), np.linalg.norm(np.asarray(a) + np.asarray(b)))


def same_cloud(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def candidates(points_f64, table):
    """For every row of points_f64 [n, 3] (doubles that hold f32 values) the indices of the rows of table [m, 4] with the same x, y, z bits."""
    key = {}
    for i, r in enumerate(np.ascontiguousarray(table[:, :3])):
        key.setdefault(r.tobytes(), []).append(i)
    p32 = np.ascontiguousarray(points_f64, dtype=np.float32)
    assert np.array_equal(p32.astype(np.float64), points_f64), "a functor point is not an f32 value"
    out = []
    for r in p32:
        assert r.tobytes() in key, "a functor point is no point of the cloud it should come from"
        out.append(key[r.tobytes()])
    return out


def assert_indices(cands, want, what):
    """Exact where the reference's point is unique in its cloud; where the cloud holds the same bits more than once (a replayed return) the
    oracle's index must be one of those rows — the functor cannot tell them apart either."""
    assert len(cands) == len(want), what
    for row, (c, w) in enumerate(zip(cands, want)):
        if len(c) == 1:
            assert int(w) == c[0], "%s, factor %d: the oracle paired index %d, the reference index %d" % (what, row, int(w), c[0])
        else:
            assert int(w) in c, "%s, factor %d: the oracle paired index %d, the reference's point sits at %s" % (what, row, int(w), c)


def compare_odometry(r, o, k, sharp, flat, tree_corner, tree_surf, prior, what):
    """After stage_lo on both: everything the module docstring lists, for sweep k."""
    n = r.num_solves(r.ODOMETRY)
    assert n == o.lo_num_outer() and n == (0 if k == 0 else 2), "%s: %d solves, oracle %d" % (what, n, o.lo_num_outer())
    for outer in range(n):
        s, os_ = r.solve(r.ODOMETRY, outer), o.lo_solve(outer)
        oc, op = o.lo_corr(outer)
        w = "%s round %d" % (what, outer)
        assert s["max_num_iterations"] == 4
        nc, npl = int(np.count_nonzero(s["types"] == 0)), int(np.count_nonzero(s["types"] == 1))
        assert nc + npl == s["types"].size and np.all(s["types"][:nc] == 0), "%s: corner factors first, then plane factors" % w
        assert (nc, npl) == (oc.shape[0], op.shape[0]), "%s: %d corner / %d plane factors, oracle %d / %d" % (w, nc, npl, oc.shape[0], op.shape[0])
        assert np.all(s["nres"][:nc] == 3) and np.all(s["nres"][nc:] == 1)
        pc, pp = s["payload"][:nc], s["payload"][nc:]
        assert np.all(pc[:, 9] == 1.0) and np.all(pp[:, 12] == 1.0), "%s: s = 1 (DISTORTION is false)" % w
        for col, (pay, table, want) in enumerate(((pc[:, 0:3], sharp, oc[:, 0]), (pc[:, 3:6], tree_corner, oc[:, 1]), (pc[:, 6:9], tree_corner, oc[:, 2]))):
            assert_indices(candidates(pay, table), want, "%s corner column %d" % (w, col))
        for col, (pay, table, want) in enumerate(((pp[:, 0:3], flat, op[:, 0]), (pp[:, 3:6], tree_surf, op[:, 1]), (pp[:, 6:9], tree_surf, op[:, 2]),
                                                  (pp[:, 9:12], tree_surf, op[:, 3]))):
            assert_indices(candidates(pay, table), want, "%s plane column %d" % (w, col))
        assert s["residuals0"].shape == os_["residuals0"].shape
        assert np.max(np.abs(s["residuals0"] - os_["residuals0"]), initial=0) < RESID_TOL, w
        if prior is not None:
            assert np.array_equal(s["q_in"], prior[0]) and np.array_equal(s["t_in"], prior[1]), "%s: the VO prior overwrites the parameters" % w
        assert np.array_equal(s["q_in"], os_["q_in"]) and np.array_equal(s["t_in"], os_["t_in"]), "%s: parameters in" % w
        assert qdist(s["q_out"], os_["q_out"]) < POSE_TOL and np.linalg.norm(s["t_out"] - os_["t_out"]) < POSE_TOL, "%s: parameters out" % w
    qw, tw = r.lo_pose()
    oqw, otw, oql, otl = o.lo_pose()
    assert qdist(qw, oqw) < POSE_TOL * (k + 1) and np.linalg.norm(tw - otw) < POSE_TOL * (k + 1), "%s world pose" % what
    pq, pt = r.published_pose(0)
    assert np.array_equal(pq, qw) and np.array_equal(pt, tw), "%s: /laser_odom_to_init carries q_w_curr / t_w_curr" % what
    if n:
        last = r.solve(r.ODOMETRY, n - 1)
        assert qdist(last["q_out"], oql) < POSE_TOL and np.linalg.norm(last["t_out"] - otl) < POSE_TOL, "%s f2f pose" % what
        fq, ft = r.tf(0)   # base_prev_LOT_base_curr: through tf2's rotation matrix, so to rounding only
        assert qdist(fq, oql) < POSE_TOL and np.linalg.norm(ft - otl) < POSE_TOL, "%s base_prev_LOT_base_curr" % what


def run_sequence(orc, params, sweeps, walk=None, priors=None, with_mapping=False, per_sweep=None, what=""):
    """The sweeps through one reference session and one oracle session, stage by stage, compared after every stage."""
    r = ref.Loam(**params)
    o = orc.Oracle(with_mapping=with_mapping, **params)
    skip = params.get("mapping_skip_frame", 1)
    tree_corner = tree_surf = np.zeros((0, 4), np.float32)
    for k, c in enumerate(sweeps):
        w = "%s sweep %d" % (what, k)
        prior = None
        if priors is not None:
            prior = r.set_vo_prior(*priors[k])
            o.set_vo_prior(*prior)     # the oracle is handed what the reference reads back out of the tf2 transform
            assert qdist(prior[0], priors[k][0]) < 1e-15 and np.array_equal(prior[1], priors[k][1])
        assert r.stage_sr(c) == 0 and o.stage_sr(c) == 0
        clouds = [r.cloud(i) for i in range(5)]
        for i in range(5):
            assert same_cloud(clouds[i], o.cloud(i)), "%s scan registration cloud %d" % (w, i)
        assert r.stage_lo() == 0 and o.stage_lo() == 0
        compare_odometry(r, o, k, clouds[1], clouds[3], tree_corner, tree_surf, prior if k > 0 else None, w)
        tree_corner, tree_surf = clouds[2], clouds[4]
        # LaserOdometry::output: frameCount % mapping_skip_frame, counted after the increment of solveLO
        want_skip = (k + 1) % skip != 0
        assert r.skip_frame() == want_skip, "%s skip_frame" % w
        if not want_skip:
            assert same_cloud(r.cloud(5), clouds[2]) and same_cloud(r.cloud(5), o.cloud(5)), "%s laserCloudCornerLast" % w
            assert same_cloud(r.cloud(6), clouds[4]) and same_cloud(r.cloud(6), o.cloud(6)), "%s laserCloudSurfLast" % w
            assert same_cloud(r.cloud(7), clouds[0]), "%s laserCloudFullRes" % w
        if per_sweep is not None:
            per_sweep(r, o, k, want_skip, None if walk is None else walk[k], w)
    return r, o


CASES = {}


def cases():
    if not CASES:
        CASES.update(ref_cases.loam_sequences())
    return CASES


NAMES = ["64x256", "64x512", "64x2048", "hdl64e", "fuzz", "no_correspondence", "fewer_than_ten", "small_map", "skip2", "skip5", "ground_only",
         "repeated_sweep", "vo_prior", "vo_prior_skip2", "VLP_16", "HDL_32", "full_turn"]


@pytest.mark.parametrize("name", NAMES)
def test_odometry_sequences(orc, name):
    params, sweeps, _, priors = cases()[name]
    r, o = run_sequence(orc, params, sweeps, priors=priors, what=name)
    rounds = [r.solve(r.ODOMETRY, i) for i in range(r.num_solves(r.ODOMETRY))]
    assert len(rounds) == 2
    if name == "full_turn":
        q, _ = r.lo_pose()
        assert abs(q[3]) > 0.9 and abs(q[2]) < 0.45, "6.6 rad of yaw should have come (almost) all the way round: q = %s" % q
    if name not in ("no_correspondence", "fewer_than_ten"):
        assert rounds[0]["types"].size > 50, "the case must do real work: %d factors" % rounds[0]["types"].size


def test_nearby_scan_bound_decides_between_two_and_three_lines_away(orc):
    """ref_cases.nearby_scan_clouds handed to LaserOdometry::input: the reference pairs the candidate 2 scan lines up although the one
    3 lines up is nearer, in the corner walk and in the plane walk, and so does the oracle."""
    corner, surf, sharp, flat, want_c, want_p = ref_cases.nearby_scan_clouds()
    sweeps = ref_cases.synth_sequence(64, 256, 2)
    r, o = ref.Loam(), orc.Oracle(with_mapping=False)
    for x in (r, o):
        assert x.stage_sr(sweeps[0]) == 0
        x.set_sr_cloud(2, corner)
        x.set_sr_cloud(4, surf)
        assert x.stage_lo() == 0
        assert x.stage_sr(sweeps[1]) == 0
        x.set_sr_cloud(1, sharp)
        x.set_sr_cloud(3, flat)
        assert x.stage_lo() == 0
    compare_odometry(r, o, 1, sharp, flat, corner, surf, None, "nearby scan")
    oc, op = o.lo_corr(0)
    assert [tuple(v) for v in oc] == [want_c] and [tuple(v) for v in op] == [want_p], (oc, op)
    s = r.solve(r.ODOMETRY, 0)
    assert np.array_equal(s["payload"][0, 6:9], corner[3, :3].astype(np.float64)), "the reference paired the corner 2 lines up"
    assert np.array_equal(s["payload"][1, 9:12], surf[4, :3].astype(np.float64)), "the reference paired the surface point 2 lines up"


def test_degenerate_cases_reach_their_branches():
    """The far sweep leaves both rounds without a residual block (and the parameters untouched); the wedge sweep leaves fewer than ten."""
    for name, lo, hi in (("no_correspondence", 0, 0), ("fewer_than_ten", 1, 9)):
        params, sweeps, _, _ = cases()[name]
        r = ref.Loam(**params)
        for k, c in enumerate(sweeps[:4]):
            assert r.stage_sr(c) == 0 and r.stage_lo() == 0
        for outer in range(2):
            s = r.solve(r.ODOMETRY, outer)
            assert lo <= s["types"].size <= hi, (name, s["types"].size)
            if hi == 0:
                assert np.array_equal(s["q_in"], s["q_out"]) and np.array_equal(s["t_in"], s["t_out"])


def test_empty_search_cloud_is_reported_not_run():
    """A sweep without a single less-sharp corner leaves the odometry's corner kd-tree empty; the next sweep's sharp corners would make
    laser_odometry.cpp:272 read pointSearchSqDis[0] of an empty vector.  The harness says so (-2) instead of calling into that."""
    sweeps = ref_cases.synth_sequence(64, 256, 3)
    r = ref.Loam()
    assert r.stage_sr(sweeps[0]) == 0
    r.set_sr_cloud(2, np.zeros((0, 4), np.float32))
    assert r.stage_lo() == 0
    assert r.stage_sr(sweeps[1]) == 0
    assert r.stage_lo() == -2


GOLDEN_CASES = ["ref_lo_16x256_prior_skip2", "ref_lo_64x128", "ref_map_16x256", "ref_map_16x256_skip2", "ref_map_64x128"]


def test_the_golden_case_list_is_complete():
    assert sorted(ref_cases.loam_golden_cases()) == GOLDEN_CASES


@pytest.mark.parametrize("stem", GOLDEN_CASES)
def test_committed_recordings_are_what_the_reference_binary_computes(stem):
    """tests/golden/ref_lo_*.npz / ref_map_*.npz (what tests/test_gpu_ref_pinned_loam.py compares the device with, on a machine without
    the reference) regenerated from the reference binary: the same keys, every array bit for bit; each file below the largest fixture."""
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    params, sweeps, priors, with_mapping = ref_cases.loam_golden_cases()[stem]
    want = ref_cases.record_loam(ref, params, sweeps, priors, with_mapping)
    got = np.load(os.path.join(golden, stem + ".npz"))
    assert sorted(got.files) == sorted(want)
    for key in got.files:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: %s differs from what the reference binary computes now" % (stem, key)
    assert os.path.getsize(os.path.join(golden, stem + ".npz")) < os.path.getsize(os.path.join(golden, "vloam_64x256_5frames.npz"))
    rounds = [int(got["lo%d_n" % k]) for k in range(int(got["n_sweeps"]))]
    assert rounds[0] == 0 and all(r == 2 for r in rounds[1:])
    if with_mapping:
        assert any(int(got["map%d_n" % k]) == 2 for k in range(int(got["n_sweeps"]))), "the recording must hold an optimised mapping frame"
