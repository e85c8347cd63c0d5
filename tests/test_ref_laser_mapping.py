"""CPU: the oracle's laser mapping against the REFERENCE'S OWN laser_mapping.cpp, compiled unmodified (oracle/_ref/libref_loam.so through
oracle/ref.py), fed by its own scan registration and laser odometry as lidar_odometry_mapping.cpp:96-150 chains them.

Compared per sweep: whether the optimisation ran (two ceres::Solve calls or none: the `> 10 && > 50` gate); the sizes of the two
down-sampled stacks; per round the residual blocks in AddResidualBlock order — LidarEdgeFactor first, LidarPlaneNormFactor after, NO
LidarDistanceFactor (the reference has those branches commented out, laser_mapping.cpp:518-534, :582-598) —, every factor's current point
against the oracle's stack point of the same index, its line points / plane against the oracle's, the raw residuals at the initial point,
the pose before and after; the published map pose on optimised and on skipped frames; the point count of EVERY cube of the 21 x 21 x 11
window, corner and surface (which pins the window centre and each of the six roll loops: a centre off by one moves every point to another
cube); the whole /laser_cloud_map and /velodyne_cloud_registered: point count, order and bits.

Tolerances are the project's (tests/test_gpu_laser_odometry.py); integers, flags and f32 clouds are exact.

NOT pinned: the minimizer, the kd-tree (ties: lowest index), the 3 x 3 eigen-solver and the 5 x 3 least squares behind the reference
are the oracle's own restatements (oracle/ref_bridge.cpp, ref_shim/): both sides share them, so the line direction and the plane
normal are expected bit for bit and what differs can only be the reference's own text against ours.
"""
import numpy as np
import pytest

import ref

from test_ref_laser_odometry import POSE_TOL, RESID_TOL, cases, qdist, run_sequence, same_cloud

pytestmark = pytest.mark.skipif(not ref.available(), reason=ref.SKIP_REASON)

N_CUBES = 21 * 21 * 11


def oracle_cubes(o):
    cubes = [[o.map_cube(kind, c) for c in range(N_CUBES)] for kind in (0, 1)]
    counts = np.array([[p.shape[0] for p in cubes[kind]] for kind in (0, 1)], dtype=np.int64)
    parts = [cubes[kind][c] for c in range(N_CUBES) for kind in (0, 1) if cubes[kind][c].shape[0]]
    return counts, (np.concatenate(parts) if parts else np.zeros((0, 4), np.float32))


class Mapping:
    """per_sweep hook of run_sequence: runs and compares the mapping stage."""

    def __init__(self, every=1, inputs=None):
        self.inputs = inputs or {}     # sweep index -> what LaserMapping::input is handed instead of the odometry's output
        self.solved = 0
        self.cens = []
        self.every = every
        self.n = 0

    def __call__(self, r, o, k, skip, offset, w):
        q = t = None
        if offset is not None:   # both sides are handed the same pose: the oracle's odometry plus the walk
            q, t, _, _ = o.lo_pose()
            t = t + offset
        kw = dict(self.inputs.get(k, {}))
        kw.setdefault("q", q)
        kw.setdefault("t", t)
        assert r.stage_map(**kw) == 0 and o.stage_map(**kw) == 0
        assert r.map_ran() == (not skip)
        pq, pt = r.published_pose(1)
        oq, ot = o.map_published_pose()
        assert qdist(pq, oq) < POSE_TOL * (k + 1) and np.linalg.norm(pt - ot) < POSE_TOL * (k + 1), "%s published map pose" % w
        mq, mt = r.tf(2)
        assert qdist(mq, oq) < POSE_TOL * (k + 1) and np.linalg.norm(mt - ot) < POSE_TOL * (k + 1), "%s world_MOT_base_last" % w
        self.n += 1
        if skip:
            assert r.num_solves(r.MAPPING) == 0, "%s: a skipped frame solves nothing" % w
            return
        n = r.num_solves(r.MAPPING)
        assert n == o.map_num_outer() and n in (0, 2), "%s: %d mapping solves, oracle %d" % (w, n, o.map_num_outer())
        self.solved += n == 2
        log = r.map_filter_log()
        stack_c, stack_s = o.cloud(7), o.cloud(8)
        assert (int(log[0, 1]), int(log[1, 1])) == (stack_c.shape[0], stack_s.shape[0]), "%s stack sizes" % w
        for outer in range(n):
            s, os_ = r.solve(r.MAPPING, outer), o.map_solve(outer)
            ci, cab, si, spl = o.map_factors(outer)
            ww = "%s round %d" % (w, outer)
            assert s["max_num_iterations"] == 4
            ne, npn = int(np.count_nonzero(s["types"] == 0)), int(np.count_nonzero(s["types"] == 2))
            assert ne + npn == s["types"].size and np.all(s["types"][:ne] == 0), "%s: edge factors, then plane-norm factors, no distance factor" % ww
            assert (ne, npn) == (os_["corner_num"], os_["surf_num"]), "%s: %d / %d factors, oracle %d / %d" % (ww, ne, npn, os_["corner_num"], os_["surf_num"])
            pe, pn = s["payload"][:ne], s["payload"][ne:]
            assert np.array_equal(pe[:, 0:3], stack_c[ci, :3].astype(np.float64)), "%s: corner factors' stack points" % ww
            assert np.array_equal(pn[:, 0:3], stack_s[si, :3].astype(np.float64)), "%s: plane factors' stack points" % ww
            assert np.all(pe[:, 9] == 1.0)
            assert np.array_equal(pe[:, 3:9], cab), "%s: point_a / point_b" % ww
            assert np.array_equal(pn[:, 3:7], spl), "%s: plane normal and negative_OA_dot_norm" % ww
            assert s["residuals0"].shape == os_["residuals0"].shape
            assert np.max(np.abs(s["residuals0"] - os_["residuals0"]), initial=0) < RESID_TOL, ww
            assert qdist(s["q_in"], os_["q_in"]) < POSE_TOL * (k + 1) and np.linalg.norm(s["t_in"] - os_["t_in"]) < POSE_TOL * (k + 1), "%s pose before" % ww
            assert qdist(s["q_out"], os_["q_out"]) < POSE_TOL * (k + 1) and np.linalg.norm(s["t_out"] - os_["t_out"]) < POSE_TOL * (k + 1), "%s pose after" % ww
        if n == 2:
            assert np.array_equal(r.solve(r.MAPPING, 1)["q_out"], pq) and np.array_equal(r.solve(r.MAPPING, 1)["t_out"], pt), "%s: the optimised pose is what is published" % w
        self.cens.append(tuple(int(c) for c in o.map_info()["cen"]))
        if self.n % self.every == 0:
            counts, whole = oracle_cubes(o)
            assert np.array_equal(r.map_cube_counts(), counts), "%s: points per cube (window centre %s)" % (w, self.cens[-1])
            assert same_cloud(r.cloud(8), whole), "%s /laser_cloud_map" % w
            assert same_cloud(r.cloud(9), o.cloud(11)), "%s /velodyne_cloud_registered" % w


NAMES = ["64x256", "64x512", "64x2048", "hdl64e", "fuzz", "no_correspondence", "small_map", "skip2", "skip5", "ground_only", "repeated_sweep",
         "vo_prior", "vo_prior_skip2", "fewer_than_ten", "VLP_16", "HDL_32", "full_turn"]


@pytest.mark.parametrize("name", NAMES)
def test_mapping_sequences(orc, name):
    params, sweeps, _, priors = cases()[name]
    m = Mapping()
    run_sequence(orc, params, sweeps, priors=priors, with_mapping=True, per_sweep=m, what=name)
    assert m.solved >= 1, "the scan-to-map optimisation never ran"


def test_tied_neighbours_empty_and_single_cell_clouds(orc):
    """branch_cases.tie_clouds through LaserMapping::input (as tests/test_gpu_branches.py drives the device): every query has a four-way tie
    for its last three neighbours, so which three the search returns (lowest index) decides the fitted line / plane — compared factor by
    factor by the hook; then an EMPTY corner cloud and a surface cloud of 40 points in one voxel."""
    import branch_cases
    import ref_cases
    seed_c, seed_s, qc, qs = branch_cases.tie_clouds()
    ident = dict(q=[0.0, 0.0, 0.0, 1.0], t=[0.0, 0.0, 0.0])
    rng = np.random.default_rng(3)
    cell = np.zeros((40, 4), np.float32)
    cell[:, :3] = (np.array([24.05, 0.05, -1.55]) + rng.uniform(0, 0.7, (40, 3))).astype(np.float32)
    inputs = {0: dict(corner=seed_c, surf=seed_s, **ident), 1: dict(corner=qc, surf=qs, **ident),
              2: dict(corner=np.zeros((0, 4), np.float32), surf=cell, **ident)}
    m = Mapping(inputs=inputs)
    r, o = run_sequence(orc, dict(), ref_cases.synth_sequence(64, 512, 3), with_mapping=True, per_sweep=m, what="ties")
    assert m.solved == 2
    assert r.map_filter_log()[:2, 1].tolist() == [0, 1], "an empty corner stack and a one-point surface stack"


def test_collinear_map_points_give_no_plane(orc):
    """A rank-deficient 5 x 3 system: the surface map holds points on the x axis only (y = z = 0 exactly), so the plane fit has two zero
    columns.  Behind the reference's text the stand-in QR then returns the zero vector, 1 / 0 = inf fails the 0.2 test
    (laser_mapping.cpp:558-573) and no plane factor is added; the oracle adds none either.  (What Eigen's pivoted QR would return there is
    third-party behaviour and not pinned.)"""
    import branch_cases
    import ref_cases
    seed_c, _, qc, _ = branch_cases.tie_clouds()
    line = branch_cases.lattice(60, 1, 1, 0.875, (1.0, 0.0, 0.0))
    queries = line[5:50].copy()
    queries[:, 0] += np.float32(0.4375)
    ident = dict(q=[0.0, 0.0, 0.0, 1.0], t=[0.0, 0.0, 0.0])
    inputs = {0: dict(corner=seed_c, surf=line, **ident), 1: dict(corner=qc, surf=queries, **ident)}
    m = Mapping(inputs=inputs)
    r, o = run_sequence(orc, dict(), ref_cases.synth_sequence(64, 256, 2), with_mapping=True, per_sweep=m, what="collinear")
    assert m.solved == 1
    s = r.solve(r.MAPPING, 0)
    assert np.count_nonzero(s["types"] == 2) == 0 and np.count_nonzero(s["types"] == 0) > 0


def test_small_map_keeps_the_gate_shut_and_then_opens_it():
    """laser_mapping.cpp:448 with a NON-empty map: no solve while the surface map holds <= 50 points, two from then on."""
    params, sweeps, _, _ = cases()["small_map"]
    r = ref.Loam(**params)
    ran = []
    for c in sweeps:
        assert r.stage_sr(c) == 0 and r.stage_lo() == 0 and r.stage_map() == 0
        ran.append(r.num_solves(r.MAPPING))
    assert ran[:3] == [0, 0, 0] and ran[-1] == 2, ran


def test_window_rolls_in_all_six_directions(orc):
    """branch_cases.six_way_walk handed to LaserMapping::input: every one of the six `while` loops of laser_mapping.cpp:218-402 runs, and
    the points per cube of the whole window agree after every sweep."""
    params, sweeps, walk, _ = cases()["six_way_walk"]
    m = Mapping()
    run_sequence(orc, params, sweeps, walk=walk, with_mapping=True, per_sweep=m, what="six-way walk")
    d = np.diff(np.array(m.cens), axis=0)
    for a in range(3):
        assert (d[:, a] > 0).any() and (d[:, a] < 0).any(), "axis %d did not roll both ways" % a
    assert m.solved >= 10


def test_gate_opens_at_exactly_51_surface_and_11_corner_map_points(orc):
    """laser_mapping.cpp:448 is `> 10 && > 50`: with exactly 11 corner and 51 surface points in the valid block both sides optimise; with one
    surface point fewer (50) or one corner point fewer (10) neither does.  The map is seeded through LaserMapping::input on frame 0 (one point
    per voxel, so VoxelGrid keeps every one), the gate is read on frame 1."""
    import branch_cases
    import ref_cases
    sweeps = ref_cases.synth_sequence(64, 256, 2)
    surf = branch_cases.lattice(17, 3, 1, 1.0, (5.0, -1.0, -1.0))
    corner = branch_cases.lattice(11, 1, 1, 0.5, (5.0, 3.0, 0.0))
    assert surf.shape[0] == 51 and corner.shape[0] == 11
    for ncorner, nsurf, want in ((11, 51, 2), (11, 50, 0), (10, 51, 0)):
        r, o = ref.Loam(), orc.Oracle(with_mapping=True)
        for k, c in enumerate(sweeps):
            assert r.stage_sr(c) == 0 and o.stage_sr(c) == 0 and r.stage_lo() == 0 and o.stage_lo() == 0
            kw = dict(corner=corner[:ncorner], surf=surf[:nsurf], q=[0, 0, 0, 1], t=[0, 0, 0])
            assert r.stage_map(**kw) == 0 and o.stage_map(**kw) == 0
            counts = r.map_cube_counts()
            if k == 0:
                assert (int(counts[0].sum()), int(counts[1].sum())) == (ncorner, nsurf)
        assert r.num_solves(r.MAPPING) == want and o.map_num_outer() == want, (ncorner, nsurf, r.num_solves(r.MAPPING), o.map_num_outer())
