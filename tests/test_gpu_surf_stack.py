"""-m gpu: the large stack tier (vloam_limits::max_surf_stack_points) against the CPU oracle.

The reference has no capacity on laserCloudSurfStack (laser_mapping.cpp:432-440); a default handle takes 24 576 surf points after VoxelGrid and
reports VLOAM_ERR_CAPACITY beyond.  The input is the default 64 x 2048 street drive under a 0.2 / 0.2 m leaf (27 244 - 27 510 surf points per
sweep; tests/test_surf_stack_config.py checks that on the oracle alone) and, for row counts no natural sweep reaches, a constructed
laserCloudSurfLast of exactly 65 536 / 65 537 voxels.  The oracle's street drive is computed once (module fixture) and shared.
"""
import ctypes as C

import numpy as np
import pytest

import branch_cases
import surf_stack_cases as cases
from test_gpu_batch import same_poses
from test_gpu_laser_mapping import compare_map_round, oracle_published_map, qdist, same_cloud
from test_gpu_launch_configs import POSE_TOL, assert_map, assert_poses
from test_gpu_scan_registration import check_cloud

pytestmark = pytest.mark.gpu

LEAF = dict(mapping_line_resolution=cases.LEAF, mapping_plane_resolution=cases.LEAF)
N = cases.STREET["n_sweeps"]


class Round:
    """What compare_map_round reads of the oracle, kept per sweep."""

    def __init__(self, o):
        self.n_outer = o.map_num_outer()
        self.factors = [o.map_factors(r) for r in range(self.n_outer)]
        self.solves = [o.map_solve(r) for r in range(self.n_outer)]
        self.stacks = {w: o.cloud(w).copy() for w in (7, 8)}
        self.sr = {w: o.cloud(w).copy() for w in range(5)}
        self.lo = o.lo_pose()
        self.map = o.map_pose()
        qm, tm = o.map_published_pose()
        self.row = np.concatenate([self.lo[0], self.lo[1], qm, tm])

    def map_factors(self, outer):
        return self.factors[outer]

    def map_solve(self, outer):
        return self.solves[outer]


@pytest.fixture(scope="module")
def street(synth, orc):
    """The six sweeps, the oracle after them (poses, map) and what it held after every sweep."""
    seq = synth.SynthSequence(**cases.STREET)
    clouds = [seq.sweep(k) for k in range(N)]
    o = orc.Oracle(line_res=cases.LEAF, plane_res=cases.LEAF)
    rounds = []
    for c in clouds:
        assert o.stage_sr(c) == 0
        o.stage_lo()
        assert o.stage_map() == 0
        rounds.append(Round(o))
    for r in rounds:   # the test cannot pass on a shrunken input
        assert r.stacks[8].shape[0] > 24576 and r.stacks[7].shape[0] < 8192
    return dict(clouds=clouds, oracle=o, rounds=rounds, rows=np.array([r.row for r in rounds]))


def test_default_handle_still_refuses(vl, street):
    c = street["clouds"][0]
    h = vl.Handle(0, **LEAF)   # (vloam_create_with_limits with the default limits)
    assert h.surf_stack_cap == 24576
    h.process_scan(c)
    with pytest.raises(vl.VloamError) as e:
        h.sync()
    assert e.value.status == vl.ERR_CAPACITY
    assert "mapping factor table full" in str(e.value) and "more than 24576 surf points after VoxelGrid; raise vloam_limits::max_surf_stack_points" in str(e.value)
    h.close()
    # ... and through vloam_create, the entry point every earlier caller uses
    L = vl.lib()
    raw = C.c_void_p()
    assert L.vloam_create(C.byref(vl.default_config(**LEAF)), 0, C.byref(raw)) == vl.VLOAM_OK
    cc = np.ascontiguousarray(c, dtype=np.float32)
    assert L.vloam_process_scan(raw, cc.ctypes.data_as(C.c_void_p), cc.shape[0]) == vl.VLOAM_OK
    assert L.vloam_sync(raw) == vl.ERR_CAPACITY
    assert L.vloam_last_error().startswith(b"mapping factor table full")
    L.vloam_destroy(raw)


def test_tier_stage_by_stage(vl, street):
    h = vl.Handle(0, max_surf_stack_points=32768, debug=1, with_mapping=1, **LEAF)
    for k, c in enumerate(street["clouds"]):
        r = street["rounds"][k]
        h.reset_frame()
        h.scan_registration(c)
        for w in range(5):
            check_cloud(h.features(w), r.sr[w], "sweep %d cloud %d" % (k, w))
        qw, tw, _, _ = h.laser_odometry()
        assert qdist(qw, r.lo[0]) < POSE_TOL and np.linalg.norm(tw - r.lo[1]) < POSE_TOL, "odometry pose, sweep %d" % k
        qm, tm = h.laser_mapping()
        for w in (7, 8):
            dv, rf = h.features(w), r.stacks[w]
            assert dv.shape == rf.shape and np.array_equal(dv[:, :4].view(np.uint32), rf[:, :4].view(np.uint32)), "stack %d, sweep %d" % (w, k)
        assert h.features(8).shape[0] > 24576
        assert r.n_outer == (0 if k == 0 else 2) and h.map_state()["do_optimize"] == (0 if k == 0 else 1)
        for outer in range(r.n_outer):
            compare_map_round(h, r, outer)
        assert qdist(qm, r.map[0]) < POSE_TOL and np.linalg.norm(tm - r.map[1]) < POSE_TOL, "map pose, sweep %d" % k
    assert_poses(h.trajectory(), street["rows"], "tier, stage by stage")
    assert_map(h, street["oracle"], "tier, stage by stage")
    assert h.health()["fallback_solves"] == 0
    h.close()


def test_tier_through_the_facade_and_in_a_batch(vl, synth, street):
    hs = vl.Handle(0, max_surf_stack_points=32768, with_mapping=1, **LEAF)
    for c in street["clouds"]:
        hs.process_scan(c)
    hs.sync()
    ts = hs.trajectory()
    assert_poses(ts, street["rows"], "tier façade")
    assert_map(hs, street["oracle"], "tier façade")
    assert hs.health()["fallback_solves"] == 0
    hs.close()
    other = synth.SynthSequence(seed_scene=1251, seed_traj=43, seed_noise=6678, **cases.STREET)
    hb = vl.Handle(0, n_sessions=2, max_surf_stack_points=32768, with_mapping=1, **LEAF)
    for k, c in enumerate(street["clouds"]):
        hb.batch_process_scan([c, other.sweep(k)])
    hb.sync()
    hb.select(0)
    tb = hb.trajectory()
    assert same_poses(tb, ts), "session 0 of the batch against the single run"
    assert_poses(tb, street["rows"], "tier batch, session 0")
    assert_map(hb, street["oracle"], "tier batch, session 0")
    hb.select(1)
    assert hb.features(8).shape[0] > 24576 and not np.array_equal(hb.trajectory(), tb)
    hb.close()


def _lattice_run(vl, orc, synth, sweeps, n):
    """Two ordinary sweeps, the third one's odometry, then LaserMapping::input with a surf cloud of n points, one per voxel."""
    rings, n_az = cases.LATTICE_SHAPE
    seq = synth.SynthSequence(n_rings=rings, n_azimuth=n_az, n_sweeps=40)   # (== the `sweeps` fixture's sequence: its ground truth pose places the lattice)
    G = cases.ground_lattice(synth, seq, n)
    assert orc.voxel_grid(G, cases.LEAF).shape[0] == n
    h = vl.Handle(0, max_surf_stack_points=65536, max_points=131072, debug=1, with_mapping=1, **LEAF)
    o = orc.Oracle(line_res=cases.LEAF, plane_res=cases.LEAF)
    for k in range(cases.LATTICE_SWEEP + 1):
        c = sweeps(rings, n_az, k)
        h.reset_frame()
        h.scan_registration(c)
        h.laser_odometry()
        assert o.stage_sr(c) == 0
        o.stage_lo()
        if k < cases.LATTICE_SWEEP:
            h.laser_mapping()
            assert o.stage_map() == 0
    h.set_mapping_input(laserCloudSurfLast=G)
    return h, o, G


def test_exact_capacity_beyond_any_natural_sweep(vl, orc, synth, sweeps):
    h, o, G = _lattice_run(vl, orc, synth, sweeps, 65536)
    qm, tm = h.laser_mapping()
    assert o.stage_map(surf=G) == 0
    h.sync()
    for w in (7, 8):
        dv, rf = h.features(w), o.cloud(w)
        assert dv.shape == rf.shape and np.array_equal(dv[:, :4].view(np.uint32), rf[:, :4].view(np.uint32)), "stack %d" % w
    assert h.features(8).shape[0] == 65536
    assert o.map_num_outer() == 2
    n_plane = o.map_factors(0)[2].size
    print("plane factors accepted in outer round 0:", n_plane)
    assert n_plane >= 1000
    for outer in range(2):
        d = h.map_debug(outer)
        ci, _, si, _ = o.map_factors(outer)
        assert d["corner_idx"].size == ci.size and d["surf_idx"].size == si.size, "factor counts, outer %d" % outer
        compare_map_round(h, o, outer)
    oq, ot, _, _ = o.map_pose()
    assert qdist(qm, oq) < POSE_TOL and np.linalg.norm(tm - ot) < POSE_TOL
    assert_map(h, o, "65 536 surf points")
    assert h.health()["fallback_solves"] == 0
    h.close()
    # one point more than the handle takes
    h, o, G = _lattice_run(vl, orc, synth, sweeps, 65537)
    h.laser_mapping()
    with pytest.raises(vl.VloamError) as e:
        h.sync()
    assert e.value.status == vl.ERR_CAPACITY and "65536" in str(e.value)
    h.close()


def test_window_roll_and_rebuild_under_the_tier(vl, orc, synth, sweeps):
    """Two shifts of the cube window along x (the first leg of branch_cases.six_way_walk: laser_mapping.cpp:218-241 runs twice) and a forced
    table rebuild between sweeps, on a tier handle: poses and the whole map against the oracle."""
    rings, n_az = cases.LATTICE_SHAPE
    walk = branch_cases.six_way_walk()[:9]   # 0 .. -440 m in x
    h = vl.Handle(0, max_surf_stack_points=32768, with_mapping=1, **LEAF)
    o = orc.Oracle(line_res=cases.LEAF, plane_res=cases.LEAF)
    cens = []
    for k, off in enumerate(walk):
        c = sweeps(rings, n_az, k)
        h.reset_frame()
        h.scan_registration(c)
        h.laser_odometry()
        assert o.stage_sr(c) == 0
        o.stage_lo()
        oq, ot, _, _ = o.lo_pose()
        h.set_mapping_input(q_wodom_curr=oq, t_wodom_curr=ot + off)
        qm, tm = h.laser_mapping()
        assert o.stage_map(q=oq, t=ot + off) == 0
        mq, mt = o.map_published_pose()
        assert qdist(qm, mq) < POSE_TOL and np.linalg.norm(tm - mt) < POSE_TOL, "map pose, sweep %d" % k
        assert np.array_equal(h.map_state()["cen"], o.map_info()["cen"]), "window position, sweep %d" % k
        cens.append(int(o.map_info()["cen"][0]))
        if k in (2, 7):   # between sweeps: slot positions change, the map does not
            h.sync()
            before = h.get_map()
            h.map_force_rebuild()
            h.sync()
            assert same_cloud(h.get_map(), before), "rebuild after sweep %d" % k
    assert len(set(cens)) == 3, "two shifts along x: %s" % cens
    h.sync()
    got, want = h.get_map(), oracle_published_map(o)
    assert got.shape == want.shape and got.shape[0] > 1000
    # (far from the origin: same points in the same order, coordinates to rounding — the rule of tests/test_gpu_window_rolls.py)
    g, w = np.ascontiguousarray(got[:, :4]), np.ascontiguousarray(want[:, :4])
    assert np.array_equal(g[:, 3].view(np.uint32), w[:, 3].view(np.uint32)), "intensities"
    ulp = np.abs(g[:, :3].view(np.int32).astype(np.int64) - w[:, :3].view(np.int32).astype(np.int64))
    absd = np.abs(g[:, :3].astype(np.float64) - w[:, :3].astype(np.float64))
    assert not ((ulp > 1) & (absd > 1e-8)).any() and float(np.mean(ulp == 0)) > 0.999
    h.close()


def test_raw_voxels_and_deferred_lists_under_the_tier(vl, orc, synth, monkeypatch):
    """Ranges up to 140 m put surf points into cubes outside the valid 5 x 5 x 3 block: they stay un-merged (raw) in the reference's cube clouds
    (laser_mapping.cpp:654-659) and /laser_cloud_map lists them in arrival order — sweep, then stack index — behind the cube's filtered part.
    On the tier the stack indices of such points go beyond 16 384 (the arrival stamp's index field is 17 bits there), the lists of raw voxels
    (newraw -> deferred, k_map_prepare_tier / k_map_finalize_tier) are not empty, and a forced table rebuild re-creates them
    (k_map_rebuild_insert): the published map against the oracle's after every sweep, order included, and the poses."""
    monkeypatch.setattr(synth, "MAX_RANGE", 140.0)
    n = 6
    seq = synth.SynthSequence(n_rings=64, n_azimuth=2048, n_sweeps=n + 1, speed=25.0)
    h = vl.Handle(0, max_surf_stack_points=32768, with_mapping=1, **LEAF)
    o = orc.Oracle(line_res=cases.LEAF, plane_res=cases.LEAF)
    ref, seen, high = [], 0, 0
    for k in range(n):
        c = seq.sweep(k)
        h.process_scan(c)
        assert o.process(c) == 0
        st = o.cloud(8)
        assert 24576 < st.shape[0] <= 32768
        high += int(np.count_nonzero(np.nonzero(np.linalg.norm(st[:, :3], axis=1) > 100.0)[0] >= 16384))
        qw, tw, _, _ = o.lo_pose()
        qm, tm = o.map_published_pose()
        ref.append(np.concatenate([qw, tw, qm, tm]))
        h.sync()
        deferred = h.map_health()["deferred"]
        seen = max(seen, sum(deferred))
        assert same_cloud(h.get_map(), oracle_published_map(o)), "published map after sweep %d" % k
        if k == 2:   # slot ids change: both lists are rebuilt from the raw flags
            h.map_force_rebuild()
            h.sync()
            assert h.map_health()["deferred"] == deferred and sum(deferred) > 0
            assert same_cloud(h.get_map(), oracle_published_map(o)), "published map after the rebuild"
    assert seen > 0, "the sequence must reach cubes outside the valid block"
    assert high > 100, "far surf points must sit at stack indices beyond 16 384"
    assert_poses(h.trajectory(), np.array(ref), "tier, far returns")
    assert h.health()["fallback_solves"] == 0
    h.close()
