"""-m gpu: the growable voxel map (vloam_map_options::grow, vloam_create_with_options) — a handle that starts at map_capacity_log2 = 10
(1 024 slots per table, full at 614 keys) and doubles its tables between sweeps instead of dying of a full map.

The drive: 40 sweeps of 16 lines x 512 columns at 1.5 m/s with the parameters of loam_velodyne_VLP_16.launch (minimum_range 0.3, leaves
0.2 / 0.4, mapping_skip_frame 1; tests/test_gpu_launch_configs.py).  CPU pre-check (the oracle alone, asserted in `drive` below): its map
holds 7 745 / 6 289 corner / surf points after sweep 9, 13 571 / 10 348 after sweep 19, 19 504 / 14 886 after sweep 29 and 25 141 / 18 942
after sweep 39 — 41 and 31 times the 614 keys a 2^10 table takes, so the corner table needs at least 2^16 slots (6 doublings) and the
surf table 2^15 (5).  The stacks hold about 1 340 / 2 100 points per sweep.

The host grows on a bound (reported keys + sweeps in flight x what a sweep can add: two records per stack point, at most
min(7 680, max_points) corner and min(24 576, max_points) surf points), so the tables end one or two doublings above the bare need;
the tests bound that from both sides.
"""
import numpy as np
import pytest

from test_gpu_laser_mapping import oracle_published_map, qdist, same_cloud

pytestmark = pytest.mark.gpu

RINGS, COLS, N_SWEEPS = 16, 512, 40
PARAMS = dict(minimum_range=0.3, mapping_line_resolution=0.2, mapping_plane_resolution=0.4, mapping_skip_frame=1)   # loam_velodyne_VLP_16.launch:3-13
POSE_TOL = 1e-8   # tests/test_gpu_launch_configs.py
START_LOG2 = 10
FULL_AT = 614     # 60 % of 1 024 slots (k_map_finalize)
MAX_POINTS = RINGS * COLS


def handle(vl, **kw):
    return vl.Handle(0, scan_line=RINGS, with_mapping=1, max_points=MAX_POINTS, max_frames=N_SWEEPS + 8, **dict(PARAMS, **kw))


def ceil_log2(x):
    return int(np.ceil(np.log2(x)))


@pytest.fixture(scope="module")
def drive(orc, synth):
    """The sweeps (host and device copies), the oracle's poses and its final /laser_cloud_map, once.  Read-only."""
    import torch
    torch.zeros(1).cuda()   # torch brings a HIP runtime of its own: up before the library's first handle, as in tests/test_gpu_host_input.py
    seq = synth.SynthSequence(n_rings=RINGS, n_azimuth=COLS, n_sweeps=N_SWEEPS + 1, speed=1.5)
    o = orc.Oracle(scan_line=RINGS, minimum_range=PARAMS["minimum_range"], line_res=PARAMS["mapping_line_resolution"],
                   plane_res=PARAMS["mapping_plane_resolution"], mapping_skip_frame=1, with_mapping=True)
    clouds, poses = [], []
    for k in range(N_SWEEPS):
        c = seq.sweep(k)
        assert c.shape[0] == MAX_POINTS
        assert o.process(c) == 0
        qw, tw, _, _ = o.lo_pose()
        qm, tm = o.map_published_pose()
        clouds.append(c)
        poses.append(np.concatenate([qw, tw, qm, tm]))
    info = o.map_info()
    counts = (int(info["total_corner"]), int(info["total_surf"]))
    # the input overflows the start tables many times over: at least 3 doublings per table
    assert counts[0] > 8 * FULL_AT and counts[1] > 8 * FULL_AT, counts
    return dict(clouds=clouds, dev=torch.from_numpy(np.stack(clouds)).cuda(), poses=np.array(poses), map=oracle_published_map(o), counts=counts)


def assert_poses(tj, ref, what):
    assert tj.shape == ref.shape, (tj.shape, ref.shape)
    for k in range(ref.shape[0]):
        assert qdist(tj[k, 0:4], ref[k, 0:4]) < POSE_TOL and np.linalg.norm(tj[k, 4:7] - ref[k, 4:7]) < POSE_TOL, "%s: LO pose, sweep %d" % (what, k)
        assert qdist(tj[k, 7:11], ref[k, 7:11]) < POSE_TOL and np.linalg.norm(tj[k, 11:14] - ref[k, 11:14]) < POSE_TOL, "%s: map pose, sweep %d" % (what, k)


def assert_sizes(hl, counts, what):
    """Growth steps and table sizes against the oracle's counts: no smaller than the keys need, no larger than the bound can ask for (block
    keys count double — a block table has half the slots — and there are no more of them than voxels; one sweep's allowance on top)."""
    inc = 2 * min(7680, MAX_POINTS), 2 * min(24576, MAX_POINTS)
    for k in (0, 1):
        need = ceil_log2(counts[k] / 0.6)
        most = ceil_log2((2 * counts[k] + inc[k]) / 0.6)
        assert need <= hl["map_log2"][k] <= most, (what, k, hl, need, most)
        assert hl["map_log2"][k] - START_LOG2 >= 3, (what, hl)
    assert hl["map_growth_steps"] == sum(hl["map_log2"]) - 2 * START_LOG2, (what, hl)


@pytest.fixture(scope="module")
def grown(vl, drive):
    """Test 2's run, kept for the burst test: trajectory, map, health of the growable handle driven with a sync every fourth sweep."""
    h = handle(vl, map_capacity_log2=START_LOG2, map_grow=1)
    for k, c in enumerate(drive["clouds"]):
        h.process_scan(c)
        if k % 4 == 3:
            h.sync()   # VLOAM_OK throughout (raises otherwise)
    h.sync()
    out = dict(tj=h.trajectory(), map=h.get_map(), health=h.health(), map_health=h.map_health())
    h.close()
    return out


def test_control_a_fixed_handle_at_log2_10_overflows(vl, drive):
    h = handle(vl, map_capacity_log2=START_LOG2)
    for c in drive["clouds"][:12]:
        h.process_scan(c)
    with pytest.raises(vl.VloamError) as e:
        h.sync()
    assert e.value.status == vl.ERR_CAPACITY and "voxel hash full (map_capacity_log2=10)" in str(e.value)
    hl = h.health()
    assert hl["map_growth_steps"] == 0 and hl["map_log2"] == (0, 0)
    h.close()


def test_growth_parity(vl, drive, grown):
    assert_poses(grown["tj"], drive["poses"], "growable")
    assert same_cloud(grown["map"], drive["map"]), "/laser_cloud_map against the oracle"
    print("growable handle: %s, table health %s" % (grown["health"], grown["map_health"]))
    assert_sizes(grown["health"], drive["counts"], "growable")
    assert grown["map_health"]["keys"] == drive["counts"] and grown["map_health"]["purged"] == (0, 0)
    # the same run on a fixed handle of 2^22 slots: slot positions must not matter
    h = handle(vl, map_capacity_log2=22)
    for k, c in enumerate(drive["clouds"]):
        h.process_scan(c)
    h.sync()
    assert h.trajectory().tobytes() == grown["tj"].tobytes(), "poses differ from the fixed handle's"
    assert h.get_map().tobytes() == grown["map"].tobytes(), "map differs from the fixed handle's"
    h.close()


def test_growth_with_products(vl, drive):
    """map_pub_number = 5 and the registered cloud on a growable handle: every published map is vloam_get_map of a stage-wise twin at that
    sweep; the publication of sweep 9 comes right behind a growth step (forced between sweeps 8 and 9, on top of the bound's own)."""
    n = 20
    h = handle(vl, map_capacity_log2=START_LOG2, map_grow=1, map_pub_number=5, publish_registered_cloud=1)
    t = handle(vl, map_capacity_log2=START_LOG2, map_grow=1)
    published = 0
    for k in range(n):
        c = drive["clouds"][k]
        if k == 9:
            before = h.health()["map_growth_steps"]
            h.map_force_grow()
            assert h.health()["map_growth_steps"] == before + 2
        h.process_scan(c)
        t.reset_frame()
        t.scan_registration(c)
        t.laser_odometry()
        t.laser_mapping()
        if (k + 1) % 5 == 0:
            h.sync()
            m, f = h.published_map()
            assert f == k and m.shape[0] > 1000
            assert same_cloud(m, t.get_map()), "published map of sweep %d against the twin's vloam_get_map" % k
            pc, fc = h.published_cloud()
            assert fc == k and same_cloud(pc, t.features(11)), "registered cloud of sweep %d" % k
            published += 1
    assert published == 4
    h.sync()
    assert h.trajectory().tobytes() == t.trajectory().tobytes()
    h.close()
    t.close()


def test_ceiling(vl, drive):
    h = handle(vl, map_capacity_log2=START_LOG2, map_grow=1, map_max_capacity_log2=11)
    for c in drive["clouds"][:12]:
        h.process_scan(c)
    with pytest.raises(vl.VloamError) as e:
        h.sync()
    assert e.value.status == vl.ERR_CAPACITY and "max_capacity_log2=11" in str(e.value), str(e.value)
    hl = h.health()
    assert hl["map_growth_steps"] == 2 and hl["map_log2"] == (11, 11), hl   # exactly one step per table
    with pytest.raises(vl.VloamError) as e:   # the bit is sticky, as on a fixed handle
        h.sync()
    assert e.value.status == vl.ERR_CAPACITY
    h.close()


def test_raw_voxels_across_a_growth(vl, orc, synth, monkeypatch):
    """The drive of test_gpu_laser_mapping.test_returns_beyond_the_valid_block (ranges up to 140 m leave raw voxels in cubes outside the
    valid block, which the next sweeps roll back in), on a growable handle that starts at 2^10: growth steps and one same-size reclamation
    while raw voxels exist (slot ids in the deferred list change), and the map still equals the oracle's.  Why this drive and not the
    six-way walk of test_gpu_window_rolls.py: that walk's returns end at the sensor model's default range, inside the valid block, so it
    never leaves a raw voxel; this one is the suite's drive that does, and its cubes turn valid again as the sensor advances."""
    monkeypatch.setattr(synth, "MAX_RANGE", 140.0)
    n = 16
    seq = synth.SynthSequence(n_rings=64, n_azimuth=512, n_sweeps=n + 1, speed=25.0)
    h = vl.Handle(0, with_mapping=1, map_capacity_log2=START_LOG2, map_grow=1, max_points=64 * 512)
    o = orc.Oracle(with_mapping=True)
    ref, forced, doubled = [], 0, 0
    for k in range(n):
        c = seq.sweep(k)
        h.process_scan(c)
        o.process(c)
        qw, tw, _, _ = o.lo_pose()
        qm, tm = o.map_published_pose()
        ref.append(np.concatenate([qw, tw, qm, tm]))
        if k in (4, 7, 10, 13):
            h.sync()
            deferred = sum(h.map_health()["deferred"])
            if deferred > 0:
                if k == 10:
                    h.map_force_rebuild()   # the reclamation path of a growable handle: a fresh table of the same size
                else:
                    lg = h.health()["map_log2"]
                    h.map_force_grow()
                    assert h.health()["map_log2"] == (lg[0] + 1, lg[1] + 1)
                    doubled += 1
                forced += 1
                assert sum(h.map_health()["deferred"]) == deferred, "raw voxels lost by a growth step after sweep %d" % k
            assert same_cloud(h.get_map(), oracle_published_map(o)), "map after sweep %d" % k
    h.sync()
    assert forced >= 2 and doubled >= 1, "the sequence must double its tables while raw voxels exist (%d forced steps, %d doublings)" % (forced, doubled)
    tj, ref = h.trajectory(), np.array(ref)
    for k in range(n):
        assert qdist(tj[k, 0:4], ref[k, 0:4]) < POSE_TOL and np.linalg.norm(tj[k, 4:7] - ref[k, 4:7]) < POSE_TOL, k
        assert qdist(tj[k, 7:11], ref[k, 7:11]) < POSE_TOL and np.linalg.norm(tj[k, 11:14] - ref[k, 11:14]) < POSE_TOL, k
    got, want = h.get_map(), oracle_published_map(o)
    assert got.shape == want.shape and same_cloud(got, want)
    h.close()


def test_burst(vl, drive, grown):
    """All 40 sweeps enqueued from device memory before the first sync: same results, and the bound does not run away — at most one
    doubling per table more than the run that synchronised every fourth sweep."""
    dev, stride = drive["dev"], MAX_POINTS * 16
    h = handle(vl, map_capacity_log2=START_LOG2, map_grow=1)
    for k in range(N_SWEEPS):
        h.process_scan_device(dev.data_ptr() + k * stride, MAX_POINTS)
    h.sync()
    assert h.trajectory().tobytes() == grown["tj"].tobytes()
    assert h.get_map().tobytes() == grown["map"].tobytes()
    hl = h.health()
    print("burst: %s (synchronised run: %s)" % (hl, grown["health"]))
    for k in (0, 1):
        assert grown["health"]["map_log2"][k] <= hl["map_log2"][k] <= grown["health"]["map_log2"][k] + 1, (hl, grown["health"])
    assert hl["map_growth_steps"] == sum(hl["map_log2"]) - 2 * START_LOG2
    h.close()
