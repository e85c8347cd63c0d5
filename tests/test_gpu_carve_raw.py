"""-m gpu: map clean-up, pose scores and localisation on a map that holds RAW VOXELS (un-merged arrivals, csrc/map_table.h), against the CPU
oracle's bookkeeping (tests/raw_tail_cases.py) and the NumPy models (tests/carve_model.py, tests/pose_score_model.py).

The drive is raw_tail_cases.out_and_back_reference: the first seven offsets of the six-way walk (55 m per sweep along -x) with the sensor
model's range at 140 m, the device fed the ORACLE's odometry poses, then six sweeps back through the wake.  Behind sweep 6 the window holds
48 corner and 15 surf raw voxels (tests/test_raw_tail_cases.py pins the counts); on the way back their cubes re-enter the valid block.
    carve      skipped_raw counts exactly those voxels, examined leaves out the points inside them, the rest equals the model on the rest;
               apply (same-size reclamation, fixed and growable table) keeps every raw point, the deferred lists and the occupancy blocks;
               a checkpoint of the carved map walks back like the handle it came from
    scores     bit for bit the model over get_map_kind's points, with feature points whose nearest map point is a raw point
    localize   the dry run of the sweep in progress equals the mapping that follows, right behind sweeps that created raw voxels (the
               newraw list k_map_prepare merges and the dry run does not)"""
import numpy as np
import pytest

import carve_model as cm
import map_archive_cases as cases
import pose_score_model as model
import raw_tail_cases as rt
from carve_scene import sorted_rows
from test_gpu_carve import COUNTERS, same_rows
from test_gpu_localize import dry_run_is_the_mapping
from test_gpu_map_archive import close_to_oracle
from test_gpu_pose_score import bits, device_scores, features_of, leaf_bounds, perturbed, thin

pytestmark = pytest.mark.gpu
K = rt.N_CARVE
# the range image of the 64 x 256 sweeps; 80 m keeps the model's per-point loop at a few seconds (every map point is in range of three sweeps)
CARVE = dict(rows=64, cols=256, elev_min_deg=-25.0, elev_max_deg=3.0, min_range=2.0, max_range=80.0, range_res=0.05, margin=0.5)
GROW = dict(map_grow=1, map_capacity_log2=12)


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings a HIP runtime of its own: up before this module's first handle (tests/test_gpu_host_input.py); the device form takes tensors."""
    import torch
    torch.zeros(1).cuda()


@pytest.fixture(scope="module")
def ref(orc, synth):
    r = rt.out_and_back_reference(orc, synth)
    assert not r["expected"], "no cube leaves the window on this drive"
    return r


def sweep(h, ref, k, dry_run=False):
    """one sweep of the drive; dry_run: vloam_map_localize of the sweep in progress, in front of its mapping"""
    h.reset_frame()
    h.scan_registration(ref["clouds"][k])
    h.laser_odometry()
    h.set_mapping_input(q_wodom_curr=ref["oq"][k], t_wodom_curr=ref["ot"][k] + ref["walk"][k])
    r = h.map_localize(None, None, None, None) if dry_run else None
    qm, tm = h.laser_mapping()
    return r, qm, tm


def driven(vl, ref, **kw):
    """a handle behind sweep K - 1, and its raw-voxel counts behind every sweep"""
    h = vl.Handle(0, scan_line=cases.RINGS, with_mapping=1, max_frames=32, sweep_log=1, **kw)
    deferred = []
    for k in range(K):
        sweep(h, ref, k)
        deferred.append(list(h.map_health()["deferred"]))
    h.sync()
    return h, deferred


def carve_args(h, ref):
    tj = h.trajectory()
    return [ref["clouds"][k] for k in range(K)], np.array([tj[k, 7:14] for k in range(K)])


@pytest.fixture(scope="module")
def base(vl, ref):
    """The fixed-size handle behind sweep K - 1: its export, which of its points lie in raw voxels, the model's carve of the rest.  Read-only."""
    h, deferred = driven(vl, ref)
    maps = [h.get_map_kind(kind) for kind in (0, 1)]
    voxels = [rt.raw_voxels(ref, K - 1, kind) for kind in (0, 1)]
    in_raw = [rt.in_voxels(maps[kind], kind, voxels[kind]) for kind in (0, 1)]
    sweeps, poses = carve_args(h, ref)
    mdl = [cm.carve(maps[kind][~in_raw[kind]], sweeps, poses, **CARVE) for kind in (0, 1)]
    yield dict(h=h, deferred=deferred, maps=maps, voxels=voxels, in_raw=in_raw, sweeps=sweeps, poses=poses, model=mdl)
    h.close()


def test_the_drive_leaves_the_oracles_raw_voxels(ref, base):
    want = [[v.shape[0] for v in (rt.raw_voxels(ref, k, 0), rt.raw_voxels(ref, k, 1))] for k in range(K)]
    assert base["deferred"] == want and sum(want[-1]) > 0, (base["deferred"], want)
    for kind in (0, 1):
        # the export is the oracle's map, the un-merged arrivals of every cube behind its filtered part
        ulp = close_to_oracle(base["maps"][kind], ref["map_after"][K - 1][kind])
        assert float(np.mean(ulp == 0)) > 0.999
        tails = ref["raw"][K - 1][kind]["points"]
        have = {row.tobytes() for row in np.ascontiguousarray(base["maps"][kind][base["in_raw"][kind]])}
        assert tails.shape[0] >= base["voxels"][kind].shape[0] > 0 and all(row.tobytes() in have for row in np.ascontiguousarray(tails))
        assert int(base["in_raw"][kind].sum()) == int(rt.in_voxels(ref["map_after"][K - 1][kind], kind, base["voxels"][kind]).sum())


def test_carve_dry_run_skips_raw_voxels_and_equals_the_model_on_the_rest(base):
    b, h = base, base["h"]
    removed, res = h.map_carve(b["sweeps"], b["poses"], **CARVE)
    want = np.concatenate([b["maps"][kind][~b["in_raw"][kind]][b["model"][kind][0]] for kind in (0, 1)])
    assert want.shape[0] >= 50 and all(b["model"][kind][1]["removed"] > 0 for kind in (0, 1)), "the model alone must remove points: %d" % want.shape[0]
    for kind in (0, 1):
        got = {k: int(res[k][kind]) for k in COUNTERS}
        print("kind %d: device %s skipped_raw %d, model %s" % (kind, got, res["skipped_raw"][kind], b["model"][kind][1]))
        assert int(res["skipped_raw"][kind]) == b["voxels"][kind].shape[0] > 0
        assert got["examined"] == b["maps"][kind].shape[0] - int(b["in_raw"][kind].sum())
        assert got == b["model"][kind][1]
        assert same_rows(h.get_map_kind(kind), b["maps"][kind]), "a dry run leaves the map as it was"
    assert res["n_removed_out"] == want.shape[0] == removed.shape[0]
    assert same_rows(sorted_rows(removed), sorted_rows(want))
    assert list(h.map_health()["deferred"]) == b["deferred"][-1]


@pytest.mark.parametrize("grow", [0, 1], ids=["fixed", "growable"])
def test_apply_keeps_raw_voxels_and_a_checkpoint_walks_back_alike(vl, ref, base, grow):
    b = base
    h, deferred = driven(vl, ref, **(GROW if grow else {}))
    h2 = vl.Handle(0, scan_line=cases.RINGS, with_mapping=1, max_frames=32, sweep_log=1, **(GROW if grow else {}))
    try:
        assert deferred == b["deferred"]
        if grow:
            assert h.health()["map_growth_steps"] >= 1
        for kind in (0, 1):
            assert same_rows(h.get_map_kind(kind), b["maps"][kind])
        rebuilds = h.health()["rebuilds"]
        removed, res = h.map_carve(b["sweeps"], b["poses"], apply=True, **CARVE)
        gone = {row.tobytes() for row in np.ascontiguousarray(removed)}
        assert removed.shape[0] == sum(b["model"][kind][1]["removed"] for kind in (0, 1)) >= 50
        assert h.health()["rebuilds"] == rebuilds + 2, "both tables went through the same-size reclamation"
        picks = 0
        for kind in (0, 1):
            assert {k: int(res[k][kind]) for k in COUNTERS} == b["model"][kind][1] and int(res["skipped_raw"][kind]) == b["voxels"][kind].shape[0]
            before = b["maps"][kind]
            keep = np.array([row.tobytes() not in gone for row in np.ascontiguousarray(before)])
            assert int((~keep).sum()) == int(res["removed"][kind]) and keep[b["in_raw"][kind]].all()
            after = h.get_map_kind(kind)
            assert same_rows(after, before[keep]), "the export is the export before minus the removed points, in the same order"
            raw = np.ascontiguousarray(before[b["in_raw"][kind]])
            have = {row.tobytes() for row in np.ascontiguousarray(after)}
            assert all(row.tobytes() in have for row in raw), "every raw point is still there, bit for bit"
            # the occupancy blocks of raw voxels survive the reclamation: raw points, by index, are found at distance 0
            idx = np.unique(np.linspace(0, raw.shape[0] - 1, 10).astype(np.int64))
            xyzi, d2, cnt = h.map_query(raw[idx], k=1, max_radius=0.05, kind=kind)
            assert (cnt == 1).all() and (d2[:, 0] == 0.0).all() and same_rows(xyzi[:, 0], raw[idx]), (kind, idx, cnt, d2)
            picks += idx.size
        assert picks == 20
        assert list(h.map_health()["deferred"]) == b["deferred"][-1], "the raw-voxel lists are what they were"
        assert h.map_health()["purged"] == (0, 0)
        # checkpoint after apply, and the way back: raw cubes re-enter the valid block
        h2.restore(h.checkpoint())
        for kind in (0, 1):
            assert same_rows(h2.get_map_kind(kind), h.get_map_kind(kind))
        assert list(h2.map_health()["deferred"]) == b["deferred"][-1]
        back = []
        for k in range(K, K + rt.N_BACK):
            for hh in (h, h2):
                sweep(hh, ref, k)
            back.append(list(h.map_health()["deferred"]))
            assert list(h2.map_health()["deferred"]) == back[-1]
        for hh in (h, h2):
            hh.sync()
        # a carve removes merged voxels only, so which voxels are raw is what the oracle's (uncarved) bookkeeping says
        assert back == [[rt.raw_voxels(ref, k, kind).shape[0] for kind in (0, 1)] for k in range(K, K + rt.N_BACK)], back
        seq = [b["deferred"][-1]] + back
        assert any(seq[i + 1][kind] < seq[i][kind] for i in range(len(back)) for kind in (0, 1)), "no raw cube re-entered the valid block: %s" % seq
        assert h.trajectory()[K:].tobytes() == h2.trajectory()[-rt.N_BACK:].tobytes() and np.isfinite(h.trajectory()).all()
        assert h.get_map().tobytes() == h2.get_map().tobytes()
        assert h.sweep_log()[K:].tobytes() == h2.sweep_log()[-rt.N_BACK:].tobytes() and not h.sweep_log()["error_bits"].any()
    finally:
        h.close()
        h2.close()


def test_pose_scores_with_raw_points_in_reach(vl, ref, base):
    b, h = base, base["h"]
    rng = np.random.default_rng(31)
    corner, surf = features_of(vl, ref["clouds"][K - 1])
    # thinned as tests/test_gpu_pose_score.py does it, but every return beyond 100 m is kept: the raw points lie 105 m and more from the sensor
    def thinned(cloud, n):
        far = np.linalg.norm(cloud[:, :3].astype(np.float64), axis=1) > 100.0
        return np.ascontiguousarray(np.concatenate([cloud[far], thin(cloud[~far], n)]), dtype=np.float32)
    corner, surf = thinned(corner, 96), thinned(surf, 256)
    true = h.trajectory()[K - 1, 7:14].copy()
    true[:4] /= np.linalg.norm(true[:4])
    poses = np.ascontiguousarray([true] + perturbed(rng, true, 10, 0.2, 1.0) + perturbed(rng, true, 5, 2.0, 10.0))
    assert poses.shape == (16, 7)
    # precondition, by brute force in f64: feature points whose nearest map point, within the radius, is a raw point (at the sweep's own pose)
    n_raw_nn = 0
    for kind, cloud in enumerate((corner, surf)):
        p = model.associate(cloud, true[:4], true[4:]).astype(np.float64)
        m = b["maps"][kind][:, :3].astype(np.float64)
        for a in range(0, p.shape[0], 128):
            d = ((p[a:a + 128, None, :] - m[None, :, :]) ** 2).sum(axis=2)
            n_raw_nn += int((b["in_raw"][kind][d.argmin(axis=1)] & (d.min(axis=1) <= 1.0)).sum())
    assert n_raw_nn >= 20, "feature points whose counted neighbour is a raw point: %d (of %d corner, %d surf)" % (n_raw_nn, corner.shape[0], surf.shape[0])
    tabs = model.dmin_tables(b["maps"], corner, surf, poses)
    for stride, radius in [(stride, radius) for stride in ((1, 1), (3, 7)) for radius in ((1.0, 1.0), (0.2, 0.4), leaf_bounds(h))]:
        want = model.records(tabs, stride, radius)
        got = h.map_score_poses(corner, surf, poses, stride=stride, radius=radius)
        what = "stride %s radius %s" % (stride, radius)
        bad = [m for m in range(16) if bits(got[m]) != bits(want[m])]
        assert not bad, "%s: poses %s, e.g. device %s model %s" % (what, bad[:8], got[bad[0]], want[bad[0]])
        assert bits(got) == bits(want)
        assert bits(device_scores(vl, h, corner, surf, poses, stride=stride, radius=radius)) == bits(got), "%s: device form" % what
    got = h.map_score_poses(corner, surf, poses)
    assert np.array_equal(vl.score_rank(got), model.rank(got)) and got["n_hit"][0].sum() > 0
    print("scores: %d corner and %d surf points, %d with a raw point as their counted neighbour, hits at the true pose %s of %s"
          % (corner.shape[0], surf.shape[0], n_raw_nn, got["n_hit"][0], got["n_used"][0]))
    h.sync()


def test_dry_run_equals_the_mapping_behind_new_raw_voxels(vl, ref, base):
    """vloam_map_localize does not merge the newraw list into the deferred list as k_map_prepare does: behind a sweep that turned voxels raw
    the dry run must still see the raw set the mapping sees."""
    h, deferred = driven(vl, ref)
    try:
        assert deferred == base["deferred"]
        solved = 0
        for k in (K, K + 1):
            # the sweep before created raw voxels: more of them than behind the sweep before it, of either kind
            assert all(deferred[-1][kind] > deferred[-2][kind] for kind in (0, 1)), deferred
            r, qm, tm = sweep(h, ref, k, dry_run=True)
            solved += dry_run_is_the_mapping(vl, h, r, qm, tm, k)
            deferred.append(list(h.map_health()["deferred"]))
        assert solved == 2, "both sweeps must solve against the map"
        h.sync()
    finally:
        h.close()
