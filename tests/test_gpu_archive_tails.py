"""-m gpu: the map archive with UN-MERGED ARRIVALS in the evicted cubes, against the CPU oracle.

tests/test_gpu_map_archive.py's walk reaches no cube outside the valid 5 x 5 x 3 block, so none of its rows is a raw voxel's point.  Here the
same six-way walk runs with the sensor model's range raised to 140 m (tests/raw_tail_cases.py; tests/test_raw_tail_cases.py pins what the
oracle's bookkeeping expects: 84 587 rows in 385 groups, 125 of them un-merged arrivals in 25 groups, 7 of those with a filtered prefix, both
kinds).  Checked: flags bit 1 (the tail bit of rec_order_key) on exactly the oracle's tail rows, behind every merged row of their group and in
arrival order; no row for a raw voxel's running sum (rec_is_point); the get order with the tail column live; an archive that fills up inside
a group with a tail; the tail rows imported into a fresh handle.

Every drive hands the device the ORACLE's odometry pose plus the walk's offset, so what is compared is the mapping stage and the archive."""
import numpy as np
import pytest

import map_archive_cases as cases
import raw_tail_cases as rt
import voxel_key_model
from test_gpu_laser_mapping import qdist
from test_gpu_map_archive import GROW_START_LOG2, POSE_TOL, close_to_oracle, rows_xyzi

pytestmark = pytest.mark.gpu
CAPACITY = 1 << 20

_runs = {}


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings a HIP runtime of its own: up before this module's first handle (tests/test_gpu_host_input.py); modules that run behind this
    one (tests/test_gpu_carve_raw.py first of all) hand torch tensors to the library."""
    import torch
    torch.zeros(1).cuda()


@pytest.fixture(scope="module")
def ref(orc, synth):
    r = rt.walk_reference(orc, synth)
    f = rt.figures(r)
    # the preconditions of tests/test_raw_tail_cases.py: a test could pass on nothing otherwise
    assert f["tail_rows"] >= 100 and f["mixed"] >= 5 and f["all_tail"] >= 1 and min(f["tail_rows_of_kind"]) >= 1, f
    return r


@pytest.fixture(scope="module", autouse=True)
def close_handles():
    yield
    for r in _runs.values():
        r["h"].close()
    _runs.clear()


def drive(vl, ref, key, archive=None, **handle_kw):
    """The walk on one handle (cached by key; the handle stays open until the module ends).  archive: capacity_rows, or None."""
    if key in _runs:
        return _runs[key]
    n = len(ref["walk"])
    h = vl.Handle(0, scan_line=cases.RINGS, with_mapping=1, max_frames=n + 8, sweep_log=1, **handle_kw)
    if archive is not None:
        h.map_archive_enable(capacity_rows=archive)
    poses = []
    for k in range(n):
        h.reset_frame()
        h.scan_registration(ref["clouds"][k])
        h.laser_odometry()
        h.set_mapping_input(q_wodom_curr=ref["oq"][k], t_wodom_curr=ref["ot"][k] + ref["walk"][k])
        poses.append(h.laser_mapping())
    h.sync()   # raises on any sticky error
    out = dict(h=h, poses=poses, traj=h.trajectory(), map=h.get_map(), log=h.sweep_log(), health=h.health(), deferred=h.map_health()["deferred"])
    if archive is not None:
        out["info"] = h.map_archive_info()
    _runs[key] = out
    return out


@pytest.mark.parametrize("kind_of_handle", ["fixed", "growable"])
def test_rows_and_tail_bits_equal_the_oracles(vl, ref, kind_of_handle):
    if kind_of_handle == "fixed":
        r = drive(vl, ref, "fixed", archive=CAPACITY)
    else:
        r = drive(vl, ref, "growable", archive=CAPACITY, map_grow=1, map_capacity_log2=GROW_START_LOG2)
        assert r["health"]["map_growth_steps"] >= 1 and max(r["health"]["map_log2"]) > GROW_START_LOG2, r["health"]
    rows = r["h"].map_archive()
    groups = rt.groups(ref)
    total = sum(g[3].shape[0] for g in groups)
    # one row per point of the oracle's clouds: a raw voxel's running sum (seq 0, kRecRaw) would be a row too many
    assert r["info"]["rows"] == total == rows.shape[0] and r["info"]["dropped"] == 0 and r["info"]["capacity_rows"] == CAPACITY
    assert r["info"]["rolls"] == int(np.count_nonzero(np.diff(np.concatenate([[[10, 10, 5]], ref["cen"]]), axis=0).any(axis=1)))
    # the key (sweep, kind, cube_k, cube_j, cube_i, tail, order) is unique and the rows come sorted by it: the tail column is live here
    kind, tail = (rows["flags"] & 1).astype(np.int64), ((rows["flags"] >> 1) & 1).astype(np.int64)
    assert not (rows["flags"] >> 2).any()
    assert int(tail.sum()) == sum(g[4] for g in groups) >= 100
    key = np.stack([rows["sweep"], kind, rows["cube_k"], rows["cube_j"], rows["cube_i"], tail, rows["order"]], 1).astype(np.int64)
    order = np.lexsort(key.T[::-1])
    assert np.array_equal(order, np.arange(rows.shape[0])), "get order"
    assert (np.diff(key, axis=0) != 0).any(axis=1).all(), "duplicate key"
    # group by group against the oracle: count, sweep, kind and cube exact; the tail bit on exactly the last `tail` rows
    at, want_pts, n_mixed, n_all_tail = 0, [], 0, 0
    for sweep, k, cube, pts, n_tail in groups:
        m = pts.shape[0]
        g = rows[at:at + m]
        assert g.shape[0] == m and (g["sweep"] == sweep).all() and ((g["flags"] & 1) == k).all() and \
            (g["cube_i"] == cube[0]).all() and (g["cube_j"] == cube[1]).all() and (g["cube_k"] == cube[2]).all(), (sweep, k, cube, m, g[:3])
        t = (g["flags"] >> 1) & 1
        assert not t[:m - n_tail].any() and t[m - n_tail:].all(), "tail bits of %s: %s, the oracle's tail is %d of %d" % ((sweep, k, cube), t, n_tail, m)
        if n_tail:
            # (every merged row before every tail row: the line above; inside the tail the arrival stamps rise)
            assert (np.diff(g["order"][m - n_tail:].astype(np.int64)) > 0).all() and (g["order"][m - n_tail:] != 0).all(), (sweep, k, cube, g["order"][m - n_tail:])
            n_mixed, n_all_tail = n_mixed + (n_tail < m), n_all_tail + (n_tail == m)
        want_pts.append(pts)
        at += m
    assert at == rows.shape[0] and n_mixed >= 5 and n_all_tail >= 1
    # row order == the oracle's cloud order: intensities bit for bit, coordinates within rounding, by position
    ulp = close_to_oracle(rows_xyzi(rows), np.concatenate(want_pts))
    assert float(np.mean(ulp == 0)) > 0.999
    # in the same run: the map poses, the final map and the raw voxels left in the window
    for k, (qm, tm) in enumerate(r["poses"]):
        assert qdist(qm, ref["map_q"][k]) < POSE_TOL and np.linalg.norm(tm - ref["map_t"][k]) < POSE_TOL, "map pose, sweep %d" % k
    assert np.array_equal(r["h"].map_state()["cen"], ref["cen"][-1])
    ulp = close_to_oracle(r["map"], ref["final_map"])
    assert float(np.mean(ulp == 0)) > 0.999
    last = len(ref["walk"]) - 1
    assert list(r["deferred"]) == [rt.raw_voxels(ref, last, kk).shape[0] for kk in (0, 1)] and sum(r["deferred"]) > 0
    print("%s handle: %d rows (%d un-merged, %d mixed groups), health %s" % (kind_of_handle, rows.shape[0], int(tail.sum()), n_mixed, r["health"]))


def test_overflow_inside_a_group_with_a_tail(vl, ref):
    """The capacity ends, in the get order, one row into the tail of the first group that has a filtered prefix and a tail.  Which rows of the
    overflowing sweep are held is not defined (they are appended as the slot walk meets them); how many, and what the sequence sees, is."""
    groups = rt.groups(ref)
    at, cap, sweep_full = 0, None, None
    for sweep, k, cube, pts, n_tail in groups:
        if 0 < n_tail < pts.shape[0]:
            cap, sweep_full = at + pts.shape[0] - n_tail + 1, sweep
            break
        at += pts.shape[0]
    total = sum(g[3].shape[0] for g in groups)
    before = sum(g[3].shape[0] for g in groups if g[0] < sweep_full)
    assert cap is not None and before < cap < before + sum(g[3].shape[0] for g in groups if g[0] == sweep_full) and cap < total
    r = drive(vl, ref, "overflow", archive=cap)   # every status on the way was VLOAM_OK, vloam_sync included, or drive() had raised
    assert r["info"]["rows"] == cap and r["info"]["rows"] + r["info"]["dropped"] == total and r["info"]["capacity_rows"] == cap
    rows = r["h"].map_archive()
    whole = drive(vl, ref, "fixed", archive=CAPACITY)["h"].map_archive()
    assert rows.shape[0] == cap and (rows["sweep"] <= sweep_full).all()
    assert rows[rows["sweep"] < sweep_full].tobytes() == whole[whole["sweep"] < sweep_full].tobytes(), "the sweeps before the archive filled up are whole"
    have = {row.tobytes() for row in whole[whole["sweep"] == sweep_full]}
    part = rows[rows["sweep"] == sweep_full]
    assert part.shape[0] == cap - before and len({row.tobytes() for row in part}) == part.shape[0] and all(row.tobytes() in have for row in part)
    plain = drive(vl, ref, "plain")
    assert r["traj"].tobytes() == plain["traj"].tobytes()
    assert r["map"].tobytes() == plain["map"].tobytes() and plain["map"].shape[0] > 1000
    assert r["log"].tobytes() == plain["log"].tobytes()


def test_tail_rows_round_trip_through_map_import(vl, ref):
    """The archived un-merged arrivals of each kind imported into a fresh handle: three of them, picked by index among those alone in their
    voxel (an import folds the points of one voxel into their centroid), are map points there."""
    r = drive(vl, ref, "fixed", archive=CAPACITY)
    rows = r["h"].map_archive()
    tails = rows[(rows["flags"] & 2) != 0]
    arch = [np.ascontiguousarray(rows_xyzi(tails[(tails["flags"] & 1) == k])) for k in (0, 1)]
    assert arch[0].shape[0] >= 3 and arch[1].shape[0] >= 3
    for k in (0, 1):
        # a window around the kind's tail rows: the cube of their median (the rows of one kind lie within a few cubes of it, or count as outside)
        centre = np.median(arch[k][:, :3].astype(np.float64), axis=0)
        h = vl.Handle(0, scan_line=cases.RINGS, with_mapping=1)
        try:
            res = h.map_import(arch[k] if k == 0 else None, arch[k] if k == 1 else None, t_wmap_wodom=centre)
            cen = res["center_cube"].astype(np.int64)
            ijk = voxel_key_model.cube_abs(arch[k][:, :3]) + cen
            inside = ((ijk >= 0) & (ijk < cases.SIZE)).all(axis=1)
            assert res["n_in"][k] == arch[k].shape[0] and res["n_in"][k] - res["n_outside_window"][k] == int(inside.sum())
            vox = rt.voxel_rows(arch[k], k)
            _, inv, cnt = np.unique(vox, axis=0, return_inverse=True, return_counts=True)
            cand = np.nonzero(inside & (cnt[inv.ravel()] == 1))[0]
            assert cand.shape[0] >= 3, cand.shape
            for i in (cand[0], cand[cand.shape[0] // 2], cand[-1]):
                p = arch[k][i:i + 1]
                xyzi, d2, count = h.map_query(p, k=1, max_radius=0.05, kind=k)
                assert count[0] == 1 and d2[0, 0] == 0.0 and np.array_equal(xyzi[0, 0].view(np.uint32), p[0].view(np.uint32)), (k, i, p, xyzi, d2)
        finally:
            h.close()
