"""-m gpu: the map archive (vloam_map_archive_*): the points of cubes that roll out of the 21 x 21 x 11 window, against the CPU oracle.

The drive is branch_cases.six_way_walk through vloam_set_mapping_input, as tests/test_gpu_window_rolls.py does it: 59 sweeps of 64 x 256, rolls
on all six faces.  The expected rows come from the oracle alone (tests/map_archive_cases.py: the clouds of the cubes a sweep's shift pushes out
of the window, taken before that sweep's LaserMapping::input).  That bookkeeping, run on the CPU, expects
    corner  124 179 rows: sweep 41: 88, 42: 2 492, 55: 1 525, 56: 25 250, 57: 68 327, 58: 26 497
    surf     65 848 rows: sweep 41: 2,  42: 1 257, 55: 514,   56: 14 685, 57: 34 983, 58: 14 407
in 346 (sweep, kind, cube) groups; the first eviction is on sweep 41.  (The walk's first leg moves the window without a cube that holds points
leaving it; the returns through mapped places evict.)  None of these rows is an un-merged arrival (the sweeps reach no cube outside the valid
block), so the tail bit is zero in every row checked here; tests/test_gpu_archive_tails.py runs the walk at 140 m, where it is not.  The tests assert that both kinds are present and that the set spans at least two sweeps.

Every drive hands the device the ORACLE's odometry pose plus the walk's offset, so what is compared is the mapping stage and the archive."""
import ctypes as C

import numpy as np
import pytest

import map_archive_cases as cases
import voxel_key_model
from test_gpu_laser_mapping import qdist

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-8                 # test_gpu_window_rolls.py's bar on the map pose
EXPECTED = {0: {41: 88, 42: 2492, 55: 1525, 56: 25250, 57: 68327, 58: 26497}, 1: {41: 2, 42: 1257, 55: 514, 56: 14685, 57: 34983, 58: 14407}}
GROW_START_LOG2 = 12            # 4 096 slots: the walk's map needs several doublings

_runs = {}


@pytest.fixture(scope="module")
def ref(orc, synth):
    r = cases.walk_reference(orc, synth)
    counts = cases.expected_counts(r)
    # the precondition: a test could pass on nothing otherwise
    assert counts[0] and counts[1] and len(set(counts[0]) | set(counts[1])) >= 2
    assert counts == EXPECTED, counts
    return r


@pytest.fixture(scope="module", autouse=True)
def close_handles():
    yield
    for r in _runs.values():
        r["h"].close()
    _runs.clear()


def drive(vl, ref, key, archive=None, drain_after=None, **handle_kw):
    """The walk on one handle (cached by key; the handle stays open until the module ends).  archive: capacity_rows, or None for a handle
    without the archive.  drain_after: a sweep behind which map_archive(clear=True) is called."""
    if key in _runs:
        return _runs[key]
    n = len(ref["walk"])
    h = vl.Handle(0, scan_line=cases.RINGS, with_mapping=1, max_frames=n + 8, sweep_log=1, **handle_kw)
    if archive is not None:
        h.map_archive_enable(capacity_rows=archive)
    poses, drained, info_after_drain = [], [], None
    for k in range(n):
        h.reset_frame()
        h.scan_registration(ref["clouds"][k])
        h.laser_odometry()
        h.set_mapping_input(q_wodom_curr=ref["oq"][k], t_wodom_curr=ref["ot"][k] + ref["walk"][k])
        poses.append(h.laser_mapping())
        if drain_after == k:
            drained.append(h.map_archive(clear=True))
            info_after_drain = h.map_archive_info()
    h.sync()   # raises on any sticky error
    out = dict(h=h, poses=poses, traj=h.trajectory(), map=h.get_map(), log=h.sweep_log(), health=h.health(), drained=drained, info_after_drain=info_after_drain)
    if archive is not None:
        out["info"] = h.map_archive_info()
    _runs[key] = out
    return out


def close_to_oracle(got, want):
    """test_gpu_window_rolls.py's rule for map coordinates at |t| ~ 600 m: intensities bit for bit; a coordinate at most 1 ulp or at most 1e-8 m off."""
    g, w = np.ascontiguousarray(got[:, :4]), np.ascontiguousarray(want[:, :4])
    assert g.shape == w.shape
    assert np.array_equal(g[:, 3].view(np.uint32), w[:, 3].view(np.uint32)), "intensities"
    ulp = np.abs(g[:, :3].view(np.int32).astype(np.int64) - w[:, :3].view(np.int32).astype(np.int64))
    absd = np.abs(g[:, :3].astype(np.float64) - w[:, :3].astype(np.float64))
    bad = (ulp > 1) & (absd > 1e-8)
    assert not bad.any(), "coordinates beyond rounding: rows %s\n%s\n%s" % (np.nonzero(bad.any(axis=1))[0][:8], g[bad.any(axis=1)][:6], w[bad.any(axis=1)][:6])
    return ulp


def rows_xyzi(rows):
    return np.stack([rows["x"], rows["y"], rows["z"], rows["intensity"]], 1)


@pytest.mark.parametrize("kind_of_handle", ["fixed", "growable"])
def test_rows_equal_the_oracles(vl, ref, kind_of_handle):
    if kind_of_handle == "fixed":
        r = drive(vl, ref, "fixed", archive=1 << 20)
    else:
        r = drive(vl, ref, "growable", archive=1 << 20, map_grow=1, map_capacity_log2=GROW_START_LOG2)
        assert r["health"]["map_growth_steps"] >= 1 and max(r["health"]["map_log2"]) > GROW_START_LOG2, r["health"]
    rows = r["h"].map_archive()
    total = sum(sum(v.values()) for v in EXPECTED.values())
    assert r["info"]["rows"] == total == rows.shape[0] and r["info"]["dropped"] == 0 and r["info"]["capacity_rows"] == 1 << 20
    assert r["info"]["rolls"] == int(np.count_nonzero(np.diff(np.concatenate([[[10, 10, 5]], ref["cen"]]), axis=0).any(axis=1)))
    # the key (sweep, kind, cube_k, cube_j, cube_i, tail, order) is unique and the rows come sorted by it
    kind, tail = (rows["flags"] & 1).astype(np.int64), ((rows["flags"] >> 1) & 1).astype(np.int64)
    assert not (rows["flags"] >> 2).any()
    key = np.stack([rows["sweep"], kind, rows["cube_k"], rows["cube_j"], rows["cube_i"], tail, rows["order"]], 1).astype(np.int64)
    order = np.lexsort(key.T[::-1])
    assert np.array_equal(order, np.arange(rows.shape[0])), "get order"
    assert (np.diff(key, axis=0) != 0).any(axis=1).all(), "duplicate key"
    # group by group against the oracle: count, sweep, kind and cube exact; order, intensities and coordinates by position
    at, want_pts = 0, []
    for sweep, k, cube, pts in ref["expected"]:
        m = pts.shape[0]
        g = rows[at:at + m]
        assert g.shape[0] == m and (g["sweep"] == sweep).all() and ((g["flags"] & 1) == k).all() and \
            (g["cube_i"] == cube[0]).all() and (g["cube_j"] == cube[1]).all() and (g["cube_k"] == cube[2]).all(), (sweep, k, cube, m, g[:3])
        want_pts.append(pts)
        at += m
    assert at == rows.shape[0]
    ulp = close_to_oracle(rows_xyzi(rows), np.concatenate(want_pts))
    assert float(np.mean(ulp == 0)) > 0.999
    # in the same run: the map poses and the final map meet test_gpu_window_rolls.py's bars
    for k, (qm, tm) in enumerate(r["poses"]):
        assert qdist(qm, ref["map_q"][k]) < POSE_TOL and np.linalg.norm(tm - ref["map_t"][k]) < POSE_TOL, "map pose, sweep %d" % k
    assert np.array_equal(r["h"].map_state()["cen"], ref["cen"][-1])
    assert r["map"].shape[0] > 1000
    ulp = close_to_oracle(r["map"], ref["final_map"])
    assert float(np.mean(ulp == 0)) > 0.999
    print("%s handle: %d rows (%d un-merged), %d rolls, health %s" % (kind_of_handle, rows.shape[0], int(tail.sum()), r["info"]["rolls"], r["health"]))


def test_archive_is_read_only(vl, ref):
    a, b = drive(vl, ref, "fixed", archive=1 << 20), drive(vl, ref, "plain")
    assert a["traj"].tobytes() == b["traj"].tobytes()
    assert a["map"].tobytes() == b["map"].tobytes() and a["map"].shape[0] > 1000
    assert a["log"].tobytes() == b["log"].tobytes() and (a["log"]["frame"] == np.arange(len(ref["walk"]))).all()


def test_overflow_counts_and_never_fails_the_sequence(vl, ref):
    total = sum(sum(v.values()) for v in EXPECTED.values())
    r = drive(vl, ref, "overflow", archive=64)   # every status on the way was VLOAM_OK, vloam_sync included, or drive() had raised
    assert r["info"]["rows"] == 64 and r["info"]["dropped"] == total - 64 and r["info"]["capacity_rows"] == 64
    rows = r["h"].map_archive()
    assert rows.shape[0] == 64 and (rows["sweep"] == ref["first_evicting"]).all()
    assert r["map"].tobytes() == drive(vl, ref, "plain")["map"].tobytes()
    assert r["traj"].tobytes() == drive(vl, ref, "plain")["traj"].tobytes()


def test_drain_in_two_parts(vl, ref):
    first = ref["first_evicting"]
    r = drive(vl, ref, "drain", archive=1 << 20, drain_after=first)
    assert r["info_after_drain"]["rows"] == 0 and r["info_after_drain"]["dropped"] == 0
    head = r["drained"][0]
    assert head.shape[0] == EXPECTED[0][first] + EXPECTED[1][first] and (head["sweep"] == first).all()
    tail = r["h"].map_archive(clear=True)
    info = r["h"].map_archive_info()
    assert info["rows"] == 0 and info["dropped"] == 0 and r["h"].map_archive().shape[0] == 0
    whole = drive(vl, ref, "fixed", archive=1 << 20)["h"].map_archive()
    assert np.concatenate([head, tail]).tobytes() == whole.tobytes()


def test_round_trip_through_map_import(vl, ref):
    """The clouds --save-map writes with --archive-rolled (the archive's rows of a kind, then the window's export) imported into a fresh handle
    that starts where the walk was on the sweep before the first eviction."""
    r = drive(vl, ref, "fixed", archive=1 << 20)
    rows = r["h"].map_archive()
    window = [r["h"].get_map_kind(k) for k in (0, 1)]
    arch = [rows_xyzi(rows[(rows["flags"] & 1) == k]) for k in (0, 1)]
    start = ref["first_evicting"] - 1
    cfg = dict(scan_line=cases.RINGS, with_mapping=1)
    with_rows, without = vl.Handle(0, **cfg), vl.Handle(0, **cfg)
    try:
        ra = with_rows.map_import(np.concatenate([arch[0], window[0]]), np.concatenate([arch[1], window[1]]), q_wmap_wodom=ref["map_q"][start], t_wmap_wodom=ref["map_t"][start])
        rb = without.map_import(window[0], window[1], q_wmap_wodom=ref["map_q"][start], t_wmap_wodom=ref["map_t"][start])
        assert np.array_equal(ra["center_cube"], rb["center_cube"])
        cen = ra["center_cube"].astype(np.int64)
        ijk = np.stack([rows["cube_i"], rows["cube_j"], rows["cube_k"]], 1).astype(np.int64) + cen
        inside = ((ijk >= 0) & (ijk < cases.SIZE)).all(axis=1)
        for k in (0, 1):
            assert ra["n_in"][k] == arch[k].shape[0] + window[k].shape[0]
            in_a, in_b = ra["n_in"][k] - ra["n_outside_window"][k], rb["n_in"][k] - rb["n_outside_window"][k]
            n_rows_inside = int(np.count_nonzero(inside & ((rows["flags"] & 1) == k)))
            assert in_a - in_b == n_rows_inside and n_rows_inside > 0, (k, in_a, in_b, n_rows_inside)
        # three archived merged-voxel points, by index, among those that share their voxel with no other point of the imported cloud (an import
        # folds the points of one voxel into their centroid; the voxel of a point: voxel_key_model, which test_gpu_voxel_faces.py holds the import to)
        alone = np.zeros(rows.shape[0], bool)
        for k, leaf in ((0, with_rows.cfg.mapping_line_resolution), (1, with_rows.cfg.mapping_plane_resolution)):
            cloud = np.ascontiguousarray(np.concatenate([arch[k], window[k]])[:, :3])
            vox = np.concatenate([voxel_key_model.cube_abs(cloud), voxel_key_model.voxel_index(cloud, leaf)], 1)
            _, inv, cnt = np.unique(vox, axis=0, return_inverse=True, return_counts=True)
            alone[np.nonzero((rows["flags"] & 1) == k)[0]] = (cnt[inv.ravel()] == 1)[:arch[k].shape[0]]
        cand = np.nonzero(inside & alone & ((rows["flags"] & 2) == 0) & (rows["sweep"] <= start + 2))[0]
        assert cand.shape[0] >= 3, cand.shape
        for i in (cand[0], cand[cand.shape[0] // 2], cand[-1]):
            k = int(rows["flags"][i] & 1)
            p = rows_xyzi(rows[i:i + 1])
            xyzi, d2, count = with_rows.map_query(p, k=1, max_radius=0.05, kind=k)
            assert count[0] == 1 and d2[0, 0] == 0.0 and np.array_equal(xyzi[0, 0].view(np.uint32), p[0].view(np.uint32)), (i, rows[i], xyzi, d2)
            _, _, none = without.map_query(p, k=1, max_radius=0.05, kind=k)
            assert none[0] == 0, (i, rows[i])
    finally:
        with_rows.close()
        without.close()


def test_refusals(vl, ref):
    L = vl.lib()

    def enable(h, size=16, cap=1 << 10):
        st = L.vloam_map_archive_enable(h.h, C.byref(vl.MapArchiveOptions(size, cap)))
        return st, L.vloam_last_error()

    msgs = []
    batched, no_map, plain = vl.Handle(0, n_sessions=2, with_mapping=1), vl.Handle(0, with_mapping=0), vl.Handle(0, with_mapping=1)
    try:
        v, n, rows = np.zeros(4, np.int64), C.c_longlong(-1), np.zeros(4, vl.MAP_ARCHIVE_ROW_DTYPE)
        p, c = C.c_void_p(), C.c_void_p()
        for name, args in (("vloam_map_archive_info", (v.ctypes.data_as(C.c_void_p),)), ("vloam_map_archive_get", (rows.ctypes.data_as(C.c_void_p), C.c_longlong(4), C.byref(n), 0)),
                           ("vloam_map_archive_device_ptr", (C.byref(p), C.byref(c)))):
            assert getattr(L, name)(plain.h, *args) == vl.ERR_INVALID and b"keeps no archive" in L.vloam_last_error(), name
        for h, kw, text in ((batched, {}, b"2 sessions"), (no_map, {}, b"with_mapping == 0"), (plain, dict(size=12), b"struct_size must be 16"),
                            (plain, dict(cap=0), b"not 0"), (plain, dict(cap=(1 << 26) + 1), b"not 67108865")):
            st, msg = enable(h, **kw)
            assert st == vl.ERR_INVALID and text in msg, (text, msg)
            msgs.append(msg)
        assert enable(plain)[0] == vl.VLOAM_OK
        st, msg = enable(plain)
        assert st == vl.ERR_INVALID and b"already keeps an archive of 1024 rows" in msg, msg
        msgs.append(msg)
        assert len(set(msgs)) == 6
        assert plain.map_archive_info() == dict(rows=0, dropped=0, capacity_rows=1024, rolls=0) and plain.map_archive().shape[0] == 0
        d_rows, d_cnt = plain.map_archive_device_ptr()
        assert d_rows and d_cnt and d_rows != d_cnt
    finally:
        for h in (batched, no_map, plain):
            h.close()
    # a buffer one row short: VLOAM_ERR_CAPACITY, n set, nothing cleared
    h = drive(vl, ref, "fixed", archive=1 << 20)["h"]
    held = h.map_archive_info()["rows"]
    buf = np.zeros(held, vl.MAP_ARCHIVE_ROW_DTYPE)
    n = C.c_longlong(-1)
    assert L.vloam_map_archive_get(h.h, buf.ctypes.data_as(C.c_void_p), C.c_longlong(held - 1), C.byref(n), 1) == vl.ERR_CAPACITY
    assert n.value == held > 0 and not buf.view(np.uint8).any() and h.map_archive_info()["rows"] == held
