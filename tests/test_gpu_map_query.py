"""-m gpu: map queries (vloam_map_query / vloam_map_query_device / vloam_get_map_kind) against a numpy brute force.

The reference model is the definition in c_api.h, nothing of the device's search: the searched set is get_map_kind(0) / get_map_kind(1) (the
two halves of vloam_get_map) at that moment, d2 = (dx*dx + dy*dy) + dz*dz in np.float32 with every product and sum rounded on its own, a
neighbour qualifies when d2 <= r*r (f32 product), the best k ascending.  `count` and the d2 lists must be equal bit for bit; every returned
point must be a row of the set at the reported d2 (two candidates at one d2: either row).  The brute force keeps the eight smallest d2 per
query once per point set; every (k, radius) case is read off those.
"""
import numpy as np
import pytest

import branch_cases

pytestmark = pytest.mark.gpu

KINDS, KS = (0, 1, 2), (1, 5, 8)
F32 = np.float32
VLP16 = dict(minimum_range=0.3, mapping_line_resolution=0.2, mapping_plane_resolution=0.4, mapping_skip_frame=1)   # loam_velodyne_VLP_16.launch:3-13


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings a HIP runtime of its own: up before this module's first handle (tests/test_gpu_host_input.py); tests 3 - 5 keep sweeps in torch tensors."""
    import torch
    torch.zeros(1).cuda()


def leaf_bound(h, kind):
    """16 leaves of the finest kind queried, as the library computes it (f32)."""
    line, plane = F32(h.cfg.mapping_line_resolution), F32(h.cfg.mapping_plane_resolution)
    return float(F32(16) * (plane if kind == 1 else (line if kind == 0 else min(line, plane))))


def point_sets(h):
    """{kind: float32 [m, 4]} for kind 0, 1 and 2 (the union), and the check that the halves make up get_map()."""
    c, s, both = h.get_map_kind(0), h.get_map_kind(1), h.get_map()
    assert c.shape[0] + s.shape[0] == both.shape[0]
    assert sorted(rows16(np.concatenate([c, s]))) == sorted(rows16(both)), "get_map_kind(0) + get_map_kind(1) is not a permutation of get_map()"
    return {0: c, 1: s, 2: np.concatenate([c, s])}


def rows16(a):
    """The 16-byte rows of a float32 [m, 4] array as bytes objects."""
    b = np.ascontiguousarray(a, dtype=F32).tobytes()
    return [b[i:i + 16] for i in range(0, len(b), 16)]


def top8(P, Q):
    """The eight smallest d2 of every query over the point set, ascending, inf where there are fewer (or the query is not finite): f32 [n, 8]."""
    out = np.full((Q.shape[0], 8), np.inf, F32)
    if P.shape[0] == 0:
        return out
    px, py, pz = (np.ascontiguousarray(P[:, a]) for a in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, Q.shape[0], 128):
            q = Q[a:a + 128]
            dx, dy, dz = q[:, None, 0] - px[None, :], q[:, None, 1] - py[None, :], q[:, None, 2] - pz[None, :]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F32
            d2[np.isnan(d2)] = np.inf
            m = min(8, d2.shape[1])
            out[a:a + 128, :m] = np.sort(np.partition(d2, m - 1, axis=1)[:, :m], axis=1)
    return out


def check(res, Q, P, best, k, r, what):
    """One map_query result against the brute force (`best` = top8(P, Q))."""
    xyzi, d2, cnt = res
    n = Q.shape[0]
    assert xyzi.shape == (n, k, 4) and d2.shape == (n, k) and cnt.shape == (n,)
    r2 = F32(r) * F32(r)
    want = best[:, :k].copy()
    ok = want <= r2
    want[~ok] = 0
    assert np.array_equal(cnt, ok.sum(axis=1).astype(np.int32)), "%s: count, first rows %s" % (what, np.nonzero(cnt != ok.sum(axis=1))[0][:8])
    assert np.array_equal(d2.view(np.uint32), want.view(np.uint32)), "%s: d2, first rows %s" % (what, np.nonzero((d2.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0][:8])
    assert not xyzi[~ok].any(), "%s: entries beyond count are zero" % what
    got = xyzi[ok]                                      # [m, 4]
    qq = np.repeat(Q[:, None, :3], k, axis=1)[ok]
    dx, dy, dz = qq[:, 0] - got[:, 0], qq[:, 1] - got[:, 1], qq[:, 2] - got[:, 2]
    assert np.array_equal(((dx * dx + dy * dy) + dz * dz).view(np.uint32), d2[ok].view(np.uint32)), "%s: a returned point is not at its reported d2" % what
    assert set(rows16(got)) <= set(rows16(P)), "%s: a returned point is no row of the map" % what
    return int(ok.sum())


def ulp_step(x, up):
    return np.nextafter(F32(x), F32(np.inf if up else -np.inf))


# ------------------------------------------------------------------------------------------------ 1. plain drive
def test_plain_drive_against_brute_force(vl, synth):
    rng = np.random.default_rng(11)
    seq = synth.SynthSequence(n_rings=64, n_azimuth=256, n_sweeps=6)
    h = vl.Handle(0, with_mapping=1, max_points=64 * 256, max_frames=16)
    for k in range(5):
        h.process_scan(seq.sweep(k))
    sets = point_sets(h)
    M = sets[2]
    assert M.shape[0] > 2000
    own = M[rng.choice(M.shape[0], 500, replace=False), :3]
    jit = (M[rng.choice(M.shape[0], 600, replace=False), :3] + rng.uniform(-0.3, 0.3, (600, 3))).astype(F32)
    reg = h.features(11)
    reg = reg[rng.choice(reg.shape[0], 500, replace=False), :3]
    # exactly on the cube borders 25 + 50 i and one ulp to either side of them, at the y / z (x / z) of map points near those planes
    border = []
    for axis in (0, 1):
        for face in (-25.0, 25.0):
            near = M[np.argsort(np.abs(M[:, axis] - face))[:24], :3]
            for v in (F32(face), ulp_step(face, True), ulp_step(face, False)):
                b = near.copy()
                b[:, axis] = v
                border.append(b)
    border = np.concatenate(border)
    far = (own[:40] + np.array([500.0, 0.0, 0.0])).astype(F32)
    outside = np.array([[600, 0, 0], [0, -700, 0], [0, 0, 400], [-1e5, 0, 0], [0, 2e7, 0], [3e38, -3e38, 3e38]], F32)
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [1, 2, -np.inf], [np.nan, np.nan, np.nan]], F32)
    Q = np.ascontiguousarray(np.concatenate([own, jit, reg, border, far, outside, odd]).astype(F32))
    n_far = slice(own.shape[0] + jit.shape[0] + reg.shape[0] + border.shape[0], Q.shape[0])
    assert 1900 <= Q.shape[0] <= 2200
    best = {kind: top8(sets[kind], Q) for kind in KINDS}
    assert (best[2][:own.shape[0], 0] == 0).all(), "the map's own points: d2 = 0 first"
    total = 0
    for kind in KINDS:
        for k in KS:
            for r in (1.0, leaf_bound(h, kind)):
                res = h.map_query(Q, k=k, max_radius=r, kind=kind)
                total += check(res, Q, sets[kind], best[kind], k, r, "kind %d, k %d, r %g" % (kind, k, r))
                assert not res[2][n_far].any(), "queries 500 m away, outside the window or not finite have no neighbours"
    print("plain drive: %d map points (%d corner), %d queries, 18 cases, %d neighbours compared" % (M.shape[0], sets[0].shape[0], Q.shape[0], total))
    # the bound itself: one ulp above it is refused with the bound in metres, a handle without mapping with VLOAM_ERR_ORDER
    with pytest.raises(vl.VloamError) as e:
        h.map_query(Q[:4], k=5, max_radius=float(ulp_step(leaf_bound(h, 2), True)), kind=2)
    assert e.value.status == vl.ERR_INVALID and "at most 6.4" in str(e.value), str(e.value)
    xyzi, d2, cnt = h.map_query(np.zeros((0, 3), F32))
    assert xyzi.shape == (0, 5, 4) and cnt.shape == (0,)
    h.close()
    h0 = vl.Handle(0, with_mapping=0, max_points=64 * 256, max_frames=16)
    with pytest.raises(vl.VloamError) as e:
        h0.map_query(Q[:4])
    assert e.value.status == vl.ERR_ORDER and "with_mapping" in str(e.value)
    h0.close()


# ------------------------------------------------------------------------------------------------ 2. raw points, points beyond the valid block
def test_raw_points_and_cubes_beyond_the_valid_block(vl, synth, monkeypatch):
    """The first leg of branch_cases.six_way_walk (55 m per sweep along -x), with the sensor model's range raised to 140 m as in the raw-voxel drives
    of test_gpu_map_growth.py: returns beyond the valid 5 x 5 x 3 block stay un-merged behind the sensor, and the places it left are cubes the
    scan-to-map search no longer reads but vloam_get_map — and so a query — still holds."""
    monkeypatch.setattr(synth, "MAX_RANGE", 140.0)
    rng = np.random.default_rng(12)
    walk = branch_cases.six_way_walk()[:7]
    seq = synth.SynthSequence(n_rings=64, n_azimuth=256, n_sweeps=len(walk) + 1)
    h = vl.Handle(0, with_mapping=1, max_points=64 * 256, max_frames=16)
    for k, off in enumerate(walk):
        h.reset_frame()
        h.scan_registration(seq.sweep(k))
        qw, tw, _, _ = h.laser_odometry()
        h.set_mapping_input(q_wodom_curr=qw, t_wodom_curr=tw + off)
        h.laser_mapping()
    assert sum(h.map_health()["deferred"]) > 0, "the drive must leave un-merged arrivals in the map"
    st = h.map_state()
    sensor_cube = st["centerCube"] - st["cen"]   # absolute cube of the sensor (laser_mapping.cpp:207-216)
    sets = point_sets(h)
    M = sets[2]
    cube = np.floor((M[:, :3].astype(np.float64) + 25.0) / 50.0).astype(np.int64)
    beyond = (np.abs(cube[:, 0] - sensor_cube[0]) > 2) | (np.abs(cube[:, 1] - sensor_cube[1]) > 2) | (np.abs(cube[:, 2] - sensor_cube[2]) > 1)
    assert beyond.sum() >= 100, "map points in cubes outside the valid block: %d" % beyond.sum()
    pick = np.concatenate([rng.choice(np.nonzero(beyond)[0], 240, replace=False), rng.choice(M.shape[0], 360, replace=False)])
    Q = np.ascontiguousarray((M[pick, :3] + rng.uniform(-0.3, 0.3, (pick.size, 3))).astype(F32))
    # brute force alone: how many queries have a point beyond the valid block as their true nearest neighbour
    nn_beyond = np.zeros(Q.shape[0], bool)
    for a in range(0, Q.shape[0], 64):
        d = ((Q[a:a + 64, None, :].astype(np.float64) - M[None, :, :3].astype(np.float64)) ** 2).sum(axis=2)
        nn_beyond[a:a + 64] = beyond[np.argmin(d, axis=1)] & (d.min(axis=1) <= 1.0)
    assert nn_beyond.sum() >= 20, "queries whose nearest neighbour lies beyond the valid block: %d" % nn_beyond.sum()
    best = {kind: top8(sets[kind], Q) for kind in KINDS}
    total = 0
    for kind, k, r in [(2, 5, 1.0), (0, 8, leaf_bound(h, 0)), (1, 1, 1.0), (2, 8, leaf_bound(h, 2))]:
        res = h.map_query(Q, k=k, max_radius=r, kind=kind)
        total += check(res, Q, sets[kind], best[kind], k, r, "kind %d, k %d, r %g" % (kind, k, r))
        if kind == 2:
            assert (res[2][nn_beyond] >= 1).all()
    print("walk: %d map points, %d beyond the valid block, raw voxels %s, %d of %d queries with their nearest neighbour beyond it, %d neighbours compared"
          % (M.shape[0], beyond.sum(), h.map_health()["deferred"], nn_beyond.sum(), Q.shape[0], total))
    h.close()


# ------------------------------------------------------------------------------------------------ shared 16-line drive of tests 3 - 5
N16, COLS16 = 6, 256


def handle16(vl, **kw):
    return vl.Handle(0, scan_line=16, with_mapping=1, max_points=16 * COLS16, max_frames=32, **dict(VLP16, **kw))


@pytest.fixture(scope="module")
def drive16(vl, synth):
    """Three 16 x 256 sequences (host and device copies); sequence 2 run alone for N16 sweeps: its point sets, a query set, the brute force's
    answers, the host form's results, a checkpoint, trajectory / map / sweep log.  Computed once, read-only."""
    import torch
    rng = np.random.default_rng(13)
    seqs = [synth.SynthSequence(n_rings=16, n_azimuth=COLS16, n_sweeps=N16 + 3, speed=1.5 + 0.5 * b, seed_traj=42 + b) for b in range(3)]
    clouds = [[np.ascontiguousarray(s.sweep(k), dtype=F32) for k in range(N16 + 2)] for s in seqs]
    h = handle16(vl, sweep_log=1)
    for k in range(N16):
        h.process_scan(clouds[2][k])
    sets = point_sets(h)
    M = sets[2]
    Q = np.ascontiguousarray((M[rng.choice(M.shape[0], 400, replace=False), :3] + rng.uniform(-0.2, 0.2, (400, 3))).astype(F32))
    cases = [(2, 5, 1.0), (0, 8, leaf_bound(h, 0)), (1, 1, 0.5)]
    best = {kind: top8(sets[kind], Q) for kind in KINDS}
    results = []
    for kind, k, r in cases:
        res = h.map_query(Q, k=k, max_radius=r, kind=kind)
        assert check(res, Q, sets[kind], best[kind], k, r, "alone: kind %d, k %d, r %g" % (kind, k, r)) > 100
        results.append(res)
    out = dict(clouds=clouds, dev=[torch.from_numpy(np.stack(c)).cuda() for c in clouds], Q=Q, cases=cases, results=results, ckpt=h.checkpoint(),
               tj=h.trajectory(), map=h.get_map(), log=h.sweep_log())
    h.close()
    return out


def assert_same_results(h, d, what):
    for (kind, k, r), want in zip(d["cases"], d["results"]):
        got = h.map_query(d["Q"], k=k, max_radius=r, kind=kind)
        for a, b, name in zip(got, want, ("points", "d2", "count")):
            assert a.tobytes() == b.tobytes(), "%s: %s of kind %d, k %d, r %g" % (what, name, kind, k, r)


# ------------------------------------------------------------------------------------------------ 3. ordering
def test_device_form_right_behind_a_sweep(vl, drive16):
    import torch
    d = drive16
    kind, k, r = d["cases"][0]
    n = d["Q"].shape[0]
    q = torch.zeros((n, 4), dtype=torch.float32)
    q[:, :3] = torch.from_numpy(d["Q"])
    q = q.cuda()
    xyzi = torch.full((n, k, 4), -1.0, dtype=torch.float32, device="cuda")
    d2 = torch.full((n, k), -1.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    h = handle16(vl)
    stride = 16 * COLS16 * 16
    for s in range(N16):
        h.process_scan_device(d["dev"][2].data_ptr() + s * stride, 16 * COLS16)
    h.map_query_device(q.data_ptr(), n, xyzi.data_ptr(), d2.data_ptr(), cnt.data_ptr(), k=k, max_radius=r, kind=kind)   # no sync in between
    h.sync()
    got = (xyzi.cpu().numpy(), d2.cpu().numpy(), cnt.cpu().numpy())
    for a, b, name in zip(got, d["results"][0], ("points", "d2", "count")):
        assert a.tobytes() == b.tobytes(), "device form behind the last sweep: %s" % name
    assert_same_results(h, d, "host form of the same handle")
    # later sweeps leave what was fetched — and the caller's buffers — alone; the map itself moves on
    for s in range(N16, N16 + 2):
        h.process_scan_device(d["dev"][2].data_ptr() + s * stride, 16 * COLS16)
    h.sync()
    for t, b, name in zip((xyzi, d2, cnt), got, ("points", "d2", "count")):
        assert t.cpu().numpy().tobytes() == b.tobytes(), "a later sweep changed the fetched %s" % name
    later = h.map_query(d["Q"], k=k, max_radius=r, kind=kind)
    assert later[1].tobytes() != got[1].tobytes(), "two more sweeps must show up in a new query"
    h.close()


# ------------------------------------------------------------------------------------------------ 4. handles
def test_session_of_a_batch(vl, drive16):
    d = drive16
    hb = vl.Handle(0, n_sessions=3, scan_line=16, with_mapping=1, max_points=16 * COLS16, max_frames=32, **VLP16)
    for s in range(N16):
        hb.batch_process_scan([d["clouds"][b][s] for b in range(3)])
    hb.select(2)
    assert hb.get_map().tobytes() == d["map"].tobytes()
    assert_same_results(hb, d, "session 2 of a 3-session batch")
    hb.select(0)
    other = hb.map_query(d["Q"], k=5, max_radius=1.0, kind=2)
    assert other[1].tobytes() != d["results"][0][1].tobytes(), "session 0 holds another sequence"
    hb.close()


def test_growable_and_restored_handles(vl, drive16):
    d = drive16
    hg = handle16(vl, map_capacity_log2=10, map_grow=1)
    for s in range(N16):
        hg.process_scan(d["clouds"][2][s])
    hg.sync()
    assert hg.health()["map_growth_steps"] > 0
    assert_same_results(hg, d, "growable handle after %d growth steps" % hg.health()["map_growth_steps"])
    hg.close()
    hr = handle16(vl)
    hr.restore(d["ckpt"])
    assert_same_results(hr, d, "handle restored from a checkpoint")
    hr.close()


# ------------------------------------------------------------------------------------------------ 5. unchanged pipeline
def test_queries_leave_the_pipeline_alone(vl, drive16):
    d = drive16
    h = handle16(vl, sweep_log=1)
    for s in range(N16):
        h.process_scan(d["clouds"][2][s])
        kind, k, r = d["cases"][s % len(d["cases"])]
        h.map_query(d["Q"], k=k, max_radius=r, kind=kind)
    h.sync()
    assert h.trajectory().tobytes() == d["tj"].tobytes(), "poses"
    assert h.get_map().tobytes() == d["map"].tobytes(), "map"
    assert h.sweep_log().tobytes() == d["log"].tobytes(), "sweep-log rows"
    assert_same_results(h, d, "after a query behind every sweep")
    h.close()
