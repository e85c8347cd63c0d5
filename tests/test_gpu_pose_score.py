"""-m gpu: pose scores (vloam_map_score_poses / vloam_map_score_poses_device) against the numpy model of tests/pose_score_model.py.

The model is the definition in c_api.h, nothing of the device's search: the searched set is get_map_kind(0) / get_map_kind(1) at that moment,
p = pointAssociateToMap in f64 rounded to f32, d2 in f32 with every product and sum rounded on its own, a hit when dmin <= r*r, the sum of
floor(dmin * 2^24) over the hits.  Every comparison is bit for bit on the whole record.  The feature clouds (features(2) / features(4) of a
handle without mapping) are thinned to a few hundred points before anything sees them, so that the brute force stays at a few seconds."""
import numpy as np
import pytest

import branch_cases
import pose_score_model as model
import test_gpu_voxel_faces as voxel_faces     # the window placements of test 6: ENDS
import test_gpu_window_rolls as window_rolls   # the drive of test 3: its walk and its sweep sizes
import voxel_key_model as V
from test_gpu_map_import import place_window

pytestmark = pytest.mark.gpu
F32 = np.float32
IDENT = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings a HIP runtime of its own: up before this module's first handle (tests/test_gpu_host_input.py); the device form takes tensors."""
    import torch
    torch.zeros(1).cuda()


def bits(v):
    return np.ascontiguousarray(v).tobytes()


def perturbed(rng, pose, n, dt, ddeg):
    out = []
    for _ in range(n):
        a = np.deg2rad(rng.uniform(-ddeg, ddeg))
        q = model.qmul(model.yaw_quat(a), pose[:4])
        out.append(np.concatenate([q / np.linalg.norm(q), pose[4:] + rng.uniform(-dt, dt, 3) * np.array([1.0, 1.0, 0.1])]))
    return out


def thin(cloud, n):
    return np.ascontiguousarray(cloud[::max(1, cloud.shape[0] // n)][:n], dtype=F32)


def leaf_bounds(h):
    return (float(F32(16) * F32(h.cfg.mapping_line_resolution)), float(F32(16) * F32(h.cfg.mapping_plane_resolution)))


def features_of(vl, cloud, rings=64):
    src = vl.Handle(0, scan_line=rings, with_mapping=0, max_points=cloud.shape[0], max_frames=4)
    src.scan_registration(cloud)
    corner, surf = src.features(2).copy(), src.features(4).copy()
    src.close()
    return corner, surf


@pytest.fixture(scope="module")
def scene(vl, synth):
    """Five 64 x 256 sweeps mapped, the fifth one's (thinned) feature clouds, 64 poses, the model's dmin tables — computed once, read-only."""
    rng = np.random.default_rng(21)
    seq = synth.SynthSequence(n_rings=64, n_azimuth=256, n_sweeps=6)
    clouds = [np.ascontiguousarray(seq.sweep(k), dtype=F32) for k in range(6)]
    h = vl.Handle(0, with_mapping=1, max_points=64 * 256, max_frames=16)
    for k in range(5):
        h.process_scan(clouds[k])
    h.sync()
    corner, surf = features_of(vl, clouds[4])
    corner, surf = thin(corner, 192), thin(surf, 768)
    true = h.trajectory()[4, 7:14].copy()
    true[:4] /= np.linalg.norm(true[:4])
    poses = [true] + perturbed(rng, true, 40, 2.0, 10.0) + perturbed(rng, true, 20, 0.2, 1.0)
    poses.append(poses[5].copy())                                   # 61: a duplicate
    poses.append(np.concatenate([true[:4], true[4:] + [500.0, 0.0, 0.0]]))   # 62: inside the window, nothing mapped there
    poses.append(np.concatenate([true[:4], true[4:] + [0.0, 2.0e7, 0.0]]))   # 63: beyond +-1e6
    poses = np.ascontiguousarray(poses)
    assert poses.shape == (64, 7)
    maps = (h.get_map_kind(0), h.get_map_kind(1))
    assert maps[0].shape[0] > 500 and maps[1].shape[0] > 500 and corner.shape[0] > 100 and surf.shape[0] > 400
    d = dict(h=h, clouds=clouds, corner=corner, surf=surf, poses=poses, maps=maps, tabs=model.dmin_tables(maps, corner, surf, poses), ckpt=h.checkpoint())
    yield d
    h.close()


def device_scores(vl, h, corner, surf, poses, **kw):
    import torch
    dc = None if corner is None else torch.from_numpy(corner).cuda()
    ds = None if surf is None else torch.from_numpy(surf).cuda()
    dp = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64)).cuda()
    out = torch.full((max(poses.shape[0], 1) * vl.POSE_SCORE_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h.map_score_poses_device(dc, ds, dp, out, **kw)   # no sync in between: the caller's buffers stay alive until sync()
    h.sync()
    return out.cpu().numpy().view(vl.POSE_SCORE_DTYPE)[:poses.shape[0]]


# ------------------------------------------------------------------------------------------------ 1. plain case
def test_plain_case_against_the_model(vl, scene):
    d, h = scene, scene["h"]
    cases = [(stride, radius) for stride in ((1, 1), (3, 7)) for radius in ((1.0, 1.0), (0.2, 0.4), leaf_bounds(h))]
    for stride, radius in cases:
        want = model.records(d["tabs"], stride, radius)
        got = h.map_score_poses(d["corner"], d["surf"], d["poses"], stride=stride, radius=radius)
        what = "stride %s radius %s" % (stride, radius)
        bad = [m for m in range(64) if bits(got[m]) != bits(want[m])]
        assert not bad, "%s: poses %s, e.g. device %s model %s" % (what, bad[:8], got[bad[0]], want[bad[0]])
        assert bits(got) == bits(want)
        dev = device_scores(vl, h, d["corner"], d["surf"], d["poses"], stride=stride, radius=radius)
        assert bits(dev) == bits(got), "%s: device form" % what
        assert bits(h.map_score_poses(d["corner"], d["surf"], d["poses"], stride=stride, radius=radius)) == bits(got), "%s: a second run" % what
        assert bits(got[61]) == bits(got[5]), "a duplicated pose"
        assert not got["n_hit"][62:].any() and not got["sum_d2_q24"][62:].any(), "500 m and 2e7 m away: no hits, no error"
        print("%s: hits at the true pose %s of %s, best of the ranking %d" % (what, got["n_hit"][0], got["n_used"][0], model.rank(got)[0]))
    got = h.map_score_poses(d["corner"], d["surf"], d["poses"])
    assert got["n_hit"][0].sum() > 0.8 * got["n_used"][0].sum(), "the sweep's own pose: most points within 1 m of the map"
    assert np.array_equal(vl.score_rank(got), model.rank(got))
    # M == 0 and empty clouds
    assert h.map_score_poses(d["corner"], d["surf"], np.zeros((0, 7))).shape == (0,)
    z = h.map_score_poses(None, None, d["poses"][:3])
    assert bits(z) == bits(np.zeros(3, vl.POSE_SCORE_DTYPE))
    h.sync()


# ------------------------------------------------------------------------------------------------ 2. edges
def hand_made_map():
    """A few dozen points: on and one ulp either side of the cube faces at +-25 m, on voxel faces of both leaves, isolated ones for the radius cases."""
    up, down = lambda v: np.nextafter(F32(v), F32(np.inf)), lambda v: np.nextafter(F32(v), F32(-np.inf))
    pts = [(3.0, 0.0, 0.0), (-7.0, 9.0, 1.0), (0.8, 0.8, 0.8), (1.6, -2.4, 0.4), (up(1.6), 4.0, 0.0), (down(2.4), -4.0, 0.0)]
    for axis in range(3):
        for face in (25.0, -25.0):
            for k, v in enumerate((F32(face), up(face), down(face))):
                p = [5.0 + 2.0 * k, -11.0 + 3.0 * k, 2.0 * k - 3.0]
                p[axis] = v
                pts.append(tuple(p))
    pts += [(25.0, 25.0, -25.0), (down(25.0), up(25.0), 25.0), (40.0, -40.0, 10.0), (-60.0, 3.0, -2.0)]
    return np.array([p + (float(i),) for i, p in enumerate(pts)], F32)


def exact_radius_points(centre, r):
    """Three points whose d2 to `centre` (its y is 0) is exactly r*r (f32), one ulp below and one ulp above it: dx an exact binary fraction, dy
    searched ulp by ulp around sqrt(r*r - dx*dx); consecutive dy move d2 by about one ulp, so one of a few dx reaches every target."""
    D = F32(r) * F32(r)
    targets = [D, np.nextafter(D, F32(0)), np.nextafter(D, F32(np.inf))]
    out = []
    for t in targets:
        for dx in (F32(0.5), F32(0.375), F32(0.25), F32(0.125), F32(0.3125), F32(0.4375)):
            dy0 = F32(np.sqrt(float(D) - float(dx) ** 2))
            dys = (dy0.view(np.uint32).astype(np.int64) + np.arange(-256, 257)).astype(np.uint32).view(F32)
            hit = np.nonzero(dx * dx + dys * dys == t)[0]
            if hit.size:
                out.append((centre[0] + dx, dys[hit[0]], centre[2]))
                break
        else:
            raise AssertionError("no (dx, dy) gives d2 = %r" % t)
    return np.array(out, F32), targets


def test_edges_on_a_hand_made_map(vl):
    rng = np.random.default_rng(22)
    pts = hand_made_map()
    ha = vl.Handle(0, with_mapping=1, max_frames=4)
    ha.map_import(pts, pts)
    hb = vl.Handle(0, with_mapping=1, max_frames=4)
    hb.map_import(pts, None)   # a kind with an empty map
    maps_a, maps_b = (ha.get_map_kind(0), ha.get_map_kind(1)), (hb.get_map_kind(0), hb.get_map_kind(1))
    assert maps_a[0].shape[0] >= 24 and maps_b[1].shape[0] == 0
    assert any(bits(row[:3]) == bits(pts[0, :3]) for row in maps_a[0]), "the isolated point at (3, 0, 0) is a map point of its own"

    def both(h, maps, corner, surf, poses, what, **kw):
        want = model.score_poses(maps, corner, surf, poses, **kw)
        got = h.map_score_poses(corner, surf, poses, **kw)
        assert bits(got) == bits(want), "%s: device %s model %s" % (what, got[:4], want[:4])
        assert bits(device_scores(vl, h, corner, surf, poses, **kw)) == bits(want), "%s: device form" % what
        return got

    # dmin exactly r*r, one ulp below, one ulp above — the point at y = 0, so centre + dy is dy itself
    r = 0.7
    cloud, targets = exact_radius_points(pts[0, :3], r)
    dm = model.point_dmin(maps_a[0], cloud)
    assert [bits(a) for a in dm] == [bits(t) for t in targets], (dm, targets)
    cloud4 = np.concatenate([cloud, np.zeros((3, 1), F32)], axis=1)
    got = both(ha, maps_a, cloud4, cloud4, IDENT[None], "dmin at r*r", radius=(r, r))
    assert got["n_hit"][0].tolist() == [2, 2] and got["n_used"][0].tolist() == [3, 3]
    for j, hit in enumerate((1, 1, 0)):
        assert both(ha, maps_a, cloud4[j:j + 1], None, IDENT[None], "dmin case %d" % j, radius=(r, r))["n_hit"][0, 0] == hit
    # points that land exactly on a cube face (and beside it), under the identity and under poses that move them onto it exactly
    face = []
    for axis in range(3):
        for f in (25.0, -25.0):
            near = pts[np.argsort(np.abs(pts[:, axis] - F32(f)))[:4]].copy()
            for v in (F32(f), np.nextafter(F32(f), F32(np.inf)), np.nextafter(F32(f), F32(-np.inf))):
                b = near.copy()
                b[:, axis] = v
                face.append(b)
    face = np.concatenate(face)
    shift = np.array([[0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 50.0, 0, 0], [0, 0, 0, 1, 0, -50.0, 0], [0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0.4, 0.8, -0.4]], np.float64)
    got = both(ha, maps_a, face, face, shift, "cube faces", radius=(1.0, 2.0))
    assert got["n_hit"][0].min() > 20
    both(ha, maps_a, face[:61], face[::5], shift, "cube faces, 16-leaf radius", radius=leaf_bounds(ha), stride=(2, 3))
    both(hb, maps_b, face, face, shift, "empty surf map")
    # one kind without points
    g = both(ha, maps_a, None, face, shift, "n_corner == 0")
    assert not g["n_used"][:, 0].any() and g["n_hit"][:, 1].any()
    g = both(ha, maps_a, face, None, shift, "n_surf == 0")
    assert not g["n_used"][:, 1].any() and g["n_hit"][:, 0].any()
    # tile remainders in both directions: M == 1, M == 257 with N = 65 and N = 1
    many = np.ascontiguousarray(perturbed(rng, IDENT, 257, 0.5, 5.0))
    jit = (pts[rng.integers(0, pts.shape[0], 65)] + np.concatenate([rng.uniform(-0.4, 0.4, (65, 3)), np.zeros((65, 1))], axis=1)).astype(F32)
    both(ha, maps_a, jit, jit[:1], many[:1], "M == 1")
    g = both(ha, maps_a, jit, jit[:1], many, "M == 257, N = 65 and 1")
    assert g["n_used"][0].tolist() == [65, 1] and g["n_hit"][:, 0].min() < g["n_hit"][:, 0].max()
    both(ha, maps_a, jit[:1], jit, many, "M == 257, N = 1 and 65")
    # every point outside the 21 x 21 x 11 window
    out = np.array([[0, 0, 0, 1, 2000.0, 0, 0], [0, 0, 0, 1, 0, -2000.0, 0], [0, 0, 0, 1, 0, 0, 900.0]], np.float64)
    g = both(ha, maps_a, jit, jit, out, "outside the window", radius=leaf_bounds(ha))
    assert not g["n_hit"].any()
    ha.sync()
    hb.sync()
    ha.close()
    hb.close()


# ------------------------------------------------------------------------------------------------ 3. a rolled window
def test_after_the_window_rolled(vl, synth):
    """The six-way walk of tests/test_gpu_window_rolls.py (64 x 256): the window ends 440 m from where it started, and the cubes mapped at
    y = -440 m have left it (the device purged their voxels; their occupancy bits stay)."""
    walk = branch_cases.six_way_walk()
    mark = window_rolls.test_window_rolls_in_all_six_directions.pytestmark[0]
    assert mark.name == "parametrize" and mark.args[0] == "rings,n_az" and len(mark.args[1][0]) == 2, "the drive's settings moved: %r" % (mark,)
    rings, n_az = mark.args[1][0]
    seq = synth.SynthSequence(n_rings=rings, n_azimuth=n_az, n_sweeps=len(walk))
    h = vl.Handle(0, scan_line=rings, with_mapping=1, max_frames=len(walk) + 8)
    at, seen_south = [], 0
    for k in range(len(walk)):
        h.reset_frame()
        h.scan_registration(seq.sweep(k))
        qw, tw, _, _ = h.laser_odometry()
        h.set_mapping_input(q_wodom_curr=qw, t_wodom_curr=tw + walk[k])
        qm, tm = h.laser_mapping()
        at.append(np.concatenate([qm / np.linalg.norm(qm), tm]))
        if walk[k][1] == -440.0 and not seen_south:
            seen_south = int((h.get_map()[:, 1] < -425.0).sum())
    assert seen_south > 100, "points mapped in the cubes around y = -440 m: %d" % seen_south
    st = h.map_state()
    assert st["cen"][0] != 10 and st["cen"][1] != 10, "the window rolled: %s" % st["cen"]
    maps = (h.get_map_kind(0), h.get_map_kind(1))
    assert not (maps[0][:, 1] < -425.0).any() and not (maps[1][:, 1] < -425.0).any(), "those cubes left the window"
    corner, surf = features_of(vl, np.ascontiguousarray(seq.sweep(len(walk) - 1), dtype=F32), rings)
    corner, surf = thin(corner, 96), thin(surf, 384)
    south = [k for k in range(len(walk)) if walk[k][1] == -440.0]
    poses = [at[-1], at[-2], at[len(walk) // 2]] + [at[k] for k in south[:3]]
    gone = at[south[0]].copy()
    gone[5] -= 150.0            # every point at y < -475 m: cubes that left the window
    poses = np.ascontiguousarray(poses + [gone])
    want = model.score_poses(maps, corner, surf, poses)
    got = h.map_score_poses(corner, surf, poses)
    assert bits(got) == bits(want), (got, want)
    assert got["n_hit"][0].sum() > 0.5 * got["n_used"][0].sum() and not got["n_hit"][-1].any()
    want = model.score_poses(maps, corner, surf, poses, radius=leaf_bounds(h), stride=(2, 5))
    assert bits(h.map_score_poses(corner, surf, poses, radius=leaf_bounds(h), stride=(2, 5))) == bits(want)
    h.sync()
    h.close()


# ------------------------------------------------------------------------------------------------ 4. handles
def test_growable_and_restored_handles(vl, scene):
    d = scene
    want = d["h"].map_score_poses(d["corner"], d["surf"], d["poses"], stride=(1, 2), radius=(0.6, 1.0))
    hg = vl.Handle(0, with_mapping=1, max_points=64 * 256, max_frames=16, map_capacity_log2=10, map_grow=1)
    for k in range(5):
        hg.process_scan(d["clouds"][k])
    got = hg.map_score_poses(d["corner"], d["surf"], d["poses"], stride=(1, 2), radius=(0.6, 1.0))   # right behind the last sweep and its growth steps
    hg.sync()
    assert hg.health()["map_growth_steps"] > 0
    assert bits(got) == bits(want), "growable handle after %d growth steps" % hg.health()["map_growth_steps"]
    hg.close()
    hr = vl.Handle(0, with_mapping=1, max_points=64 * 256, max_frames=16)
    hr.restore(d["ckpt"])
    assert bits(hr.map_score_poses(d["corner"], d["surf"], d["poses"], stride=(1, 2), radius=(0.6, 1.0))) == bits(want), "handle restored from a checkpoint"
    hr.close()


# ------------------------------------------------------------------------------------------------ 5. nothing visible changes
def test_scores_and_relocalisations_leave_the_sequence_alone(vl, scene):
    d = scene

    def drive(score):
        h = vl.Handle(0, with_mapping=1, max_points=64 * 256, max_frames=16)
        for k in range(5):
            h.process_scan(d["clouds"][k])
        sticky = h.L.vloam_sync(h.h)   # the status itself: what a sticky error word would turn it into
        before = dict(map=h.get_map(), traj=h.trajectory(), frames=h.frame_count(), state=h.map_state(), health=h.health(), map_health=h.map_health())
        if score:
            h.map_score_poses(d["corner"], d["surf"], d["poses"])
            r = h.map_relocalize(d["corner"], d["surf"], d["poses"][3, :4], d["poses"][3, 4:], n_xy=(3, 3), n_yaw=3, top_k=2)
            assert r["n_refined"] == 2 and r["n_candidates"] == 27
        assert h.L.vloam_sync(h.h) == sticky == vl.VLOAM_OK, "the sticky error of vloam_sync before and after"
        after = dict(map=h.get_map(), traj=h.trajectory(), frames=h.frame_count(), state=h.map_state(), health=h.health(), map_health=h.map_health())
        assert bits(before["map"]) == bits(after["map"]) and bits(before["traj"]) == bits(after["traj"]) and before["frames"] == after["frames"] == 5
        assert all(bits(before["state"][k]) == bits(after["state"][k]) for k in before["state"])
        assert before["health"] == after["health"] and before["map_health"] == after["map_health"]
        h.process_scan(d["clouds"][5])
        h.sync()
        out = (h.trajectory(), h.get_map())
        h.close()
        return out
    a, b = drive(True), drive(False)
    assert a[0].shape == (6, 14) and bits(a[0]) == bits(b[0]), "the sweep behind a score and a relocalisation: its pose"
    assert bits(a[1]) == bits(b[1]), "... and the map"


# ------------------------------------------------------------------------------------------------ 6. the ends of the key range
END_CUBES = {"x+511": (511, 0, 0), "y-512,z-128": (0, -512, -128)}   # the last cubes the voxel key holds, where voxel_faces.ENDS put the window's edge


def end_cube_case(end):
    """Pure numpy: per kind ten points to import — eight in the end cube, of which three lie 0.3, 0.6 and 2 m inside its outer faces and one
    0.3 m inside the opposite ones, and one 0.4 m beyond those, in the neighbouring cube —, per kind a cloud of 16 (those points seen from the
    cube's centre and six strays) and 13 poses that put the cloud on the points, 0.3 to 1.1 m off them (towards and across the outer faces
    too), turn it about the centre, and move it past the end of the range and into the neighbouring cube."""
    rng = np.random.default_rng(24)
    A = np.array(END_CUBES[end], np.float64)
    centre, out = 50.0 * A, np.sign(A)   # out: towards the end of the range on the axes that have one here, 0 on the others
    local, cloud = [], []
    for kind in (0, 1):
        s = rng.uniform(-20.0, 20.0, (10, 3))
        for j, d in enumerate((0.3, 0.6, 2.0)):
            s[j] = np.where(out != 0, out * (25.0 - d), s[j])
        s[3] = np.where(out != 0, -out * (25.0 - 0.3), s[3])
        s[4] = np.where(out != 0, -out * (25.0 + 0.4), s[3])
        s = s.astype(F32).astype(np.float64)
        local.append(s)
        c = np.concatenate([s, rng.uniform(-20.0, 20.0, (6, 3))])
        cloud.append(np.concatenate([c, np.arange(16.0)[:, None]], axis=1).astype(F32))
    pts = [np.concatenate([(centre + s).astype(F32), np.arange(10, dtype=F32)[:, None]], axis=1) for s in local]
    offs = [(0, 0, 0), (0.3, 0, 0), (0, -0.6, 0), (0, 0, 0.9), (0.6, 0.6, 0.4), (0.6, 0.6, 0.6), (1.1, 0, 0), 0.5 * out, -0.5 * out]
    poses = [np.concatenate([IDENT[:4], centre + np.asarray(o, np.float64)]) for o in offs]
    poses += [np.concatenate([model.yaw_quat(np.deg2rad(a)), centre]) for a in (2.0, 3.5)]
    poses += [np.concatenate([IDENT[:4], centre + 60.0 * out]), np.concatenate([IDENT[:4], centre - 50.0 * out])]
    return pts, cloud, np.ascontiguousarray(poses)


@pytest.mark.parametrize("end", sorted(voxel_faces.ENDS))
def test_scores_at_the_ends_of_the_key_range(vl, end):
    """Scores in the last cubes the voxel key holds (absolute cube +511 on x; -512 on y and -128 on z), which are the window's last here, so
    every cube beyond the key's range is outside the window too: this checks the keys, boxes and cube ranges at the extreme cube numbers, not
    the walk's key-range bound by itself (that takes a window that reaches past the range, as in
    tests/test_gpu_voxel_faces.py::test_points_beyond_the_key_range).  Built with map_import, as there."""
    t = voxel_faces.ENDS[end]
    pts, cloud, poses = end_cube_case(end)
    assert poses.shape[0] < 16
    h = vl.Handle(0, with_mapping=1, max_frames=4)
    h.map_import(pts[0], pts[1], t_wmap_wodom=t)
    assert list(h.map_state()["cen"]) == list(place_window(t))
    maps = (h.get_map_kind(0), h.get_map_kind(1))
    for k in (0, 1):
        assert maps[k].shape[0] == 10, "every imported point is inside the window and a map point of its own"
        assert (V.cube_abs(maps[k][:, :3]) == END_CUBES[end]).all(axis=1).sum() >= 8, "the last cube holds map points"
    want = model.score_poses(maps, cloud[0], cloud[1], poses)
    print("%s: model hits per pose %s of %s" % (end, want["n_hit"].tolist(), want["n_used"][0].tolist()))
    # the model itself tells the poses apart: everything on the points, partial hits off them, nothing beyond the end of the range
    assert (want["n_hit"][0] >= 10).all() and not want["n_hit"][11].any() and want["n_hit"][7].sum() >= 16
    assert (want["n_hit"] < want["n_used"]).all() and len(set(want["n_hit"].sum(axis=1).tolist())) >= 4
    got = h.map_score_poses(cloud[0], cloud[1], poses)
    assert bits(got) == bits(want), "device %s model %s" % (got, want)
    assert bits(device_scores(vl, h, cloud[0], cloud[1], poses)) == bits(want), "device form"
    h.sync()
    h.close()
