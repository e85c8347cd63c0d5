"""-m gpu: map import (vloam_map_import / vloam_map_import_device) — two map-frame clouds and a start transform into a fresh handle.

This file is about the MERGE paths, not the keys: its clouds keep away from every voxel and cube face (points on faces, where the f32 voxel
key differs from the f64 floor used here, are tests/test_gpu_voxel_faces.py's).

What is checked: the per-voxel merge against a numpy model (f32 sums in input order, divided by f32(n)) and the CPU oracle's per-cube VoxelGrid,
bit for bit, on a cloud that takes all three ordering paths; an exported map comes back bit for bit in a handle of another capacity and a growable
one, and answers localisations and queries like the handle that built it; the first real mapping in an imported map is the builder's dry run;
a start away from the origin places the window as the reference's shift loops do; a sequence that began with an import checkpoints and
resumes byte for byte; the refusals leave the handle usable."""
import numpy as np
import pytest

from test_gpu_localize import bits, qmul, qrot, rot_z, same_record, staged_sweep
from voxel_key_model import cube_abs

pytestmark = pytest.mark.gpu

RINGS, AZ = 16, 256          # the smallest synthetic sweeps that give the mapping stage a solvable problem
LEAF = (0.4, 0.8)            # mapping_line_resolution / mapping_plane_resolution of a default handle
DIMS = np.array([21, 21, 11])
CEN0 = np.array([10, 10, 5])


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings a HIP runtime of its own: up before this module's first handle (tests/test_gpu_host_input.py); the device form takes tensors."""
    import torch
    torch.zeros(1).cuda()


# ---------------------------------------------------------------------------------------------- the independent model
def place_window(t):
    """laser_mapping.cpp:207-402 on an empty grid: the centre offsets laserCloudCen{Width,Height,Depth} for a sensor at t"""
    cen = CEN0.copy()
    for a in range(3):
        c = int(cube_abs(t[a])) + cen[a]
        while c < 3:
            c += 1
            cen[a] += 1
        while c >= DIMS[a] - 3:
            c -= 1
            cen[a] -= 1
    return cen


def model(pts, leaf, cen):
    """What get_map_kind must return for cloud pts (float32 [n, 4]) imported at leaf with window offsets cen, and the result's figures.
    Plain f64 floor keying: the test clouds keep 1e-3 leaf from every voxel face and 1e-3 m from every cube face."""
    pts = np.asarray(pts, dtype=np.float32)
    finite = np.isfinite(pts).all(axis=1)
    xyz = np.where(finite[:, None], pts[:, :3], 0).astype(np.float64)
    A = cube_abs(xyz)
    w = A + cen
    inside = finite & ((w >= 0) & (w < DIMS)).all(axis=1)
    g = np.floor(xyz / leaf).astype(np.int64)
    idx = np.flatnonzero(inside)
    cube = w[idx, 0] + 21 * w[idx, 1] + 441 * w[idx, 2]
    # export order: cube, then voxel (z, y, x); ties (the points of one voxel) in input order
    order = np.lexsort((idx, g[idx, 0], g[idx, 1], g[idx, 2], cube))
    rows = idx[order]
    key = np.stack([cube[order], g[rows, 2], g[rows, 1], g[rows, 0]], axis=1)
    first = np.ones(rows.size, bool)
    first[1:] = (key[1:] != key[:-1]).any(axis=1)
    gid = np.cumsum(first) - 1
    start = np.flatnonzero(first)
    cnt = np.diff(np.append(start, rows.size))
    rank = np.arange(rows.size) - start[gid]
    acc = np.zeros((start.size, 4), np.float32)
    by_rank = np.argsort(rank, kind="stable")
    edges = np.searchsorted(rank[by_rank], np.arange(int(cnt.max(initial=0)) + 1))
    for r in range(edges.size - 1):   # one f32 addition per voxel and round: the sequential sum in input order
        sel = by_rank[edges[r]:edges[r + 1]]
        acc[gid[sel]] = acc[gid[sel]] + pts[rows[sel]]
    out = acc / cnt.astype(np.float32)[:, None]
    return dict(cloud=out, n_voxels=int(start.size), n_outside=int((finite & ~inside).sum()), n_nonfinite=int((~finite).sum()),
                max_per_voxel=int(cnt.max(initial=0)), cube=key[first, 0], rows=rows, gid=gid)


def merge_cloud(seed, leaf):
    """~22 000 points over 24 cubes: ~4 000 voxels of 1 - 5 points, voxels of 32 / 33 / 256 / 257 / 1000 / 4096 points (one lane, the LDS
    network at its smallest and largest size) and one of 4097 (ranking), shuffled; 300 points beyond the window."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-60.0, -30.0, -10.0]), np.array([90.0, 60.0, 30.0])
    nvox = 4000
    g = np.unique(np.floor(rng.uniform(lo, hi, size=(nvox + 64, 3)) / leaf).astype(np.int64), axis=0)
    g = g[rng.permutation(g.shape[0])][:nvox + 7]
    # the seven full voxels do not straddle a 50 m cube face (a straddling voxel is one voxel per cube: two keys)
    safe = (np.floor((g * leaf + 25.0) / 50.0) == np.floor(((g + 1) * leaf + 25.0 - 1e-6) / 50.0)).all(axis=1)
    g = np.concatenate([g[~safe], g[safe]])
    counts = np.concatenate([rng.integers(1, 6, size=nvox), [32, 33, 256, 257, 1000, 4096, 4097]])
    centre = np.repeat((g + 0.5) * leaf, counts, axis=0)
    xyz = centre + rng.uniform(-0.3, 0.3, size=centre.shape) * leaf
    far = np.concatenate([rng.uniform(540.0, 900.0, size=(100, 3)) * [1, 0.1, 0.1], rng.uniform(-40.0, 40.0, size=(100, 3)) + [0, 0, 300.0],
                          rng.uniform(-40.0, 40.0, size=(100, 3)) + [0, -3.0e6, 0]])
    xyz = np.concatenate([xyz, far])
    pts = np.concatenate([xyz, rng.uniform(0.0, 63.0, size=(xyz.shape[0], 1))], axis=1).astype(np.float32)
    # 1e-3 m off every cube face (the voxel faces are 0.2 leaf away by construction, the f32 rounding of a coordinate moves it by < 1e-4 leaf)
    f = np.mod(pts[:, :3].astype(np.float64) + 25.0, 50.0)
    pts = pts[((f > 2e-3) & (f < 50.0 - 2e-3)).all(axis=1)]
    return pts[rng.permutation(pts.shape[0])]


def check_import(vl, h, res, want, n_in):
    for k in (0, 1):
        m = want[k]
        assert res["n_in"][k] == n_in[k] and res["n_voxels"][k] == m["n_voxels"] and res["n_outside_window"][k] == m["n_outside"], (k, res)
        assert res["n_nonfinite"][k] == m["n_nonfinite"] and res["max_per_voxel"][k] == m["max_per_voxel"], (k, res)
        got = h.get_map_kind(k)
        assert got.shape == m["cloud"].shape, (k, got.shape, m["cloud"].shape)
        bad = np.flatnonzero((got.view(np.uint32) != m["cloud"].view(np.uint32)).any(axis=1))
        assert bad.size == 0, "kind %d: %d of %d map points differ from the model, first %s vs %s" % (k, bad.size, got.shape[0], got[bad[:1]], m["cloud"][bad[:1]])
    assert list(res["center_cube"]) == list(CEN0)
    st = h.map_health()
    assert st["keys"] == (want[0]["n_voxels"], want[1]["n_voxels"]) and st["purged"] == (0, 0) and st["deferred"] == (0, 0)
    h.sync()


def test_merge_arithmetic_against_the_model(vl, orc):
    import torch
    clouds = [merge_cloud(11, LEAF[0]), merge_cloud(12, LEAF[1])]
    want = [model(clouds[k], LEAF[k], CEN0) for k in (0, 1)]
    for k in (0, 1):
        m = want[k]
        assert 20000 < clouds[k].shape[0] < 25000 and np.unique(m["cube"]).size >= 6 and m["n_outside"] >= 250 and m["max_per_voxel"] == 4097
        big = m["rows"][m["gid"] == np.bincount(m["gid"]).argmax()]
        assert np.ptp(big) > clouds[k].shape[0] // 2 and (np.diff(big) > 1).any()   # a voxel's indices are scattered through the input
        # the CPU oracle's VoxelGrid, cube by cube (stable order within a voxel == input order): the same bits
        kept = clouds[k][np.sort(m["rows"])]
        kc = cube_abs(kept[:, :3]) + CEN0
        kcube = kc[:, 0] + 21 * kc[:, 1] + 441 * kc[:, 2]
        ref = np.concatenate([orc.voxel_grid(kept[kcube == c], LEAF[k]) for c in np.unique(kcube)])
        assert ref.shape == m["cloud"].shape and bits(ref) == bits(m["cloud"]), "oracle VoxelGrid per cube differs from the numpy model, kind %d" % k
    n_in = [c.shape[0] for c in clouds]
    maps = []
    for kw in (dict(map_capacity_log2=16), dict(map_capacity_log2=12, map_grow=1)):
        h = vl.Handle(0, scan_line=RINGS, with_mapping=1, **kw)
        res = h.map_import(clouds[0], clouds[1])
        check_import(vl, h, res, want, n_in)
        maps.append((bits(h.get_map()), {k: bits(np.asarray(v)) for k, v in res.items()}))
        if "map_grow" in kw:
            assert min(h.health()["map_log2"]) >= 14   # the tables stepped before the import: 4 000 voxels do not fit 60 % of 2^12 slots
        h.close()
    assert maps[0] == maps[1], "two imports of the same arrays differ"
    # the device form: the same arrays with a handful of non-finite points in between, dropped and counted
    rng = np.random.default_rng(5)
    dev, dwant = [], []
    for k in (0, 1):
        at = np.sort(rng.choice(clouds[k].shape[0], size=7, replace=False))
        c = np.insert(clouds[k], at, clouds[k][at], axis=0)
        for j, (col, val) in enumerate(((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (0, np.inf), (3, -np.inf), (1, np.nan))):
            c[at[j] + j, col] = val
        dev.append(torch.from_numpy(np.ascontiguousarray(c)).cuda())
        dwant.append(model(c, LEAF[k], CEN0))
        assert dwant[k]["n_nonfinite"] == 7 and bits(dwant[k]["cloud"]) == bits(want[k]["cloud"])
    h = vl.Handle(0, scan_line=RINGS, with_mapping=1, map_capacity_log2=15)
    res = h.map_import_device(dev[0], dev[1])
    check_import(vl, h, res, dwant, [int(d.shape[0]) for d in dev])
    assert bits(h.get_map()) == maps[0][0]
    with pytest.raises(vl.VloamError) as e:   # the host form refuses what the device form drops
        vl.Handle(0, scan_line=RINGS, with_mapping=1, map_capacity_log2=12).map_import(dev[0].cpu().numpy(), None)
    assert e.value.status == vl.ERR_INVALID and "not finite" in str(e.value)
    h.close()


def test_a_fixed_table_that_cannot_hold_the_voxels(vl):
    cloud = merge_cloud(11, LEAF[0])
    h = vl.Handle(0, scan_line=RINGS, with_mapping=1, map_capacity_log2=12)   # 4 007 voxels > 60 % of 4 096 slots
    with pytest.raises(vl.VloamError) as e:
        h.map_import(cloud, None)
    assert e.value.status == vl.ERR_CAPACITY and "corner" in str(e.value) and "60 %" in str(e.value)
    with pytest.raises(vl.VloamError) as e:   # sticky, as after a sweep that filled the table
        h.sync()
    assert e.value.status == vl.ERR_CAPACITY
    h.close()


# ---------------------------------------------------------------------------------------------- a map that a handle built
@pytest.fixture(scope="module")
def built(vl, orc, sweeps):
    """Handle A maps four sweeps; its two halves, a foreign sweep's feature clouds with a map-frame guess, and A's own answers."""
    # the input condition, on the CPU oracle's map of the same sweeps: no roll, every cube inside the valid block (no raw voxels), no centroid
    # within 1e-5 m of a voxel face — re-keying an exported point then cannot land in a neighbouring voxel
    o = orc.Oracle(scan_line=RINGS, with_mapping=True)
    for k in range(4):
        assert o.process(sweeps(RINGS, AZ, k)) == 0
    assert list(o.map_info()["cen"]) == list(CEN0)
    for which in (0, 1):
        inv = float(np.float32(1.0) / np.float32(LEAF[which]))
        for c in range(21 * 21 * 11):
            p = o.map_cube(which, c)
            if p.shape[0] == 0:
                continue
            assert abs(c % 21 - 10) <= 2 and abs((c // 21) % 21 - 10) <= 2 and abs(c // 441 - 5) <= 1, c
            v = p[:, :3].astype(np.float64) * inv
            assert np.abs(v - np.round(v)).min() / inv > 1e-5
    A = vl.Handle(0, scan_line=RINGS, with_mapping=1, map_capacity_log2=18)
    for k in range(4):
        staged_sweep(A, sweeps(RINGS, AZ, k))
        q, t = A.laser_mapping()
    st = A.map_state()
    assert list(st["cen"]) == list(CEN0) and st["deferred"] == 0
    halves = [A.get_map_kind(0).copy(), A.get_map_kind(1).copy()]
    assert halves[0].shape[0] > 1000 and halves[1].shape[0] > 500
    src = vl.Handle(0, scan_line=RINGS, with_mapping=0)
    src.scan_registration(sweeps(RINGS, AZ, 4))
    corner, surf, full = src.features(2).copy(), src.features(4).copy(), src.features(0).copy()
    src.close()
    guess = (rot_z(q, 0.5), t + np.array([0.1, -0.05, 0.02]))
    loc = A.map_localize(corner, surf, guess[0], guess[1], pose_frame=1)
    assert loc["flags"] & vl.LOC_SOLVED and not loc["flags"] & vl.LOC_WOULD_ROLL and loc["error_bits"] == 0
    rng = np.random.default_rng(3)
    qp = np.concatenate([halves[0][::9, :3], halves[1][::7, :3]])[:400] + rng.uniform(-0.3, 0.3, size=(400, 3)).astype(np.float32)
    query = A.map_query(qp, k=5, max_radius=1.5, kind=2)
    assert (query[2] > 0).sum() > 300
    out = dict(halves=halves, whole=A.get_map().copy(), pose=(q, t), corner=corner, surf=surf, full=full, guess=guess, loc=loc, qp=qp, query=query)
    A.close()
    return out


def imported(vl, built, **kw):
    h = vl.Handle(0, scan_line=RINGS, with_mapping=1, **kw)
    res = h.map_import(built["halves"][0], built["halves"][1])
    return h, res


@pytest.mark.parametrize("kw", [dict(map_capacity_log2=16), dict(map_capacity_log2=12, map_grow=1)], ids=["fixed-2^16", "growable"])
def test_round_trip_and_same_answers(vl, built, kw):
    B, res = imported(vl, built, **kw)
    for k in (0, 1):
        got = B.get_map_kind(k)
        assert got.shape == built["halves"][k].shape and bits(got) == bits(built["halves"][k]), "kind %d came back changed" % k
        assert res["n_voxels"][k] == res["n_in"][k] == built["halves"][k].shape[0] and res["n_outside_window"][k] == 0 and res["max_per_voxel"][k] == 1
    assert bits(B.get_map()) == bits(built["whole"])
    loc = B.map_localize(built["corner"], built["surf"], built["guess"][0], built["guess"][1], pose_frame=1)
    assert same_record(loc, built["loc"]), (loc, built["loc"])
    query = B.map_query(built["qp"], k=5, max_radius=1.5, kind=2)
    assert all(bits(a) == bits(b) for a, b in zip(query, built["query"]))
    B.sync()
    B.close()


def test_first_mapping_in_an_imported_map(vl, built, sweeps):
    B, _ = imported(vl, built, map_capacity_log2=16)
    n0 = B.get_map().shape[0]
    staged_sweep(B, sweeps(RINGS, AZ, 4))
    # with q_wmap_wodom = identity the guess LaserMapping::input forms from this odometry pose is the pose itself
    B.set_mapping_input(built["corner"], built["surf"], built["full"], built["guess"][0], built["guess"][1])
    q, t = B.laser_mapping()
    assert bits(q) == bits(built["loc"]["q_map"]) and bits(t) == bits(built["loc"]["t_map"]), (q, t, built["loc"]["q_map"], built["loc"]["t_map"])
    B.sync()
    assert B.get_map().shape[0] > n0 and B.trajectory().shape == (1, 14) and B.frame_count() == 1
    B.close()


def test_start_away_from_the_origin(vl, built, sweeps):
    t0 = np.array([730.0, -410.0, 60.0])
    q0 = rot_z(np.array([0.0, 0.0, 0.0, 1.0]), 37.0)
    moved = []
    for half in built["halves"]:
        m = half.copy()
        m[:, :3] = (np.array([qrot(q0, p) for p in half[:, :3].astype(np.float64)]) + t0).astype(np.float32)
        far = m[:40].copy()
        far[:20, 0] += 600.0
        far[20:, 2] -= 400.0
        moved.append(np.concatenate([m[:100], far, m[100:]]))
    C = vl.Handle(0, scan_line=RINGS, with_mapping=1, map_capacity_log2=16)
    res = C.map_import(moved[0], moved[1], q_wmap_wodom=q0, t_wmap_wodom=t0)
    cen = place_window(t0)
    assert list(cen) == [2, 11, 5] and list(res["center_cube"]) == list(cen)
    st = C.map_state()
    assert list(st["cen"]) == list(cen) and bits(st["q_wmap_wodom"]) == bits(q0) and bits(st["t_wmap_wodom"]) == bits(t0)
    assert list(st["centerCube"]) == [int(cube_abs(t0[a])) + cen[a] for a in range(3)]
    for k in (0, 1):   # structural: a rotated export may merge on re-keying, so no centroid is compared here
        assert res["n_outside_window"][k] == 40 and res["n_nonfinite"][k] == 0 and res["n_in"][k] == moved[k].shape[0]
        got = C.get_map_kind(k)
        assert got.shape[0] == res["n_voxels"][k] and 0 < got.shape[0] <= moved[k].shape[0] - 40
        assert np.abs(got[:, :3] - t0.astype(np.float32)).max() < 300.0   # nothing of the far points
    q, t = built["pose"]
    loc = C.map_localize(built["corner"], built["surf"], qmul(q0, q) / np.linalg.norm(qmul(q0, q)), qrot(q0, t) + t0, pose_frame=1)
    assert loc["flags"] & vl.LOC_SOLVED and not loc["flags"] & vl.LOC_WOULD_ROLL and loc["error_bits"] == 0, loc
    for k in range(3):
        C.process_scan(sweeps(RINGS, AZ, k))
    C.sync()
    tj = C.trajectory()
    assert tj.shape == (3, 14) and np.isfinite(tj).all() and np.linalg.norm(tj[0, 11:14] - t0) < 5.0
    assert list(C.map_state()["cen"]) == list(cen)
    C.close()


def test_lifecycle_checkpoint_and_refusals(vl, built, sweeps):
    clouds = [sweeps(RINGS, AZ, k) for k in range(4, 9)]

    def run(h, first, last):
        for k in range(first, last):
            h.process_scan(clouds[k])
        h.sync()

    U, _ = imported(vl, built, map_capacity_log2=16)
    run(U, 0, 5)
    V, _ = imported(vl, built, map_capacity_log2=16)
    run(V, 0, 3)
    ckpt = V.checkpoint()
    W = vl.Handle(0, scan_line=RINGS, with_mapping=1, map_capacity_log2=17)
    W.restore(ckpt)
    run(W, 3, 5)
    assert bits(W.trajectory()) == bits(U.trajectory()) and U.trajectory().shape == (5, 14)
    assert bits(W.get_map()) == bits(U.get_map()) and U.get_map().shape[0] > built["whole"].shape[0]
    assert all(bits(W.map_state()[k]) == bits(U.map_state()[k]) for k in U.map_state())
    run(V, 3, 5)   # the saving handle goes on as if nothing had happened
    assert bits(V.trajectory()) == bits(U.trajectory())
    # refusals: a second import, an import after a sweep
    for h in (U, W):
        with pytest.raises(vl.VloamError) as e:
            h.map_import(built["halves"][0], built["halves"][1])
        assert e.value.status == vl.ERR_ORDER
        h.sync()
    for h in (U, V, W):
        h.close()
    F = vl.Handle(0, scan_line=RINGS, with_mapping=1, map_capacity_log2=16)
    F.map_import(None, None)   # both clouds empty: the window and the start pose only
    assert F.get_map().shape[0] == 0
    with pytest.raises(vl.VloamError) as e:
        F.map_import(built["halves"][0], built["halves"][1])
    assert e.value.status == vl.ERR_ORDER and "already imported" in str(e.value)
    with pytest.raises(vl.VloamError) as e:
        F.restore(ckpt)
    assert e.value.status == vl.ERR_ORDER
    F.process_scan(clouds[0])
    F.sync()
    F.close()
    G = vl.Handle(0, n_sessions=2, scan_line=RINGS, with_mapping=1, map_capacity_log2=14)
    with pytest.raises(vl.VloamError) as e:
        G.map_import(built["halves"][0], built["halves"][1])
    assert e.value.status == vl.ERR_INVALID and "n_sessions" in str(e.value)
    G.batch_process_scan([clouds[0], clouds[1]])
    G.sync()
    G.close()
    N = vl.Handle(0, scan_line=RINGS, with_mapping=0)
    with pytest.raises(vl.VloamError) as e:
        N.map_import(built["halves"][0], built["halves"][1])
    assert e.value.status == vl.ERR_ORDER and "with_mapping" in str(e.value)
    N.process_scan(clouds[0])
    N.sync()
    N.close()
