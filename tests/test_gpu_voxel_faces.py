"""-m gpu: the voxel keying arithmetic (cube by the reference's f64 rule, voxel by an f32 multiply and floor) on the places where it can go
wrong — points exactly on cube faces and voxel faces and one ulp to either side, voxels that a cube face cuts, zeros and denormals, and the two
ends of the key range — in every copy of it: the mapping's insert, the import's own keying lines, the cube ranges of the query and of the
scan-to-map association.

Judged by tests/voxel_key_model.py (pinned to the CPU oracle and the reference in tests/test_voxel_key_model.py), the CPU oracle itself, and
the brute force of tests/test_gpu_map_query.py.  Every comparison is bit for bit; the poses of the association test keep the tolerance of
tests/test_gpu_branches.py."""
import numpy as np
import pytest

import branch_cases
import voxel_key_model as V
from test_gpu_laser_mapping import compare_map_round, lexsort_rows, oracle_map_points
from test_gpu_localize import bits, staged_sweep
from test_gpu_map_import import model as f64_model, place_window
from test_gpu_map_query import check, point_sets, top8

pytestmark = pytest.mark.gpu

RINGS, AZ = 16, 256
F32 = np.float32
PAIRS = [(0.4, 0.8), (0.2, 0.4), (0.3, 0.6)]
IDENT_Q, IDENT_T = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch brings a HIP runtime of its own: up before this module's first handle (tests/test_gpu_host_input.py); the device form takes tensors."""
    import torch
    torch.zeros(1).cuda()


def handle(vl, leaves, **kw):
    kw.setdefault("map_capacity_log2", 14)   # ~3 000 voxels of a kind
    return vl.Handle(0, scan_line=RINGS, with_mapping=1, mapping_line_resolution=leaves[0], mapping_plane_resolution=leaves[1], **kw)


def check_import(h, res, want, clouds, cen):
    for k in (0, 1):
        m = want[k]
        assert res["n_in"][k] == clouds[k].shape[0] and res["n_voxels"][k] == m["n_voxels"] and res["n_outside_window"][k] == m["n_outside"], (k, res)
        assert res["n_nonfinite"][k] == 0 and res["max_per_voxel"][k] == m["max_per_voxel"], (k, res)
        got = h.get_map_kind(k)
        assert got.shape == m["cloud"].shape, (k, got.shape, m["cloud"].shape)
        bad = np.flatnonzero((got.view(np.uint32) != m["cloud"].view(np.uint32)).any(axis=1))
        assert bad.size == 0, "kind %d: %d of %d map points differ from the model, first %s vs %s" % (k, bad.size, got.shape[0], got[bad[:1]], m["cloud"][bad[:1]])
    assert list(res["center_cube"]) == list(cen)
    assert h.map_health()["keys"] == (want[0]["n_voxels"], want[1]["n_voxels"])
    h.sync()


def face_queries(rng, M, clouds, leaf):
    """Every point of the clouds (the face points and their one-ulp neighbours among them); at the place of every map point on a cube face or
    one ulp from it, the face and its two neighbours (so each is asked for from the other side of the face); and, at the place of map points
    near each cube face, points within one leaf of the face"""
    out = [clouds[0][:, :3], clouds[1][:, :3]]
    for axis in range(3):
        for face in V.CUBE_FACES:
            three = V.with_neighbours([face])
            at = M[np.isin(M[:, axis], three), :3]
            assert at.shape[0] >= 3, (axis, face)
            b = M[np.argsort(np.abs(M[:, axis] - face))[:16], :3].copy()
            b[:, axis] = (face + rng.uniform(-leaf, leaf, 16)).astype(F32)
            out.append(b)
            for v in three:
                c = at.copy()
                c[:, axis] = v
                out.append(c)
    return np.ascontiguousarray(np.concatenate(out).astype(F32))


# ---------------------------------------------------------------------------------------------- a. import on faces
@pytest.mark.parametrize("leaves", PAIRS, ids=lambda p: "%g-%g" % p)
def test_import_on_faces(vl, leaves):
    import torch
    clouds = [V.face_cloud(leaves[k], 41 + k) for k in (0, 1)]
    want = [V.model(clouds[k], leaves[k], V.CEN0) for k in (0, 1)]
    for k in (0, 1):   # a green result means something: the f64-floor key of tests/test_gpu_map_import.py gives another map here
        old = f64_model(clouds[k], leaves[k], V.CEN0)
        assert old["n_voxels"] != want[k]["n_voxels"] or bits(old["cloud"]) != bits(want[k]["cloud"])
    h = handle(vl, leaves)
    check_import(h, h.map_import(clouds[0], clouds[1]), want, clouds, V.CEN0)
    whole = bits(h.get_map())
    h.close()
    h = handle(vl, leaves)
    dev = [torch.from_numpy(c).cuda() for c in clouds]
    check_import(h, h.map_import_device(dev[0], dev[1]), want, clouds, V.CEN0)
    assert bits(h.get_map()) == whole
    h.close()


# ---------------------------------------------------------------------------------------------- b, c. insert on faces; insert == import
def seed_device(h, sweep, corner, surf):
    staged_sweep(h, sweep)
    h.set_mapping_input(corner, surf, None, IDENT_Q, IDENT_T)
    h.laser_mapping()
    h.sync()


def seed_oracle(o, sweep, corner, surf):
    assert o.stage_sr(sweep) == 0
    o.stage_lo()
    assert o.stage_map(corner=corner, surf=surf, q=IDENT_Q, t=IDENT_T) == 0


@pytest.mark.parametrize("leaves", [PAIRS[0], PAIRS[2]], ids=lambda p: "%g-%g" % p)
def test_insert_on_faces_is_the_oracles_and_the_imports(vl, orc, sweeps, leaves):
    single = [V.face_cloud(leaves[k], 51 + k, single=True) for k in (0, 1)]
    many = [V.face_cloud(leaves[k], 53 + k) for k in (0, 1)]
    seeded_map = None
    for clouds in (single, many):   # many: the sweep's own VoxelGrid (map_stack.hip) merges first, the per-cube filter second
        h = handle(vl, leaves)
        o = orc.Oracle(scan_line=RINGS, line_res=leaves[0], plane_res=leaves[1], with_mapping=True)
        seed_device(h, sweeps(RINGS, AZ, 0), *clouds)
        seed_oracle(o, sweeps(RINGS, AZ, 0), *clouds)
        assert list(h.map_state()["cen"]) == list(o.map_info()["cen"]) == list(V.CEN0)
        for k in (0, 1):
            got, ref = h.get_map_kind(k), oracle_map_points(o, k)
            assert ref.shape[0] > 2500 and got.shape == ref.shape, (k, got.shape, ref.shape)
            bad = np.flatnonzero((got.view(np.uint32) != ref.view(np.uint32)).any(axis=1))
            assert bad.size == 0, "kind %d: %d of %d map points differ from the oracle's cubes, first %s vs %s" % (k, bad.size, got.shape[0], got[bad[:1]], ref[bad[:1]])
        if clouds is single:
            for k in (0, 1):   # the exact negative faces went into the lower cubes, nothing was merged
                assert h.get_map_kind(k).shape[0] == single[k].shape[0]
            seeded_map = h.get_map().copy()
        h.close()
    # c. the same single-occupancy clouds imported: the same map
    h = handle(vl, leaves)
    res = h.map_import(single[0], single[1])
    assert list(res["n_voxels"]) == [c.shape[0] for c in single] and list(res["max_per_voxel"]) == [1, 1]
    got = h.get_map()
    assert got.shape == seeded_map.shape and bits(got) == bits(seeded_map), "import and insert key the same points differently"
    h.sync()
    h.close()


# ---------------------------------------------------------------------------------------------- d. queries across faces
@pytest.mark.parametrize("leaves", [PAIRS[0], PAIRS[2]], ids=lambda p: "%g-%g" % p)
def test_queries_across_faces(vl, leaves):
    rng = np.random.default_rng(6)
    clouds = [V.face_cloud(leaves[k], 41 + k) for k in (0, 1)]
    h = handle(vl, leaves)
    h.map_import(clouds[0], clouds[1])
    M = point_sets(h)[2]
    # the map point on x = -75 m lies in the lower cube: the query one ulp above it (in the upper cube) must find it, and the query on the face
    # must find the map point one ulp above
    on, above = M[M[:, 0] == F32(-75.0)][:1, :3], M[M[:, 0] == V.step(-75.0, True)][:1, :3]
    assert on.shape[0] == 1 and above.shape[0] == 1
    cross = np.array([np.append(V.step(-75.0, True), on[0, 1:]), np.append(V.step(-75.0, False), on[0, 1:]), np.append(F32(-75.0), above[0, 1:])], F32)
    Q = np.concatenate([cross, face_queries(rng, M, clouds, leaves[0])])
    assert 6000 < Q.shape[0] < 7000
    best = top8(M, Q)
    total = 0
    for k, r in ((8, 1.5), (1, 0.5)):
        res = h.map_query(Q, k=k, max_radius=r, kind=2)
        total += check(res, Q, M, best, k, r, "leaves %s, k %d, r %g" % (leaves, k, r))
        ulp2 = (V.step(-75.0, True) - F32(-75.0)) ** 2
        assert (res[2][:3] >= 1).all() and res[1][0, 0] == ulp2 and res[1][2, 0] == ulp2
        assert bits(res[0][0, 0, :3]) == bits(on[0]) and bits(res[0][1, 0, :3]) == bits(on[0]) and bits(res[0][2, 0, :3]) == bits(above[0])
    assert total > 10000
    h.sync()
    h.close()


# ---------------------------------------------------------------------------------------------- e. association across the negative faces
def test_association_across_the_negative_cube_faces(vl, orc, synth):
    from test_gpu_branches import POSE_TOL, qdist, run_map_ties
    clouds = branch_cases.negative_face_tie_clouds()
    seq = synth.SynthSequence(n_rings=RINGS, n_azimuth=AZ, n_sweeps=3)
    h = vl.Handle(0, scan_line=RINGS, with_mapping=1, debug=1, map_capacity_log2=14)
    o = orc.Oracle(scan_line=RINGS, with_mapping=True)
    qm, tm = run_map_ties(h, seq, clouds=clouds)
    run_map_ties(o, seq, oracle=True, clouds=clouds)
    assert o.map_num_outer() == 2
    for which in (7, 8):
        assert np.array_equal(h.features(which)[:, :4].view(np.uint32), o.cloud(which)[:, :4].view(np.uint32))
    for outer in range(2):
        compare_map_round(h, o, outer)
    assert o.map_solve(0)["corner_num"] == clouds[2].shape[0] and o.map_solve(0)["surf_num"] == clouds[3].shape[0]
    oq, ot, _, _ = o.map_pose()
    assert qdist(qm, oq) < POSE_TOL and np.linalg.norm(tm - ot) < POSE_TOL
    for kind in (0, 1):
        _, pts = h.map_dump(kind)
        ref = oracle_map_points(o, kind)
        assert pts.shape == ref.shape and np.array_equal(lexsort_rows(pts)[:, :4].view(np.uint32), lexsort_rows(ref)[:, :4].view(np.uint32))
    h.sync()
    h.close()


# ---------------------------------------------------------------------------------------------- f. the ends of the key range
ENDS = {"x+511": np.array([25400.0, 0.0, 0.0]), "y-512,z-128": np.array([0.0, -25450.0, -6250.0])}


@pytest.mark.parametrize("end", sorted(ENDS))
def test_import_and_queries_at_the_ends_of_the_key_range(vl, end):
    """The window's last cubes are the key's last: absolute cube +511 on x; -512 on y and -128 on z.  (Built with map_import alone: a sequence
    cannot drive that far in a test's time.)"""
    rng = np.random.default_rng(7)
    t, leaves = ENDS[end], PAIRS[0]
    cen = place_window(t)
    edge = -cen   # absolute cube of window index 0
    assert (edge[0] + 20 == 511) if end == "x+511" else (edge[1] == -512 and edge[2] == -128)
    clouds = [V.face_cloud(leaves[k], 61 + k, centre=t) for k in (0, 1)]
    want = [V.model(clouds[k], leaves[k], cen) for k in (0, 1)]
    for k in (0, 1):
        x = clouds[k][:, :3]
        same_product = np.floor(x.astype(np.float64) * float(F32(1) / F32(leaves[k]))).astype(np.int64)
        assert (V.voxel_index(x, leaves[k]) != same_product).any(axis=1).sum() >= 100
        A = V.cube_abs(x[want[k]["rows"]])
        assert (A[:, 0] == 511).any() if end == "x+511" else ((A[:, 1] == -512).any() and (A[:, 2] == -128).any()), "the last cube holds map points"
    h = handle(vl, leaves)
    check_import(h, h.map_import(clouds[0], clouds[1], t_wmap_wodom=t), want, clouds, cen)
    M = point_sets(h)[2]
    Q = np.ascontiguousarray((M[rng.choice(M.shape[0], 200, replace=False), :3] + rng.uniform(-0.3, 0.3, (200, 3))).astype(F32))
    best = top8(M, Q)
    for k, r in ((8, 1.5), (1, 0.5)):
        assert check(h.map_query(Q, k=k, max_radius=r, kind=2), Q, M, best, k, r, "%s, k %d, r %g" % (end, k, r)) > 100
    h.sync()
    h.close()


BEYOND = {"x+512": (np.array([25450.0, 0.0, 0.0]), np.array([150.5, 1.0, 1.0])),
          "y-513,z-129": (np.array([0.0, -25500.0, -6300.0]), np.array([1.0, -150.5, -150.5]))}


@pytest.mark.parametrize("end", sorted(BEYOND))
def test_points_beyond_the_key_range(vl, sweeps, end):
    """Cubes of the window that the voxel key cannot hold (absolute cube 512; -513 and -129): an import counts their points as outside the
    window and goes on; a sweep that brings such points reports the sticky capacity error at sync, as a full table does."""
    t, off = BEYOND[end]
    leaves = PAIRS[0]
    cen = place_window(t)
    rng = np.random.default_rng(8)
    beyond = np.zeros((60, 4), F32)
    beyond[:, :3] = (t + off + rng.uniform(-8.0, 8.0, (60, 3))).astype(F32)
    A, w = V.cube_abs(beyond[:, :3]), V.cube_abs(beyond[:, :3]) + cen
    assert ((w >= 0) & (w < V.DIMS)).all(), "inside the window"
    assert (A[:, 0] == 512).all() if end == "x+512" else ((A[:, 1] == -513).all() and (A[:, 2] == -129).all())
    clouds = [V.face_cloud(leaves[k], 71 + k, centre=t) for k in (0, 1)]
    clouds = [np.concatenate([c[:1000], beyond[30 * k:30 * k + 30], c[1000:]]) for k, c in enumerate(clouds)]
    want = [V.model(clouds[k], leaves[k], cen) for k in (0, 1)]
    inside = [V.model(np.delete(clouds[k], np.arange(1000, 1030), axis=0), leaves[k], cen) for k in (0, 1)]
    for k in (0, 1):
        assert want[k]["n_outside"] == inside[k]["n_outside"] + 30 and bits(want[k]["cloud"]) == bits(inside[k]["cloud"])
    h = handle(vl, leaves)
    check_import(h, h.map_import(clouds[0], clouds[1], t_wmap_wodom=t), want, clouds, cen)
    M = point_sets(h)[2]
    Q = np.ascontiguousarray(np.concatenate([beyond[:, :3], M[::40, :3]]))
    best = top8(M, Q)
    res = h.map_query(Q, k=8, max_radius=1.5, kind=2)
    check(res, Q, M, best, 8, 1.5, end)
    assert not res[2][:60].any() and (res[2][60:] >= 1).all()
    h.sync()
    h.close()
    # the same points through k_map_insert: an empty map at the same start, one sweep whose stage input holds them (sensor frame: minus t, exact)
    h = handle(vl, leaves)
    h.map_import(None, None, t_wmap_wodom=t)
    local = beyond.copy()
    local[:, :3] = (beyond[:, :3].astype(np.float64) - t).astype(F32)
    assert np.array_equal((local[:, :3].astype(np.float64) + t).astype(F32), beyond[:, :3])
    with pytest.raises(vl.VloamError) as e:
        staged_sweep(h, sweeps(RINGS, AZ, 0))
        h.set_mapping_input(local[:30], local[30:], None, IDENT_Q, IDENT_T)
        h.laser_mapping()
        h.sync()
    assert e.value.status == vl.ERR_CAPACITY
    with pytest.raises(vl.VloamError) as e:   # sticky
        h.sync()
    assert e.value.status == vl.ERR_CAPACITY
    h.close()
