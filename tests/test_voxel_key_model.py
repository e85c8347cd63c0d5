"""CPU: tests/voxel_key_model.py against the oracle, before any device result is judged by it.

The merge model against the oracle's VoxelGrid restatement cube by cube, bit for bit, on clouds that sit on voxel faces (where the f32 key
differs from an f64 floor), on cube faces and in voxels that a cube face cuts; the cube rule against the oracle's map — and, where it is
built, the reference's own laser_mapping.cpp — seeded through LaserMapping::input: a point exactly on -75 m or -125 m lies in the lower cube."""
import numpy as np
import pytest

import ref
import voxel_key_model as V

RINGS, AZ = 16, 256
IDENT = dict(q=[0.0, 0.0, 0.0, 1.0], t=[0.0, 0.0, 0.0])


def rows_sorted(a):
    b = np.ascontiguousarray(a, dtype=np.float32).tobytes()
    return sorted(b[i:i + 16] for i in range(0, len(b), 16))


def window_cube(xyz, cen=V.CEN0):
    w = V.cube_abs(xyz) + cen
    return w[:, 0] + 21 * w[:, 1] + 441 * w[:, 2]


@pytest.mark.parametrize("leaf", [0.4, 0.8, 0.2, 0.3])
def test_model_is_the_oracles_voxel_grid_cube_by_cube(orc, leaf):
    cloud = V.face_cloud(leaf, 21)
    m = V.model(cloud, leaf, V.CEN0)
    assert m["n_outside"] == 0 and m["n_voxels"] > 2500 and m["max_per_voxel"] == 40
    cube = window_cube(cloud[:, :3])
    ref_cloud = np.concatenate([orc.voxel_grid(cloud[cube == c], leaf) for c in np.unique(cube)])   # stable within a voxel == input order
    assert ref_cloud.shape == m["cloud"].shape and ref_cloud.tobytes() == m["cloud"].tobytes(), "oracle VoxelGrid per cube differs from the model"
    f64 = V.model(cloud, leaf, V.CEN0, index=V.f64_floor_index)
    assert f64["cloud"].tobytes() != m["cloud"].tobytes(), "the cloud must tell the f32 key from the f64 floor"
    if not V.divides_cube(leaf):   # a voxel cut by a cube face is one map point per cube: more map points than global voxels
        assert m["n_voxels"] >= np.unique(V.voxel_index(cloud[:, :3], leaf), axis=0).shape[0] + 10


def seeded(x, sweep, corner, surf):
    assert x.stage_sr(sweep) == 0
    x.stage_lo()
    assert x.stage_map(corner=corner, surf=surf, **IDENT) == 0
    return x


def check_cubes(o, clouds):
    """Every cube of the oracle's window holds exactly the points cube_abs assigns to it"""
    assert list(o.map_info()["cen"]) == list(V.CEN0)
    for kind in (0, 1):
        want = np.float32(0) + clouds[kind]   # one point per voxel: VoxelGrid's (0 + p) / 1 is p, but for -0.0
        cube = window_cube(want[:, :3])
        total = 0
        for c in range(21 * 21 * 11):
            got = o.map_cube(kind, c)
            assert rows_sorted(got) == rows_sorted(want[cube == c]), "kind %d, cube %d" % (kind, c)
            total += got.shape[0]
        assert total == clouds[kind].shape[0]
        # the exact negative faces: -75 m in cube -2, -125 m in cube -3 (floor would say -1 and -2)
        for axis, (lo, dim) in enumerate(((1, 21), (21, 21), (441, 11))):
            for face, A in ((-75.0, -2), (-125.0, -3)):
                on = clouds[kind][clouds[kind][:, axis] == np.float32(face)]
                assert on.shape[0] >= 1
                for p in on:
                    c = int(window_cube(p[None, :3])[0])
                    assert (c // lo) % dim == A + V.CEN0[axis] and p.tobytes() in rows_sorted(o.map_cube(kind, c))


@pytest.mark.parametrize("leaves", [(0.4, 0.8), (0.3, 0.6)])
def test_cube_rule_is_the_oracles(orc, sweeps, leaves):
    clouds = [V.face_cloud(leaves[k], 31 + k, single=True) for k in (0, 1)]
    o = seeded(orc.Oracle(scan_line=RINGS, line_res=leaves[0], plane_res=leaves[1], with_mapping=True), sweeps(RINGS, AZ, 0), *clouds)
    check_cubes(o, clouds)


@pytest.mark.skipif(not ref.available(), reason=ref.SKIP_REASON)
def test_cube_rule_is_the_references(orc, sweeps):
    from test_ref_laser_mapping import oracle_cubes
    from test_ref_laser_odometry import same_cloud
    clouds = [V.face_cloud(leaf, 31 + k, single=True) for k, leaf in enumerate((0.4, 0.8))]
    o = seeded(orc.Oracle(scan_line=RINGS, with_mapping=True), sweeps(RINGS, AZ, 0), *clouds)
    r = seeded(ref.Loam(scan_line=RINGS), sweeps(RINGS, AZ, 0), *clouds)
    counts, whole = oracle_cubes(o)
    assert counts.sum() == clouds[0].shape[0] + clouds[1].shape[0]
    assert np.array_equal(r.map_cube_counts(), counts), "points per cube: the reference against the oracle"
    assert same_cloud(r.cloud(8), whole), "/laser_cloud_map"
