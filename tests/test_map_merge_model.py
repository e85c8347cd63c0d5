"""CPU: tests/map_merge_model.py, the NumPy statement of vloam_map_merge that the GPU tests judge the device by, against what it restates —
the reference's rule for a cube that gets points appended and is re-filtered (laser_mapping.cpp:654-659, 689-702: the CPU oracle's VoxelGrid
over concatenate([the cube's map points, the new points of the cube in input order]), cube by cube, bit for bit) and the pose arithmetic of
capi_carve.cpp (carve_model.pose_matrix)."""
import numpy as np
import pytest

import map_merge_model as mm
from carve_model import pose_matrix
from voxel_key_model import CEN0

LEAF = (0.4, 0.8)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.fixture(scope="module")
def pairs():
    return [mm.cloud_pair(21 + k, LEAF[k]) for k in (0, 1)]


def test_transform_is_the_carve_pose_arithmetic():
    q, t = mm.POSE
    assert abs(np.linalg.norm(q) - 1.0) < 1e-12
    R, tt = pose_matrix(list(q) + list(t))
    yaw = np.deg2rad(37.0)
    assert abs(R[0, 0] - np.cos(yaw)) < 1e-12 and abs(R[1, 0] - np.sin(yaw)) < 1e-12 and bits(tt) == bits(np.asarray(t))   # Rz(37) Rx(2): the first column is Rz's
    rng = np.random.default_rng(1)
    p = np.concatenate([rng.uniform(-100, 100, size=(500, 3)), rng.uniform(0, 63, size=(500, 1))], axis=1).astype(np.float32)
    got = mm.transform(p, q, t)
    for i in range(0, 500, 7):   # scalar by scalar, Python floats: every operation rounded on its own
        x, y, z = (float(v) for v in p[i, :3])
        for r in range(3):
            want = np.float32(((float(R[r, 0]) * x + float(R[r, 1]) * y) + float(R[r, 2]) * z) + float(tt[r]))
            assert got[i, r].tobytes() == want.tobytes(), (i, r)
    assert bits(got[:, 3]) == bits(p[:, 3])
    # the identity takes the point as it is, the sign of a zero included
    z = np.array([[-0.0, 1.5, -0.0, 7.0]], np.float32)
    assert bits(mm.transform(z)) == bits(z) and bits(mm.transform(z, [0, 0, 0, 1], [0, 0, 0])) == bits(z)
    assert bits(mm.transform(z, [0, 0, 0, 1], [0, 0, 1e-9])[:, :2]) != bits(z[:, :2])   # ... and nothing else does: -0 + 0 = +0


def test_clouds_reach_every_path_and_keep_off_the_faces(pairs):
    for k, (A, B) in enumerate(pairs):
        a = mm.merge(np.zeros((0, 4), np.float32), A, LEAF[k])
        assert a["res"]["n_new_voxels"] == 4000 and a["res"]["n_outside_window"] == 0 and 10000 < A.shape[0] < 14000
        m = mm.merge(a["cloud"], B, LEAF[k], q=mm.POSE[0], t=mm.POSE[1])
        r = m["res"]
        assert 20000 < B.shape[0] < 25000 and r["n_outside_window"] == 300 and r["max_per_voxel"] == 4097 and r["n_new_voxels"] == 2000
        assert r["n_hit_points"] > sum(mm.BIG) + 4000 and r["n_new_points"] > 4000 and r["n_in"] == r["n_hit_points"] + r["n_new_points"] + 300
        on_old = m["cnt"][m["held"] == 1]
        assert all(c in on_old for c in mm.BIG) and np.unique(m["cube"]).size >= 6   # the big voxels sit on existing map points
        for xyz in (A[:, :3], m["xp"][m["rows"], :3], a["cloud"][:, :3], m["cloud"][:, :3]):
            dv, dc = mm.face_margins(xyz, LEAF[k])
            assert dv > 1e-3 and dc > 2e-3, (k, dv, dc)


def test_fold_is_the_reference_rule_cube_by_cube(orc, pairs):
    for k, (A, B) in enumerate(pairs):
        a = mm.merge(np.zeros((0, 4), np.float32), A, LEAF[k])
        # from nothing: vloam_map_import's rule, the oracle's VoxelGrid over the cube's points in input order
        _, ka = mm.key_rows(A[:, :3], LEAF[k], CEN0)
        ref = np.concatenate([orc.voxel_grid(A[ka[:, 0] == c], LEAF[k]) for c in np.unique(ka[:, 0])])
        assert ref.shape == a["cloud"].shape and bits(ref) == bits(a["cloud"]), "kind %d: the fold from nothing" % k
        # onto a map: concatenate([existing centroids of the cube, new points of the cube in input order])
        m = mm.merge(a["cloud"], B, LEAF[k], q=mm.POSE[0], t=mm.POSE[1])
        new = m["xp"][m["rows"]]
        _, kn = mm.key_rows(new[:, :3], LEAF[k], CEN0)
        parts = []
        for c in np.unique(np.concatenate([a["cube"], kn[:, 0]])):
            parts.append(orc.voxel_grid(np.concatenate([a["cloud"][a["cube"] == c], new[kn[:, 0] == c]]), LEAF[k]))
        ref = np.concatenate(parts)
        assert ref.shape == m["cloud"].shape and bits(ref) == bits(m["cloud"]), "kind %d: the fold onto a map" % k
        # a voxel that got nothing keeps its bits
        same = m["cnt"] == 0
        old = set(bits(r) for r in a["cloud"])
        assert same.sum() > 1900 and all(bits(r) in old for r in m["cloud"][same])


def test_raw_voxels_and_drops_are_counted():
    A, B = mm.cloud_pair(33, LEAF[0], n_vox=400)
    a = mm.merge(np.zeros((0, 4), np.float32), A, LEAF[0])
    xp = mm.transform(B, *mm.POSE)
    inside, _ = mm.key_rows(xp[:, :3], LEAF[0], CEN0)
    raw_at = xp[np.flatnonzero(inside)[:50]]
    keep = ~np.isin(mm.key_rows(a["cloud"][:, :3], LEAF[0], CEN0)[1].view("V32").reshape(-1), mm.key_rows(raw_at[:, :3], LEAF[0], CEN0)[1].view("V32").reshape(-1))
    m = mm.merge(a["cloud"][keep], mm.with_nonfinite(B), LEAF[0], q=mm.POSE[0], t=mm.POSE[1], raw_at=raw_at)
    r = m["res"]
    assert r["n_nonfinite"] == 7 and r["n_skipped_raw"] >= 50 and r["n_in"] == B.shape[0] + 7
    assert r["n_in"] == r["n_new_points"] + r["n_hit_points"] + r["n_skipped_raw"] + r["n_outside_window"] + r["n_nonfinite"]
    plain = mm.merge(a["cloud"][keep], B, LEAF[0], q=mm.POSE[0], t=mm.POSE[1], raw_at=raw_at)
    assert bits(plain["cloud"]) == bits(m["cloud"])
