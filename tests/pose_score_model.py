"""The numpy model of a pose score (vloam_map_score_poses, c_api.h): the definition, nothing of the device's search.

Per pose, kind and used point: p = pointAssociateToMap in f64 rounded to f32 (the expression of tests/test_oracle_pipeline.py), the searched set
the kind's map cloud (Handle.get_map_kind), d2 = (dx*dx + dy*dy) + dz*dz in f32 with every product and sum rounded on its own
(tests/test_gpu_map_query.py::top8), dmin the smallest, a hit when dmin <= r*r (f32 product); sum_d2_q24 adds floor(dmin * 2^24) over the hits.
A p with a non-finite component or one beyond +-1e6 is no hit.  Brute force, in chunks."""
import numpy as np

F32 = np.float32
SCORE_DTYPE = np.dtype([("n_hit", "<i4", (2,)), ("n_used", "<i4", (2,)), ("sum_d2_q24", "<u8", (2,))])


def associate(points, q, t):
    """float32 [n, 3]: the sensor-frame points under the map-frame pose (q xyzw, t), f64 throughout, rounded once."""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    v = np.asarray(points)[:, :3].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        uv = np.cross(q[:3], v)
        uv = uv + uv
        return (v + q[3] * uv + np.cross(q[:3], uv) + t).astype(F32)


def nearest_d2(P, Q, chunk=256):
    """float32 [n]: the smallest d2 of every row of Q (float32 [n, 3]) over the point set P (float32 [m, >= 3]); inf for an empty set."""
    out = np.full(Q.shape[0], np.inf, F32)
    if P.shape[0] == 0 or Q.shape[0] == 0:
        return out
    px, py, pz = (np.ascontiguousarray(P[:, a], dtype=F32) for a in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, Q.shape[0], chunk):
            q = Q[a:a + chunk]
            dx, dy, dz = q[:, None, 0] - px[None, :], q[:, None, 1] - py[None, :], q[:, None, 2] - pz[None, :]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F32
            d2[np.isnan(d2)] = np.inf
            out[a:a + chunk] = d2.min(axis=1)
    return out


def point_dmin(P, p_map):
    """float32 [n]: dmin of map-frame points p_map (float32 [n, 3]) over the set P; inf where the point is not searched."""
    with np.errstate(invalid="ignore"):
        ok = (np.abs(p_map) <= F32(1.0e6)).all(axis=1)   # false for NaN and inf
    dmin = np.full(p_map.shape[0], np.inf, F32)
    dmin[ok] = nearest_d2(P, p_map[ok])
    return dmin


def dmin_tables(maps, corner, surf, poses):
    """The radius- and stride-free part, computed once per scene: per kind float32 [M, n] — dmin of EVERY point of the kind's cloud under every pose."""
    poses = np.asarray(poses, np.float64).reshape(-1, 7)
    tabs = []
    for kind, cloud in enumerate((corner, surf)):
        pts = np.zeros((0, 4), F32) if cloud is None else np.asarray(cloud, F32).reshape(-1, 4)
        tab = np.full((poses.shape[0], pts.shape[0]), np.inf, F32)
        if pts.shape[0]:
            for m, pose in enumerate(poses):
                tab[m] = point_dmin(maps[kind], associate(pts, pose[:4], pose[4:]))
        tabs.append(tab)
    return tabs


def records(tabs, stride=(1, 1), radius=(1.0, 1.0)):
    """SCORE_DTYPE [M] from dmin_tables(): points 0, s, 2s, ... of each kind, hits within the kind's radius, quantised sums."""
    out = np.zeros(tabs[0].shape[0], SCORE_DTYPE)
    for kind, tab in enumerate(tabs):
        d = tab[:, ::int(stride[kind])]
        out["n_used"][:, kind] = d.shape[1]
        hit = d <= F32(radius[kind]) * F32(radius[kind])
        q24 = np.floor(np.where(hit, d, F32(0)).astype(np.float64) * 2.0 ** 24).astype(np.uint64)
        out["n_hit"][:, kind] = hit.sum(axis=1)
        out["sum_d2_q24"][:, kind] = q24.sum(axis=1, dtype=np.uint64)
    return out


def score_poses(maps, corner, surf, poses, stride=(1, 1), radius=(1.0, 1.0)):
    """SCORE_DTYPE [M]: maps = (corner map, surf map) as get_map_kind returns them; corner / surf float32 [n, 4] or None; poses float64 [M, 7]."""
    return records(dmin_tables(maps, corner, surf, poses), stride, radius)


def rank(scores):
    """Indices best first: more hits (both kinds), then the smaller sum (both kinds), then the smaller index."""
    s = np.asarray(scores)
    return np.lexsort((np.arange(s.shape[0]), s["sum_d2_q24"].sum(axis=1, dtype=np.uint64), -s["n_hit"].sum(axis=1, dtype=np.int64)))


def before(a, ia, b, ib):
    """Does record a (index ia) come before record b (index ib) in the ranking?"""
    ka = (-int(a["n_hit"].sum()), int(a["sum_d2_q24"].sum(dtype=np.uint64)), ia)
    kb = (-int(b["n_hit"].sum()), int(b["sum_d2_q24"].sum(dtype=np.uint64)), ib)
    return ka < kb


def yaw_quat(a):
    return np.array([0.0, 0.0, np.sin(a / 2.0), np.cos(a / 2.0)])


def qmul(a, b):
    x1, y1, z1, w1 = a
    x2, y2, z2, w2 = b
    return np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2,
                     w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])


def grid_pose(m, q_center, t_center, n_xy, n_z, n_yaw, half_extent, half_yaw):
    """Candidate m of vloam_map_relocalize's grid: (q, t) in f64."""
    steps = (n_xy[0], n_xy[1], n_z, n_yaw)
    ext = (half_extent[0], half_extent[1], half_extent[2], half_yaw)
    idx = (m % steps[0], (m // steps[0]) % steps[1], (m // (steps[0] * steps[1])) % steps[2], m // (steps[0] * steps[1] * steps[2]))
    off = [0.0 if n == 1 else -e + 2.0 * e * i / (n - 1) for n, e, i in zip(steps, ext, idx)]
    return qmul(yaw_quat(off[3]), np.asarray(q_center, np.float64)), np.asarray(t_center, np.float64) + np.array(off[:3])
