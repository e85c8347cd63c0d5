"""NumPy statement of vloam_map_merge's definition (c_api.h) and the clouds its tests use (plain module:
tests/test_map_merge_model.py pins it to the CPU oracle's VoxelGrid and to carve_model.pose_matrix, tests/test_gpu_map_merge.py and
tests/test_gpu_merge_tool.py judge the device by it).

The transform is f64 from the f32 components, ((R_r0*x + R_r1*y) + R_r2*z) + t_r with every operation rounded on its own, rounded to f32; the
key is the f64 floor of tests/test_gpu_map_import.py's model (the clouds here keep 1e-3 leaf from every voxel face and 2e-3 m from every cube
face after the transform, where it equals the device's f32 key); the fold starts from the map point a voxel holds and adds the new points one
f32 addition at a time in input order, then divides by float32(1 + n) — or float32(n) from zero where the voxel held nothing."""
import numpy as np

from carve_model import pose_matrix
from voxel_key_model import CEN0, DIMS, cube_abs, f64_floor_index

F32 = np.float32
POSE = None   # set below: the transform of the tests, yaw 37 degrees, a small roll, t = (12.3, -4.1, 0.7)


def quat_yaw_roll(yaw_deg, roll_deg):
    """(x, y, z, w) of Rz(yaw) Rx(roll)"""
    a, b = np.deg2rad(yaw_deg) / 2.0, np.deg2rad(roll_deg) / 2.0
    return np.array([np.cos(a) * np.sin(b), np.sin(a) * np.sin(b), np.sin(a) * np.cos(b), np.cos(a) * np.cos(b)])


POSE = (quat_yaw_roll(37.0, 2.0), np.array([12.3, -4.1, 0.7]))


def is_identity(q, t):
    return q is None and t is None or (tuple(np.asarray(q if q is not None else [0, 0, 0, 1], float)) == (0.0, 0.0, 0.0, 1.0)
                                         and not np.any(np.asarray(t if t is not None else [0, 0, 0], float)))


def transform(pts, q=None, t=None):
    """float32 [n, 4]: this map <- the clouds' frame.  The identity takes the points as they are."""
    p = np.ascontiguousarray(pts, dtype=F32).reshape(-1, 4)
    if is_identity(q, t):
        return p.copy()
    R, tt = pose_matrix(list(q if q is not None else [0, 0, 0, 1]) + list(t if t is not None else [0, 0, 0]))
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    out = p.copy()
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = (((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + tt[r]).astype(F32)
    return out


def key_rows(xyz, leaf, cen, index=f64_floor_index):
    """(inside bool [n], rows int64 [n, 4]: window cube index, voxel z, y, x) of f32 points in the map frame.  index: the f64 floor (right away
    from the faces only), or voxel_key_model.voxel_index, the device's f32 arithmetic, for clouds that were not built to keep off the faces"""
    xyz = np.asarray(xyz, dtype=F32)
    ok = np.isfinite(xyz).all(axis=1) & (np.abs(xyz) < 1.0e6).all(axis=1)
    v = np.where(ok[:, None], xyz, F32(0)).astype(np.float64)
    w = cube_abs(v) + np.asarray(cen)
    inside = ok & ((w >= 0) & (w < DIMS)).all(axis=1)
    g = index(v.astype(F32), leaf)
    return inside, np.stack([w[:, 0] + 21 * w[:, 1] + 441 * w[:, 2], g[:, 2], g[:, 1], g[:, 0]], axis=1)


def face_margins(xyz, leaf):
    """(smallest distance to a voxel face in leaves, to a cube face in metres) of map-frame points"""
    v = np.asarray(xyz, dtype=np.float64)
    fv = v / leaf - np.floor(v / leaf)
    fc = np.mod(v + 25.0, 50.0)
    return float(np.minimum(fv, 1.0 - fv).min(initial=1.0)), float(np.minimum(fc, 50.0 - fc).min(initial=50.0))


def merge(existing, new, leaf, cen=CEN0, q=None, t=None, raw_at=None, index=f64_floor_index):
    """existing: float32 [m, 4], the merged map points of one kind (one per voxel); new: float32 [n, 4] in the clouds' frame; raw_at: float32
    [r, >= 3] points inside the voxels that hold un-merged raw points (those voxels are not part of `existing` and stay out of `cloud`).
    Returns cloud (what get_map_kind gives for the merged voxels afterwards, export order: cube, voxel z, y, x), the fields of
    vloam_map_merge_result for this kind, per map point its window cube (cube), what it held (held) and got (cnt), the transformed points (xp)
    and the input rows that were folded (rows)."""
    ex = np.ascontiguousarray(existing, dtype=F32).reshape(-1, 4)
    new = np.ascontiguousarray(new, dtype=F32).reshape(-1, 4)
    finite = np.isfinite(new).all(axis=1)
    xp = transform(np.where(finite[:, None], new, F32(0)), q, t)
    in_ex, k_ex = key_rows(ex[:, :3], leaf, cen, index)
    assert in_ex.all(), "the existing map lies inside the window"
    in_new, k_new = key_rows(xp[:, :3], leaf, cen, index)
    in_new &= finite
    rows = np.flatnonzero(in_new)
    k_raw = np.zeros((0, 4), np.int64)
    if raw_at is not None and len(raw_at):
        in_raw, k_raw = key_rows(np.asarray(raw_at, dtype=F32)[:, :3], leaf, cen, index)
        k_raw = np.unique(k_raw[in_raw], axis=0)
    uniq, inv = np.unique(np.concatenate([k_ex, k_new[rows], k_raw]), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    g_ex, g_new, g_raw = inv[:ex.shape[0]], inv[ex.shape[0]:ex.shape[0] + rows.size], inv[ex.shape[0] + rows.size:]
    assert np.unique(g_ex).size == g_ex.size, "one existing map point per voxel"
    n_grp = uniq.shape[0]
    raw = np.zeros(n_grp, bool)
    raw[g_raw] = True
    assert not raw[g_ex].any()
    held = np.zeros(n_grp, np.int64)
    held[g_ex] = 1
    acc = np.zeros((n_grp, 4), F32)
    acc[g_ex] = ex
    keep = ~raw[g_new]
    cnt = np.bincount(g_new[keep], minlength=n_grp)
    # rank of every point inside its voxel, input order; one f32 addition per voxel and round: the sequential sum
    order = np.lexsort((rows, g_new))
    gs, rs = g_new[order], rows[order]
    start = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]]) if gs.size else np.zeros(0, np.int64)
    rank = np.arange(gs.size) - np.repeat(start, np.diff(np.r_[start, gs.size]))
    sel_ok = ~raw[gs]
    for r in range(int(rank.max(initial=-1)) + 1):
        sel = np.flatnonzero((rank == r) & sel_ok)
        acc[gs[sel]] = acc[gs[sel]] + xp[rs[sel]]
    total = held + cnt
    live = (total > 0) & ~raw
    out = acc.copy()
    touched = live & (cnt > 0)
    out[touched] = acc[touched] / total[touched].astype(F32)[:, None]
    pts_new = int(cnt[(held == 0) & ~raw].sum())
    res = dict(n_in=new.shape[0], n_new_points=pts_new, n_hit_points=int(cnt[(held == 1) & ~raw].sum()), n_skipped_raw=int((~keep).sum()),
               n_outside_window=int((finite & ~in_new).sum()), n_nonfinite=int((~finite).sum()), n_new_voxels=int(((held == 0) & (cnt > 0) & ~raw).sum()),
               max_per_voxel=int(cnt[~raw].max(initial=0)))
    return dict(cloud=out[live], cube=uniq[live, 0], res=res, xp=xp, rows=rows[keep], held=held[live], cnt=cnt[live])


# ---------------------------------------------------------------------------------------------- the clouds of the tests
def _voxels(rng, lo, hi, leaf, n):
    """n distinct voxels (int64 [n, 3]) between lo and hi that do not straddle a 50 m cube face"""
    g = np.unique(np.floor(rng.uniform(lo, hi, size=(2 * n + 64, 3)) / leaf).astype(np.int64), axis=0)
    safe = (np.floor((g * leaf + 25.0) / 50.0) == np.floor(((g + 1) * leaf + 25.0 - 1e-6) / 50.0)).all(axis=1)
    g = g[safe]
    g = g[rng.permutation(g.shape[0])]
    assert g.shape[0] >= n
    return g[:n]


def _fill(rng, g, counts, leaf):
    """points inside voxels g, counts[i] of them in voxel i, 0.2 leaf away from the voxel's faces; float64 [sum, 3]"""
    centre = np.repeat((g + 0.5) * leaf, counts, axis=0)
    return centre + rng.uniform(-0.3, 0.3, size=centre.shape) * leaf


def _with_intensity(rng, xyz):
    return np.concatenate([xyz, rng.uniform(0.0, 63.0, size=(xyz.shape[0], 1))], axis=1).astype(F32)


BIG = (32, 33, 256, 257, 4096, 4097)   # one lane at its largest, the LDS network at its smallest and largest size, ranking


def cloud_pair(seed, leaf, q=POSE[0], t=POSE[1], n_vox=4000):
    """(A, B): A float32 [~12 000, 4] in the map frame — n_vox voxels of 1 - 5 points over 24 cubes, one map point each once imported; B
    float32 [~22 000, 4] in a frame that (q, t) takes into the map: after the transform half of its n_vox small voxels are A's and half are
    new, six more voxels of BIG points sit on voxels of A, 200 points lie beyond the window and 100 beyond any window; shuffled."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-60.0, -30.0, -10.0]), np.array([90.0, 60.0, 30.0])
    g = _voxels(rng, lo, hi, leaf, n_vox + n_vox // 2)
    gA, g_fresh = g[:n_vox], g[n_vox:]
    A = _with_intensity(rng, _fill(rng, gA, rng.integers(1, 6, size=n_vox), leaf))
    A = A[rng.permutation(A.shape[0])]
    gB = np.concatenate([gA[:n_vox // 2], g_fresh, gA[n_vox // 2:n_vox // 2 + len(BIG)]])
    counts = np.concatenate([rng.integers(1, 6, size=n_vox // 2 + g_fresh.shape[0]), BIG])
    target = _fill(rng, gB, counts, leaf)
    far = np.concatenate([rng.uniform(540.0, 900.0, size=(100, 3)) * [1, 0.1, 0.1], rng.uniform(-40.0, 40.0, size=(100, 3)) + [0, 0, 330.0],
                          rng.uniform(-40.0, 40.0, size=(100, 3)) + [0, -3.0e6, 0]])
    target = np.concatenate([target, far])
    R, tt = pose_matrix(list(q) + list(t))
    src = (target - tt[None, :]) @ R      # R^T (p - t), row by row
    B = _with_intensity(rng, src)
    return A, B[rng.permutation(B.shape[0])]


def with_nonfinite(cloud, seed=5):
    """the cloud with seven duplicated rows made non-finite in between (the device form drops and counts them)"""
    rng = np.random.default_rng(seed)
    at = np.sort(rng.choice(cloud.shape[0], size=7, replace=False))
    c = np.insert(cloud, at, cloud[at], axis=0)
    for j, (col, val) in enumerate(((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (0, np.inf), (3, -np.inf), (1, np.nan))):
        c[at[j] + j, col] = val
    return np.ascontiguousarray(c)
