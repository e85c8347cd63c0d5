"""NumPy statement of vloam_map_carve's definition (c_api.h): the range images of the sweeps and the vote over a list of map
points.  f32 arithmetic in the kernel's operation order (every product and sum rounded on its own), the two arctangents through
tests/fdlibm_np.py (glibc's, which csrc/fdlibm_f32.h restates for the device), f64 for the pose.  Works from map points, sweeps and poses
alone: it knows nothing of voxel tables, so raw voxels (skipped_raw) are outside it."""
import numpy as np

import fdlibm_np

f32 = np.float32
EMPTY = np.uint32(0xffffffff)
PI_F = np.array([0x40490fdb], np.uint32).view(np.float32)[0]
DEG_F = f32(0.017453292)

DEFAULTS = dict(kind_mask=3, rows=64, cols=1024, elev_min_deg=-25.0, elev_max_deg=3.0, min_range=2.0, max_range=80.0, range_res=0.05,
                margin=0.5, min_votes=1)


class Geom:
    def __init__(self, **kw):
        o = dict(DEFAULTS)
        o.update(kw)
        self.rows, self.cols, self.min_votes = int(o["rows"]), int(o["cols"]), int(o["min_votes"])
        self.min_range, self.max_range, self.range_res = f32(o["min_range"]), f32(o["max_range"]), f32(o["range_res"])
        self.elev_min = f32(o["elev_min_deg"]) * DEG_F
        elev_max = f32(o["elev_max_deg"]) * DEG_F
        self.row_scale = f32(self.rows) / (elev_max - self.elev_min)
        self.col_scale = f32(self.cols) / (f32(2.0) * PI_F)
        self.margin_q = int(np.floor(f32(o["margin"]) / self.range_res))


def project(G, xyz):
    """(ok bool [n], row, col int64 [n], q int64 [n]) of f32 points [n, 3]; row / col / q are 0 where ok is False."""
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    n = p.shape[0]
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    row, col, q = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        h2 = x * x + y * y
        r = np.sqrt(h2 + z * z)
        ok &= (r >= G.min_range) & (r <= G.max_range)
        t = z / np.sqrt(h2)
    for i in np.nonzero(ok)[0]:
        rf = (fdlibm_np.atanf(t[i]) - G.elev_min) * G.row_scale
        if not (rf >= f32(0.0) and rf < f32(G.rows)):
            ok[i] = False
            continue
        cf = (fdlibm_np.atan2f(y[i], x[i]) + PI_F) * G.col_scale
        c = int(np.floor(cf))
        if c >= G.cols:
            c -= G.cols
        row[i], col[i] = int(np.floor(rf)), min(max(c, 0), G.cols - 1)
        q[i] = int(np.floor(r[i] / G.range_res))
    return ok, row, col, q


def range_image(G, sweep):
    """uint32 [rows, cols]: the smallest quantised range per pixel, EMPTY where no point of the sweep (float32 [n, >= 3]) projects."""
    ok, row, col, q = project(G, np.asarray(sweep, dtype=np.float32)[:, :3])
    img = np.full((G.rows, G.cols), EMPTY, np.uint32)
    np.minimum.at(img, (row[ok], col[ok]), q[ok].astype(np.uint32))
    return img


def pose_matrix(pose7):
    """(R [3, 3], t [3]) f64 of (qx qy qz qw tx ty tz): q normalised, then the rotation matrix, in the order capi_carve.cpp computes them."""
    p = [np.float64(v) for v in pose7]
    nrm = np.sqrt(((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]) + p[3] * p[3])
    x, y, z, w = p[0] / nrm, p[1] / nrm, p[2] / nrm, p[3] / nrm
    R = np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                  [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                  [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]], np.float64)
    return R, np.array(p[4:7], np.float64)


def to_sensor(points, pose7):
    """f32 [n, 3]: R^T (p - t) in f64, each component (R0c*d0 + R1c*d1) + R2c*d2, rounded to f32."""
    R, t = pose_matrix(pose7)
    d = np.asarray(points, dtype=np.float32)[:, :3].astype(np.float64) - t[None, :]
    out = np.empty((d.shape[0], 3), np.float32)
    for c in range(3):
        out[:, c] = ((R[0, c] * d[:, 0] + R[1, c] * d[:, 1]) + R[2, c] * d[:, 2]).astype(np.float32)
    return out


def votes(G, points, images, poses):
    """Per map point (float32 [n, >= 3]): (in_view, seen_through, confirmed) int [n] — the number of sweeps for which the point projects, is
    seen through, is confirmed."""
    n = np.asarray(points).shape[0]
    view, through, confirm = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for img, pose in zip(images, poses):
        ok, row, col, q = project(G, to_sensor(points, pose))
        img = img.astype(np.int64)
        cen = img[row, col]
        m = cen.copy()
        for dr in (-1, 0, 1):
            rr = np.clip(row + dr, 0, G.rows - 1)
            for dc in (-1, 0, 1):
                m = np.minimum(m, img[rr, (col + dc) % G.cols])
        ret = ok & (cen != int(EMPTY))
        view += ok
        through += ret & (q + G.margin_q < m)
        confirm += ret & (np.abs(q - cen) <= G.margin_q)
    return view, through, confirm


def carve(points, sweeps, poses, **options):
    """The dry run on one kind's map points: (removed mask bool [n], counters dict of ints: examined, in_view, seen_through, confirmed, removed)."""
    G = Geom(**options)
    images = [range_image(G, s) for s in sweeps]
    view, through, confirm = votes(G, points, images, poses)
    removed = (through >= G.min_votes) & (confirm == 0)
    return removed, dict(examined=int(len(view)), in_view=int((view > 0).sum()), seen_through=int((through > 0).sum()),
                         confirmed=int((confirm > 0).sum()), removed=int(removed.sum()))
