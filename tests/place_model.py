"""NumPy model of the place descriptor and its match (include/vloam_hip/c_api.h, "Place recognition"): the yardstick of tests/test_gpu_place.py,
tests/test_gpu_place_tool.py and tools/place_probe.py.  Every f32 operation is a numpy float32 operation of its own (numpy never fuses), atan2f
is tests/fdlibm_np.py's glibc-exact one, and everything behind the cell index is integers — so the device and this file agree bit for bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fdlibm_np  # noqa: E402

f32 = np.float32
PI_F = np.array([0x40490fdb], dtype=np.uint32).view(np.float32)[0]
MATCH_DTYPE = np.dtype([("row", "<i4"), ("tag", "<i4"), ("shift", "<i4"), ("dist", "<i4"), ("n_occupied_query", "<i4"), ("n_occupied_row", "<i4"),
                        ("pad", "<i4", (2,))])


class Geometry:
    """vloam_place_options with min_range already resolved (0 means the handle's minimum_range: pass that value here)."""

    def __init__(self, n_ring=20, n_sector=60, min_range=0.1, max_range=80.0, z_min=-3.0, z_step=0.05):
        self.R, self.S = int(n_ring), int(n_sector)
        self.W = (self.R + 3) // 4
        self.words = self.S * self.W
        self.min_range, self.max_range, self.z_min, self.z_step = f32(min_range), f32(max_range), f32(z_min), f32(z_step)
        self.min2, self.max2 = f32(self.min_range * self.min_range), f32(self.max_range * self.max_range)
        self.k = f32(f32(self.S) / f32(f32(2.0) * PI_F))
        w = f32(self.max_range / f32(self.R))
        e = np.array([f32(f32(i) * w) for i in range(self.R)], dtype=np.float32)
        self.edge2 = (e * e).astype(np.float32)   # [0] unused
        self.w = w


_angle_cache = {}


def _angles(x, y):
    """atan2f(y, x) per point (glibc's algorithm, scalar); cached on the coordinates: the angle does not depend on the geometry."""
    key = (x.tobytes(), y.tobytes())
    if key not in _angle_cache:
        if len(_angle_cache) > 64:
            _angle_cache.clear()
        _angle_cache[key] = np.array([fdlibm_np.atan2f(b, a) for a, b in zip(x, y)], dtype=np.float32).reshape(-1)
    return _angle_cache[key]


def cells_of(cloud, g):
    """(cells int32 [S, R] — the largest q per cell, 0 empty —, n_used) of a cloud float32 [n, >= 3]."""
    c = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 4)
    cells = np.zeros((g.S, g.R), np.int32)
    if c.shape[0] == 0:
        return cells, 0
    x, y, z = c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy()
    with np.errstate(all="ignore"):
        r2 = (x * x + y * y).astype(np.float32)   # two products and a sum, each rounded to f32
        use = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (r2 >= g.min2) & (r2 < g.max2)
    x, y, z, r2 = x[use], y[use], z[use], r2[use]
    if x.shape[0] == 0:
        return cells, 0
    ring = np.zeros(x.shape[0], np.int64)
    for i in range(1, g.R):
        ring += r2 >= g.edge2[i]
    a = _angles(x, y)
    with np.errstate(all="ignore"):
        fs = np.floor(((a + PI_F).astype(np.float32) * g.k).astype(np.float32))
        sector = np.minimum(g.S - 1, fs.astype(np.int64))
        # the clamps are taken in f32 before the conversion, where (int)floorf(...) of a huge quotient would not be defined; elsewhere equal
        fz = np.floor(((z - g.z_min).astype(np.float32) / g.z_step).astype(np.float32))
        q = np.clip(fz, f32(0.0), f32(254.0)).astype(np.int64) + 1
    np.maximum.at(cells, (sector, ring), q.astype(np.int32))
    return cells, int(x.shape[0])


def pack(cells, g):
    """Sector-major bytes desc[sector][ring], rings padded with zeros to W little-endian words: uint32 [S * W]."""
    b = np.zeros((g.S, 4 * g.W), np.uint8)
    b[:, :g.R] = cells.astype(np.uint8)
    return b.reshape(-1).view("<u4").astype(np.uint32)


def unpack(desc, g):
    b = np.ascontiguousarray(desc, dtype="<u4").reshape(-1).view(np.uint8).reshape(g.S, 4 * g.W)
    return b[:, :g.R].astype(np.int32)


def describe(cloud, g):
    """(desc uint32 [S * W], (n_used, n_occupied))."""
    cells, used = cells_of(cloud, g)
    return pack(cells, g), (used, int(np.count_nonzero(cells)))


def dists(Q, D):
    """dist(Q, D, s) for s = 0 .. S - 1; Q [S, R], D [..., S, R] integer cells."""
    Q, D = np.asarray(Q, np.int16), np.asarray(D, np.int16)
    S = Q.shape[0]
    out = np.zeros(D.shape[:-2] + (S,), np.int64)
    for s in range(S):
        out[..., s] = np.abs(np.roll(Q, -s, axis=0) - D).sum(axis=(-2, -1), dtype=np.int64)   # roll(Q, -s)[j] = Q[(j + s) mod S]
    return out


def best(Q, D):
    """(dist, shift) of the smallest dist over the shifts, ties to the smallest shift; arrays when D holds several rows."""
    d = dists(Q, D)
    s = np.argmin(d, axis=-1)   # the first minimum
    return np.take_along_axis(d, s[..., None], axis=-1)[..., 0], s


def match_all(qdesc, db_desc, g, chunk=4096):
    """Per row of db_desc [count, S * W]: (dist, shift, n_occupied_row) arrays, and the query's n_occupied."""
    db_desc = np.ascontiguousarray(db_desc, dtype=np.uint32).reshape(-1, g.words)
    n = db_desc.shape[0]
    Q = unpack(qdesc, g)
    dist, shift, occ = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        D = db_desc[a:b].view(np.uint8).reshape(b - a, g.S, 4 * g.W)[:, :, :g.R]
        dist[a:b], shift[a:b] = best(Q, D)
        occ[a:b] = np.count_nonzero(D, axis=(1, 2))
    return dist, shift, occ, int(np.count_nonzero(Q))


def records(matched, tags, count, k=1, exclude_last=0):
    """The k match records over rows 0 .. count - 1 of match_all's result: dist ascending, then row ascending, the youngest exclude_last skipped."""
    dist, shift, occ, nq = matched
    out = np.zeros(k, MATCH_DTYPE)
    out["row"] = -1
    limit = max(0, int(count) - int(exclude_last))
    order = np.lexsort((np.arange(limit), dist[:limit]))[:k]
    for r, row in enumerate(order):
        out[r] = (row, int(tags[row]), shift[row], dist[row], nq, occ[row], (0, 0))
    return out


def query(qdesc, db_desc, tags, g, k=1, exclude_last=0):
    """The k match records for a packed query against packed rows db_desc [count, S * W] with tags [count]."""
    db_desc = np.ascontiguousarray(db_desc, dtype=np.uint32).reshape(-1, g.words)
    return records(match_all(qdesc, db_desc, g), tags, db_desc.shape[0], k, exclude_last)


def polar_cloud(sector, ring, level, g):
    """Points at bin centres: sector / ring / height level (0 .. 254) index arrays -> float32 [n, 4].  Half a bin is far more than any f32
    rounding, so cells_of puts every point into exactly the cell it was made for."""
    sector, ring, level = (np.asarray(v, np.float64) for v in (sector, ring, level))
    a = -np.pi + (sector + 0.5) * 2.0 * np.pi / g.S
    r = (ring + 0.5) * float(g.max_range) / g.R
    z = float(g.z_min) + (level + 0.5) * float(g.z_step)
    return np.stack([r * np.cos(a), r * np.sin(a), z, np.zeros_like(z)], axis=1).astype(np.float32)
