"""The voxel key of a map-frame point as the device and the reference compute it, a numpy model of a map built from keyed points, and clouds
that sit on the places where that arithmetic can go wrong (plain module: tests/test_voxel_key_model.py pins it to the CPU oracle,
tests/test_gpu_voxel_faces.py judges the device by it).

The cube is laser_mapping.cpp's int() truncation plus its "< 0" correction on f64: NOT floor — a point exactly on a negative cube face
(-75 m, -125 m, ...) belongs to the LOWER cube.  The voxel is one correctly rounded f32 multiply and a floor, as PCL's VoxelGrid keys a point
(voxel_grid.hpp: floor(x * inverse_leaf_size)): on a voxel face float32(k * leaf) it can differ from the f64 floor of x / leaf by one."""
import numpy as np

F32 = np.float32
DIMS = np.array([21, 21, 11])    # the cube window, laser_mapping.h:110-117
CEN0 = np.array([10, 10, 5])     # its centre offsets at the start
CUBE_FACES = (-125.0, -75.0, -25.0, 25.0, 75.0, 125.0)
KEY_CUBES = np.array([512, 512, 128])   # the voxel key holds absolute cubes [-512, 512) horizontally and [-128, 128) vertically


def cube_abs(v):
    """laser_mapping.cpp:207-216 / 643-652: C int() truncation plus the "< 0" correction, on f64"""
    v = np.asarray(v, dtype=np.float64)
    c = np.trunc((v + 25.0) / 50.0).astype(np.int64)
    return c - (v + 25.0 < 0)


def voxel_index(p32, leaf):
    """floor(p * inv) in float32 with inv = 1 / leaf in float32: what the device and PCL's VoxelGrid compute"""
    p32 = np.asarray(p32)
    assert p32.dtype == F32
    inv = F32(1) / F32(leaf)
    v = np.floor(p32 * inv)
    assert v.dtype == F32
    return v.astype(np.int64)


def f64_floor_index(p32, leaf):
    """The key of tests/test_gpu_map_import.py's model: right away from the faces only"""
    return np.floor(np.asarray(p32).astype(np.float64) / leaf).astype(np.int64)


def model(pts, leaf, cen, index=voxel_index):
    """What get_map_kind must return for cloud pts (float32 [n, 4]) imported at leaf with window offsets cen, and the result's figures:
    key = (window cube, voxel z, y, x), sequential f32 sum in input order, division by float32(n).  A point whose absolute cube the voxel
    key cannot hold counts as outside the window (c_api.h, vloam_map_import_result)."""
    pts = np.asarray(pts, dtype=F32)
    finite = np.isfinite(pts).all(axis=1)
    xyz = np.where(finite[:, None], pts[:, :3], F32(0)).astype(F32)
    A = cube_abs(xyz)
    w = A + cen
    inside = finite & ((w >= 0) & (w < DIMS)).all(axis=1) & ((A >= -KEY_CUBES) & (A < KEY_CUBES)).all(axis=1)
    g = index(xyz, leaf)
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
    acc = np.zeros((start.size, 4), F32)
    by_rank = np.argsort(rank, kind="stable")
    edges = np.searchsorted(rank[by_rank], np.arange(int(cnt.max(initial=0)) + 1))
    for r in range(edges.size - 1):   # one f32 addition per voxel and round: the sequential sum in input order
        sel = by_rank[edges[r]:edges[r + 1]]
        acc[gid[sel]] = acc[gid[sel]] + pts[rows[sel]]
    out = acc / cnt.astype(F32)[:, None]
    return dict(cloud=out, n_voxels=int(start.size), n_outside=int((finite & ~inside).sum()), n_nonfinite=int((~finite).sum()),
                max_per_voxel=int(cnt.max(initial=0)), cube=key[first, 0], rows=rows, gid=gid)


def step(x, up):
    """The float32 next to x"""
    return np.nextafter(F32(x), F32(np.inf if up else -np.inf))


def with_neighbours(v):
    """v (float32 [m]) -> [3 m]: every value, one ulp below, one ulp above"""
    v = np.asarray(v, F32)
    return np.concatenate([v, np.nextafter(v, F32(-np.inf)), np.nextafter(v, F32(np.inf))])


TINY = np.array([0.0, -0.0, np.finfo(F32).tiny, -np.finfo(F32).tiny, 3e-42, -3e-42], F32)   # +-0, the smallest normals, a denormal of each sign


def divides_cube(leaf):
    """Does a voxel face lie on every cube face (25 / leaf whole, as for 0.2 m)?  Otherwise the voxel that holds a cube face straddles it."""
    return abs(25.0 / leaf - round(25.0 / leaf)) < 1e-9


def face_values(leaf, centre, axis, spread=150):
    """The special values of one axis around centre[axis]: (float32 values, on_face flags)"""
    c = float(centre[axis])
    cube = with_neighbours(np.array(CUBE_FACES) + c)
    k0 = int(round(c / leaf))
    vox = with_neighbours((np.arange(k0 - spread, k0 + spread + 1) * float(leaf)).astype(F32))
    n = [len(CUBE_FACES), 2 * spread + 1]
    flag = np.concatenate([np.arange(cube.size) < n[0], np.arange(vox.size) < n[1], TINY == 0])
    return np.concatenate([cube, vox, TINY]), flag


def face_cloud(leaf, seed, centre=(0.0, 0.0, 0.0), single=False):
    """A few thousand float32 points [n, 4] around centre, shuffled, on and next to the faces of the keying arithmetic:
    cube faces  on every axis -125 ... 125 m from centre: the face, one ulp below, one ulp above
    voxel faces float32(k * leaf) for 301 k around centre / leaf (both signs about the origin) with their one-ulp neighbours
    tiny        +-0, the smallest normals and a denormal of each sign, in each coordinate (outside the window of a centre far from the origin)
    straddling  voxels cut by a cube face, a point on either side: one voxel per cube, two map points (where leaf does not divide 25 m)
    many        most voxels hold one point; >= 30 hold 2 - 5 points of which one lies exactly on a face, with scattered input indices; one holds 40
    The two coordinates a special value does not occupy lie well inside a voxel within 20 m of centre.  The categories are asserted here.
    single=True: one point of every GLOBAL voxel only, a face point first (nothing for a VoxelGrid over the whole cloud, or a cube's, to merge)."""
    rng = np.random.default_rng(seed)
    centre = np.asarray(centre, np.float64)
    leaf = float(leaf)
    assert (np.mod(centre, 50.0) == 0).all(), "centre: a cube's centre, so that the faces lie 25 + 50 i from it"

    def inside_voxel(n):   # [n, 3] coordinates 0.25 - 0.75 leaf into a random voxel within 20 m of centre
        u = centre + rng.uniform(-20.0, 20.0, size=(n, 3))
        return ((np.floor(u / leaf) + rng.uniform(0.25, 0.75, size=(n, 3))) * leaf).astype(F32)

    xyz, on_face, n_below = [], [], 0
    for axis in range(3):
        vals, flag = face_values(leaf, centre, axis)
        p = inside_voxel(vals.size)
        p[:, axis] = vals
        xyz.append(p)
        on_face.append(flag)
        ks = np.arange(-150, 151) + int(round(centre[axis] / leaf))
        n_below += int(((ks * leaf).astype(F32) * (F32(1) / F32(leaf)) < ks.astype(F32)).sum())   # f32 product of a face point below its k
    # voxels cut by a cube face: a point 0.05 leaf to either side of the face, inside the voxel index of the face itself
    n_straddle = 0
    for axis in range(3):
        for face in CUBE_FACES:
            f = F32(face + centre[axis])
            pair = np.array([f - F32(0.05 * leaf), f + F32(0.05 * leaf)], F32)
            if np.unique(voxel_index(np.append(pair, f), leaf)).size != 1:
                continue   # the leaf puts a voxel face on (or within 0.05 leaf of) this cube face
            assert cube_abs(pair[0]) + 1 == cube_abs(pair[1])
            p = np.repeat(inside_voxel(1), 2, axis=0)
            p[:, axis] = pair
            xyz.append(p)
            on_face.append(np.zeros(2, bool))
            n_straddle += 1
    xyz, on_face = np.concatenate(xyz), np.concatenate(on_face)
    # company for face points: 1 - 4 more points in the voxel (and cube) of 60 voxel-face points and the 6 cube-face points of y, 39 more for one
    faces = np.flatnonzero(on_face)   # per axis: six cube faces, 301 voxel faces, two zeros
    per_axis = faces.size // 3
    ycube = faces[per_axis:per_axis + 6]   # the cube faces of the y axis get company; those of x and z stay alone in their voxels
    hosts = np.concatenate([rng.choice(np.setdiff1d(faces, faces[np.arange(faces.size) % per_axis < 6]), 60, replace=False), ycube])
    extra = []
    for j, host in enumerate(hosts):
        g = voxel_index(xyz[host], leaf)
        m = 39 if j == 0 else int(rng.integers(1, 5))
        q = ((g + rng.uniform(0.3, 0.7, size=(4 * m, 3))) * leaf).astype(F32)
        q = q[(voxel_index(q, leaf) == g).all(axis=1) & (cube_abs(q) == cube_abs(xyz[host])).all(axis=1)]
        extra.append(q[:m])
    xyz = np.concatenate([xyz] + extra)
    on_face = np.concatenate([on_face, np.zeros(xyz.shape[0] - on_face.size, bool)])
    perm = rng.permutation(xyz.shape[0])
    xyz, on_face = xyz[perm], on_face[perm]
    pts = np.concatenate([xyz, rng.uniform(0.0, 63.0, size=(xyz.shape[0], 1)).astype(F32)], axis=1)
    if single:
        first = np.argsort(~on_face, kind="stable")   # of a voxel's points the one on a face, if there is one
        _, keep = np.unique(voxel_index(xyz[first], leaf), axis=0, return_index=True)
        keep = np.sort(first[keep])
        pts, xyz, on_face = pts[keep], xyz[keep], on_face[keep]

    # ---- the categories are there
    assert pts.dtype == F32 and 2500 < pts.shape[0] < 5000, pts.shape
    for axis in range(3):
        c = F32(centre[axis])
        for face in CUBE_FACES:
            f = F32(face + centre[axis])
            for v in (f, step(f, False), step(f, True)):
                assert single or (xyz[:, axis] == v).any(), (axis, face)
            if face < -25.0 and c == 0:   # the reference's rule on an exact negative face: the lower cube
                assert cube_abs(f) == np.floor((float(f) + 25.0) / 50.0) - 1
        near_origin = np.abs(centre[axis]) < 30.0
        for v in TINY:
            assert single or (xyz[:, axis].view(np.uint32) == v.view(np.uint32)).any()
        if near_origin and not single:
            assert (xyz[:, axis] < 0).sum() > 300 and (xyz[:, axis] > 0).sum() > 300
    differ = int((voxel_index(xyz, leaf) != f64_floor_index(xyz, leaf)).any(axis=1).sum())
    if single:
        return pts
    if np.allclose(centre, 0):
        if leaf in (0.4, 0.8):
            assert differ >= 50, differ
        if leaf == 0.3:
            assert n_below >= 20, n_below
    assert divides_cube(leaf) or n_straddle >= 10, n_straddle
    m = model(pts, leaf, CEN0 + (-cube_abs(centre)))   # (offsets that centre the window on `centre`: grouping only)
    per = np.bincount(m["gid"])
    assert (per == 1).sum() > per.size // 2 and (per == 40).sum() == 1 and m["max_per_voxel"] == 40, np.bincount(per)
    face_in = np.bincount(m["gid"], weights=on_face[m["rows"]]) > 0
    some = (per >= 2) & (per <= 5) & face_in
    assert some.sum() >= 30, some.sum()
    big = m["rows"][m["gid"] == per.argmax()]
    assert on_face[big].any() and np.ptp(big) > pts.shape[0] // 2, "the 40-point voxel holds a face point, its indices are scattered"
    return pts
