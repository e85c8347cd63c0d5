"""Arguments for the device probes (vloam_debug_probe) and their host statements, shared by tests/test_dev_probe_host.py (CPU) and
tests/test_gpu_dev_probe.py (GPU).  Every generator is seeded and deterministic: gen(n) returns n elements in the probe's layout, the
constructed edge cases first (all of them, whatever n — n below their count is an error) and random cases filling the rest.  Also here: the
NumPy statements of the three __device__-only primitives (associate_to_map, dquat_mul / dquat_rot, the sort) and the branch census of
tf_get_rotation, computed from the inputs."""
import numpy as np

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64
N_GPU = 1 << 20      # elements per generator in the GPU tests
N_CPU = 1 << 14      # ... where the reference is a scalar Python transcription (tests/fdlibm_np.py)


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _around(values, ulps):
    """Every f32 in `values` and its neighbours up to +-ulps encodings away, both signs."""
    b = np.asarray(values, dtype=np.float32).view(np.uint32).astype(np.int64)
    b = (b[:, None] + np.arange(-ulps, ulps + 1)[None, :]).ravel()
    b = b[(b >= 0) & (b <= 0x7f800000)]
    return _f32(np.concatenate([b, b | 0x80000000]).astype(np.uint32))


def _random_bits_f32(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)


def _fill(parts, n, filler):
    head = np.concatenate(parts, axis=0)
    assert head.shape[0] <= n, "the constructed cases alone are %d elements" % head.shape[0]
    return np.ascontiguousarray(np.concatenate([head, filler(n - head.shape[0]).astype(head.dtype)], axis=0))


SPECIALS_F32 = _f32([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff])


# ---------------------------------------------------------------------------------------------------------------- fd_atanf
def gen_atanf(n=N_GPU, seed=11):
    rng = np.random.default_rng(seed)
    binades = _around(_f32((np.arange(1, 255, dtype=np.uint32) << 23)), 1)                     # every binade boundary +- 1 ulp
    breaks = _around([0.4375, 0.6875, 1.1875, 2.4375], 4)                                      # the four break points
    early = _around([2.0 ** -29, 2.0 ** 25], 4)                                                # thresholds of the early returns
    den = np.concatenate([_around(_f32([1, 2, 3, 0x00400000, 0x007fffff, 0x00800000]), 1),    # denormals: atanf(x) == x
                          _f32(rng.integers(1, 0x00800000, 256, dtype=np.uint32)), _f32(rng.integers(1, 0x00800000, 256, dtype=np.uint32) | 0x80000000)])

    def filler(m):
        a = _random_bits_f32(rng, m)
        k = m // 2                                                                             # u / v of LiDAR-like u, v
        u = rng.uniform(-30.0, 30.0, k).astype(F32)
        v = (rng.uniform(0.3, 120.0, k) * rng.choice([-1.0, 1.0], k)).astype(F32)
        a[:k] = u / v
        return a
    return _fill([binades, breaks, early, den, SPECIALS_F32, _f32([0x3f800000, 0xbf800000])], n, filler)


# ---------------------------------------------------------------------------------------------------------------- fd_atan2f
def gen_atan2f(n=N_GPU, seed=12):
    rng = np.random.default_rng(seed)
    nine = _f32([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x3f800000, 0xbf800000, 0x7f800000, 0xff800000, 0x7fc00000])
    grid = np.stack(np.meshgrid(nine, nine, indexing="ij"), -1).reshape(-1, 2)                 # every combination, (y, x)
    x_one = np.stack([np.concatenate([_random_bits_f32(rng, 256), rng.uniform(-3, 3, 256).astype(F32)]), np.ones(512, F32)], -1)
    # exponent differences around the cut-offs of the quotient: +-26 (fdlibm's classic form) and +-60 (the form restated here), all quadrants
    rows = []
    for k in list(range(-63, -56)) + list(range(-29, -22)) + list(range(23, 30)) + list(range(57, 64)):
        for sy in (0, 1):
            for sx in (0, 1):
                ex = rng.integers(max(1, 1 - k), min(254, 254 - k) + 1, 12)
                ey = ex + k
                y = _f32(((ey.astype(np.uint32) << 23) | rng.integers(0, 1 << 23, 12, dtype=np.uint32) | U32(sy << 31)).astype(np.uint32))
                x = _f32(((ex.astype(np.uint32) << 23) | rng.integers(0, 1 << 23, 12, dtype=np.uint32) | U32(sx << 31)).astype(np.uint32))
                rows.append(np.stack([y, x], -1))
    cut = np.concatenate(rows)
    # y / x overflows, underflows or is denormal
    big = _f32(rng.integers(0x7e000000, 0x7f800000, 256, dtype=np.uint32))
    tiny = _f32(rng.integers(1, 0x01800000, 256, dtype=np.uint32))
    mid = rng.uniform(0.5, 2.0, 256).astype(F32)
    sg = lambda a: (a * rng.choice([-1.0, 1.0], a.shape[0]).astype(F32)).astype(F32)
    quot = np.concatenate([np.stack([sg(big), sg(tiny)], -1), np.stack([sg(tiny), sg(big)], -1),
                           np.stack([sg((mid * F32(2.0 ** -100)).astype(F32)), sg((mid[::-1] * F32(2.0 ** 30)).astype(F32))], -1),   # quotient ~2^-130: denormal
                           np.stack([sg((mid * F32(2.0 ** -120)).astype(F32)), sg((mid[::-1] * F32(2.0 ** 20)).astype(F32))], -1)])  # ~2^-140
    # returns at 0.3 - 120 m with x or y within a few ulp of 0
    r = rng.uniform(0.3, 120.0, 512).astype(F32)
    near0 = np.tile(_f32([0, 1, 2, 3, 4, 0x80000000, 0x80000001, 0x80000002, 0x80000003, 0x80000004]), 52)[:512]
    axis = np.concatenate([np.stack([sg(r), near0], -1), np.stack([near0, sg(r)], -1)])

    def filler(m):
        a = np.stack([_random_bits_f32(rng, m), _random_bits_f32(rng, m)], -1)
        k = (2 * m) // 3                                                                       # LiDAR returns, all four quadrants
        az = rng.uniform(-np.pi, np.pi, k)
        rr = rng.uniform(0.3, 120.0, k)
        a[:k, 0] = (rr * np.sin(az)).astype(F32)
        a[:k, 1] = (rr * np.cos(az)).astype(F32)
        return a
    return _fill([grid, x_one, cut, quot, axis], n, filler)


# ---------------------------------------------------------------------------------------------------------------- elevation of a return
def _elevation_tables():
    hdl64 = np.concatenate([2.0 - np.arange(32) / 3.0, -8.83 - 0.5 * np.arange(32)])          # nominal HDL-64E: 1/3 deg upper, 1/2 deg lower block
    hdl32 = 10.67 - (4.0 / 3.0) * np.arange(32)
    vlp16 = -15.0 + 2.0 * np.arange(16)
    return np.radians(np.concatenate([hdl64, hdl32, vlp16]))


def gen_elev(n=N_GPU, seed=13):
    rng = np.random.default_rng(seed)
    tab = _elevation_tables()

    def returns(m):
        el = tab[rng.integers(0, tab.size, m)]
        az = rng.uniform(-np.pi, np.pi, m)
        r = rng.uniform(0.3, 120.0, m)
        return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], -1).astype(F32)
    edge = []
    z_vals = _f32([0x00000000, 0x80000000, 0x3f800000, 0xbf800000, 0x00000001, 0x7f7fffff, 0x7f800000, 0x7fc00000])
    for sc in (1e-19, 1e-20, 1e-21, 1e-22, 1e-23, 1e-30, 1e-45, 0.0, 1e19, 2e19, 1e20, 3e38):   # x*x + y*y denormal, 0, overflowing
        with np.errstate(over="ignore"):                                                       # (3e38 * 1.5: an infinite coordinate)
            xy = (rng.uniform(0.5, 1.5, (64, 2)) * rng.choice([-1.0, 1.0], (64, 2)) * sc).astype(F32)
            z = np.concatenate([z_vals, (rng.uniform(-2.0, 2.0, 56) * (sc if sc else 1.0)).astype(F32)])
        edge.append(np.concatenate([xy, z[:, None]], -1).astype(F32))
    z0 = returns(256)
    z0[:, 2] = _f32([0, 0x80000000] * 128)                                                     # z = +-0
    one_axis = returns(256)
    one_axis[:128, 0] = 0.0
    one_axis[128:, 1] = 0.0
    return _fill(edge + [z0, one_axis, returns(3 * 80 * 8)], n, returns)


# ---------------------------------------------------------------------------------------------------------------- tf_set_rotation / tf_get_rotation
LD = np.longdouble


def rotation_ld(q):
    """The rotation matrix of the quaternion(s) q (xyzw, any non-zero norm) in np.longdouble, rows of nine."""
    q = np.asarray(q, dtype=LD)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    two = LD(2)
    return np.stack([1 - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w),
                     two * (x * y + z * w), 1 - two * (x * x + z * z), two * (y * z - x * w),
                     two * (x * z - y * w), two * (y * z + x * w), 1 - two * (x * x + y * y)], -1)


def _axis_angle_q_ld(axis, angle):
    axis = np.asarray(axis, dtype=LD)
    axis = axis / np.sqrt((axis * axis).sum(-1, keepdims=True))
    half = np.asarray(angle, dtype=LD)[..., None] / LD(2)
    return np.concatenate([axis * np.sin(half), np.cos(half)], -1)


def _random_axes(rng, m):
    a = rng.normal(size=(m, 3))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


_PI_LD = LD(4) * np.arctan(LD(1))
_DELTAS = (0.0, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3)
TIE_NAMES = ("m0==m4>m8", "m0==m4<m8", "m4==m8>m0", "m4==m8<m0", "m0==m8>m4", "m0==m8<m4", "m0==m4==m8")


def _near_pi_quaternions(rng, per_delta):
    """Rotations by pi + d, d = 0, +-1e-12 .. +-1e-3, about x, y, z and about random axes (longdouble quaternions)."""
    out = []
    for d in _DELTAS:
        axes = np.concatenate([np.eye(3), -np.eye(3), _random_axes(rng, per_delta - 6)])
        out.append(_axis_angle_q_ld(axes, np.full(axes.shape[0], _PI_LD + LD(d))))
    return np.concatenate(out)


def _tie_quaternions():
    """Rotations by exactly pi about axes with two (or three) equal components: R = 2 a a^T - I has the equal diagonal entries bit for bit."""
    q = []
    for a, c in ((0.6, 0.2), (0.3, 0.9)):           # the equal pair above / below the third diagonal entry
        for pos in (2, 0, 1):                       # the odd component: m0==m4, m4==m8, m0==m8
            ax = [a, a, a]
            ax[pos] = c
            q.append(ax + [0.0])
    q = np.array(q, dtype=LD)[[0, 3, 1, 4, 2, 5]]   # TIE_NAMES order
    return np.concatenate([q, np.array([[1.0, 1.0, 1.0, 0.0]], dtype=LD)])


def gen_tf_getrot(n=N_GPU, seed=14):
    """(matrices f64 [n, 9], is_rotation bool [n]): is_rotation marks the rows that are a rotation matrix rounded to f64 entry by entry."""
    rng = np.random.default_rng(seed)
    near_pi = rotation_ld(_near_pi_quaternions(rng, 600)).astype(F64)
    ties = rotation_ld(_tie_quaternions()).astype(F64)
    ties = np.concatenate([ties, np.array([[0, 0, 1, 1, 0, 0, 0, 1, 0], [0, 1, 0, 0, 0, 1, 1, 0, 0]], F64)])   # +-120 deg about (1,1,1)/sqrt 3: trace == 0, all equal
    # trace == 0 exactly and +- a few ulp: 120 deg about random axes, m8 := -(m0 + m4), then stepped (no longer exactly a rotation)
    t0 = rotation_ld(_axis_angle_q_ld(_random_axes(rng, 2400), np.full(2400, LD(2) * _PI_LD / LD(3)))).astype(F64)
    t0[:, 8] = -(t0[:, 0] + t0[:, 4])
    for k, step in enumerate((0, 1, -1, 2, -2, 3, -3, 0)):
        sl = slice(k * 300, (k + 1) * 300)
        for _ in range(abs(step)):
            t0[sl, 8] = np.nextafter(t0[sl, 8], np.inf if step > 0 else -np.inf)
    any_m = np.concatenate([np.zeros((1, 9)), np.full((1, 9), np.nan), np.full((1, 9), np.inf), -np.eye(3).reshape(1, 9), np.eye(3).reshape(1, 9),
                            rng.normal(size=(256, 9)) * 10.0 ** rng.uniform(-300, 300, (256, 1))])
    n_rot = near_pi.shape[0] + ties.shape[0]
    head = [near_pi, ties, t0, any_m]

    def filler(m):
        q = rng.normal(size=(m, 4))
        return rotation_ld(q).astype(F64)
    cases = _fill(head, n, filler)
    is_rot = np.ones(n, bool)
    is_rot[n_rot:n_rot + t0.shape[0] + any_m.shape[0]] = False
    return cases, is_rot


def getrot_census(m):
    """Which branch of Matrix3x3::getRotation a matrix takes (0 trace > 0, 1 x-, 2 y-, 3 z-largest; -1 NaN trace -> the else half by the
    comparison's falsehood) and which tie it sits on, from the inputs alone."""
    m = np.asarray(m, F64)
    m0, m4, m8 = m[:, 0], m[:, 4], m[:, 8]
    with np.errstate(all="ignore"):
        tr = (m0 + m4) + m8
        pos = tr > 0.0
        i = np.where(m0 < m4, np.where(m4 < m8, 2, 1), np.where(m0 < m8, 2, 0))
    branch = np.where(pos, 0, 1 + i)
    neg = ~pos & np.isfinite(tr)
    ties = {"m0==m4>m8": neg & (m0 == m4) & (m0 > m8), "m0==m4<m8": neg & (m0 == m4) & (m0 < m8),
            "m4==m8>m0": neg & (m4 == m8) & (m4 > m0), "m4==m8<m0": neg & (m4 == m8) & (m4 < m0),
            "m0==m8>m4": neg & (m0 == m8) & (m0 > m4), "m0==m8<m4": neg & (m0 == m8) & (m0 < m4),
            "m0==m4==m8": neg & (m0 == m4) & (m4 == m8), "trace==0": tr == 0.0}
    return branch, ties


def gen_tf_roundtrip(n=N_GPU, seed=15):
    """Quaternions f64 [n, 4] (xyzw), not necessarily unit; row 0 is the zero quaternion."""
    rng = np.random.default_rng(seed)
    near_pi = _near_pi_quaternions(rng, 600).astype(F64)
    ties = _tie_quaternions().astype(F64)
    t0 = _axis_angle_q_ld(_random_axes(rng, 600), np.full(600, LD(2) * _PI_LD / LD(3))).astype(F64)
    t0 = np.concatenate([t0, np.array([[0.5, 0.5, 0.5, 0.5], [0.5, 0.5, 0.5, -0.5], [1.0, 1.0, 1.0, 1.0]])])
    base = np.concatenate([near_pi[::9], rng.normal(size=(600, 4))])
    scaled = np.concatenate([base * 10.0 ** e for e in (-150, -100, -30, -3, 3, 30, 100, 150)])
    special = np.array([[0, 0, 0, 0], [0, 0, 0, 1], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, -1], [np.nan, 0, 0, 1], [np.inf, 0, 0, 1],
                        [1e200, 0, 0, 1e200], [1e-200, 0, 0, 1e-200], [-0.0, 0.0, -0.0, 1.0]], F64)

    def filler(m):
        q = rng.normal(size=(m, 4))
        return q / np.linalg.norm(q, axis=1, keepdims=True)
    return _fill([special, near_pi, ties, t0, scaled], n, filler)


# ---------------------------------------------------------------------------------------------------------------- tf_mul(a, tf_inverse(b))
def _rigid(rng, m, scale):
    r = rotation_ld(rng.normal(size=(m, 4))).astype(F64)
    o = rng.uniform(-1.0, 1.0, (m, 3)) * scale
    return np.concatenate([r, o], -1)


def gen_tf_chain(n=N_GPU, seed=16):
    """f64 [n, 24]: a.m, a.o, b.m, b.o."""
    rng = np.random.default_rng(seed)

    def pairs(m):
        sc = 10.0 ** rng.uniform(-3, 5, (m, 1))                          # |o| up to 1e5
        a, b = _rigid(rng, m, sc), _rigid(rng, m, sc)
        same = rng.random(m) < 0.25                                      # a == b: the rotation is the identity up to rounding
        b[same] = a[same]
        return np.concatenate([a, b], -1)
    ident = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    head = np.array([np.concatenate([ident, ident])])
    big = pairs(512)
    big[:, 9:12] = np.sign(big[:, 9:12]) * 1e5
    big[:256, 12:] = big[:256, :12]
    return _fill([head, big], n, pairs)


# ---------------------------------------------------------------------------------------------------------------- associate_to_map
ASSOC_DTYPE = np.dtype([("p", "<f4", (4,)), ("q", "<f8", (4,)), ("t", "<f8", (3,))])
assert ASSOC_DTYPE.itemsize == 72
KEY_SPAN = 2.6e4      # metres a voxel key spans around the origin


def np_associate_to_map(c):
    """map_device.h associate_to_map: f64 arithmetic in its order, one f32 rounding per output component; f32 [n, 4]."""
    q, t, p = c["q"], c["t"], c["p"]
    ux, uy, uz, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    vx, vy, vz = p[:, 0].astype(F64), p[:, 1].astype(F64), p[:, 2].astype(F64)
    with np.errstate(all="ignore"):
        cx, cy, cz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
        cx, cy, cz = cx + cx, cy + cy, cz + cz
        dx, dy, dz = uy * cz - uz * cy, uz * cx - ux * cz, ux * cy - uy * cx
        o = np.stack([((vx + w * cx) + dx) + t[:, 0], ((vy + w * cy) + dy) + t[:, 1], ((vz + w * cz) + dz) + t[:, 2]], -1).astype(F32)
    return np.concatenate([o, p[:, 3:4]], -1)


def gen_assoc(n=N_GPU, seed=17):
    rng = np.random.default_rng(seed)

    def poses(m):
        q = rng.normal(size=(m, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        q *= 1.0 + rng.choice([0.0, 1e-9, -1e-9], (m, 1))                # norm 1 +- 1e-9
        t = rng.uniform(-1.0, 1.0, (m, 3)) * KEY_SPAN * 10.0 ** rng.uniform(-4, 0, (m, 1))
        return q, t

    def make(p, q, t):
        c = np.zeros(p.shape[0], ASSOC_DTYPE)
        c["p"], c["q"], c["t"] = p, q, t
        return c

    def plain(m):
        q, t = poses(m)
        p = np.concatenate([rng.uniform(-200.0, 200.0, (m, 3)), rng.uniform(0.0, 64.0, (m, 1))], -1).astype(F32)
        return make(p, q, t)
    # results within an ulp(f32) of a multiple of a default leaf (0.2, 0.4) or of a cube face (50 k - 25; 50 k as well): the pose inverted in
    # f64 on a world point with one component on the boundary, the sensor point nudged by +-1 ulp
    m = 1800
    q, t = poses(m)
    leaf = np.repeat(np.array([F32(0.2), F32(0.4), F32(50.0)]).astype(F64), m // 3)
    centre = t + rng.uniform(-100.0, 100.0, (m, 3))
    comp = rng.integers(0, 3, m)
    k = np.round(centre[np.arange(m), comp] / leaf)
    world = centre.copy()
    world[np.arange(m), comp] = k * leaf - np.where(leaf == 50.0, rng.choice([0.0, 25.0], m), 0.0)
    qn = q / np.linalg.norm(q, axis=1, keepdims=True)
    r = rotation_ld(qn).astype(F64).reshape(m, 3, 3)
    sensor = np.einsum("nji,nj->ni", r, world - t).astype(F32)          # R^T (w - t)
    on_face = []
    for step in (0, 1, -1):
        p = sensor.copy()
        if step:
            p = np.nextafter(p, np.where(step > 0, F32(np.inf), F32(-np.inf)).astype(F32))
        on_face.append(make(np.concatenate([p, np.ones((m, 1), F32)], -1), q, t))
    # non-finite point components
    bad = plain(64 * 4)
    vals = _f32([0x7fc00000, 0x7f800000, 0xff800000, 0xffc00000])
    for j in range(4):
        bad["p"][j * 64:(j + 1) * 64, j] = np.tile(vals, 16)
    ident = make(np.array([[1, 2, 3, 4], [0, 0, 0, 0], [-0.0, -0.0, -0.0, -0.0]], F32), np.tile([0.0, 0, 0, 1], (3, 1)), np.zeros((3, 3)))
    far = plain(512)
    far["t"] = np.sign(far["t"]) * KEY_SPAN
    return _fill([ident, bad, far] + on_face, n, plain)


# ---------------------------------------------------------------------------------------------------------------- dquat_mul / dquat_rot
def np_dquat(c):
    """map_device.h dquat_mul(a, b) and dquat_rot(a, v) in f64, in their order; f64 [n, 7]."""
    a, b, v = c[:, 0:4], c[:, 4:8], c[:, 8:11]
    with np.errstate(all="ignore"):
        r = np.stack([a[:, 3] * b[:, 0] + a[:, 0] * b[:, 3] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                      a[:, 3] * b[:, 1] + a[:, 1] * b[:, 3] + a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 3] * b[:, 2] + a[:, 2] * b[:, 3] + a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0],
                      a[:, 3] * b[:, 3] - a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1] - a[:, 2] * b[:, 2]], -1)
        ux, uy, uz, w = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
        cx, cy, cz = uy * v[:, 2] - uz * v[:, 1], uz * v[:, 0] - ux * v[:, 2], ux * v[:, 1] - uy * v[:, 0]
        cx, cy, cz = cx + cx, cy + cy, cz + cz
        dx, dy, dz = uy * cz - uz * cy, uz * cx - ux * cz, ux * cy - uy * cx
        o = np.stack([(v[:, 0] + w * cx) + dx, (v[:, 1] + w * cy) + dy, (v[:, 2] + w * cz) + dz], -1)
    return np.concatenate([r, o], -1)


def gen_quat(n=N_GPU, seed=18):
    """f64 [n, 11]: a, b (xyzw), v."""
    rng = np.random.default_rng(seed)

    def plain(m):
        a, b = rng.normal(size=(m, 4)), rng.normal(size=(m, 4))
        unit = rng.random(m) < 0.75
        a[unit] /= np.linalg.norm(a[unit], axis=1, keepdims=True)
        b[unit] /= np.linalg.norm(b[unit], axis=1, keepdims=True)
        v = rng.uniform(-1.0, 1.0, (m, 3)) * 10.0 ** rng.uniform(-3, 5, (m, 1))
        return np.concatenate([a, b, v], -1)
    sp = plain(11 * 5)
    for j in range(11):
        sp[j * 5:(j + 1) * 5, j] = [np.nan, np.inf, -np.inf, 0.0, -0.0]
    scaled = np.concatenate([plain(128) * 10.0 ** e for e in (-160, -100, 100, 160)])      # products under- and overflow
    ident = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 1, 2, 3]], F64)
    return _fill([ident, sp, scaled], n, plain)


# ---------------------------------------------------------------------------------------------------------------- block_bitonic_sort_u64
SORT_PROBLEMS = 64
# the (P2, workgroup size) pairs block_bitonic_sort_u64 is called with: 256 lanes on up to 4096 keys (map_stack.hip, map_output.hip,
# map_cloud_dev.h), 512 lanes on up to 4096 (a sector) and on 8192 / 16384 keys (a long ring) in sr_ring_long.hip
SORT_PAIRS = tuple((p2, 256) for p2 in (256, 512, 1024, 2048, 4096)) + tuple((p2, 512) for p2 in (256, 512, 1024, 2048, 4096, 8192, 16384))
PAD = np.uint64(0xffffffffffffffff)      # the callers' padding value


def gen_sort(p2, seed=19):
    """u64 [SORT_PROBLEMS, p2]: one problem per row."""
    rng = np.random.default_rng(seed + p2)

    def rnd(m):
        return rng.integers(0, 1 << 64, m, dtype=np.uint64)
    rows = []
    for k in range(SORT_PROBLEMS):
        kind = k % 16
        a = rnd(p2)
        if kind == 1:
            a = np.sort(a)                                               # already sorted
        elif kind == 2:
            a = np.sort(a)[::-1].copy()                                  # reverse sorted
        elif kind == 3:
            a[:] = [rnd(1)[0], PAD, np.uint64(0), np.uint64(1)][(k // 16) % 4]   # all keys equal
        elif kind == 4:
            a = rng.choice(rnd(2), p2)                                   # two distinct values
        elif kind == 5:
            a = rng.choice(np.array([0, PAD], U64), p2)                  # only 0 and the padding value
        elif kind == 6:
            a[rng.random(p2) < 0.3] = PAD                                # the padding value mixed with others
            a[rng.random(p2) < 0.1] = 0
        elif kind == 7:
            m = int(rng.integers(1, p2))                                 # a caller's shape: m keys, padding behind them
            a[m:] = PAD
            a[rng.integers(0, m)] = PAD                                  # ... and one real key that equals the padding
        elif kind == 8:
            a = (rnd(p2) << np.uint64(32)) | np.uint64(0x12345678)       # differ only in the top word
        elif kind == 9:
            a = np.uint64(0xabcdef01 << 32) | (rnd(p2) >> np.uint64(32))  # differ only in the bottom word
        elif kind == 10:
            a = rng.integers(0, 8, p2, dtype=np.uint64)                  # many duplicates
        elif kind == 11:
            a = (rng.integers(0, 4, p2, dtype=np.uint64) << np.uint64(32)) | np.arange(p2, dtype=np.uint64)   # (voxel, index) keys: unique, few top words
        elif kind == 12:
            a = np.sort(a)
            a[[0, p2 - 1]] = a[[p2 - 1, 0]]                              # sorted but for the two ends
        elif kind == 13:
            a = np.sort(a).reshape(2, -1)[::-1].ravel().copy()           # two sorted halves, swapped
        rows.append(a.astype(U64))
    return np.ascontiguousarray(np.stack(rows))
