"""CPU: pose scores and relocalisation — the structs, the entry points, the option checks (before any device call, before the handle is looked
at: every refusal is made with a NULL handle), and the numpy model of tests/pose_score_model.py against a ten-point case worked out by hand.
The GPU side: tests/test_gpu_pose_score.py, tests/test_gpu_relocalize.py."""
import ctypes as C
import re

import numpy as np

import pose_score_model as model
from test_sweep_log_config import header

F32 = np.float32
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def test_structs_defaults_and_exports(vl):
    assert C.sizeof(vl.ScoreOptions) == 24 and vl.ScoreOptions.radius.offset == 16
    assert vl.POSE_SCORE_DTYPE.itemsize == 32 and vl.POSE_SCORE_DTYPE.fields["sum_d2_q24"][1] == 16 and vl.POSE_SCORE_DTYPE == model.SCORE_DTYPE
    assert C.sizeof(vl.RelocalizeOptions) == 88 and vl.RelocalizeOptions.half_extent.offset == 32 and vl.RelocalizeOptions.score.offset == 64
    assert vl.RELOCALIZE_RESULT_DTYPE.itemsize == 2288 == 48 + 8 * 32 + 8 * vl.LOCALIZE_RESULT_DTYPE.itemsize + 8 * 32
    assert [vl.RELOCALIZE_RESULT_DTYPE.fields[k][1] for k in ("candidate", "coarse", "refined", "fine")] == [16, 48, 304, 2032]
    L = vl.lib()
    plain = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for sym in ("vloam_map_score_poses", "vloam_map_score_poses_device", "vloam_map_relocalize"):
        assert hasattr(L, sym), sym
        assert re.search(r"vloam_status\s+%s\(vloam_handle\*\s*h," % sym, plain), sym
    for sym in ("vloam_default_score_options", "vloam_default_relocalize_options"):
        assert hasattr(L, sym) and re.search(r"void\s+%s\(" % sym, plain), sym
    for name, fields in (("vloam_score_options", "struct_size stride reserved radius"), ("vloam_pose_score", "n_hit n_used sum_d2_q24")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), plain, flags=re.S).group(1)
        assert re.findall(r"\b([a-z_0-9]+)(?:\[\d+\])?;", body) == fields.split(), name
    opt = vl.ScoreOptions(-1, (C.c_int * 2)(-1, -1), -1, (C.c_float * 2)(-1.0, -1.0))
    L.vloam_default_score_options(C.byref(opt))
    assert (opt.struct_size, list(opt.stride), opt.reserved, list(opt.radius)) == (24, [1, 1], 0, [1.0, 1.0])
    ro = vl.RelocalizeOptions()
    L.vloam_default_relocalize_options(C.byref(ro))
    assert (ro.struct_size, list(ro.n_xy), ro.n_z, ro.n_yaw, ro.top_k, list(ro.reserved)) == (88, [9, 9], 1, 9, 4, [0, 0])
    assert list(ro.half_extent) == [2.0, 2.0, 0.0] and abs(ro.half_yaw - np.deg2rad(10.0)) < 1e-15
    assert (ro.score.struct_size, list(ro.score.stride), list(ro.score.radius)) == (24, [1, 1], [1.0, 1.0])
    # the score kernels are launched outside the per-kernel profile table: ids and count are what they were
    L.vloam_profile_kernel_name.restype = C.c_char_p
    names = [L.vloam_profile_kernel_name(k).decode() for k in range(L.vloam_profile_kernel_count())]
    assert names[-2:] == ["k_pose_info_lo", "k_pose_info_map"] and "k_map_score" not in names


def test_every_score_refusal_with_a_null_handle(vl):
    L = vl.lib()
    corner, surf = np.ones((4, 4), F32), np.ones((6, 4), F32)
    poses = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float64), (3, 1))
    out = np.zeros(3, vl.POSE_SCORE_DTYPE)

    def opts(size=24, stride=(1, 1), reserved=0, radius=(1.0, 1.0)):
        return vl.ScoreOptions(size, (C.c_int * 2)(*stride), reserved, (C.c_float * 2)(*radius))

    def call(opt, c=corner, nc=4, s=surf, ns=6, p=poses, M=3, o=out, forms=(0, 1)):
        res = []
        for k, fn in enumerate((L.vloam_map_score_poses, L.vloam_map_score_poses_device)):
            if k in forms:
                st = fn(None, C.byref(opt) if opt is not None else None, P(c), nc, P(s), ns, P(p), M, P(o))
                res.append((st, L.vloam_last_error()))
                assert res[-1][1].startswith(b"vloam_map_score_poses_device:" if k else b"vloam_map_score_poses:"), res[-1]
        assert all(r[0] == res[0][0] and r[1].split(b":", 1)[1] == res[0][1].split(b":", 1)[1] for r in res), res
        return res[0]

    for ok in (opts(), opts(stride=(3, 7), radius=(1e-3, 1e30))):   # accepted options get as far as the (null) handle
        st, msg = call(ok)
        assert st == vl.ERR_INVALID and b"null handle" in msg, msg
    st, msg = call(opts(), c=None, nc=0, s=None, ns=0, p=None, M=0, o=None)
    assert st == vl.ERR_INVALID and b"null handle" in msg, msg
    st, msg = call(None)
    assert st == vl.ERR_INVALID and b"null options" in msg
    for size in (0, 20, 23, 28, -24):
        st, msg = call(opts(size=size))
        assert st == vl.ERR_INVALID and b"struct_size must be 24" in msg, (size, msg)
    st, msg = call(opts(reserved=1))
    assert st == vl.ERR_INVALID and b"reserved must be 0" in msg, msg
    for stride in ((0, 1), (1, 0), (-3, 1), (1, -(1 << 30))):
        st, msg = call(opts(stride=stride))
        assert st == vl.ERR_INVALID and b"stride[%d] must be at least 1" % (0 if stride[0] < 1 else 1) in msg, (stride, msg)
    for bad in (0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        for k in (0, 1):
            r = [1.0, 1.0]
            r[k] = bad
            st, msg = call(opts(radius=r))
            assert st == vl.ERR_INVALID and b"radius[%d] must be positive and finite" % k in msg, (r, msg)
    for nc, ns in ((-1, 6), (4, -1)):
        st, msg = call(opts(), nc=nc, ns=ns)
        assert st == vl.ERR_INVALID and b"negative cloud size" in msg, msg
    for M in (-1, 65537, 1 << 30):
        st, msg = call(opts(), M=M)
        assert st == vl.ERR_INVALID and b"M must be 0 .. 65536" in msg, (M, msg)
    for nc, ns in ((7681, 6), (4, (1 << 24) + 1)):
        st, msg = call(opts(), nc=nc, ns=ns)
        assert st == vl.ERR_INVALID and b"at most 7680 corner and 16777216 surf points" in msg, msg
    for kw in (dict(c=None), dict(s=None), dict(p=None), dict(o=None)):
        st, msg = call(opts(), **kw)
        assert st == vl.ERR_INVALID and b"null buffer with a positive count" in msg, (kw, msg)
    # host form only: the values
    for k, name in ((0, b"corner cloud, point 2: component 3"), (1, b"surf cloud, point 2: component 3")):
        for v in (np.nan, np.inf):
            clouds = [corner.copy(), surf.copy()]
            clouds[k][2, 3] = v
            st, msg = call(opts(), c=clouds[0], s=clouds[1], forms=(0,))
            assert st == vl.ERR_INVALID and name in msg and b"not finite" in msg, msg
            st, msg = call(opts(), c=clouds[0], s=clouds[1], forms=(1,))
            assert b"null handle" in msg, "the device form trusts its caller: %s" % msg
    for col, name in ((1, b"q[1]"), (6, b"t[2]")):
        bad = poses.copy()
        bad[1, col] = np.nan
        st, msg = call(opts(), p=bad, forms=(0,))
        assert st == vl.ERR_INVALID and b"pose 1: component " + name + b" is not finite" in msg, msg
    for w in (1.0 + 2e-6, 1.0 - 2e-6, 0.0):
        bad = poses.copy()
        bad[2, 3] = w
        st, msg = call(opts(), p=bad, forms=(0,))
        assert st == vl.ERR_INVALID and b"pose 2: the quaternion's norm" in msg and b"within 1e-6 of 1" in msg, msg
    near = poses.copy()
    near[2, 3] = 1.0 + 5e-7
    assert b"null handle" in call(opts(), p=near, forms=(0,))[1]
    # the order of the checks: the first offence listed is the one reported
    worst = dict(nc=-1, M=-1, c=None)
    for o, word in ((opts(size=0, reserved=1, stride=(0, 0), radius=(-1, -1)), b"struct_size"), (opts(reserved=1, stride=(0, 0), radius=(-1, -1)), b"reserved"),
                    (opts(stride=(0, 0), radius=(-1, -1)), b"stride[0]"), (opts(radius=(-1, -1)), b"radius[0]"), (opts(), b"negative cloud size")):
        assert word in call(o, **worst)[1], word
    assert b"M must be" in call(opts(), M=-1, c=None)[1]
    assert b"at most 7680" in call(opts(), nc=7681, c=None)[1]


def test_every_relocalize_refusal_with_a_null_handle(vl):
    L = vl.lib()
    corner, surf = np.ones((4, 4), F32), np.ones((6, 4), F32)
    q, t = np.array([0, 0, 0, 1.0]), np.zeros(3)
    out = np.zeros(1, vl.RELOCALIZE_RESULT_DTYPE)

    def call(c=corner, s=surf, qq=q, tt=t, o=out, null_options=False, **fields):
        opt = vl.RelocalizeOptions()
        L.vloam_default_relocalize_options(C.byref(opt))
        for k, v in fields.items():
            if k in ("n_xy", "reserved", "half_extent"):
                getattr(opt, k)[:] = v
            elif k in ("stride", "radius"):
                getattr(opt.score, k)[:] = v
            elif k.startswith("score_"):
                setattr(opt.score, k[6:], v)
            else:
                setattr(opt, k, v)
        st = L.vloam_map_relocalize(None, None if null_options else C.byref(opt), P(c), 4, P(s), 6, P(qq), P(tt), P(o))
        msg = L.vloam_last_error()
        assert st == vl.ERR_INVALID and msg.startswith(b"vloam_map_relocalize:"), (st, msg)
        return msg

    assert b"null handle" in call()
    assert b"null handle" in call(n_xy=[256, 256], n_z=1, n_yaw=1, top_k=8, half_extent=[0.0, 0.0, 0.0], half_yaw=np.pi)
    assert b"null options" in call(null_options=True)
    assert b"struct_size must be 88" in call(struct_size=80)
    assert b"reserved must be 0" in call(reserved=[0, 1])
    for kw in (dict(n_xy=[0, 9]), dict(n_xy=[9, -1]), dict(n_z=0), dict(n_yaw=0)):
        assert b"every step count is 1 .. 65536" in call(**kw), kw
    assert b"more than 65536 candidates" in call(n_xy=[257, 256], n_z=1, n_yaw=1)
    assert b"more than 65536 candidates" in call(n_xy=[65536, 65536], n_z=65536, n_yaw=65536)
    for k in (0, 9, -1):
        assert b"top_k must be 1 .. 8" in call(top_k=k)
    for e in ([-1.0, 0, 0], [0, np.nan, 0], [0, 0, np.inf]):
        assert b"half_extent" in call(half_extent=e)
    for a in (-0.1, 3.2, np.nan):
        assert b"half_yaw must be 0 .. pi" in call(half_yaw=a)
    assert b"corner AND surf" in call(c=None) and b"corner AND surf" in call(s=None)
    assert b"the centre is q AND t" in call(qq=None) and b"the centre is q AND t" in call(tt=None)
    assert b"null result" in call(o=None)
    # the score options and the values travel through the score's own check
    assert b"vloam_score_options: struct_size must be 24" in call(score_struct_size=20)
    assert b"stride[1] must be at least 1" in call(stride=[1, 0])
    assert b"radius[0] must be positive and finite" in call(radius=[0.0, 1.0])
    bad = surf.copy()
    bad[5, 0] = np.inf
    assert b"surf cloud, point 5: component 0 is not finite" in call(s=bad)
    assert b"the quaternion's norm" in call(qq=np.array([0, 0, 0, 1.1]))
    assert b"component t[1] is not finite" in call(tt=np.array([0, np.nan, 0]))


def test_model_against_a_hand_computed_case():
    """Ten points, two poses, every d2 an exact binary fraction: worked out by hand (the comments), not by the model.  It checks the model
    alone, so it passes with or without the library's new entry points; the other tests of this file need them."""
    maps = (np.array([[0, 0, 0, 1], [1, 0, 0, 2], [0, 2, 0, 3]], F32), np.array([[10, 10, 10, 4]], F32))
    corner = np.array([[0, 0, 0, 0], [0.5, 0, 0, 0], [1, 0, 1, 0], [0, 1, 0, 0], [3, 0, 0, 0], [0, 2, 0.5, 0]], F32)
    surf = np.array([[10, 10, 10, 0], [10, 10, 10.5, 0], [9, 9, 9, 0], [np.inf, 0, 0, 0]], F32)
    # pose 0 the identity; pose 1 half a turn about z, then + (1, 0, 0): (x, y, z) -> (1 - x, -y, z), exact in f64
    poses = np.array([[0, 0, 0, 1, 0, 0, 0], [0, 0, 1, 0, 1, 0, 0]], np.float64)
    assert np.array_equal(model.associate(corner, poses[1, :4], poses[1, 4:]), np.array([[1, 0, 0], [0.5, 0, 0], [0, 0, 1], [1, -1, 0], [-2, 0, 0], [1, -2, 0.5]], F32))
    r = model.score_poses(maps, corner, surf, poses, radius=(1.0, 0.5))
    # pose 0, corner: dmin 0, 1/4, 1, 1, 4, 1/4 -> five within 1 (1 <= 1 counts), sum 2.5; surf: 0, 1/4 (= r*r, a hit), 3, not searched -> two, sum 1/4
    assert r["n_used"].tolist() == [[6, 4], [6, 4]]
    assert r["n_hit"][0].tolist() == [5, 2] and r["sum_d2_q24"][0].tolist() == [int(2.5 * 2 ** 24), 2 ** 22]
    # pose 1, corner: dmin 0, 1/4, 1, 1, 4, 4.25 -> four, sum 2.25; surf: everything is more than 19 m away
    assert r["n_hit"][1].tolist() == [4, 0] and r["sum_d2_q24"][1].tolist() == [int(2.25 * 2 ** 24), 0]
    # every other corner point (0, 2, 4): dmin 0, 1, 4 under pose 0; a radius one ulp below 1/2 drops the surf point at exactly 1/4
    r = model.score_poses(maps, corner, surf, poses, stride=(2, 1), radius=(1.0, float(np.nextafter(F32(0.5), F32(0)))))
    assert r["n_used"][0].tolist() == [3, 4] and r["n_hit"][0].tolist() == [2, 1] and r["sum_d2_q24"][0].tolist() == [2 ** 24, 0]
    # truncation: dmin = 3 * 2^-26 scales to 0.75 and counts as a hit with nothing added
    tiny = np.array([[np.sqrt(3.0) * 2.0 ** -13, 0, 0, 0]], F32)
    d = model.point_dmin(maps[0], tiny[:, :3])
    assert 0 < d[0] < 2.0 ** -24
    r = model.score_poses(maps, tiny, None, poses[:1])
    assert r["n_hit"].tolist() == [[1, 0]] and r["sum_d2_q24"].tolist() == [[0, 0]] and r["n_used"].tolist() == [[1, 0]]
    # ranking: hits first, then the smaller sum, then the index
    s = np.zeros(5, model.SCORE_DTYPE)
    s["n_hit"] = [[1, 1], [3, 0], [0, 3], [2, 0], [0, 0]]
    s["sum_d2_q24"] = [[5, 5], [9, 0], [0, 9], [1, 0], [0, 0]]
    assert model.rank(s).tolist() == [1, 2, 3, 0, 4]   # 3 hits twice at equal sums: the index; 2 hits twice: sum 1 before sum 10
    assert model.before(s[1], 1, s[2], 2) and not model.before(s[2], 2, s[1], 1) and model.before(s[3], 3, s[0], 0)
    # the grid: corners and centre of a 3 x 3 x 1 x 3 grid
    q0, t0 = model.yaw_quat(0.3), np.array([1.0, 2.0, 3.0])
    g = dict(n_xy=(3, 3), n_z=1, n_yaw=3, half_extent=(2.0, 1.0, 5.0), half_yaw=0.2)
    q, t = model.grid_pose(0, q0, t0, **g)
    assert np.allclose(t, [-1.0, 1.0, 3.0], atol=0, rtol=0) and np.allclose(q, model.yaw_quat(0.1), atol=1e-15)
    q, t = model.grid_pose(13, q0, t0, **g)
    assert np.array_equal(t, t0) and np.allclose(q, q0, atol=1e-15)
    q, t = model.grid_pose(26, q0, t0, **g)
    assert np.array_equal(t, [3.0, 3.0, 3.0]) and np.allclose(q, model.yaw_quat(0.5), atol=1e-15)
