"""ctypes driver for the reference's own scan registration and cost functors (oracle/_ref/libref.so, oracle/ref_harness.cpp), laser
odometry and mapping (libref_loam.so, ref_loam_harness.cpp), depth-enhanced visual odometry (libref_vo.so, ref_vo_harness.cpp) and the coupled
frame loop over vloam_tf.cpp and lidar_odometry_mapping.cpp (libref_vloam.so, ref_vloam_harness.cpp).

TEST INFRASTRUCTURE ONLY.  libref.so is the reference's scan_registration.cpp / lidarFactor.hpp / ceres_cost_function.h compiled
unmodified against the stand-in headers of oracle/ref_shim/.  It is built from a checkout of the reference and is never committed; on a
machine without the reference an already built oracle/_ref/ is used as it is.

Where the reference is looked for: the environment variable VLOAM_REFERENCE_DIR; when that is unset, REFERENCE_DIR_DEFAULT.  The default is
a DEPENDENCY ON A LOCATION OUTSIDE THIS REPOSITORY — the place the development container keeps its read-only checkout of the reference, the
same path oracle/orc_loam.cpp's line references name — kept only so that build() finds the reference there without configuration.  Nothing
else depends on it: set VLOAM_REFERENCE_DIR (or `make -C oracle ref REF_DIR=...`) anywhere else.  Mirrors orc.py's calls for the pieces it covers.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
REF_OUT = os.path.join(_DIR, "_ref")
REFERENCE_DIR_DEFAULT = "/root/reference"   # outside the repository: see the module docstring
VARIANTS = ("libref.so", "libref_cmath_only.so", "libref_loam.so")


def reference_dir():
    """The reference checkout to compile from, or None."""
    d = os.environ.get("VLOAM_REFERENCE_DIR") or REFERENCE_DIR_DEFAULT
    return d if os.path.isfile(os.path.join(d, "src", "lidar_odometry_mapping", "src", "scan_registration.cpp")) else None


def available():
    return reference_dir() is not None or all(os.path.exists(os.path.join(REF_OUT, v)) for v in VARIANTS)


SKIP_REASON = ("neither a checkout of the reference (VLOAM_REFERENCE_DIR / %s) nor a built oracle/_ref/libref.so exists on this machine"
               % REFERENCE_DIR_DEFAULT)


def build():
    """make -C oracle ref when the reference exists (a failure raises: it is never a reason to skip); otherwise leave oracle/_ref/ alone.
    Returns the path of libref.so, or None when there is neither a reference nor a built library."""
    d = reference_dir()
    if d is not None:
        subprocess.check_call(["make", "-C", _DIR, "-s", "ref", "REF_DIR=" + d])
    so = os.path.join(REF_OUT, "libref.so")
    return so if os.path.exists(so) else None


_libs = {}
F, I, D, LD = C.c_float, C.c_int, C.c_double, C.c_longdouble


def lib(variant="libref.so"):
    if variant not in _libs:
        if build() is None:
            raise RuntimeError(SKIP_REASON)
        L = C.CDLL(os.path.join(REF_OUT, variant))
        L.ref_sr_create.restype = C.c_void_p
        L.ref_sr_create.argtypes = [I, D]
        L.ref_sr_destroy.argtypes = [C.c_void_p]
        L.ref_sr_run.argtypes = [C.c_void_p, C.c_void_p, I, I]
        L.ref_sr_get_cloud.argtypes = [C.c_void_p, I, C.c_void_p, I]
        L.ref_eval_factor.argtypes = [I] + [C.c_void_p] * 5
        L.ref_eval_factor_ld.argtypes = [I] + [C.c_void_p] * 5
        _libs[variant] = L
    return _libs[variant]


def math_overloads_are_float(variant="libref.so"):
    """What the compiler found for the unqualified atan(float) / sqrt(float) of scan_registration.cpp:192 in this build."""
    return bool(lib(variant).ref_math_overloads_are_float())


class ScanRegistration:
    """One vloam::ScanRegistration object (init once; reset / input / output per sweep).  voxel_stable: VoxelGrid's within-voxel order,
    False = std::sort as PCL calls it (what liborc_stdsort.so restates), True = input order (what liborc.so and the device compute)."""

    def __init__(self, scan_line=64, minimum_range=5.0, variant="libref.so", voxel_stable=False):
        self.L = lib(variant)
        self.voxel_stable = voxel_stable
        self.h = C.c_void_p(self.L.ref_sr_create(scan_line, minimum_range))

    def __del__(self):
        try:
            self.L.ref_sr_destroy(self.h)
        except Exception:
            pass

    def run(self, cloud, is_dense=False):
        """0, or -1 when no point survives the input filters (the reference itself would index an empty cloud)."""
        c = np.ascontiguousarray(cloud, dtype=np.float32)
        assert c.ndim == 2 and c.shape[1] == 4
        self.L.ref_set_voxel_stable_order(int(self.voxel_stable))
        return self.L.ref_sr_run(self.h, c.ctypes.data_as(C.c_void_p), c.shape[0], int(is_dense))

    def cloud(self, which):
        n = self.L.ref_sr_get_cloud(self.h, which, None, 0)
        buf = np.zeros((max(n, 1), 4), dtype=np.float32)
        self.L.ref_sr_get_cloud(self.h, which, buf.ctypes.data_as(C.c_void_p), n)
        return buf[:n]

    def clouds(self):
        return [self.cloud(w) for w in range(5)]


# factor types of ref_eval_factor: (name, residuals, size of parameter block 0, payload length)
FACTORS = {0: ("LidarEdgeFactor", 3, 4, 10), 1: ("LidarPlaneFactor", 1, 4, 13), 2: ("LidarPlaneNormFactor", 1, 4, 7),
           3: ("LidarDistanceFactor", 3, 4, 6), 4: ("CostFunctor33", 3, 3, 6), 5: ("CostFunctor32", 2, 3, 5), 6: ("CostFunctor23", 2, 3, 5),
           7: ("CostFunctor22", 1, 3, 4)}


def eval_factor(ftype, payload, p0, p1, long_double=False):
    """(residuals [nres], Jacobian [nres, n0 + 3] with respect to the RAW parameters) of one reference functor; long_double: evaluated
    with Jet<long double, N> and returned as np.longdouble."""
    L = lib()
    _, nres, n0, npay = FACTORS[ftype]
    d = np.ascontiguousarray(payload, dtype=np.float64)
    a = np.ascontiguousarray(p0, dtype=np.float64)
    b = np.ascontiguousarray(p1, dtype=np.float64)
    assert d.shape == (npay,) and a.shape == (n0,) and b.shape == (3,)
    dt = np.longdouble if long_double else np.float64
    r, J = np.zeros(3, dtype=dt), np.zeros((3, n0 + 3), dtype=dt)
    fn = L.ref_eval_factor_ld if long_double else L.ref_eval_factor
    n = fn(ftype, d.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p),
           J.ctypes.data_as(C.c_void_p))
    assert n == nres
    return r[:n].copy(), J.reshape(-1)[:n * (n0 + 3)].reshape(n, n0 + 3).copy()


# ---------------------------------------------------------------- laser odometry and mapping (oracle/_ref/libref_loam.so, ref_loam_harness.cpp)
LOAM_LIB = "libref_loam.so"
U32 = C.c_uint
_P = C.c_void_p


def loam_lib():
    if LOAM_LIB not in _libs:
        if build() is None or not os.path.exists(os.path.join(REF_OUT, LOAM_LIB)):
            raise RuntimeError(SKIP_REASON)
        L = C.CDLL(os.path.join(REF_OUT, LOAM_LIB))
        L.ref_loam_create.restype = _P
        L.ref_loam_create.argtypes = [I, D, D, D, I, I]
        L.ref_loam_destroy.argtypes = [_P]
        L.ref_loam_set_vo_prior.argtypes = [_P] * 5
        L.ref_loam_stage_sr.argtypes = [_P, _P, I]
        L.ref_loam_set_sr_cloud.argtypes = [_P, I, _P, I]
        L.ref_loam_set_map_cloud.argtypes = [_P, I, _P, I]
        L.ref_loam_stage_lo.argtypes = [_P]
        L.ref_loam_stage_map.argtypes = [_P, _P, _P]
        L.ref_loam_skip_frame.argtypes = [_P]
        L.ref_loam_get_cloud.argtypes = [_P, I, _P, I]
        L.ref_loam_get_map_cube_counts.argtypes = [_P, _P, I]
        L.ref_loam_get_lo_pose.argtypes = [_P, _P, _P]
        L.ref_loam_get_published_pose.argtypes = [_P, I, _P, _P]
        L.ref_loam_get_tf.argtypes = [_P, I, _P, _P]
        L.ref_loam_map_ran.argtypes = [_P]
        L.ref_loam_get_map_filter_log.argtypes = [_P, _P, I]
        L.ref_loam_num_solves.argtypes = [_P, I]
        L.ref_loam_get_solve.argtypes = [_P, I, I, _P, _P, _P]
        L.ref_loam_get_solve_blocks.argtypes = [_P, I, I, _P, _P, _P, _P]
        _libs[LOAM_LIB] = L
    return _libs[LOAM_LIB]


def _vp(a):
    return a.ctypes.data_as(_P)


class Loam:
    """The reference's ScanRegistration, LaserOdometry and LaserMapping objects chained as its façade chains them; mirrors orc.Oracle's
    stage calls.  Sessions may coexist: each keeps its own copies of what it published and observed (the stand-in parameter server is
    process-wide, but it is only read while a session is being created).  Not thread-safe."""
    ODOMETRY, MAPPING = 0, 1
    N_CUBES = 21 * 21 * 11

    def __init__(self, scan_line=64, minimum_range=5.0, line_res=0.4, plane_res=0.8, mapping_skip_frame=1, detach_vo_lo=True, voxel_stable=True):
        self.L = loam_lib()
        self.voxel_stable = voxel_stable
        self.h = _P(self.L.ref_loam_create(scan_line, minimum_range, float(np.float32(line_res)), float(np.float32(plane_res)), mapping_skip_frame, int(detach_vo_lo)))

    def __del__(self):
        try:
            self.L.ref_loam_destroy(self.h)
        except Exception:
            pass

    def set_vo_prior(self, q, t):
        """Stores velo_last_VOT_velo_curr; returns (q, t) as the reference will read them back out of the tf2 transform."""
        q = np.ascontiguousarray(q, dtype=np.float64)
        t = np.ascontiguousarray(t, dtype=np.float64)
        qb, tb = np.zeros(4), np.zeros(3)
        self.L.ref_loam_set_vo_prior(self.h, _vp(q), _vp(t), _vp(qb), _vp(tb))
        return qb, tb

    def stage_sr(self, cloud):
        c = np.ascontiguousarray(cloud, dtype=np.float32)
        self.L.ref_set_voxel_stable_order(int(self.voxel_stable))
        return self.L.ref_loam_stage_sr(self.h, _vp(c), c.shape[0])

    def set_sr_cloud(self, which, pts):
        c = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 4)
        assert self.L.ref_loam_set_sr_cloud(self.h, which, _vp(c), c.shape[0]) == 0

    def stage_lo(self):
        self.L.ref_set_voxel_stable_order(int(self.voxel_stable))
        return self.L.ref_loam_stage_lo(self.h)

    def stage_map(self, corner=None, surf=None, full=None, q=None, t=None):
        self.L.ref_set_voxel_stable_order(int(self.voxel_stable))
        for which, a in ((5, corner), (6, surf), (7, full)):
            if a is not None:
                c = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4)
                assert self.L.ref_loam_set_map_cloud(self.h, which, _vp(c), c.shape[0]) == 0
        qa = None if q is None else np.ascontiguousarray(q, dtype=np.float64)
        ta = None if t is None else np.ascontiguousarray(t, dtype=np.float64)
        return self.L.ref_loam_stage_map(self.h, None if qa is None else _vp(qa), None if ta is None else _vp(ta))

    def skip_frame(self):
        return bool(self.L.ref_loam_skip_frame(self.h))

    def cloud(self, which):
        """0-4 scan registration; 5 / 6 / 7 the hand-over of output(); 8 /laser_cloud_map; 9 /velodyne_cloud_registered (None before the first)."""
        n = self.L.ref_loam_get_cloud(self.h, which, None, 0)
        if n < 0:
            return None
        buf = np.zeros((max(n, 1), 4), dtype=np.float32)
        self.L.ref_loam_get_cloud(self.h, which, _vp(buf), n)
        return buf[:n]

    def map_cube_counts(self):
        """[2, 4851] points per cube of the last published map: row 0 corner, row 1 surface."""
        buf = np.zeros(2 * self.N_CUBES, dtype=np.uint32)
        n = self.L.ref_loam_get_map_cube_counts(self.h, _vp(buf), buf.shape[0])
        assert n == 2 * self.N_CUBES, n
        return buf.reshape(self.N_CUBES, 2).T.astype(np.int64)

    def lo_pose(self):
        q, t = np.zeros(4), np.zeros(3)
        self.L.ref_loam_get_lo_pose(self.h, _vp(q), _vp(t))
        return q, t

    def published_pose(self, topic):
        q, t = np.zeros(4), np.zeros(3)
        assert self.L.ref_loam_get_published_pose(self.h, topic, _vp(q), _vp(t)) == 0
        return q, t

    def tf(self, which):
        """0 base_prev_LOT_base_curr, 1 world_LOT_base_last, 2 world_MOT_base_last of VloamTF, rotation as tf2 returns it."""
        q, t = np.zeros(4), np.zeros(3)
        self.L.ref_loam_get_tf(self.h, which, _vp(q), _vp(t))
        return q, t

    def map_ran(self):
        return bool(self.L.ref_loam_map_ran(self.h))

    def map_filter_log(self):
        n = self.L.ref_loam_get_map_filter_log(self.h, None, 0)
        buf = np.zeros((max(n, 1), 2), dtype=np.int32)
        self.L.ref_loam_get_map_filter_log(self.h, _vp(buf), n)
        return buf[:n]

    def num_solves(self, stage):
        return self.L.ref_loam_num_solves(self.h, stage)

    def solve(self, stage, k):
        """One ceres::Solve of the last stage call: q_in / t_in / q_out / t_out, max_num_iterations, types [blocks] (0 LidarEdgeFactor,
        1 LidarPlaneFactor, 2 LidarPlaneNormFactor, 3 LidarDistanceFactor), nres [blocks], payload [blocks, 13] (the functor's members in
        declaration order), residuals0 (raw, at the initial point, in AddResidualBlock order)."""
        b, a = np.zeros(7), np.zeros(7)
        cnt = np.zeros(3, dtype=np.int32)
        assert self.L.ref_loam_get_solve(self.h, stage, k, _vp(b), _vp(a), _vp(cnt)) == 0
        nb, nr = int(cnt[0]), int(cnt[1])
        types, nres = np.zeros(max(nb, 1), dtype=np.int32), np.zeros(max(nb, 1), dtype=np.int32)
        payload, raw = np.zeros((max(nb, 1), 13)), np.zeros(max(nr, 1))
        assert self.L.ref_loam_get_solve_blocks(self.h, stage, k, _vp(types), _vp(nres), _vp(payload), _vp(raw)) == 0
        return dict(q_in=b[:4], t_in=b[4:], q_out=a[:4], t_out=a[4:], max_num_iterations=int(cnt[2]), types=types[:nb], nres=nres[:nb],
                    payload=payload[:nb], residuals0=raw[:nr])


# ---------------------------------------------------------------- visual odometry (oracle/_ref/libref_vo.so, ref_vo_harness.cpp)
VO_LIB = "libref_vo.so"


def vo_available():
    return reference_dir() is not None or os.path.exists(os.path.join(REF_OUT, VO_LIB))


def vo_lib():
    if VO_LIB not in _libs:
        if build() is None or not os.path.exists(os.path.join(REF_OUT, VO_LIB)):
            raise RuntimeError(SKIP_REASON)
        L = C.CDLL(os.path.join(REF_OUT, VO_LIB))
        L.ref_vo_create.restype = _P
        L.ref_vo_create.argtypes = [_P, _P, _P, I, I, I]
        L.ref_vo_destroy.argtypes = [_P]
        L.ref_vo_frame.argtypes = [_P, _P, I]
        L.ref_vo_count.argtypes = [_P]
        L.ref_vo_get_points2d.argtypes = [_P, I, _P, I]
        L.ref_vo_get_dnsp.argtypes = [_P, I, _P, I]
        L.ref_vo_get_buckets.argtypes = [_P, I, _P, _P, _P, _P, I, _P]
        L.ref_vo_query_depth.argtypes = [_P, I, _P, I, _P, _P]
        L.ref_vo_solve.argtypes = [_P, _P, I, _P, I, _P, _P, _P, I, _P, _P]
        L.ref_vo_get_result.argtypes = [_P, _P, _P, _P]
        L.ref_vo_get_match_rows.argtypes = [_P, _P, I]
        _libs[VO_LIB] = L
    return _libs[VO_LIB]


class VO:
    """The reference's VisualOdometry object with its two PointCloudUtil objects; mirrors orc.VOOracle.  which_map: 0 the current frame's
    depth map (point_cloud_utils[i]), 1 the previous frame's.  optical_flow_match chooses which match containers solveNlsAll reads."""
    N_BUCKETS = 249 * 75

    def __init__(self, cam_T_velo, rect0_T_cam, P_rect0, remove_outlier=100, reset_to_identity=True, optical_flow_match=False):
        self.L = vo_lib()
        a = np.ascontiguousarray(cam_T_velo, dtype=np.float32)
        b = np.ascontiguousarray(rect0_T_cam, dtype=np.float32)
        c = np.ascontiguousarray(P_rect0, dtype=np.float32)
        assert a.shape == (4, 4) and b.shape == (4, 4) and c.shape == (3, 4)
        self.optical_flow_match = bool(optical_flow_match)
        self.h = _P(self.L.ref_vo_create(_vp(a), _vp(b), _vp(c), int(remove_outlier), int(reset_to_identity), int(optical_flow_match)))

    def __del__(self):
        try:
            self.L.ref_vo_destroy(self.h)
        except Exception:
            pass

    def frame(self, cloud):
        """VisualOdometry::reset, then processPointCloud on the sweep [n, 4] (x, y, z, anything)."""
        c = np.ascontiguousarray(cloud, dtype=np.float32)
        assert c.ndim == 2 and c.shape[1] == 4
        self.L.ref_vo_frame(self.h, _vp(c), c.shape[0])

    def count(self):
        return self.L.ref_vo_count(self.h)

    def _rows3(self, fn, which_map):
        n = fn(self.h, which_map, None, 0)
        buf = np.zeros((max(n, 1), 3), dtype=np.float32)
        fn(self.h, which_map, _vp(buf), n)
        return buf[:n]

    def points2d(self, which_map=0):
        return self._rows3(self.L.ref_vo_get_points2d, which_map)

    def dnsp(self, which_map=0):
        return self._rows3(self.L.ref_vo_get_dnsp, which_map)

    def buckets(self, which_map=0):
        """(bucket_x, bucket_y, bucket_depth, bucket_count), each flattened index_x * new_height + index_y like orc.VOOracle.buckets."""
        nb = self.N_BUCKETS
        bx, by, bd = [np.zeros(nb, dtype=np.float32) for _ in range(3)]
        bc = np.zeros(nb, dtype=np.int32)
        dims = np.zeros(2, dtype=np.int32)
        n = self.L.ref_vo_get_buckets(self.h, which_map, _vp(bx), _vp(by), _vp(bd), _vp(bc), nb, _vp(dims))
        assert n == nb and tuple(dims) == (249, 75), (n, dims)
        return bx, by, bd, bc

    def query_depth(self, which_map, xy):
        """(queryDepth per pixel of xy [n, 2] f32, tie flags: the third and fourth smallest neighbour distance are equal)."""
        p = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        d, tie = np.zeros(p.shape[0], dtype=np.float32), np.zeros(p.shape[0], dtype=np.uint8)
        self.L.ref_vo_query_depth(self.h, which_map, _vp(p), p.shape[0], _vp(d), _vp(tie))
        return d, tie.astype(bool)

    def solve(self, kp_prev, kp_curr, query_idx=None, train_idx=None, status=None, prior_q=None, prior_t=None):
        """solveNlsAll.  ORB configuration: keypoints of both images [n, 2] f32 and (query_idx, train_idx); optical-flow configuration: the
        two point lists of equal length and status.  match_rows [n_match, 11]: kind (32 / 22; 0 skipped by the outlier gate; -1 no match:
        status != 1), depth0, obs[5], and the integer pixel pair the reference derived (prev x, y, curr x, y)."""
        a = np.ascontiguousarray(kp_prev, dtype=np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(kp_curr, dtype=np.float32).reshape(-1, 2)
        if self.optical_flow_match:
            st = np.ascontiguousarray(status, dtype=np.uint8)
            assert a.shape == b.shape and st.shape == (a.shape[0],)
            n, q, t = a.shape[0], None, None
        else:
            q = np.ascontiguousarray(query_idx, dtype=np.int32)
            t = np.ascontiguousarray(train_idx, dtype=np.int32)
            assert q.shape == t.shape and (q.size == 0 or (q.min() >= 0 and q.max() < a.shape[0] and t.min() >= 0 and t.max() < b.shape[0]))
            n, st = q.shape[0], None
        pq = None if prior_q is None else np.ascontiguousarray(prior_q, dtype=np.float64)
        pt = None if prior_t is None else np.ascontiguousarray(prior_t, dtype=np.float64)
        rc = self.L.ref_vo_solve(self.h, _vp(a), a.shape[0], _vp(b), b.shape[0], None if q is None else _vp(q), None if t is None else _vp(t),
                                 None if st is None else _vp(st), n, None if pq is None else _vp(pq), None if pt is None else _vp(pt))
        assert rc == 0, "ref_vo_solve: %d (the residual blocks could not be attributed to the matches)" % rc
        out, inn, cnt = np.zeros(6), np.zeros(6), np.zeros(2, dtype=np.int32)
        self.L.ref_vo_get_result(self.h, _vp(out), _vp(inn), _vp(cnt))
        rows = np.zeros((max(n, 1), 11))
        assert self.L.ref_vo_get_match_rows(self.h, _vp(rows), n) == n
        return dict(angles=out[:3], t=out[3:], angles_in=inn[:3], t_in=inn[3:], counter32=int(cnt[0]), counter22=int(cnt[1]), match_rows=rows[:n])


# ---------------------------------------------------------------- the coupled frame loop (oracle/_ref/libref_vloam.so, ref_vloam_harness.cpp)
VLOAM_LIB = "libref_vloam.so"
TF_NAMES = ("imu_T_velo", "imu_T_cam0", "base_T_imu", "base_T_cam0", "velo_T_cam0", "world_VOT_base_last", "base_last_VOT_base_curr",
            "cam0_curr_VOT_cam0_last", "velo_last_VOT_velo_curr", "cam0_init_VOT_cam0_last", "cam0_init_VOT_cam0_start", "cam0_start_VOT_cam0_last",
            "world_LOT_base_last", "cam0_init_LOT_cam0_last", "cam0_init_LOT_cam0_start", "cam0_start_LOT_cam0_last", "base_prev_LOT_base_curr",
            "cam0_curr_LOT_cam0_prev", "world_MOT_base_last", "cam0_init_MOT_cam0_last", "cam0_init_MOT_cam0_start", "cam0_start_MOT_cam0_last",
            "VO.cam0_curr_T_cam0_last")


def vloam_available():
    return reference_dir() is not None or os.path.exists(os.path.join(REF_OUT, VLOAM_LIB))


def vloam_lib():
    if VLOAM_LIB not in _libs:
        if build() is None or not os.path.exists(os.path.join(REF_OUT, VLOAM_LIB)):
            raise RuntimeError(SKIP_REASON)
        L = C.CDLL(os.path.join(REF_OUT, VLOAM_LIB))
        L.ref_vloam_create.restype = _P
        L.ref_vloam_create.argtypes = [_P, _P, _P, _P, _P, D, D, D]
        L.ref_vloam_destroy.argtypes = [_P]
        L.ref_vloam_frame.argtypes = [_P, _P, I, _P, _P, I]
        L.ref_vloam_count.argtypes = [_P]
        L.ref_vloam_get_tfs.argtypes = [_P, _P]
        L.ref_vloam_get_tf_rotation.argtypes = [_P, I, _P]
        L.ref_vloam_get_eigen_statics.argtypes = [_P, _P]
        L.ref_vloam_get_vo.argtypes = [_P, _P, _P, _P]
        L.ref_vloam_get_vo_rows.argtypes = [_P, _P, I]
        L.ref_vloam_get_cloud.argtypes = [_P, I, _P, I]
        L.ref_vloam_get_buckets.argtypes = [_P, _P, _P, _P, _P, I, _P]
        L.ref_vloam_skip_frame.argtypes = [_P]
        L.ref_vloam_map_ran.argtypes = [_P]
        L.ref_vloam_get_lo_pose.argtypes = [_P, _P, _P]
        L.ref_vloam_get_published_pose.argtypes = [_P, I, _P, _P]
        L.ref_vloam_num_solves.argtypes = [_P]
        L.ref_vloam_get_solve.argtypes = [_P, I, _P, _P, _P]
        L.ref_vloam_get_solve_blocks.argtypes = [_P, I, _P, _P, _P, _P]
        L.ref_vloam_get_rows_text.restype = C.c_long
        L.ref_vloam_get_rows_text.argtypes = [_P, I, _P, C.c_long]
        _libs[VLOAM_LIB] = L
    return _libs[VLOAM_LIB]


class Vloam:
    """The reference's VloamTF, VisualOdometry and LidarOdometryMapping objects wired and driven like vloam_main_node.cpp's init() and
    callback(); mirrors orc_vloam.VloamOracle.  statics: (imu_T_velo, imu_T_cam0, base_T_imu), each (q xyzw, t) as tf's lookups hand them
    out.  frame() returns 0 or the harness's status (ref_vloam_harness.cpp: -1 / -2 / -5 close the session before the reference would run
    into undefined behaviour; -5 after laserOdometryIO, so everything but the mapping can still be read)."""
    VO, ODOMETRY, MAPPING = 0, 1, 2

    def __init__(self, cam_T_velo, rect0_T_cam, P_rect0, statics, scan_line=64, minimum_range=5.0, line_res=0.4, plane_res=0.8, mapping_skip_frame=1,
                 detach_VO_LO=False, reset_VO_to_identity=False, remove_VO_outlier=100, save_traj=False, start_frame=0, end_frame=-1, voxel_stable=True):
        self.L = vloam_lib()
        self.voxel_stable = voxel_stable
        a = np.ascontiguousarray(cam_T_velo, dtype=np.float32)
        b = np.ascontiguousarray(rect0_T_cam, dtype=np.float32)
        c = np.ascontiguousarray(P_rect0, dtype=np.float32)
        st = np.ascontiguousarray(np.concatenate([np.concatenate([np.asarray(q, dtype=np.float64), np.asarray(t, dtype=np.float64)]) for q, t in statics]))
        assert a.shape == (4, 4) and b.shape == (4, 4) and c.shape == (3, 4) and st.shape == (21,)
        ints = np.array([scan_line, mapping_skip_frame, int(detach_VO_LO), int(reset_VO_to_identity), remove_VO_outlier, int(save_traj), start_frame, end_frame],
                        dtype=np.int32)
        self.h = _P(self.L.ref_vloam_create(_vp(a), _vp(b), _vp(c), _vp(st), _vp(ints), minimum_range, float(np.float32(line_res)), float(np.float32(plane_res))))

    def __del__(self):
        try:
            self.L.ref_vloam_destroy(self.h)
        except Exception:
            pass

    def frame(self, cloud, prev_uv=None, curr_uv=None):
        c = np.ascontiguousarray(cloud, dtype=np.float32)
        assert c.ndim == 2 and c.shape[1] == 4
        p = np.zeros((0, 2), np.int32) if prev_uv is None else np.ascontiguousarray(prev_uv, dtype=np.int32).reshape(-1, 2)
        q = np.zeros((0, 2), np.int32) if curr_uv is None else np.ascontiguousarray(curr_uv, dtype=np.int32).reshape(-1, 2)
        assert p.shape == q.shape
        self.L.ref_set_voxel_stable_order(int(self.voxel_stable))
        return self.L.ref_vloam_frame(self.h, _vp(c), c.shape[0], _vp(p), _vp(q), p.shape[0])

    def count(self):
        return self.L.ref_vloam_count(self.h)

    def tfs(self):
        """[23, 12]: the transforms TF_NAMES, each its basis row-major and its origin."""
        out = np.zeros((len(TF_NAMES), 12))
        assert self.L.ref_vloam_get_tfs(self.h, _vp(out)) == len(TF_NAMES)
        return out

    def tf_rotation(self, which):
        q = np.zeros(4)
        self.L.ref_vloam_get_tf_rotation(self.h, which, _vp(q))
        return q

    def eigen_statics(self):
        out = np.zeros((2, 4, 4), dtype=np.float32)
        self.L.ref_vloam_get_eigen_statics(self.h, _vp(out))
        return out

    def vo(self, n_match):
        """None when solveNlsAll did not run in the last frame (count 0); else x_in / x_out (angles, t), counters, match_rows [n_match, 11]."""
        a, b, cnt = np.zeros(6), np.zeros(6), np.zeros(2, dtype=np.int32)
        if not self.L.ref_vloam_get_vo(self.h, _vp(a), _vp(b), _vp(cnt)):
            return None
        rows = np.zeros((max(n_match, 1), 11))
        assert self.L.ref_vloam_get_vo_rows(self.h, _vp(rows), n_match) == n_match
        return dict(x_in=a, x_out=b, counter32=int(cnt[0]), counter22=int(cnt[1]), match_rows=rows[:n_match])

    def buckets(self):
        """(bucket_x, bucket_y, bucket_depth, bucket_count) of the current frame's depth map, flattened like VO.buckets."""
        nb = VO.N_BUCKETS
        bx, by, bd = [np.zeros(nb, dtype=np.float32) for _ in range(3)]
        bc = np.zeros(nb, dtype=np.int32)
        dims = np.zeros(2, dtype=np.int32)
        n = self.L.ref_vloam_get_buckets(self.h, _vp(bx), _vp(by), _vp(bd), _vp(bc), nb, _vp(dims))
        assert n == nb and tuple(dims) == (249, 75), (n, dims)
        return bx, by, bd, bc

    def cloud(self, which):
        n = self.L.ref_vloam_get_cloud(self.h, which, None, 0)
        if n < 0:
            return None
        buf = np.zeros((max(n, 1), 4), dtype=np.float32)
        self.L.ref_vloam_get_cloud(self.h, which, _vp(buf), n)
        return buf[:n]

    def skip_frame(self):
        return bool(self.L.ref_vloam_skip_frame(self.h))

    def map_ran(self):
        return bool(self.L.ref_vloam_map_ran(self.h))

    def lo_pose(self):
        q, t = np.zeros(4), np.zeros(3)
        self.L.ref_vloam_get_lo_pose(self.h, _vp(q), _vp(t))
        return q, t

    def published_pose(self, topic):
        q, t = np.zeros(4), np.zeros(3)
        return (q, t) if self.L.ref_vloam_get_published_pose(self.h, topic, _vp(q), _vp(t)) == 0 else None

    def solves(self):
        """Every ceres::Solve of the last frame in call order: stage (VO / ODOMETRY / MAPPING), x_in, x_out, max_num_iterations, types, nres,
        payload [blocks, 13], residuals0."""
        out = []
        for k in range(self.L.ref_vloam_num_solves(self.h)):
            b, a, info = np.zeros(7), np.zeros(7), np.zeros(5, dtype=np.int32)
            assert self.L.ref_vloam_get_solve(self.h, k, _vp(b), _vp(a), _vp(info)) == 0
            nb, nr, npar = int(info[1]), int(info[2]), int(info[4])
            types, nres = np.zeros(max(nb, 1), dtype=np.int32), np.zeros(max(nb, 1), dtype=np.int32)
            payload, raw = np.zeros((max(nb, 1), 13)), np.zeros(max(nr, 1))
            assert self.L.ref_vloam_get_solve_blocks(self.h, k, _vp(types), _vp(nres), _vp(payload), _vp(raw)) == 0
            out.append(dict(stage=int(info[0]), x_in=b[:npar].copy(), x_out=a[:npar].copy(), max_num_iterations=int(info[3]), types=types[:nb], nres=nres[:nb],
                            payload=payload[:nb], residuals0=raw[:nr]))
        return out

    def rows_text(self, which):
        """The bytes written so far by VO2Cam0StartFrame (0), LO2Cam0StartFrame (1), MO2Cam0StartFrame (2); None when save_traj is off."""
        n = self.L.ref_vloam_get_rows_text(self.h, which, None, 0)
        if n < 0:
            return None
        buf = C.create_string_buffer(max(n, 1))
        self.L.ref_vloam_get_rows_text(self.h, which, buf, n)
        return buf.raw[:n]
