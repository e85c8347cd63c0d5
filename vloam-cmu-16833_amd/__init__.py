"""vloam-cmu-16833_amd — MI355X-native (gfx950) per-scan LiDAR(-visual) odometry hot path of VLOAM.

Thin ctypes binding over ``libvloam_hip.so`` (hand-written HIP kernels + C ABI, see
``include/vloam_hip/c_api.h``) plus a Python mirror of the reference's pull-style class surface
(``ScanRegistration`` / ``LaserOdometry`` / ``LaserMapping`` / ``LidarOdometryMapping``;
reference: src/lidar_odometry_mapping/include/lidar_odometry_mapping/*.h) used by the tests and the bench.

There is no CPU path in this package: importing it requires the built shared library and creating a
handle requires a HIP device.  (The CPU oracle lives in ``oracle/`` and is test infrastructure only.)
"""
import os as _os
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # the stage streams of a handle must not share hardware queues — with each other or with the host's own streams (before the HIP runtime loads)
import ctypes as C
import os
import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
# VLOAM_HIP_LIB: another build of the SAME library (A/B runs of kernel variants, stamp builds); never a different implementation
LIB_PATH = os.environ.get("VLOAM_HIP_LIB") or os.path.join(_DIR, "libvloam_hip.so")

VLOAM_OK, ERR_INVALID, ERR_HIP, ERR_CAPACITY, ERR_EMPTY, ERR_NO_DEVICE, ERR_ORDER = 0, -1, -2, -3, -4, -5, -6

K_MAX_RINGS, K_SECTORS = 64, 6
K_MAX_SHARP, K_MAX_LESS_SHARP, K_MAX_FLAT = 768, 7680, 1536
K_MAX_LO_FACTORS = K_MAX_SHARP + K_MAX_FLAT
K_IMG_MAX_CORNERS = 1024   # image_util.cpp:23 maxCorners
K_LM_MAX_TRACE = 104
K_STACK_CAP_CORNER, K_STACK_CAP_SURF = 8192, 24576
K_MAP_FACTOR_CAP = K_STACK_CAP_CORNER + K_STACK_CAP_SURF


class VloamError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("vloam status %d: %s" % (status, msg))
        self.status = status


class Config(C.Structure):
    _fields_ = [("scan_line", C.c_int), ("minimum_range", C.c_double), ("mapping_skip_frame", C.c_int),
                ("mapping_line_resolution", C.c_float), ("mapping_plane_resolution", C.c_float), ("detach_VO_LO", C.c_int),
                ("reset_VO_to_identity", C.c_int), ("remove_VO_outlier", C.c_int), ("with_mapping", C.c_int),
                ("max_points", C.c_int), ("max_frames", C.c_int), ("map_capacity_log2", C.c_int), ("debug", C.c_int),
                ("timing", C.c_int), ("image_width", C.c_int), ("image_height", C.c_int), ("CLAHE", C.c_int),
                ("max_ring_points", C.c_int)]


class Limits(C.Structure):
    """vloam_limits: capacities that are not in vloam_config (c_api.h)."""
    _fields_ = [("struct_size", C.c_int), ("max_surf_stack_points", C.c_int), ("map_pub_number", C.c_int),
                ("max_published_map_points", C.c_int), ("publish_registered_cloud", C.c_int)]


class LimitsExt(C.Structure):
    """vloam_limits_ext: vloam_limits (which keeps its size) and, right behind it, the field that came later (c_api.h)."""
    _fields_ = [("limits", Limits), ("sweep_log", C.c_int)]


class MapOptions(C.Structure):
    """vloam_map_options: the growable voxel map (c_api.h; vloam_create_with_options)."""
    _fields_ = [("struct_size", C.c_int), ("grow", C.c_int), ("max_capacity_log2", C.c_int)]


class MapQueryOptions(C.Structure):
    """vloam_map_query_options (c_api.h; vloam_map_query / vloam_map_query_device)."""
    _fields_ = [("struct_size", C.c_int), ("kind", C.c_int), ("k", C.c_int), ("reserved", C.c_int), ("max_radius", C.c_float)]


class LocalizeOptions(C.Structure):
    """vloam_localize_options (c_api.h; vloam_map_localize / vloam_map_localize_device)."""
    _fields_ = [("struct_size", C.c_int), ("pose_frame", C.c_int), ("reserved", C.c_int * 2)]


# vloam_localize_result (c_api.h): 18 ints (the last one padding) then 18 doubles, 216 bytes
LOCALIZE_RESULT_DTYPE = np.dtype([
    ("flags", "<i4"), ("error_bits", "<i4"), ("center_cube", "<i4", (3,)), ("n_stack", "<i4", (2,)), ("n_map", "<i4", (2,)),
    ("n_factors", "<i4", (2, 2)), ("iterations", "<i4", (2,)), ("termination", "<i4", (2,)), ("pad", "<i4"),
    ("q_guess", "<f8", (4,)), ("t_guess", "<f8", (3,)), ("q_map", "<f8", (4,)), ("t_map", "<f8", (3,)),
    ("initial_cost", "<f8", (2,)), ("final_cost", "<f8", (2,))])
LOC_SOLVED, LOC_NOT_OPTIMIZED, LOC_WOULD_ROLL, LOC_DEGRADED = 1, 2, 4, 8


class ScoreOptions(C.Structure):
    """vloam_score_options (c_api.h; vloam_map_score_poses / vloam_map_score_poses_device)."""
    _fields_ = [("struct_size", C.c_int), ("stride", C.c_int * 2), ("reserved", C.c_int), ("radius", C.c_float * 2)]


class RelocalizeOptions(C.Structure):
    """vloam_relocalize_options (c_api.h; vloam_map_relocalize)."""
    _fields_ = [("struct_size", C.c_int), ("n_xy", C.c_int * 2), ("n_z", C.c_int), ("n_yaw", C.c_int), ("top_k", C.c_int), ("reserved", C.c_int * 2),
                ("half_extent", C.c_double * 3), ("half_yaw", C.c_double), ("score", ScoreOptions)]


# vloam_pose_score (c_api.h): 4 ints then 2 unsigned 64-bit sums, 32 bytes
POSE_SCORE_DTYPE = np.dtype([("n_hit", "<i4", (2,)), ("n_used", "<i4", (2,)), ("sum_d2_q24", "<u8", (2,))])
# vloam_relocalize_result (c_api.h): 12 ints, 8 scores, 8 localisation records, 8 scores, 2288 bytes
RELOCALIZE_RESULT_DTYPE = np.dtype([
    ("n_candidates", "<i4"), ("n_refined", "<i4"), ("best", "<i4"), ("pad", "<i4"), ("candidate", "<i4", (8,)),
    ("coarse", POSE_SCORE_DTYPE, (8,)), ("refined", LOCALIZE_RESULT_DTYPE, (8,)), ("fine", POSE_SCORE_DTYPE, (8,))])
assert C.sizeof(ScoreOptions) == 24 and C.sizeof(RelocalizeOptions) == 88 and POSE_SCORE_DTYPE.itemsize == 32 and RELOCALIZE_RESULT_DTYPE.itemsize == 2288
SCORE_MAX_POSES = 65536


def score_rank(scores):
    """The ranking of c_api.h over POSE_SCORE_DTYPE records: indices, best first (more hits, then the smaller sum, then the smaller index)."""
    s = np.asarray(scores)
    return np.lexsort((np.arange(s.shape[0]), s["sum_d2_q24"].sum(axis=1, dtype=np.uint64), -s["n_hit"].sum(axis=1, dtype=np.int64)))


class PlaceOptions(C.Structure):
    """vloam_place_options (c_api.h; vloam_place_enable)."""
    _fields_ = [("struct_size", C.c_int), ("n_ring", C.c_int), ("n_sector", C.c_int), ("capacity", C.c_int), ("min_range", C.c_float),
                ("max_range", C.c_float), ("z_min", C.c_float), ("z_step", C.c_float), ("reserved", C.c_int)]


class PlaceQueryOptions(C.Structure):
    """vloam_place_query_options (c_api.h; vloam_place_query*)."""
    _fields_ = [("struct_size", C.c_int), ("k", C.c_int), ("exclude_last", C.c_int), ("reserved", C.c_int)]


# vloam_place_match (c_api.h): 8 ints, 32 bytes
PLACE_MATCH_DTYPE = np.dtype([("row", "<i4"), ("tag", "<i4"), ("shift", "<i4"), ("dist", "<i4"), ("n_occupied_query", "<i4"), ("n_occupied_row", "<i4"),
                              ("pad", "<i4", (2,))])
assert C.sizeof(PlaceOptions) == 36 and C.sizeof(PlaceQueryOptions) == 16 and PLACE_MATCH_DTYPE.itemsize == 32
PLACE_MAX_K = 8


def place_yaw_pose(q_row, shift, n_sector):
    """The yaw convention of c_api.h: the query sensor's orientation q_row * Rz(-shift * 2 pi / n_sector) (xyzw) for a match with that shift."""
    a = -float(shift) * 2.0 * np.pi / float(n_sector)
    x, y, z, w = (float(v) for v in q_row)
    sz, cw = np.sin(a / 2.0), np.cos(a / 2.0)
    return np.array([x * cw + y * sz, y * cw - x * sz, z * cw + w * sz, w * cw - z * sz])


class MapImportOptions(C.Structure):
    """vloam_map_import_options (c_api.h; vloam_map_import / vloam_map_import_device)."""
    _fields_ = [("struct_size", C.c_int), ("reserved", C.c_int * 3), ("q_wmap_wodom", C.c_double * 4), ("t_wmap_wodom", C.c_double * 3)]


# vloam_map_import_result (c_api.h): 8 long long then 6 ints (the last one padding), 88 bytes
MAP_IMPORT_RESULT_DTYPE = np.dtype([
    ("n_in", "<i8", (2,)), ("n_voxels", "<i8", (2,)), ("n_outside_window", "<i8", (2,)), ("n_nonfinite", "<i8", (2,)),
    ("max_per_voxel", "<i4", (2,)), ("center_cube", "<i4", (3,)), ("pad", "<i4")])


class MapMergeOptions(C.Structure):
    """vloam_map_merge_options (c_api.h; vloam_map_merge / vloam_map_merge_device)."""
    _fields_ = [("struct_size", C.c_int), ("apply", C.c_int), ("reserved", C.c_int * 2), ("q_map_src", C.c_double * 4), ("t_map_src", C.c_double * 3)]


# vloam_map_merge_result (c_api.h): 14 long long then 2 ints, 120 bytes; the pairs are [corner, surf]
MAP_MERGE_RESULT_DTYPE = np.dtype([
    ("n_in", "<i8", (2,)), ("n_new_points", "<i8", (2,)), ("n_hit_points", "<i8", (2,)), ("n_skipped_raw", "<i8", (2,)),
    ("n_outside_window", "<i8", (2,)), ("n_nonfinite", "<i8", (2,)), ("n_new_voxels", "<i8", (2,)), ("max_per_voxel", "<i4", (2,))])


class CarveOptions(C.Structure):
    """vloam_carve_options (c_api.h; vloam_map_carve / vloam_map_carve_device)."""
    _fields_ = [("struct_size", C.c_int), ("kind_mask", C.c_int), ("rows", C.c_int), ("cols", C.c_int), ("elev_min_deg", C.c_float),
                ("elev_max_deg", C.c_float), ("min_range", C.c_float), ("max_range", C.c_float), ("range_res", C.c_float), ("margin", C.c_float),
                ("min_votes", C.c_int), ("apply", C.c_int)]


# vloam_carve_result (c_api.h): 13 long long, 104 bytes; the pairs are [corner map, surf map]
CARVE_RESULT_DTYPE = np.dtype([
    ("examined", "<i8", (2,)), ("in_view", "<i8", (2,)), ("seen_through", "<i8", (2,)), ("confirmed", "<i8", (2,)), ("removed", "<i8", (2,)),
    ("skipped_raw", "<i8", (2,)), ("n_removed_out", "<i8")])
CARVE_MAX_SWEEPS = 16


class MapArchiveOptions(C.Structure):
    """vloam_map_archive_options (c_api.h; vloam_map_archive_enable)."""
    _fields_ = [("struct_size", C.c_int), ("capacity_rows", C.c_longlong)]


# vloam_map_archive_row (c_api.h), 32 bytes: a point evicted by a roll of the window
MAP_ARCHIVE_ROW_DTYPE = np.dtype([
    ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("order", "<u4"), ("cube_i", "<i2"), ("cube_j", "<i2"), ("cube_k", "<i2"),
    ("flags", "<u2"), ("sweep", "<i4")])
MAP_ARCHIVE_KIND, MAP_ARCHIVE_TAIL = 1, 2   # bits of flags


# vloam_sweep_record (c_api.h): 32 ints then 8 doubles, 192 bytes
SWEEP_RECORD_DTYPE = np.dtype([
    ("frame", "<i4"), ("error_bits", "<i4"), ("flags", "<i4"), ("n_in", "<i4"), ("n_cloud", "<i4"), ("n_sharp", "<i4"), ("n_less_sharp", "<i4"),
    ("n_flat", "<i4"), ("n_less_flat", "<i4"), ("lo_corner_factors", "<i4", (2,)), ("lo_plane_factors", "<i4", (2,)), ("lo_iterations", "<i4", (2,)),
    ("lo_termination", "<i4", (2,)), ("n_corner_stack", "<i4"), ("n_surf_stack", "<i4"), ("n_map_corner", "<i4"), ("n_map_surf", "<i4"),
    ("map_corner_factors", "<i4", (2,)), ("map_surf_factors", "<i4", (2,)), ("map_iterations", "<i4", (2,)), ("map_termination", "<i4", (2,)),
    ("reserved", "<i4", (3,)), ("lo_initial_cost", "<f8", (2,)), ("lo_final_cost", "<f8", (2,)), ("map_initial_cost", "<f8", (2,)),
    ("map_final_cost", "<f8", (2,))])
SWEEP_EMPTY, SWEEP_RING_TOO_LONG, SWEEP_MAP_FULL, SWEEP_MAP_RAW_CAPACITY, SWEEP_STACK_FULL, SWEEP_DS_TIMEOUT, SWEEP_VO_DEGENERATE = 1, 2, 4, 8, 16, 32, 64
SWEEP_FLAG_FIRST, SWEEP_FLAG_MAP_SKIPPED, SWEEP_FLAG_MAP_NOT_OPTIMIZED, SWEEP_FLAG_LO_LESS_CORR_0, SWEEP_FLAG_LO_LESS_CORR_1, SWEEP_FLAG_SOLVE_DEGRADED = 1, 2, 4, 8, 16, 32


class PoseInfoOptions(C.Structure):
    """vloam_pose_info_options (c_api.h; vloam_pose_info_enable)."""
    _fields_ = [("struct_size", C.c_int), ("reserved", C.c_int), ("lo_min_eigenvalue", C.c_double), ("map_min_eigenvalue", C.c_double)]


# vloam_pose_info_record (c_api.h): 8 ints then 100 doubles, 832 bytes
POSE_INFO_DTYPE = np.dtype([
    ("frame", "<i4"), ("flags", "<i4"), ("lo_factors", "<i4", (2,)), ("map_factors", "<i4", (2,)), ("reserved", "<i4", (2,)),
    ("lo_x", "<f8", (7,)), ("lo_cost", "<f8"), ("lo_H", "<f8", (36,)), ("lo_eig", "<f8", (6,)),
    ("map_x", "<f8", (7,)), ("map_cost", "<f8"), ("map_H", "<f8", (36,)), ("map_eig", "<f8", (6,))])
POSE_INFO_LO_VALID, POSE_INFO_MAP_VALID, POSE_INFO_LO_DEGENERATE, POSE_INFO_MAP_DEGENERATE = 1, 2, 4, 8


class PoseCovOptions(C.Structure):
    """vloam_pose_cov_options (c_api.h; vloam_pose_cov_enable)."""
    _fields_ = [("struct_size", C.c_int), ("reserved", C.c_int), ("lo_min_eigenvalue", C.c_double), ("map_min_eigenvalue", C.c_double),
                ("vo_min_eigenvalue", C.c_double)]


# vloam_pose_cov_record (c_api.h): 8 ints then 282 doubles, 2288 bytes
POSE_COV_DTYPE = np.dtype([
    ("frame", "<i4"), ("flags", "<i4"), ("rank", "<i4", (3,)), ("vo_factors", "<i4", (2,)), ("reserved", "<i4"),
    ("sigma2", "<f8", (3,)), ("reserved_d", "<f8"),
    ("lo_eig", "<f8", (6,)), ("lo_V", "<f8", (36,)), ("lo_cov", "<f8", (36,)),
    ("map_eig", "<f8", (6,)), ("map_V", "<f8", (36,)), ("map_cov", "<f8", (36,)),
    ("vo_x", "<f8", (6,)), ("vo_cost", "<f8"), ("vo_reserved", "<f8"), ("vo_H", "<f8", (36,)), ("vo_eig", "<f8", (6,)), ("vo_V", "<f8", (36,)),
    ("vo_cov", "<f8", (36,))])
POSE_COV_LO_VALID, POSE_COV_MAP_VALID, POSE_COV_VO_VALID, POSE_COV_LO_TRUNCATED, POSE_COV_MAP_TRUNCATED, POSE_COV_VO_TRUNCATED = 1, 2, 4, 8, 16, 32


class Calib(C.Structure):
    _fields_ = [("cam_T_velo", C.c_float * 16), ("rect0_T_cam", C.c_float * 16), ("P_rect0", C.c_float * 12)]


class LMRecord(C.Structure):
    _fields_ = [("x_in", C.c_double * 7), ("x_out", C.c_double * 7), ("H0", C.c_double * 36), ("g0", C.c_double * 6),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("n_iterations", C.c_double),
                ("termination", C.c_double), ("n_factors", C.c_double), ("n_evals", C.c_double),
                ("cyc", C.c_double * 4), ("trace", (C.c_double * 8) * K_LM_MAX_TRACE)]

    def to_dict(self):
        n = int(self.n_iterations)
        tr = np.ctypeslib.as_array(self.trace).reshape(K_LM_MAX_TRACE, 8)[:n].copy()
        return dict(x_in=np.array(self.x_in), x_out=np.array(self.x_out), H0=np.array(self.H0).reshape(6, 6),
                    g0=np.array(self.g0), initial_cost=self.initial_cost, final_cost=self.final_cost, trace=tr,
                    termination=int(self.termination), n_factors=int(self.n_factors), n_evals=int(self.n_evals),
                    cyc=np.array(self.cyc))


_lib = None


def lib():
    """Load libvloam_hip.so.  Raises (loudly) if it has not been built — there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libvloam_hip.so is not built (%s). Run __graft_entry__.build() or "
                              "`make -C vloam-cmu-16833_amd/csrc`. This package has no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.vloam_last_error.restype = C.c_char_p
        L.vloam_version.restype = C.c_char_p
        _lib = L
    return _lib


def default_config(**kw):
    c = Config()
    lib().vloam_default_config(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError("vloam_config has no field %r" % k)
        setattr(c, k, v)
    return c


def default_limits(**kw):
    lim = Limits()
    lib().vloam_default_limits(C.byref(lim))
    for k, v in kw.items():
        if not hasattr(lim, k):
            raise AttributeError("vloam_limits has no field %r" % k)
        setattr(lim, k, v)
    return lim


def default_limits_ext(sweep_log=0, **kw):
    ext = LimitsExt()
    lib().vloam_default_limits_ext(C.byref(ext))
    for k, v in kw.items():
        if not hasattr(ext.limits, k):
            raise AttributeError("vloam_limits has no field %r" % k)
        setattr(ext.limits, k, v)
    ext.sweep_log = int(sweep_log)
    return ext


def default_map_options(**kw):
    opt = MapOptions()
    lib().vloam_default_map_options(C.byref(opt))
    for k, v in kw.items():
        if not hasattr(opt, k):
            raise AttributeError("vloam_map_options has no field %r" % k)
        setattr(opt, k, v)
    return opt


def _fp(a):
    return a.ctypes.data_as(C.c_void_p)


# vloam_debug_probe (c_api.h): probe id -> (bytes per input element, bytes per output element)
PROBE_ATANF, PROBE_ATAN2F, PROBE_ELEV, PROBE_TF_ROUNDTRIP, PROBE_TF_GETROT, PROBE_TF_CHAIN, PROBE_ASSOC, PROBE_QUAT = 1, 2, 3, 4, 5, 6, 7, 8
PROBE_ELEMENT_BYTES = {PROBE_ATANF: (4, 4), PROBE_ATAN2F: (8, 4), PROBE_ELEV: (12, 4), PROBE_TF_ROUNDTRIP: (32, 104), PROBE_TF_GETROT: (72, 32),
                       PROBE_TF_CHAIN: (192, 96), PROBE_ASSOC: (72, 16), PROBE_QUAT: (88, 56)}
# the (P2, workgroup size) pairs of the sort probe: those the library's own kernels call block_bitonic_sort_u64 with (dev_probe.hip)
PROBE_SORT_PAIRS = tuple((p2, 256) for p2 in (256, 512, 1024, 2048, 4096)) + tuple((p2, 512) for p2 in (256, 512, 1024, 2048, 4096, 8192, 16384))


def probe_sort(p2, t):
    """VLOAM_PROBE_SORT(P2, T) of c_api.h."""
    return 0x40000000 | (int(t) << 16) | (int(p2) >> 4)


def debug_probe(which, data, device=0):
    """Test hook (vloam_debug_probe): the device primitive `which` on the elements of `data` (any array whose bytes are whole input elements in
    the probe's layout; for a sort probe, whole problems of P2 u64 keys).  Returns the raw output bytes as a uint8 array."""
    a = np.ascontiguousarray(data)
    in_b, out_b = PROBE_ELEMENT_BYTES.get(which, (8, 8))
    if a.nbytes % in_b:
        raise ValueError("%d bytes are no whole number of %d-byte elements" % (a.nbytes, in_b))
    n = a.nbytes // in_b
    out = np.zeros(max(n * out_b, 8), dtype=np.uint8)
    L = lib()
    st = L.vloam_debug_probe(C.c_int(device), C.c_int(which), _fp(a), C.c_longlong(n), _fp(out), C.c_longlong(n * out_b))
    if st != VLOAM_OK:
        raise VloamError(st, L.vloam_last_error().decode())
    return out[:n * out_b]


class Handle:
    """One sequence on one GPU (``vloam_handle``)."""

    def __init__(self, device=0, n_sessions=1, max_surf_stack_points=None, map_pub_number=None, max_published_map_points=None,
                 publish_registered_cloud=None, sweep_log=None, map_grow=None, map_max_capacity_log2=None, **cfg):
        """n_sessions > 1: a batched handle — that many independent sequences advanced in lock step by batch_process_scan*;
        select(b) chooses the session the getters read.  max_surf_stack_points: vloam_limits::max_surf_stack_points (None: the default,
        24576; multiples of 8192 up to 131072 add the large stack tier).  map_pub_number / max_published_map_points /
        publish_registered_cloud: the clouds of LaserMapping::publish as products of the mapping stream (vloam_limits; None: off),
        read with published_map() / published_cloud() / published_device_ptr().  sweep_log: vloam_limits_ext::sweep_log (None / 0: off): one
        diagnostics record per sweep, written by the stage streams, read with sweep_log().  map_grow / map_max_capacity_log2:
        vloam_map_options (None: no options struct is passed): a single-sequence handle whose voxel tables start at map_capacity_log2 and
        double whenever they could fill, up to the ceiling; health() then reports the growth steps and the tables' sizes."""
        self.L = lib()
        self.cfg = default_config(**cfg)
        lim = dict(max_surf_stack_points=max_surf_stack_points, map_pub_number=map_pub_number, max_published_map_points=max_published_map_points,
                   publish_registered_cloud=publish_registered_cloud)
        self.limits = default_limits(**{k: int(v) for k, v in lim.items() if v is not None})
        self.limits_ext = None
        if sweep_log is not None:   # the library is told by struct_size that sweep_log lies behind the limits
            self.limits_ext = LimitsExt(self.limits, int(sweep_log))
            self.limits_ext.limits.struct_size = C.sizeof(LimitsExt)
        self.surf_stack_cap = self.limits.max_surf_stack_points or K_STACK_CAP_SURF
        self.h = C.c_void_p()
        self.n_sessions = int(n_sessions)
        self.map_options = None
        if map_grow is not None or map_max_capacity_log2 is not None:
            self.map_options = default_map_options(grow=int(map_grow or 0), max_capacity_log2=int(map_max_capacity_log2 or 0))
            self._chk(self.L.vloam_create_with_options(C.byref(self.cfg), C.byref(self.limits_ext or self.limits), C.byref(self.map_options), int(device),
                                                       self.n_sessions, C.byref(self.h)))
        else:
            self._chk(self.L.vloam_create_with_limits(C.byref(self.cfg), C.byref(self.limits_ext or self.limits), int(device), self.n_sessions, C.byref(self.h)))

    def _chk(self, st):
        if st != VLOAM_OK:
            raise VloamError(st, self.L.vloam_last_error().decode())

    def close(self):
        if self.h:
            self.L.vloam_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- façade stages (LidarOdometryMapping::reset / scanRegistrationIO / laserOdometryIO / laserMappingIO)
    def reset_frame(self):
        self._chk(self.L.vloam_reset_frame(self.h))

    def scan_registration(self, cloud):
        cloud = np.ascontiguousarray(cloud, dtype=np.float32)
        assert cloud.ndim == 2 and cloud.shape[1] == 4
        self._chk(self.L.vloam_scan_registration(self.h, _fp(cloud), cloud.shape[0]))

    def scan_registration_device(self, dptr, n):
        self._chk(self.L.vloam_scan_registration_device(self.h, C.c_void_p(dptr), int(n)))

    def features(self, which):
        n = C.c_int(0)
        self._chk(self.L.vloam_get_features(self.h, which, None, 0, C.byref(n)))
        buf = np.zeros((max(n.value, 1), 4), dtype=np.float32)
        self._chk(self.L.vloam_get_features(self.h, which, _fp(buf), n.value, C.byref(n)))
        return buf[:n.value]

    def set_lo_prior(self, q, t):
        q = np.ascontiguousarray(q, dtype=np.float64)
        t = np.ascontiguousarray(t, dtype=np.float64)
        self._chk(self.L.vloam_set_lo_prior(self.h, _fp(q), _fp(t)))

    @staticmethod
    def _cloud_arg(c):
        if c is None:
            return None, None, 0
        a = np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 4)
        if a.shape[0] == 0:
            a = np.zeros((1, 4), np.float32)   # a non-null address for an empty substituted cloud
            return a, _fp(a), 0
        return a, _fp(a), a.shape[0]

    def set_odometry_input(self, laserCloud=None, cornerPointsSharp=None, cornerPointsLessSharp=None, surfPointsFlat=None, surfPointsLessFlat=None):
        """LaserOdometry::input with clouds that are not scan registration's (laser_odometry.cpp:135-146); None keeps the device's."""
        a = [self._cloud_arg(c) for c in (laserCloud, cornerPointsSharp, cornerPointsLessSharp, surfPointsFlat, surfPointsLessFlat)]
        self._chk(self.L.vloam_set_odometry_input(self.h, a[0][1], a[0][2], a[1][1], a[1][2], a[2][1], a[2][2], a[3][1], a[3][2], a[4][1], a[4][2]))

    def odometry_pose(self):
        q, t = np.zeros(4), np.zeros(3)
        self._chk(self.L.vloam_get_odometry_pose(self.h, _fp(q), _fp(t)))
        return q, t

    def set_mapping_input(self, laserCloudCornerLast=None, laserCloudSurfLast=None, laserCloudFullRes=None, q_wodom_curr=None, t_wodom_curr=None):
        """LaserMapping::input with clouds / an odometry pose that are not LaserOdometry::output's (laser_mapping.cpp:167-196)."""
        a = [self._cloud_arg(c) for c in (laserCloudCornerLast, laserCloudSurfLast, laserCloudFullRes)]
        q = None if q_wodom_curr is None else np.ascontiguousarray(q_wodom_curr, dtype=np.float64)
        t = None if t_wodom_curr is None else np.ascontiguousarray(t_wodom_curr, dtype=np.float64)
        self._chk(self.L.vloam_set_mapping_input(self.h, a[0][1], a[0][2], a[1][1], a[1][2], a[2][1], a[2][2], None if q is None else _fp(q),
                                                 None if t is None else _fp(t)))

    def laser_odometry(self):
        qw, tw, ql, tl = np.zeros(4), np.zeros(3), np.zeros(4), np.zeros(3)
        self._chk(self.L.vloam_laser_odometry(self.h, _fp(qw), _fp(tw), _fp(ql), _fp(tl)))
        return qw, tw, ql, tl

    def laser_mapping(self):
        q, t = np.zeros(4), np.zeros(3)
        self._chk(self.L.vloam_laser_mapping(self.h, _fp(q), _fp(t)))
        return q, t

    # ---- asynchronous whole-sweep path
    def process_scan(self, cloud):
        cloud = np.ascontiguousarray(cloud, dtype=np.float32)
        self._chk(self.L.vloam_process_scan(self.h, _fp(cloud), cloud.shape[0]))

    def process_scan_host_ptr(self, hptr, n):
        """vloam_process_scan on a raw HOST address (e.g. a pinned torch tensor's data_ptr()): n packed float4."""
        self._chk(self.L.vloam_process_scan(self.h, C.c_void_p(hptr), int(n)))

    def process_scan_device(self, dptr, n):
        self._chk(self.L.vloam_process_scan_device(self.h, C.c_void_p(dptr), int(n)))

    # ---- batched execution (n_sessions sequences per launch chain)
    def batch_process_scan(self, clouds):
        clouds = [np.ascontiguousarray(c, dtype=np.float32) for c in clouds]
        assert len(clouds) == self.n_sessions
        ptrs = (C.c_void_p * self.n_sessions)(*[c.ctypes.data for c in clouds])
        ns = (C.c_int * self.n_sessions)(*[c.shape[0] for c in clouds])
        self._chk(self.L.vloam_batch_process_scan(self.h, ptrs, ns))

    def batch_process_scan_device(self, dptrs, ns):
        assert len(dptrs) == self.n_sessions and len(ns) == self.n_sessions
        ptrs = (C.c_void_p * self.n_sessions)(*[int(p) for p in dptrs])
        nn = (C.c_int * self.n_sessions)(*[int(n) for n in ns])
        self._chk(self.L.vloam_batch_process_scan_device(self.h, ptrs, nn))

    def select(self, session):
        self._chk(self.L.vloam_select_session(self.h, int(session)))
        return self

    def sync(self):
        self._chk(self.L.vloam_sync(self.h))

    def checkpoint(self):
        """The sequence as bytes (vloam_checkpoint_save): drains and synchronises, leaves the handle as it was.  Single-sequence handles
        driven by scans only; for the same build of the library."""
        n = C.c_longlong(0)
        self._chk(self.L.vloam_checkpoint_size(self.h, C.byref(n)))
        buf = C.create_string_buffer(max(n.value, 1))
        self._chk(self.L.vloam_checkpoint_save(self.h, buf, C.c_longlong(n.value), C.byref(n)))
        return buf.raw[:n.value]

    def restore(self, data):
        """Resume the sequence of checkpoint() in this handle, which must be fresh (vloam_checkpoint_load); its capacities may differ from
        the saver's, its algorithmic parameters may not."""
        data = bytes(data)
        self._chk(self.L.vloam_checkpoint_load(self.h, data, C.c_longlong(len(data))))

    def frame_count(self):
        n = C.c_int(0)
        self._chk(self.L.vloam_frame_count(self.h, C.byref(n)))
        return n.value

    def trajectory(self, first=0, count=None):
        if count is None:
            count = self.frame_count() - first
        out = np.zeros((max(count, 1), 14))
        self._chk(self.L.vloam_get_trajectory(self.h, first, count, _fp(out)))
        return out[:count]

    def trajectory_device_ptr(self):
        p, b = C.c_void_p(), C.c_longlong(0)
        self._chk(self.L.vloam_trajectory_device_ptr(self.h, C.byref(p), C.byref(b)))
        return p.value, b.value

    def sweep_log(self, first=0, count=None):
        """vloam_get_sweep_log: the diagnostics rows of sweeps first .. first + count - 1 of the selected session as a structured array
        (SWEEP_RECORD_DTYPE).  Waits for the work behind the last row asked for only, not for the pipeline."""
        if count is None:
            count = self.frame_count() - first
        out = np.zeros(max(count, 1), dtype=SWEEP_RECORD_DTYPE)
        self._chk(self.L.vloam_get_sweep_log(self.h, int(first), int(count), _fp(out)))
        return out[:count]

    def sweep_log_device_ptr(self):
        p, b = C.c_void_p(), C.c_longlong(0)
        self._chk(self.L.vloam_sweep_log_device_ptr(self.h, C.byref(p), C.byref(b)))
        return p.value, b.value

    def enable_pose_info(self, lo_min_eigenvalue=0.0, map_min_eigenvalue=0.0):
        """vloam_pose_info_enable, on a fresh handle: from now on every sweep leaves a vloam_pose_info_record (information matrices of the last
        odometry / mapping round at the returned pose, eigenvalues, degeneracy flags against the two thresholds; 0 = never degenerate)."""
        opt = PoseInfoOptions()
        self.L.vloam_default_pose_info_options(C.byref(opt))
        opt.lo_min_eigenvalue, opt.map_min_eigenvalue = float(lo_min_eigenvalue), float(map_min_eigenvalue)
        self._chk(self.L.vloam_pose_info_enable(self.h, C.byref(opt)))

    def pose_info(self, first=0, count=None):
        """vloam_get_pose_info: the rows of sweeps first .. first + count - 1 of the selected session as a structured array (POSE_INFO_DTYPE).
        Waits for the work behind the last row asked for only, not for the pipeline."""
        if count is None:
            count = self.frame_count() - first
        out = np.zeros(max(count, 1), dtype=POSE_INFO_DTYPE)
        self._chk(self.L.vloam_get_pose_info(self.h, int(first), int(count), _fp(out)))
        return out[:count]

    def pose_info_device_ptr(self):
        p, b = C.c_void_p(), C.c_longlong(0)
        self._chk(self.L.vloam_pose_info_device_ptr(self.h, C.byref(p), C.byref(b)))
        return p.value, b.value

    def pose_cov_enable(self, lo_min_eigenvalue=0.0, map_min_eigenvalue=0.0, vo_min_eigenvalue=0.0):
        """vloam_pose_cov_enable, on a fresh handle right after enable_pose_info: from now on every sweep also leaves a vloam_pose_cov_record
        (eigenvectors, rank, sigma^2 and pseudo-inverse covariance of the odometry, mapping and VO problems; the thresholds are the eigenvalues
        below which a direction counts as unobserved, 0 = only lambda <= 1e-12 lambda_max)."""
        opt = PoseCovOptions()
        self.L.vloam_default_pose_cov_options(C.byref(opt))
        opt.lo_min_eigenvalue, opt.map_min_eigenvalue, opt.vo_min_eigenvalue = float(lo_min_eigenvalue), float(map_min_eigenvalue), float(vo_min_eigenvalue)
        self._chk(self.L.vloam_pose_cov_enable(self.h, C.byref(opt)))

    def get_pose_cov(self, first=0, count=None):
        """vloam_get_pose_cov: the rows of sweeps first .. first + count - 1 of the selected session as a structured array (POSE_COV_DTYPE).
        Waits for the work behind the last row asked for only, not for the pipeline."""
        if count is None:
            count = self.frame_count() - first
        out = np.zeros(max(count, 1), dtype=POSE_COV_DTYPE)
        self._chk(self.L.vloam_get_pose_cov(self.h, int(first), int(count), _fp(out)))
        return out[:count]

    def pose_cov_device_ptr(self):
        p, b = C.c_void_p(), C.c_longlong(0)
        self._chk(self.L.vloam_pose_cov_device_ptr(self.h, C.byref(p), C.byref(b)))
        return p.value, b.value

    def profile_kernel(self, name, max_launches=4096):
        """HIP-event pair around every launch of the kernel named `name` (its __global__ symbol) on the handle's stream."""
        self._chk(self.L.vloam_profile_kernel(self.h, name.encode(), int(max_launches)))

    def profile_read(self):
        ms, n = C.c_double(0), C.c_int(0)
        self._chk(self.L.vloam_profile_read(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_table(self):
        """{kernel symbol: (total ms, launches)} of the launches recorded since profile_kernel("*", n)."""
        self.L.vloam_profile_kernel_name.restype = C.c_char_p
        nk = self.L.vloam_profile_kernel_count()
        ms = np.zeros(nk)
        cnt = np.zeros(nk, dtype=np.int32)
        self._chk(self.L.vloam_profile_read_table(self.h, nk, _fp(ms), _fp(cnt)))
        return {self.L.vloam_profile_kernel_name(k).decode(): (float(ms[k]), int(cnt[k])) for k in range(1, nk) if cnt[k] > 0}

    def stage_ms(self):
        ms = np.zeros(4)
        n = C.c_int(0)
        self._chk(self.L.vloam_get_stage_ms(self.h, _fp(ms), C.byref(n)))
        return ms, n.value

    def counts(self):
        c = np.zeros(16, dtype=np.int64)
        self._chk(self.L.vloam_get_counts(self.h, _fp(c)))
        names = ["N_in", "N2", "n_sharp", "n_lessSharp", "n_flat", "n_lessFlat", "C", "S", "F_corner", "F_plane", "E_o", "n_c",
                 "n_s", "K_m", "E_m", "M"]
        return dict(zip(names, [int(v) for v in c]))

    def health(self):
        """vloam_get_health: cooperative solves that degraded to one workgroup, whether the handle switched to one-workgroup solves, table rebuilds;
        on a growable handle (map_grow=1) the growth steps enqueued so far and the log2 of the corner / surf table (0 on any other handle)."""
        v = np.zeros(8, dtype=np.int64)
        self._chk(self.L.vloam_get_health(self.h, _fp(v)))
        return dict(fallback_solves=int(v[0]), one_workgroup_solves=bool(v[1]), rebuilds=int(v[2]), map_growth_steps=int(v[3]),
                    map_log2=(int(v[4]), int(v[5])))

    # ---- VO
    def vo_set_calib(self, cam_T_velo, rect0_T_cam, P_rect0):
        c = Calib()
        c.cam_T_velo[:] = [float(v) for v in np.asarray(cam_T_velo, dtype=np.float32).ravel()]
        c.rect0_T_cam[:] = [float(v) for v in np.asarray(rect0_T_cam, dtype=np.float32).ravel()]
        c.P_rect0[:] = [float(v) for v in np.asarray(P_rect0, dtype=np.float32).ravel()]
        self._chk(self.L.vloam_vo_set_calib(self.h, C.byref(c)))

    def vo_process_point_cloud(self, cloud):
        cloud = np.ascontiguousarray(cloud, dtype=np.float32)
        self._chk(self.L.vloam_vo_process_point_cloud(self.h, _fp(cloud), cloud.shape[0]))

    def vo_solve(self, prev_uv, curr_uv, angle_axis, t):
        pu = np.ascontiguousarray(prev_uv, dtype=np.int32)
        cu = np.ascontiguousarray(curr_uv, dtype=np.int32)
        aa = np.array(angle_axis, dtype=np.float64)
        tt = np.array(t, dtype=np.float64)
        cnt = np.zeros(2, dtype=np.int32)
        self._chk(self.L.vloam_vo_solve(self.h, _fp(pu), _fp(cu), pu.shape[0], _fp(aa), _fp(tt), _fp(cnt)))
        return aa, tt, int(cnt[0]), int(cnt[1])

    # ---- coupled VLOAM frame loop (configs[3])
    def set_extrinsics(self, base_T_cam0, velo_T_cam0):
        a = np.ascontiguousarray(base_T_cam0, dtype=np.float64).reshape(16)
        b = np.ascontiguousarray(velo_T_cam0, dtype=np.float64).reshape(16)
        self._chk(self.L.vloam_set_extrinsics(self.h, _fp(a), _fp(b)))

    def _matches(self, prev_uv, curr_uv):
        if prev_uv is None or curr_uv is None:
            return None, None, None, None, 0
        pu = np.ascontiguousarray(prev_uv, dtype=np.int32)
        cu = np.ascontiguousarray(curr_uv, dtype=np.int32)
        return pu, cu, _fp(pu), _fp(cu), pu.shape[0]

    def process_frame(self, cloud, prev_uv=None, curr_uv=None):
        cloud = np.ascontiguousarray(cloud, dtype=np.float32)
        pu, cu, pp, cp, n = self._matches(prev_uv, curr_uv)
        self._chk(self.L.vloam_process_frame(self.h, _fp(cloud), cloud.shape[0], pp, cp, n))

    def process_frame_device(self, dptr, n_pts, prev_uv=None, curr_uv=None):
        pu, cu, pp, cp, n = self._matches(prev_uv, curr_uv)
        self._chk(self.L.vloam_process_frame_device(self.h, C.c_void_p(dptr), int(n_pts), pp, cp, n))

    def batch_process_frame_device(self, dptrs, ns, matches):
        """One coupled VLOAM frame for every session: matches[b] = (prev_uv, curr_uv) int32 [m, 2] (or (None, None))."""
        B = self.n_sessions
        assert len(dptrs) == B and len(ns) == B and len(matches) == B
        keep = [self._matches(m[0], m[1]) for m in matches]
        ptrs = (C.c_void_p * B)(*[int(p) for p in dptrs])
        nn = (C.c_int * B)(*[int(n) for n in ns])
        IP = C.POINTER(C.c_int)
        pp = (IP * B)(*[C.cast(k[2], IP) for k in keep])
        cp = (IP * B)(*[C.cast(k[3], IP) for k in keep])
        nm = (C.c_int * B)(*[int(k[4]) for k in keep])
        self._chk(self.L.vloam_batch_process_frame_device(self.h, ptrs, nn, pp, cp, nm))

    def batch_process_frame(self, clouds, matches):
        """Host-memory variant of batch_process_frame_device: clouds[b] float32 [n, 4]."""
        B = self.n_sessions
        assert len(clouds) == B and len(matches) == B
        cl = [np.ascontiguousarray(c, dtype=np.float32) for c in clouds]
        keep = [self._matches(m[0], m[1]) for m in matches]
        FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int)
        ptrs = (FP * B)(*[C.cast(_fp(c), FP) for c in cl])
        nn = (C.c_int * B)(*[int(c.shape[0]) for c in cl])
        pp = (IP * B)(*[C.cast(k[2], IP) for k in keep])
        cp = (IP * B)(*[C.cast(k[3], IP) for k in keep])
        nm = (C.c_int * B)(*[int(k[4]) for k in keep])
        self._chk(self.L.vloam_batch_process_frame(self.h, ptrs, nn, pp, cp, nm))

    def vo_trajectory(self, first=0, count=None):
        if count is None:
            count = self.frame_count() - first
        out = np.zeros((max(count, 1), 7))
        self._chk(self.L.vloam_get_vo_trajectory(self.h, first, count, _fp(out)))
        return out[:count]

    def vo_result(self):
        aa, t, cnt, pq, pt = np.zeros(3), np.zeros(3), np.zeros(2, dtype=np.int32), np.zeros(4), np.zeros(3)
        self._chk(self.L.vloam_get_vo_result(self.h, _fp(aa), _fp(t), _fp(cnt), _fp(pq), _fp(pt)))
        return dict(angles=aa, t=t, counter32=int(cnt[0]), counter22=int(cnt[1]), prior_q=pq, prior_t=pt)

    # ---- image front-end (optical-flow configuration; needs image_width / image_height in the config)
    def vo_process_image(self, gray):
        """VisualOdometry::processImage (visual_odometry.cpp:91-132, optical_flow_match = true): uint8 [h, w]."""
        g = np.ascontiguousarray(gray, dtype=np.uint8)
        self._chk(self.L.vloam_vo_process_image(self.h, _fp(g), g.shape[1], g.shape[0], g.shape[1]))

    def vo_process_image_device(self, dptr, width, height, stride=None):
        self._chk(self.L.vloam_vo_process_image_device(self.h, C.c_void_p(dptr), int(width), int(height), int(stride or width)))

    def vo_keypoints(self):
        n = C.c_int(0)
        out = np.zeros((K_IMG_MAX_CORNERS, 2), dtype=np.float32)
        self._chk(self.L.vloam_vo_get_keypoints(self.h, _fp(out), K_IMG_MAX_CORNERS, C.byref(n)))
        return out[:n.value]

    def vo_flow(self):
        """(corner in the previous image, tracked position in the new image, status) per corner of the last image."""
        n = C.c_int(0)
        a = np.zeros((K_IMG_MAX_CORNERS, 2), dtype=np.float32)
        b = np.zeros((K_IMG_MAX_CORNERS, 2), dtype=np.float32)
        st = np.zeros(K_IMG_MAX_CORNERS, dtype=np.uint8)
        self._chk(self.L.vloam_vo_get_flow(self.h, _fp(a), _fp(b), _fp(st), K_IMG_MAX_CORNERS, C.byref(n)))
        return a[:n.value], b[:n.value], st[:n.value]

    def vo_flow_matches(self):
        n = C.c_int(0)
        a = np.zeros((K_IMG_MAX_CORNERS, 2), dtype=np.int32)
        b = np.zeros((K_IMG_MAX_CORNERS, 2), dtype=np.int32)
        self._chk(self.L.vloam_vo_get_flow_matches(self.h, _fp(a), _fp(b), K_IMG_MAX_CORNERS, C.byref(n)))
        return a[:n.value], b[:n.value]

    def vo_set_orb_pattern(self, pattern):
        """ORB + brute-force configuration (optical_flow_match = false): OpenCV's bit_pattern_31_ as int8 [256, 4]; None = optical flow."""
        if pattern is None:
            self._chk(self.L.vloam_vo_set_orb_pattern(self.h, None))
            return
        p = np.ascontiguousarray(pattern, dtype=np.int8).reshape(256, 4)
        self._chk(self.L.vloam_vo_set_orb_pattern(self.h, _fp(p)))

    def vo_descriptors(self):
        """(keypoints [n, 2] f32 after ORB's border filter, descriptors [n, 32] u8) of the latest image."""
        n = C.c_int(0)
        self._chk(self.L.vloam_vo_get_descriptors(self.h, None, None, 0, C.byref(n)))
        xy = np.zeros((max(n.value, 1), 2), np.float32)
        d = np.zeros((max(n.value, 1), 32), np.uint8)
        self._chk(self.L.vloam_vo_get_descriptors(self.h, _fp(xy), _fp(d), n.value, C.byref(n)))
        return xy[:n.value], d[:n.value]

    def vo_match_descriptors(self, desc_prev, desc_curr, knn=True):
        """ImageUtil::matchDescriptors (BF, NORM_HAMMING): (queryIdx, trainIdx) int32 arrays in query order."""
        a = np.ascontiguousarray(desc_prev, dtype=np.uint8)
        b = np.ascontiguousarray(desc_curr, dtype=np.uint8)
        q = np.zeros(max(a.shape[0], 1), dtype=np.int32)
        t = np.zeros(max(a.shape[0], 1), dtype=np.int32)
        n = C.c_int(0)
        self._chk(self.L.vloam_vo_match_descriptors(self.h, _fp(a), a.shape[0], _fp(b), b.shape[0], a.shape[1] if a.ndim == 2 else 0, int(knn), _fp(q), _fp(t),
                                                    q.shape[0], C.byref(n)))
        return q[:n.value], t[:n.value]

    def process_frame_image(self, cloud, gray):
        """One frame of the coupled loop from raw inputs: sweep + grey image (matches come from the image front-end)."""
        cloud = np.ascontiguousarray(cloud, dtype=np.float32)
        g = np.ascontiguousarray(gray, dtype=np.uint8)
        self._chk(self.L.vloam_process_frame_image(self.h, _fp(cloud), cloud.shape[0], _fp(g), g.shape[1], g.shape[0], g.shape[1]))

    def batch_process_frame_image(self, clouds, grays):
        """One coupled frame of every session of a batched handle from raw inputs: clouds[b] float32 [n, 4], grays[b] uint8 [h, w] (one size)."""
        B = self.n_sessions
        assert len(clouds) == B and len(grays) == B
        cl = [np.ascontiguousarray(c, dtype=np.float32) for c in clouds]
        gs = [np.ascontiguousarray(g, dtype=np.uint8) for g in grays]
        assert all(g.shape == gs[0].shape for g in gs), "the images of one call share their size"
        FP, BP = C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
        ptrs = (FP * B)(*[C.cast(_fp(c), FP) for c in cl])
        nn = (C.c_int * B)(*[int(c.shape[0]) for c in cl])
        gp = (BP * B)(*[C.cast(_fp(g), BP) for g in gs])
        self._chk(self.L.vloam_batch_process_frame_image(self.h, ptrs, nn, gp, gs[0].shape[1], gs[0].shape[0], gs[0].shape[1]))

    def batch_process_frame_image_device(self, dptrs, n_pts, gptrs, width, height, stride=None):
        B = self.n_sessions
        assert len(dptrs) == B and len(n_pts) == B and len(gptrs) == B
        ptrs = (C.c_void_p * B)(*[C.c_void_p(int(p)) for p in dptrs])
        nn = (C.c_int * B)(*[int(v) for v in n_pts])
        gp = (C.c_void_p * B)(*[C.c_void_p(int(p)) for p in gptrs])
        self._chk(self.L.vloam_batch_process_frame_image_device(self.h, ptrs, nn, gp, int(width), int(height), int(stride or width)))

    def process_frame_image_device(self, dptr, n_pts, gptr, width, height, stride=None):
        self._chk(self.L.vloam_process_frame_image_device(self.h, C.c_void_p(dptr), int(n_pts), C.c_void_p(gptr), int(width), int(height),
                                                          int(stride or width)))

    def img_debug(self, width, height):
        """eig map f32 [h, w] and the pyramid of the last image: [(u8 [h_l, w_l], int16 [h_l, w_l, 2])]."""
        eig = self.debug_raw(4, 0, np.float32).reshape(height, width)
        lv = []
        w, h = width, height
        for l in range(3):
            try:
                im = self.debug_raw(4, 1 + l, np.uint8)
            except VloamError:
                break
            lv.append((im.reshape(h, w).copy(), self.debug_raw(4, 4 + l, np.int16).reshape(h, w, 2).copy()))
            w, h = (w + 1) // 2, (h + 1) // 2
        return eig, lv

    # ---- parity hooks
    def debug_raw(self, stage, item, dtype, max_bytes=1 << 26):
        n = C.c_longlong(0)
        self._chk(self.L.vloam_debug_get(self.h, stage, item, None, C.c_longlong(0), C.byref(n)))
        nb = min(n.value, max_bytes)
        buf = np.zeros(max(nb, 8), dtype=np.uint8)
        self._chk(self.L.vloam_debug_get(self.h, stage, item, _fp(buf), C.c_longlong(nb), C.byref(n)))
        return buf[:nb].view(dtype)

    def debug_lm_record(self, stage, item):
        raw = self.debug_raw(stage, item, np.uint8)
        rec = LMRecord.from_buffer_copy(raw.tobytes())
        return rec.to_dict()

    def sr_debug(self):
        sc = self.debug_raw(0, 9, np.float32)
        return dict(curvature=self.debug_raw(0, 0, np.float32), sort=self.debug_raw(0, 1, np.int32),
                    picked=self.debug_raw(0, 2, np.int32), label=self.debug_raw(0, 3, np.int32),
                    scanStartInd=self.debug_raw(0, 4, np.int32), scanEndInd=self.debug_raw(0, 5, np.int32),
                    sharpInd=self.debug_raw(0, 6, np.int32), lessSharpInd=self.debug_raw(0, 7, np.int32),
                    flatInd=self.debug_raw(0, 8, np.int32), startOri=sc[0], endOri=sc[1], istar=int(sc[2]),
                    n_after_s1=int(sc[3]), N2=int(sc[4]))

    def lo_debug(self, outer):
        c = self.debug_raw(1, outer * 16 + 0, np.int32).reshape(-1, 4)
        p = self.debug_raw(1, outer * 16 + 1, np.int32).reshape(-1, 4)
        rec = self.debug_lm_record(1, outer * 16 + 2)
        resid = self.debug_raw(1, outer * 16 + 3, np.float64).reshape(3, K_MAX_LO_FACTORS)
        return dict(corner=c[c[:, 0] >= 0][:, :3], plane=p[p[:, 0] >= 0], corner_slots=np.nonzero(c[:, 0] >= 0)[0],
                    plane_slots=np.nonzero(p[:, 0] >= 0)[0] + K_MAX_SHARP, rec=rec, resid=resid)


    def map_debug(self, outer):
        cap = K_STACK_CAP_CORNER + self.surf_stack_cap   # (== K_MAP_FACTOR_CAP on a default handle)
        types = self.debug_raw(2, outer * 16 + 0, np.int32)
        A = self.debug_raw(2, outer * 16 + 1, np.float64).reshape(3, cap).T
        B = self.debug_raw(2, outer * 16 + 2, np.float64).reshape(3, cap).T
        resid = self.debug_raw(2, outer * 16 + 4, np.float64).reshape(3, cap)
        rec = self.debug_lm_record(2, outer * 16 + 3)
        cs = np.nonzero(types[:K_STACK_CAP_CORNER] == 1)[0]
        ss = np.nonzero(types[K_STACK_CAP_CORNER:] == 3)[0]
        return dict(corner_idx=cs, corner_ab=np.hstack([A[cs], B[cs]]), surf_idx=ss,
                    surf_plane=np.hstack([A[ss + K_STACK_CAP_CORNER], B[ss + K_STACK_CAP_CORNER, :1]]), rec=rec, resid=resid,
                    corner_slots=cs, surf_slots=ss + K_STACK_CAP_CORNER)

    def vo_debug(self, n_match):
        nb = 249 * 75
        cur = [self.debug_raw(3, k, np.float32 if k < 3 else np.int32)[:nb] for k in range(4)]
        prev = [self.debug_raw(3, 4 + k, np.float32 if k < 3 else np.int32)[:nb] for k in range(4)]
        rows = self.debug_raw(3, 8, np.float64).reshape(-1, 7)[:n_match]
        return dict(cur=cur, prev=prev, match_rows=rows, rec=self.debug_lm_record(3, 9))

    def map_state(self):
        raw = self.debug_raw(2, 64, np.uint8)
        d = raw[:21 * 8].view(np.float64)
        i = raw[21 * 8:21 * 8 + 13 * 4].view(np.int32)
        return dict(parameters=d[:7].copy(), q_wmap_wodom=d[7:11].copy(), t_wmap_wodom=d[11:14].copy(), cen=i[0:3].copy(),
                    centerCube=i[3:6].copy(), n_corner_stack=int(i[6]), n_surf_stack=int(i[7]), do_optimize=int(i[8]),
                    n_map_corner=int(i[9]), n_map_surf=int(i[10]), deferred=int(i[11]))

    def get_map(self):
        """/laser_cloud_map (laser_mapping.cpp:778-793) as float32 [n, 4]: per cube the corner cloud then the surf cloud."""
        n = C.c_longlong(0)
        self._chk(self.L.vloam_get_map(self.h, None, C.c_longlong(0), C.byref(n)))
        buf = np.zeros((max(n.value, 1), 4), dtype=np.float32)
        self._chk(self.L.vloam_get_map(self.h, _fp(buf), C.c_longlong(n.value), C.byref(n)))
        return buf[:n.value]

    def get_map_kind(self, kind):
        """The corner (kind 0) or surf (kind 1) half of get_map(), same order within the half (vloam_get_map_kind)."""
        n = C.c_longlong(0)
        self._chk(self.L.vloam_get_map_kind(self.h, int(kind), None, C.c_longlong(0), C.byref(n)))
        buf = np.zeros((max(n.value, 1), 4), dtype=np.float32)
        self._chk(self.L.vloam_get_map_kind(self.h, int(kind), _fp(buf), C.c_longlong(n.value), C.byref(n)))
        return buf[:n.value]

    def _query_options(self, k, max_radius, kind):
        opt = MapQueryOptions()
        self.L.vloam_default_map_query_options(C.byref(opt))
        opt.kind, opt.k, opt.max_radius = int(kind), int(k), float(max_radius)
        return opt

    def map_query(self, points, k=5, max_radius=1.0, kind=2):
        """vloam_map_query: the k nearest map points within max_radius of every row of points (float32 [n, 3] or [n, 4], map frame) in the
        corner map (kind 0), the surf map (1) or both (2), of the selected session: (xyzi [n, k, 4], d2 [n, k] ascending, count [n]); entries
        beyond count are zero.  Runs behind everything handed over so far and waits for the mapping stream only."""
        p = np.asarray(points, dtype=np.float32)
        q = np.zeros((p.shape[0], 4), dtype=np.float32)
        q[:, :3] = p[:, :3]
        n, k = q.shape[0], int(k)
        xyzi = np.zeros((max(n, 1), max(k, 1), 4), dtype=np.float32)
        d2 = np.zeros((max(n, 1), max(k, 1)), dtype=np.float32)
        cnt = np.zeros(max(n, 1), dtype=np.int32)
        opt = self._query_options(k, max_radius, kind)
        self._chk(self.L.vloam_map_query(self.h, C.byref(opt), _fp(q), n, _fp(xyzi), _fp(d2), _fp(cnt)))
        return xyzi[:n], d2[:n], cnt[:n]

    def map_query_device(self, d_points, n, d_xyzi, d_d2, d_count, k=5, max_radius=1.0, kind=2):
        """vloam_map_query_device: the same with device addresses (n packed float4 in; [n][k] float4, [n][k] float32 and [n] int32 out).  Enqueues
        and returns: the results are complete after sync(), and the buffers must stay valid until then."""
        opt = self._query_options(k, max_radius, kind)
        self._chk(self.L.vloam_map_query_device(self.h, C.byref(opt), C.c_void_p(d_points), int(n), C.c_void_p(d_xyzi), C.c_void_p(d_d2), C.c_void_p(d_count)))

    def _localize_args(self, q, t, pose_frame):
        opt = LocalizeOptions()
        self.L.vloam_default_localize_options(C.byref(opt))
        opt.pose_frame = int(pose_frame)
        q = None if q is None else np.ascontiguousarray(q, dtype=np.float64)
        t = None if t is None else np.ascontiguousarray(t, dtype=np.float64)
        return opt, q, t

    def map_localize(self, corner=None, surf=None, q=None, t=None, pose_frame=0):
        """vloam_map_localize: a dry run of the mapping stage against the map as it is — where would this sweep be registered?  corner / surf:
        float32 [n, 4] (x, y, z, intensity) in the sensor frame, what set_mapping_input takes; (q, t): an odometry-frame pose (pose_frame 0)
        or the guess itself in the map frame (1).  corner = surf = None: the sweep in progress (between laser_odometry and laser_mapping),
        with q = t = None under its own odometry pose.  Returns the fields of vloam_localize_result as a dict; nothing of the sequence
        changes.  Runs behind everything handed over so far and waits for the mapping stream only."""
        opt, q, t = self._localize_args(q, t, pose_frame)
        c, s = self._cloud_arg(corner), self._cloud_arg(surf)
        out = np.zeros(1, dtype=LOCALIZE_RESULT_DTYPE)
        self._chk(self.L.vloam_map_localize(self.h, C.byref(opt), c[1], c[2], s[1], s[2], None if q is None else _fp(q), None if t is None else _fp(t), _fp(out)))
        return {k: (out[0][k].copy() if out[0][k].ndim else out[0][k].item()) for k in LOCALIZE_RESULT_DTYPE.names if k != "pad"}

    def map_localize_device(self, corner, surf, q, t, result, pose_frame=0):
        """vloam_map_localize_device: the same with torch tensors on the device — corner / surf float32 [n, 4] (or both None), result a uint8
        tensor of LOCALIZE_RESULT_DTYPE.itemsize bytes.  Enqueues and returns: the record is complete after sync(), the tensors must stay
        alive until then."""
        opt, q, t = self._localize_args(q, t, pose_frame)
        assert result.is_cuda and result.is_contiguous() and result.numel() * result.element_size() >= LOCALIZE_RESULT_DTYPE.itemsize
        ptr = [None, None]
        n = [0, 0]
        for k, c in enumerate((corner, surf)):
            if c is not None:
                assert c.is_cuda and c.is_contiguous() and c.dtype.is_floating_point and c.element_size() == 4 and c.shape[-1] == 4
                ptr[k], n[k] = C.c_void_p(c.data_ptr() or result.data_ptr()), int(c.shape[0])   # (an empty tensor has no address: any non-null one will do)
        self._chk(self.L.vloam_map_localize_device(self.h, C.byref(opt), ptr[0], n[0], ptr[1], n[1], None if q is None else _fp(q),
                                                   None if t is None else _fp(t), C.c_void_p(result.data_ptr())))

    def _score_options(self, stride, radius):
        opt = ScoreOptions()
        self.L.vloam_default_score_options(C.byref(opt))
        opt.stride[:] = [int(v) for v in stride]
        opt.radius[:] = [float(v) for v in radius]
        return opt

    def map_score_poses(self, corner, surf, poses, stride=(1, 1), radius=(1.0, 1.0)):
        """vloam_map_score_poses: corner / surf (float32 [n, 4], sensor frame, what map_localize takes; None: empty) under every row of poses
        (float64 [M, 7]: q xyzw, t in the map frame) against the corner / surf map — per pose the points of each kind whose nearest map point
        lies within radius[kind] (every stride[kind]-th point is scored) and the quantised sum of their squared distances, as an array of
        POSE_SCORE_DTYPE [M].  Runs behind everything handed over so far and waits for the mapping stream only."""
        opt = self._score_options(stride, radius)
        c, s = self._cloud_arg(corner), self._cloud_arg(surf)
        p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        out = np.zeros(max(p.shape[0], 1), dtype=POSE_SCORE_DTYPE)
        self._chk(self.L.vloam_map_score_poses(self.h, C.byref(opt), c[1], c[2], s[1], s[2], _fp(p), int(p.shape[0]), _fp(out)))
        return out[:p.shape[0]]

    def map_score_poses_device(self, corner, surf, poses, out, stride=(1, 1), radius=(1.0, 1.0)):
        """vloam_map_score_poses_device: the same with torch tensors on the device — corner / surf float32 [n, 4] (or None), poses float64 [M, 7],
        out a uint8 tensor of M * POSE_SCORE_DTYPE.itemsize bytes.  Enqueues and returns: the records are complete after sync(), the tensors
        must stay alive until then."""
        opt = self._score_options(stride, radius)
        M = int(poses.shape[0])
        assert poses.is_cuda and poses.is_contiguous() and poses.element_size() == 8 and poses.dtype.is_floating_point and poses.shape[-1] == 7
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() >= M * POSE_SCORE_DTYPE.itemsize
        ptr, n = [None, None], [0, 0]
        for k, c in enumerate((corner, surf)):
            if c is not None and c.shape[0] > 0:
                assert c.is_cuda and c.is_contiguous() and c.dtype.is_floating_point and c.element_size() == 4 and c.shape[-1] == 4
                ptr[k], n[k] = C.c_void_p(c.data_ptr()), int(c.shape[0])
        self._chk(self.L.vloam_map_score_poses_device(self.h, C.byref(opt), ptr[0], n[0], ptr[1], n[1], C.c_void_p(poses.data_ptr()) if M else None, M,
                                                      C.c_void_p(out.data_ptr()) if M else None))

    def map_relocalize(self, corner, surf, q_center, t_center, n_xy=(9, 9), n_z=1, n_yaw=9, half_extent=(2.0, 2.0, 0.0), half_yaw=np.deg2rad(10.0),
                       top_k=4, stride=(1, 1), radius=(1.0, 1.0)):
        """vloam_map_relocalize: a grid of n_xy[0] x n_xy[1] x n_z x n_yaw candidate poses around (q_center, t_center) — t_center -+ half_extent
        along the map's axes, -+ half_yaw about its +z — scored against the map, the top_k refined by map_localize (pose_frame 1) and scored
        again.  Returns the fields of vloam_relocalize_result as a dict: candidate / coarse / fine arrays of n_refined entries, refined a list
        of map_localize dicts, best the index of the winner in them.  Nothing of the sequence changes."""
        opt = RelocalizeOptions()
        self.L.vloam_default_relocalize_options(C.byref(opt))
        opt.n_xy[:] = [int(v) for v in n_xy]
        opt.n_z, opt.n_yaw, opt.top_k, opt.half_yaw = int(n_z), int(n_yaw), int(top_k), float(half_yaw)
        opt.half_extent[:] = [float(v) for v in half_extent]
        opt.score = self._score_options(stride, radius)
        c, s = self._cloud_arg(corner), self._cloud_arg(surf)
        q, t = np.ascontiguousarray(q_center, dtype=np.float64), np.ascontiguousarray(t_center, dtype=np.float64)
        out = np.zeros(1, dtype=RELOCALIZE_RESULT_DTYPE)
        self._chk(self.L.vloam_map_relocalize(self.h, C.byref(opt), c[1], c[2], s[1], s[2], _fp(q), _fp(t), _fp(out)))
        r, k = out[0], int(out[0]["n_refined"])
        refined = [{f: (r["refined"][j][f].copy() if r["refined"][j][f].ndim else r["refined"][j][f].item()) for f in LOCALIZE_RESULT_DTYPE.names if f != "pad"}
                   for j in range(k)]
        return dict(n_candidates=int(r["n_candidates"]), n_refined=k, best=int(r["best"]), candidate=r["candidate"][:k].copy(), coarse=r["coarse"][:k].copy(),
                    refined=refined, fine=r["fine"][:k].copy())

    # ---- place recognition (vloam_place_*): sweep descriptors, a database of them on the device, one descriptor against every row and yaw shift
    def place_enable(self, n_ring=None, n_sector=None, capacity=None, min_range=None, max_range=None, z_min=None, z_step=None):
        """vloam_place_enable, once per handle: the descriptor's geometry (None: the defaults of vloam_default_place_options — 20 rings, 60
        sectors, 16384 rows, min_range 0 = the handle's minimum_range, 80 m, -3 m, 0.05 m).  Returns the options as used."""
        opt = PlaceOptions()
        self.L.vloam_default_place_options(C.byref(opt))
        for k, v in dict(n_ring=n_ring, n_sector=n_sector, capacity=capacity).items():
            if v is not None:
                setattr(opt, k, int(v))
        for k, v in dict(min_range=min_range, max_range=max_range, z_min=z_min, z_step=z_step).items():
            if v is not None:
                setattr(opt, k, float(v))
        self._chk(self.L.vloam_place_enable(self.h, C.byref(opt)))
        self.place_options = opt
        self.place_words = opt.n_sector * ((opt.n_ring + 3) // 4)
        return opt

    def _place_words(self):
        if not getattr(self, "place_words", 0):
            raise VloamError(ERR_ORDER, "vloam_place_enable has not been called on this handle")
        return self.place_words

    @staticmethod
    def _place_cloud(cloud):
        a = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 4)
        return a, (_fp(a) if a.shape[0] else None), int(a.shape[0])

    @staticmethod
    def _place_dev(cloud):
        n = int(cloud.shape[0])
        assert cloud.is_cuda and cloud.is_contiguous() and cloud.dtype.is_floating_point and cloud.element_size() == 4 and cloud.shape[-1] == 4
        return (C.c_void_p(cloud.data_ptr()) if n else None), n

    def _place_query_options(self, k, exclude_last):
        opt = PlaceQueryOptions()
        self.L.vloam_default_place_query_options(C.byref(opt))
        opt.k, opt.exclude_last = int(k), int(exclude_last)
        return opt

    def place_describe(self, cloud):
        """vloam_place_describe: (descriptor uint32 [S * W], (n_used, n_occupied)) of a cloud (float32 [n, 4], sensor frame); the database is untouched."""
        a, ptr, n = self._place_cloud(cloud)
        desc, info = np.zeros(self._place_words(), np.uint32), np.zeros(2, np.int32)
        self._chk(self.L.vloam_place_describe(self.h, ptr, n, _fp(desc), _fp(info)))
        return desc, (int(info[0]), int(info[1]))

    def place_describe_device(self, cloud, desc, info=None):
        """vloam_place_describe_device: torch tensors on the device — cloud float32 [n, 4], desc int32 [S * W], info int32 [2] or None.  Enqueues
        and returns: complete after sync()."""
        ptr, n = self._place_dev(cloud)
        assert desc.is_cuda and desc.is_contiguous() and desc.numel() * desc.element_size() >= 4 * self._place_words()
        assert info is None or (info.is_cuda and info.is_contiguous() and info.numel() * info.element_size() >= 8)
        self._chk(self.L.vloam_place_describe_device(self.h, ptr, n, C.c_void_p(desc.data_ptr()), None if info is None else C.c_void_p(info.data_ptr())))

    def place_add(self, cloud, tag):
        """vloam_place_add: describe and append with the caller's tag; returns the row's index.  A full database: VloamError(ERR_CAPACITY)."""
        a, ptr, n = self._place_cloud(cloud)
        row = C.c_int(-1)
        self._chk(self.L.vloam_place_add(self.h, ptr, n, int(tag), C.byref(row)))
        return row.value

    def place_add_device(self, cloud, tag):
        """vloam_place_add_device: the same with a torch tensor on the device; enqueues and returns the row's index."""
        ptr, n = self._place_dev(cloud)
        row = C.c_int(-1)
        self._chk(self.L.vloam_place_add_device(self.h, ptr, n, int(tag), C.byref(row)))
        return row.value

    def place_count(self):
        n = C.c_int(0)
        self._chk(self.L.vloam_place_count(self.h, C.byref(n)))
        return n.value

    def place_get(self, first=0, count=None):
        """vloam_place_get: rows first .. first + count - 1 (None: to the end) as (desc uint32 [count, S * W], tags int32 [count], info int32
        [count, 2]: n_used — -1 for loaded rows — and n_occupied)."""
        words = self._place_words()
        if count is None:
            count = self.place_count() - int(first)
        desc, tags, info = np.zeros((max(count, 1), words), np.uint32), np.zeros(max(count, 1), np.int32), np.zeros((max(count, 1), 2), np.int32)
        self._chk(self.L.vloam_place_get(self.h, int(first), int(count), _fp(desc), _fp(tags), _fp(info)))
        return desc[:max(count, 0)], tags[:max(count, 0)], info[:max(count, 0)]

    def place_load(self, desc, tags):
        """vloam_place_load: append rows made elsewhere (desc uint32 [count, S * W], pad bytes zero; tags int32 [count])."""
        d = np.ascontiguousarray(desc, dtype=np.uint32).reshape(-1, self._place_words())
        t = np.ascontiguousarray(tags, dtype=np.int32).reshape(-1)
        assert t.shape[0] == d.shape[0]
        self._chk(self.L.vloam_place_load(self.h, _fp(d) if d.shape[0] else None, _fp(t) if d.shape[0] else None, int(d.shape[0])))

    def place_query(self, cloud, k=1, exclude_last=0):
        """vloam_place_query: the k best rows for a cloud as PLACE_MATCH_DTYPE [k] (unused places row == -1): smallest distance over every yaw
        shift, ties to the smaller shift, then the smaller row; the youngest exclude_last rows are skipped."""
        opt = self._place_query_options(k, exclude_last)
        a, ptr, n = self._place_cloud(cloud)
        out = np.zeros(PLACE_MAX_K, dtype=PLACE_MATCH_DTYPE)
        self._chk(self.L.vloam_place_query(self.h, C.byref(opt), ptr, n, _fp(out)))
        return out[:int(k)]

    def place_query_device(self, cloud, out, k=1, exclude_last=0):
        """vloam_place_query_device: cloud float32 [n, 4] and out (k * 32 bytes) torch tensors on the device; complete after sync()."""
        opt = self._place_query_options(k, exclude_last)
        ptr, n = self._place_dev(cloud)
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() >= int(k) * PLACE_MATCH_DTYPE.itemsize
        self._chk(self.L.vloam_place_query_device(self.h, C.byref(opt), ptr, n, C.c_void_p(out.data_ptr())))

    def place_query_descriptor(self, desc, k=1, exclude_last=0):
        """vloam_place_query_descriptor: the same for a packed descriptor (uint32 [S * W], pad bytes zero)."""
        opt = self._place_query_options(k, exclude_last)
        d = np.ascontiguousarray(desc, dtype=np.uint32).reshape(-1)
        assert d.shape[0] == self._place_words()
        out = np.zeros(PLACE_MAX_K, dtype=PLACE_MATCH_DTYPE)
        self._chk(self.L.vloam_place_query_descriptor(self.h, C.byref(opt), _fp(d), _fp(out)))
        return out[:int(k)]

    def place_time_query(self, desc, repeats, k=1, exclude_last=0):
        """vloam_place_time_query: HIP-event milliseconds of `repeats` back-to-back matches of a packed descriptor (float32 [repeats])."""
        opt = self._place_query_options(k, exclude_last)
        d = np.ascontiguousarray(desc, dtype=np.uint32).reshape(-1)
        assert d.shape[0] == self._place_words()
        ms = np.zeros(int(repeats), np.float32)
        self._chk(self.L.vloam_place_time_query(self.h, C.byref(opt), _fp(d), int(repeats), _fp(ms)))
        return ms

    def _import_options(self, q_wmap_wodom, t_wmap_wodom):
        opt = MapImportOptions()
        self.L.vloam_default_map_import_options(C.byref(opt))
        if q_wmap_wodom is not None:
            opt.q_wmap_wodom[:] = [float(v) for v in q_wmap_wodom]
        if t_wmap_wodom is not None:
            opt.t_wmap_wodom[:] = [float(v) for v in t_wmap_wodom]
        return opt

    @staticmethod
    def _import_result(out):
        return {k: (out[0][k].copy() if out[0][k].ndim else out[0][k].item()) for k in MAP_IMPORT_RESULT_DTYPE.names if k != "pad"}

    def map_import(self, corner, surf, q_wmap_wodom=None, t_wmap_wodom=None):
        """vloam_map_import: on a fresh handle, corner / surf (float32 [n, 4]: x, y, z, intensity in the MAP frame, e.g. get_map_kind(0 / 1) of
        another handle; None: empty) become the map, points of one voxel merged into their centroid in input order, and (q_wmap_wodom xyzw,
        t_wmap_wodom) the map<-odometry transform the sequence starts with (None: identity / zero).  Returns the fields of
        vloam_map_import_result as a dict."""
        opt = self._import_options(q_wmap_wodom, t_wmap_wodom)
        c, s = self._cloud_arg(corner), self._cloud_arg(surf)
        out = np.zeros(1, dtype=MAP_IMPORT_RESULT_DTYPE)
        self._chk(self.L.vloam_map_import(self.h, C.byref(opt), c[1], C.c_longlong(c[2]), s[1], C.c_longlong(s[2]), _fp(out)))
        return self._import_result(out)

    def map_import_device(self, corner, surf, q_wmap_wodom=None, t_wmap_wodom=None):
        """vloam_map_import_device: the same with torch tensors on the device (float32 [n, 4], or None); points with a non-finite float are
        dropped and counted in n_nonfinite, where map_import() refuses them.  Returns the result as a dict."""
        import torch
        opt = self._import_options(q_wmap_wodom, t_wmap_wodom)
        ptr, n = [None, None], [0, 0]
        for k, c in enumerate((corner, surf)):
            if c is not None and c.shape[0] > 0:
                assert c.is_cuda and c.is_contiguous() and c.dtype == torch.float32 and c.shape[-1] == 4
                ptr[k], n[k] = C.c_void_p(c.data_ptr()), int(c.shape[0])
        res = torch.zeros(MAP_IMPORT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=next((c.device for c in (corner, surf) if c is not None), "cuda"))
        self._chk(self.L.vloam_map_import_device(self.h, C.byref(opt), ptr[0], C.c_longlong(n[0]), ptr[1], C.c_longlong(n[1]), C.c_void_p(res.data_ptr())))
        return self._import_result(res.cpu().numpy().view(MAP_IMPORT_RESULT_DTYPE))

    def _merge_options(self, q, t, apply):
        opt = MapMergeOptions()
        self.L.vloam_default_map_merge_options(C.byref(opt))
        if q is not None:
            opt.q_map_src[:] = [float(v) for v in q]
        if t is not None:
            opt.t_map_src[:] = [float(v) for v in t]
        opt.apply = int(apply)
        return opt

    @staticmethod
    def _merge_result(out):
        return {k: out[0][k].copy() for k in MAP_MERGE_RESULT_DTYPE.names}

    def map_merge(self, corner, surf, q=None, t=None, apply=True):
        """vloam_map_merge: corner / surf (float32 [n, 4]: x, y, z, intensity in ANOTHER map's frame, e.g. a --save-map directory's files; None:
        empty) are folded into this handle's live map under (q xyzw, t): this map <- the clouds' frame (None: identity / zero).  Points of one
        voxel join the voxel's map point in input order; apply=False looks up only.  Returns the fields of vloam_map_merge_result as a dict."""
        opt = self._merge_options(q, t, apply)
        c, s = self._cloud_arg(corner), self._cloud_arg(surf)
        out = np.zeros(1, dtype=MAP_MERGE_RESULT_DTYPE)
        self._chk(self.L.vloam_map_merge(self.h, C.byref(opt), c[1], C.c_longlong(c[2]), s[1], C.c_longlong(s[2]), _fp(out)))
        return self._merge_result(out)

    def map_merge_device(self, corner, surf, q=None, t=None, apply=True):
        """vloam_map_merge_device: the same with torch tensors on the device (float32 [n, 4], or None); points with a non-finite float are
        dropped and counted in n_nonfinite, where map_merge() refuses them.  Returns the result as a dict."""
        import torch
        opt = self._merge_options(q, t, apply)
        ptr, n = [None, None], [0, 0]
        for k, c in enumerate((corner, surf)):
            if c is not None and c.shape[0] > 0:
                assert c.is_cuda and c.is_contiguous() and c.dtype == torch.float32 and c.shape[-1] == 4
                ptr[k], n[k] = C.c_void_p(c.data_ptr()), int(c.shape[0])
        res = torch.zeros(MAP_MERGE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=next((c.device for c in (corner, surf) if c is not None), "cuda"))
        self._chk(self.L.vloam_map_merge_device(self.h, C.byref(opt), ptr[0], C.c_longlong(n[0]), ptr[1], C.c_longlong(n[1]), C.c_void_p(res.data_ptr())))
        return self._merge_result(res.cpu().numpy().view(MAP_MERGE_RESULT_DTYPE))

    def _carve_options(self, apply, **kw):
        opt = CarveOptions()
        self.L.vloam_default_carve_options(C.byref(opt))
        for k, v in kw.items():
            if not hasattr(opt, k) or k == "struct_size":
                raise AttributeError("vloam_carve_options has no field %r" % k)
            setattr(opt, k, v)
        opt.apply = int(apply)
        return opt

    @staticmethod
    def _carve_poses(poses, n_sweeps):
        if poses is None:
            return None
        p = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        assert p.shape[0] == n_sweeps, "one pose (qx qy qz qw tx ty tz, map <- sensor) per sweep"
        return p

    @staticmethod
    def _carve_result(res):
        return {k: (res[0][k].copy() if res[0][k].ndim else res[0][k].item()) for k in CARVE_RESULT_DTYPE.names}

    def map_carve(self, sweeps, poses=None, apply=False, cap=None, **options):
        """vloam_map_carve: remove (apply) or list (dry run, the default) the map voxels that the given sweeps see through.  sweeps: up to 16
        arrays float32 [n, 4] (x, y, z, -) in the sensor frame, NaN rows allowed; poses: [n_sweeps, 7] (qx qy qz qw tx ty tz, map <- sensor),
        None with one sweep: the last mapped pose; options: fields of vloam_carve_options (kind_mask, rows, cols, elev_min_deg, elev_max_deg,
        min_range, max_range, range_res, margin, min_votes).  cap: capacity of the removed list (None: a dry run sizes it first).  Returns
        (removed float32 [n, 4] in unspecified order, the fields of vloam_carve_result as a dict).  Synchronises the handle."""
        clouds = [np.ascontiguousarray(s, dtype=np.float32).reshape(-1, 4) for s in sweeps]
        ns = len(clouds)
        ptrs = (C.c_void_p * max(ns, 1))(*[c.ctypes.data if c.shape[0] else None for c in clouds])
        n = (C.c_int * max(ns, 1))(*[c.shape[0] for c in clouds])
        p = self._carve_poses(poses, ns)
        res = np.zeros(1, dtype=CARVE_RESULT_DTYPE)

        def call(apply_now, buf, cap_now):
            opt = self._carve_options(apply_now, **options)
            return self.L.vloam_map_carve(self.h, C.byref(opt), ptrs, n, None if p is None else _fp(p), ns, None if buf is None else _fp(buf),
                                          C.c_longlong(cap_now), _fp(res))
        if cap is None:   # a dry run with an empty list: VLOAM_OK when nothing leaves, else the capacity needed
            st = call(False, None, 0)
            if st != ERR_CAPACITY:
                self._chk(st)
                if not apply:
                    return np.zeros((0, 4), np.float32), self._carve_result(res)
            cap = int(res[0]["n_removed_out"])
        buf = np.zeros((max(int(cap), 1), 4), dtype=np.float32)
        self._chk(call(apply, buf if cap else None, int(cap)))
        return buf[:int(res[0]["n_removed_out"])].copy(), self._carve_result(res)

    def map_carve_device(self, sweeps, poses, removed, apply=False, **options):
        """vloam_map_carve_device: the same with torch tensors on the device — sweeps float32 [n, 4] each, removed a float32 [cap, 4] tensor
        the removed points are written into.  Returns the fields of vloam_carve_result as a dict (n_removed_out rows of removed are valid);
        more removals than cap raise VloamError(ERR_CAPACITY)."""
        ns = len(sweeps)
        for c in sweeps:
            assert c.is_cuda and c.is_contiguous() and c.element_size() == 4 and c.dtype.is_floating_point and c.shape[-1] == 4
        assert removed.is_cuda and removed.is_contiguous() and removed.element_size() == 4 and removed.shape[-1] == 4
        ptrs = (C.c_void_p * max(ns, 1))(*[c.data_ptr() if c.shape[0] else None for c in sweeps])
        n = (C.c_int * max(ns, 1))(*[int(c.shape[0]) for c in sweeps])
        p = self._carve_poses(poses, ns)
        res = np.zeros(1, dtype=CARVE_RESULT_DTYPE)
        opt = self._carve_options(apply, **options)
        cap = int(removed.shape[0])
        self._chk(self.L.vloam_map_carve_device(self.h, C.byref(opt), ptrs, n, None if p is None else _fp(p), ns,
                                                C.c_void_p(removed.data_ptr()) if cap else None, C.c_longlong(cap), _fp(res)))
        return self._carve_result(res)

    def map_archive_enable(self, capacity_rows=None):
        """vloam_map_archive_enable: from the next mapped sweep on, the points of cubes that roll out of the map's window are kept in a list of
        capacity_rows rows (None: the default, 2^20) on the device instead of being lost.  Single-sequence handles with mapping, once."""
        opt = MapArchiveOptions()
        self.L.vloam_default_map_archive_options(C.byref(opt))
        if capacity_rows is not None:
            opt.capacity_rows = int(capacity_rows)
        self._chk(self.L.vloam_map_archive_enable(self.h, C.byref(opt)))

    def map_archive_info(self):
        """vloam_map_archive_info: rows held, rows dropped since the last clear (the archive was full), the capacity, rolls seen.  Synchronises."""
        v = np.zeros(4, dtype=np.int64)
        self._chk(self.L.vloam_map_archive_info(self.h, _fp(v)))
        return dict(rows=int(v[0]), dropped=int(v[1]), capacity_rows=int(v[2]), rolls=int(v[3]))

    def map_archive(self, clear=False):
        """vloam_map_archive_get: the rows held as a structured array (MAP_ARCHIVE_ROW_DTYPE), sorted by (sweep, kind, cube_k, cube_j, cube_i,
        tail, order) — within one cube and kind the order get_map_kind() had.  clear: rows held and rows dropped start over.  Synchronises."""
        n = C.c_longlong(0)
        st = self.L.vloam_map_archive_get(self.h, None, C.c_longlong(0), C.byref(n), 0)
        if st != ERR_CAPACITY:
            self._chk(st)
        out = np.zeros(max(n.value, 1), dtype=MAP_ARCHIVE_ROW_DTYPE)
        self._chk(self.L.vloam_map_archive_get(self.h, _fp(out), C.c_longlong(n.value), C.byref(n), 1 if clear else 0))
        return out[:n.value]

    def map_archive_device_ptr(self):
        """(device address of the unsorted rows, device address of the counters: int32 rows held, rows dropped); complete after sync()."""
        p, c = C.c_void_p(), C.c_void_p()
        self._chk(self.L.vloam_map_archive_device_ptr(self.h, C.byref(p), C.byref(c)))
        return p.value, c.value

    def published_map(self):
        """The latest /laser_cloud_map the mapping stream published (vloam_limits::map_pub_number): (float32 [n, 4], 0-based sweep index),
        ([0, 4], -1) before the first publication.  Waits for that publication only, not for the pipeline."""
        n, f = C.c_longlong(0), C.c_int(-1)
        self._chk(self.L.vloam_get_published_map(self.h, None, C.c_longlong(0), C.byref(n), C.byref(f)))
        buf = np.zeros((max(n.value, 1), 4), dtype=np.float32)
        self._chk(self.L.vloam_get_published_map(self.h, _fp(buf), C.c_longlong(n.value), C.byref(n), C.byref(f)))
        return buf[:n.value], f.value

    def published_cloud(self):
        """The latest registered full-resolution cloud the mapping stream published (vloam_limits::publish_registered_cloud), like published_map()."""
        n, f = C.c_int(0), C.c_int(-1)
        self._chk(self.L.vloam_get_published_cloud(self.h, None, 0, C.byref(n), C.byref(f)))
        buf = np.zeros((max(n.value, 1), 4), dtype=np.float32)
        self._chk(self.L.vloam_get_published_cloud(self.h, _fp(buf), n.value, C.byref(n), C.byref(f)))
        return buf[:n.value], f.value

    def published_device_ptr(self, which):
        """(device address, points, sweep index) of the latest published map (which = 0) / registered cloud (1): packed float4, valid until
        the next call that enqueues a sweep."""
        p, n, f = C.c_void_p(), C.c_longlong(0), C.c_int(-1)
        self._chk(self.L.vloam_published_device_ptr(self.h, int(which), C.byref(p), C.byref(n), C.byref(f)))
        return p.value, n.value, f.value

    def map_health(self):
        v = self.debug_raw(2, 69, np.int32)
        return dict(keys=(int(v[0]), int(v[4])), purged=(int(v[1]), int(v[5])), block_keys=(int(v[2]), int(v[6])), rebuilds=int(v[8]),
                    max_candidates=int(v[9]), deferred=(int(v[10]), int(v[11])))

    def map_force_rebuild(self):
        n = C.c_longlong(0)
        self._chk(self.L.vloam_debug_get(self.h, 2, 70, None, C.c_longlong(0), C.byref(n)))

    def map_force_grow(self):
        """Test hook: one growth step of both tables of a growable handle (map_grow=1) now, between two sweeps."""
        n = C.c_longlong(0)
        self._chk(self.L.vloam_debug_get(self.h, 2, 74, None, C.c_longlong(0), C.byref(n)))

    def map_dump(self, kind):
        """Live voxels of the corner (0) / surf (1) map as (count int32[n], xyzi float32[n, 4])."""
        rows = self.debug_raw(2, 67 + kind, np.uint32, max_bytes=1 << 30).reshape(-1, 7)
        return rows[:, 2].astype(np.int32), rows[:, 3:7].copy().view(np.float32)


# ------------------------------------------------------------------------------------------------
# Python mirror of the reference's class surface (same method names / call order / error behaviour).
def _same_cloud(given, own):
    """A handed-in cloud is the device's own when all four floats of every point are equal bit for bit (compat.hpp same_cloud)."""
    a = np.ascontiguousarray(given, dtype=np.float32).reshape(-1, 4)
    return a.shape == own.shape and np.array_equal(a.view(np.uint32), np.ascontiguousarray(own).view(np.uint32))


class ScanRegistration:
    """vloam::ScanRegistration (scan_registration.h:71-77): init / reset / input / output."""

    def __init__(self, handle):
        self.hd = handle

    def init(self):
        pass  # parameters were bound at vloam_create (the reference reads them from the ROS parameter server here)

    def reset(self):
        self.hd.reset_frame()

    def input(self, laserCloudIn):
        self.hd.scan_registration(laserCloudIn)

    def output(self):
        return tuple(self.hd.features(k) for k in range(5))


class LaserOdometry:
    """vloam::LaserOdometry (laser_odometry.h:70-84): init / input / solveLO / output."""

    def __init__(self, handle):
        self.hd = handle
        self._pose = None

    def init(self):
        pass

    def input(self, *clouds):
        """laser_odometry.cpp:135-146 deep-copies the five clouds it is handed (laserCloud, cornerPointsSharp, cornerPointsLessSharp,
        surfPointsFlat, surfPointsLessFlat).  Scan registration's clouds are resident on the device; a cloud that differs from the device's bit
        for bit is uploaded (vloam_set_odometry_input, under the rule c_api.h states).  No arguments: keep the device's."""
        if not clouds:
            return
        if len(clouds) != 5:
            raise TypeError("LaserOdometry.input takes the five clouds of ScanRegistration.output")
        edits = {}
        for k, (name, c) in enumerate(zip(("laserCloud", "cornerPointsSharp", "cornerPointsLessSharp", "surfPointsFlat", "surfPointsLessFlat"), clouds)):
            if not _same_cloud(c, self.hd.features(k)):
                edits[name] = c
        if edits:
            self.hd.set_odometry_input(**edits)

    def solveLO(self):
        self._pose = self.hd.laser_odometry()

    # the public pose members of the reference class (laser_odometry.h:86-98), x y z w
    q_w_curr = property(lambda self: self._pose[0])
    t_w_curr = property(lambda self: self._pose[1])
    q_last_curr = property(lambda self: self._pose[2])
    t_last_curr = property(lambda self: self._pose[3])

    def output(self):
        qw, tw, _, _ = self._pose
        # laser_odometry.cpp:535,618: frameCount is incremented by solveLO before output() tests it.  The handle counts a sweep when its last
        # stage is done: with mapping that is still to come here, without it solveLO was the last stage
        skip = (self.hd.frame_count() + (1 if self.hd.cfg.with_mapping else 0)) % self.hd.cfg.mapping_skip_frame != 0
        return qw, tw, self.hd.features(5), self.hd.features(6), self.hd.features(0), skip


class LaserMapping:
    """vloam::LaserMapping (laser_mapping.h:85-94): init / reset / input / solveMapping."""

    def __init__(self, handle):
        self.hd = handle
        self.pose = None

    def init(self):
        pass

    def reset(self):
        pass

    def input(self, *args):
        """laser_mapping.cpp:167-196: input(laserCloudCornerLast, laserCloudSurfLast, laserCloudFullRes, q_wodom_curr, t_wodom_curr, skip_frame)
        copies the three clouds (unless skip_frame) and the odometry pose.  What differs bit for bit from LaserOdometry.output's is uploaded
        (vloam_set_mapping_input).  No arguments: keep the device's."""
        if not args:
            return
        if len(args) != 6:
            raise TypeError("LaserMapping.input takes (corner, surf, full, q_wodom_curr, t_wodom_curr, skip_frame)")
        corner, surf, full, q, t, skip = args
        if bool(skip) != ((self.hd.frame_count() + 1) % self.hd.cfg.mapping_skip_frame != 0):   # (this sweep is not counted yet: see LaserOdometry.output)
            raise ValueError("LaserMapping.input: skip_frame differs from frameCount % mapping_skip_frame (laser_odometry.cpp:618)")
        edits = {}
        if not skip:
            for name, c, which in (("laserCloudCornerLast", corner, 5), ("laserCloudSurfLast", surf, 6), ("laserCloudFullRes", full, 0)):
                if not _same_cloud(c, self.hd.features(which)):
                    edits[name] = c
        qd, td = self.hd.odometry_pose()
        q = np.asarray(q, dtype=np.float64)
        t = np.asarray(t, dtype=np.float64)
        if not (np.array_equal(q, qd) and np.array_equal(t, td)):
            edits.update(q_wodom_curr=q, t_wodom_curr=t)
        if edits:
            self.hd.set_mapping_input(**edits)

    def solveMapping(self):
        self.pose = self.hd.laser_mapping()

    q_w_curr = property(lambda self: self.pose[0])   # laser_mapping.h:129-130
    t_w_curr = property(lambda self: self.pose[1])


class LidarOdometryMapping:
    """vloam::LidarOdometryMapping façade (lidar_odometry_mapping.cpp:65-154)."""

    def __init__(self, device=0, **cfg):
        self.hd = Handle(device, **cfg)
        self.scan_registration = ScanRegistration(self.hd)
        self.laser_odometry = LaserOdometry(self.hd)
        self.laser_mapping = LaserMapping(self.hd)

    def reset(self):
        self.scan_registration.reset()
        self.laser_mapping.reset()

    def scanRegistrationIO(self, laserCloudIn):
        self.scan_registration.input(laserCloudIn)

    def laserOdometryIO(self):
        self.laser_odometry.solveLO()
        return self.laser_odometry._pose

    def laserMappingIO(self):
        self.laser_mapping.solveMapping()
        return self.laser_mapping.pose
