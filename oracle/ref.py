"""ctypes driver for the reference's own scan registration and cost functors (oracle/_ref/libref.so, oracle/ref_harness.cpp).

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
VARIANTS = ("libref.so", "libref_cmath_only.so")


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
