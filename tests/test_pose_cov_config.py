"""CPU: the opt-in per-sweep pose covariance rows — vloam_pose_cov_options, vloam_pose_cov_record and the entry points, and the option check
(before any device call, before the handle is looked at).  The GPU side: tests/test_gpu_pose_cov.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from test_pose_info_config import c_offsets
from test_sweep_log_config import header, struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OFFSETS = [("frame", 0), ("flags", 4), ("rank", 8), ("vo_factors", 20), ("reserved", 28), ("sigma2", 32), ("reserved_d", 56),
           ("lo_eig", 64), ("lo_V", 112), ("lo_cov", 400), ("map_eig", 688), ("map_V", 736), ("map_cov", 1024),
           ("vo_x", 1312), ("vo_cost", 1360), ("vo_reserved", 1368), ("vo_H", 1376), ("vo_eig", 1664), ("vo_V", 1712), ("vo_cov", 2000)]


def test_record_is_2288_bytes_and_the_dtype_mirrors_it(vl):
    text = header()
    assert re.search(r"static_assert\(sizeof\(vloam_pose_cov_record\) == 2288", text)
    fields = struct_fields(text, "vloam_pose_cov_record")
    dt = vl.POSE_COV_DTYPE
    assert dt.itemsize == 2288
    assert [n for _, n, _ in fields] == list(dt.names) == [n for n, _ in OFFSETS]
    offs, size = c_offsets(fields)
    assert size == 2288
    for (name, t, length, off), (_, want) in zip(offs, OFFSETS):
        sub, o = dt.fields[name][:2]
        assert o == off == want, (name, o, off, want)
        assert sub.base == np.dtype("<i4" if t == "int" else "<f8") and sub.shape == ((length,) if length else ()), name
    n_int = sum((l or 1) for t, _, l in fields if t == "int")
    n_dbl = sum((l or 1) for t, _, l in fields if t == "double")
    assert (n_int, n_dbl) == (8, 282)
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, val in [("LO_VALID", 1), ("MAP_VALID", 2), ("VO_VALID", 4), ("LO_TRUNCATED", 8), ("MAP_TRUNCATED", 16), ("VO_TRUNCATED", 32)]:
        assert re.search(r"VLOAM_POSE_COV_%s = %d\b" % (name, val), plain), name
        assert getattr(vl, "POSE_COV_" + name) == val


def test_record_layout_through_a_c_compile(vl, tmp_path):
    """The same offsets as a C99 and as a C++14 compiler lay the header's struct out; the 832-byte record next to it is what it was."""
    lines = ["#include <stddef.h>", "#include <vloam_hip/c_api.h>", "#define CHECK2(c, l) typedef char check_##l[(c) ? 1 : -1]", "#define CHECK1(c, l) CHECK2(c, l)"]
    lines += ["CHECK1(sizeof(vloam_pose_cov_record) == 2288, __LINE__);", "CHECK1(sizeof(vloam_pose_cov_options) == 32, __LINE__);",
              "CHECK1(sizeof(vloam_pose_info_record) == 832, __LINE__);", "CHECK1(offsetof(vloam_pose_cov_options, vo_min_eigenvalue) == 24, __LINE__);"]
    lines += ["CHECK1(offsetof(vloam_pose_cov_record, %s) == %d, __LINE__);" % (n, o) for n, o in OFFSETS]
    lines += ["int enable_is_declared(vloam_handle* h) { vloam_pose_cov_options o; vloam_default_pose_cov_options(&o); return (int)vloam_pose_cov_enable(h, &o); }"]
    for name, cmd in (("layout.c", ["gcc", "-std=c99"]), ("layout.cpp", ["g++", "-std=c++14"])):
        src = tmp_path / name
        src.write_text("\n".join(lines) + "\n")
        subprocess.check_call(cmd + ["-Wall", "-Werror", "-Wno-unused-local-typedefs", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / (name + ".o"))])


def test_options_struct_defaults_and_exports(vl):
    text = header()
    ctype = {"int": C.c_int, "double": C.c_double, "float": C.c_float}
    assert [(n, ctype[t]) for t, n, _ in struct_fields(text, "vloam_pose_cov_options")] == list(vl.PoseCovOptions._fields_)
    assert C.sizeof(vl.PoseCovOptions) == 32
    assert [getattr(vl.PoseCovOptions, n).offset for n in ("lo_min_eigenvalue", "map_min_eigenvalue", "vo_min_eigenvalue")] == [8, 16, 24]
    L = vl.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert hasattr(L, "vloam_default_pose_cov_options") and re.search(r"void\s+vloam_default_pose_cov_options\(vloam_pose_cov_options\*", plain)
    for sym in ("vloam_pose_cov_enable", "vloam_get_pose_cov", "vloam_pose_cov_device_ptr"):
        assert hasattr(L, sym), sym
        assert re.search(r"vloam_status\s+%s\(vloam_handle\*\s*h," % sym, plain), sym
    opt = vl.PoseCovOptions(-1, -1, -1.0, -1.0, -1.0)
    L.vloam_default_pose_cov_options(C.byref(opt))
    assert (opt.struct_size, opt.reserved, opt.lo_min_eigenvalue, opt.map_min_eigenvalue, opt.vo_min_eigenvalue) == (32, 0, 0.0, 0.0, 0.0)
    L.vloam_default_pose_cov_options(None)   # a null pointer is ignored
    # the pose information options and its refusals are what they were
    assert C.sizeof(vl.PoseInfoOptions) == 24
    assert L.vloam_pose_info_enable(None, C.byref(vl.PoseInfoOptions(32, 0, 0.0, 0.0))) == vl.ERR_INVALID and b"struct_size must be 24" in L.vloam_last_error()


def test_option_check_needs_no_device(vl):
    """The options are checked before the handle is looked at: a refused struct is VLOAM_ERR_INVALID with a message of its own, an accepted one
    gets as far as the (null) handle."""
    L = vl.lib()

    def enable(*fields):
        st = L.vloam_pose_cov_enable(None, C.byref(vl.PoseCovOptions(*fields)))
        return st, L.vloam_last_error()

    for ok in [(32, 0, 0.0, 0.0, 0.0), (32, 0, 1e-3, 5.0, 7.0), (32, 0, 1e300, 0.0, 1e-300)]:
        st, msg = enable(*ok)
        assert st == vl.ERR_INVALID and b"null handle" in msg, (ok, msg)
    assert L.vloam_pose_cov_enable(None, None) == vl.ERR_INVALID and b"null handle" in L.vloam_last_error()
    for size in (0, 8, 24, 31, 40, -32):
        st, msg = enable(size, 0, 0.0, 0.0, 0.0)
        assert st == vl.ERR_INVALID and b"struct_size must be 32" in msg, (size, msg)
    st, msg = enable(32, 1, 0.0, 0.0, 0.0)
    assert st == vl.ERR_INVALID and b"reserved" in msg and b"struct_size" not in msg
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        for k in range(3):
            thr = [0.0, 0.0, 0.0]
            thr[k] = bad
            st, msg = enable(32, 0, *thr)
            assert st == vl.ERR_INVALID and b"min_eigenvalue" in msg and b"null handle" not in msg, (thr, msg)


def test_getters_refuse_a_null_handle(vl):
    L = vl.lib()
    p, b = C.c_void_p(), C.c_longlong(0)
    rows = np.zeros(1, dtype=vl.POSE_COV_DTYPE)
    assert L.vloam_get_pose_cov(None, 0, 1, rows.ctypes.data_as(C.c_void_p)) == vl.ERR_INVALID
    assert L.vloam_pose_cov_device_ptr(None, C.byref(p), C.byref(b)) == vl.ERR_INVALID
