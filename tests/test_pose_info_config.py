"""CPU: the opt-in per-sweep pose information product — vloam_pose_info_options, vloam_pose_info_record and the entry points, and the option check
(before any device call, before the handle is looked at).  The GPU side: tests/test_gpu_pose_info.py."""
import ctypes as C
import os
import re

import numpy as np

from test_sweep_log_config import header, struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def c_offsets(fields):
    """Offsets as a C compiler lays the fields out (ints of 4, doubles of 8 aligned to 8): [(name, type, length, offset)], total size."""
    off, out = 0, []
    for t, name, length in fields:
        size = 4 if t == "int" else 8
        off = (off + size - 1) // size * size
        out.append((name, t, length, off))
        off += size * (length or 1)
    return out, (off + 7) // 8 * 8


def test_record_is_832_bytes_and_the_dtype_mirrors_it(vl):
    text = header()
    assert re.search(r"static_assert\(sizeof\(vloam_pose_info_record\) == 832", text)
    fields = struct_fields(text, "vloam_pose_info_record")
    dt = vl.POSE_INFO_DTYPE
    assert dt.itemsize == 832
    assert [n for _, n, _ in fields] == list(dt.names)
    offs, size = c_offsets(fields)
    assert size == 832
    for name, t, length, off in offs:
        sub, o = dt.fields[name][:2]
        assert o == off, (name, o, off)
        assert sub.base == np.dtype("<i4" if t == "int" else "<f8") and sub.shape == ((length,) if length else ()), name
    n_int = sum((l or 1) for t, _, l in fields if t == "int")
    n_dbl = sum((l or 1) for t, _, l in fields if t == "double")
    assert (n_int, n_dbl) == (8, 100)
    assert [dt.fields[n][1] for n in ("frame", "flags", "lo_factors", "map_factors", "reserved", "lo_x", "lo_cost", "lo_H", "lo_eig", "map_x", "map_cost",
                                      "map_H", "map_eig")] == [0, 4, 8, 16, 24, 32, 88, 96, 384, 432, 488, 496, 784]
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, val in [("LO_VALID", 1), ("MAP_VALID", 2), ("LO_DEGENERATE", 4), ("MAP_DEGENERATE", 8)]:
        assert re.search(r"VLOAM_POSE_INFO_%s = %d\b" % (name, val), plain), name
        assert getattr(vl, "POSE_INFO_" + name) == val


def test_options_struct_and_exports(vl):
    text = header()
    ctype = {"int": C.c_int, "double": C.c_double, "float": C.c_float}
    assert [(n, ctype[t]) for t, n, _ in struct_fields(text, "vloam_pose_info_options")] == list(vl.PoseInfoOptions._fields_)
    assert C.sizeof(vl.PoseInfoOptions) == 24 and vl.PoseInfoOptions.lo_min_eigenvalue.offset == 8 and vl.PoseInfoOptions.map_min_eigenvalue.offset == 16
    L = vl.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert hasattr(L, "vloam_default_pose_info_options") and re.search(r"void\s+vloam_default_pose_info_options\(vloam_pose_info_options\*", plain)
    for sym in ("vloam_pose_info_enable", "vloam_get_pose_info", "vloam_pose_info_device_ptr"):
        assert hasattr(L, sym), sym
        assert re.search(r"vloam_status\s+%s\(vloam_handle\*\s*h," % sym, plain), sym
    opt = vl.PoseInfoOptions(-1, -1, -1.0, -1.0)
    L.vloam_default_pose_info_options(C.byref(opt))
    assert (opt.struct_size, opt.reserved, opt.lo_min_eigenvalue, opt.map_min_eigenvalue) == (24, 0, 0.0, 0.0)
    L.vloam_profile_kernel_name.restype = C.c_char_p
    names = [L.vloam_profile_kernel_name(k).decode() for k in range(L.vloam_profile_kernel_count())]
    assert names[-2:] == ["k_pose_info_lo", "k_pose_info_map"], "the new kernel ids come last"
    assert names.index("k_sweep_log_map") == len(names) - 3


def test_option_check_needs_no_device(vl):
    """The options are checked before the handle is looked at: a refused struct is VLOAM_ERR_INVALID with a message that names it, an accepted
    one gets as far as the (null) handle."""
    L = vl.lib()

    def enable(*fields):
        st = L.vloam_pose_info_enable(None, C.byref(vl.PoseInfoOptions(*fields)))
        return st, L.vloam_last_error()

    for ok in [(24, 0, 0.0, 0.0), (24, 0, 1e-3, 5.0), (24, 0, 1e300, 0.0)]:
        st, msg = enable(*ok)
        assert st == vl.ERR_INVALID and b"null handle" in msg, (ok, msg)
    assert L.vloam_pose_info_enable(None, None) == vl.ERR_INVALID and b"null handle" in L.vloam_last_error()
    for size in (0, 8, 16, 23, 32, -24):
        st, msg = enable(size, 0, 0.0, 0.0)
        assert st == vl.ERR_INVALID and b"struct_size must be 24" in msg, (size, msg)
    st, msg = enable(24, 1, 0.0, 0.0)
    assert st == vl.ERR_INVALID and b"reserved" in msg
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        for fields in ((24, 0, bad, 0.0), (24, 0, 0.0, bad)):
            st, msg = enable(*fields)
            assert st == vl.ERR_INVALID and b"min_eigenvalue" in msg, (fields, msg)


def test_getters_refuse_a_null_handle(vl):
    L = vl.lib()
    p, b = C.c_void_p(), C.c_longlong(0)
    rows = np.zeros(1, dtype=vl.POSE_INFO_DTYPE)
    assert L.vloam_get_pose_info(None, 0, 1, rows.ctypes.data_as(C.c_void_p)) == vl.ERR_INVALID
    assert L.vloam_pose_info_device_ptr(None, C.byref(p), C.byref(b)) == vl.ERR_INVALID
