"""CPU: the map archive — vloam_map_archive_row and vloam_map_archive_options as a C and a C++ compiler lay them out, the NumPy dtype that
mirrors the row, the exported entry points, and the refusals that need no device (options first, then the null handle).  The GPU side:
tests/test_gpu_map_archive.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from test_sweep_log_config import header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the table of c_api.h: field, offset, NumPy type
ROW = [("x", 0, "<f4"), ("y", 4, "<f4"), ("z", 8, "<f4"), ("intensity", 12, "<f4"), ("order", 16, "<u4"), ("cube_i", 20, "<i2"), ("cube_j", 22, "<i2"),
       ("cube_k", 24, "<i2"), ("flags", 26, "<u2"), ("sweep", 28, "<i4")]
SYMBOLS = ("vloam_default_map_archive_options", "vloam_map_archive_enable", "vloam_map_archive_info", "vloam_map_archive_get", "vloam_map_archive_device_ptr")


def test_row_layout_through_a_c_compile(tmp_path):
    lines = ["#include <stddef.h>", "#include <vloam_hip/c_api.h>", "#define CHECK2(c, l) typedef char check_##l[(c) ? 1 : -1]", "#define CHECK1(c, l) CHECK2(c, l)",
             "CHECK1(sizeof(vloam_map_archive_row) == 32, __LINE__);", "CHECK1(sizeof(vloam_map_archive_options) == 16, __LINE__);",
             "CHECK1(offsetof(vloam_map_archive_options, capacity_rows) == 8, __LINE__);"]
    lines += ["CHECK1(offsetof(vloam_map_archive_row, %s) == %d, __LINE__);" % (n, o) for n, o, _ in ROW]
    lines += ["int calls_are_declared(vloam_handle* h) { vloam_map_archive_options o; vloam_map_archive_row r; long long v[4], n; void* p; int* c;",
              "  vloam_default_map_archive_options(&o);",
              "  return (int)vloam_map_archive_enable(h, &o) + (int)vloam_map_archive_info(h, v) + (int)vloam_map_archive_get(h, &r, 1, &n, 0) + (int)vloam_map_archive_device_ptr(h, &p, &c); }"]
    for name, cmd in (("layout.c", ["gcc", "-std=c99"]), ("layout.cpp", ["g++", "-std=c++14"])):
        src = tmp_path / name
        src.write_text("\n".join(lines) + "\n")
        subprocess.check_call(cmd + ["-Wall", "-Werror", "-Wno-unused-local-typedefs", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / (name + ".o"))])


def test_dtype_mirrors_the_row(vl):
    dt = vl.MAP_ARCHIVE_ROW_DTYPE
    assert dt.itemsize == 32 and list(dt.names) == [n for n, _, _ in ROW]
    for name, off, t in ROW:
        sub, o = dt.fields[name][:2]
        assert o == off and sub == np.dtype(t), name
    assert (vl.MAP_ARCHIVE_KIND, vl.MAP_ARCHIVE_TAIL) == (1, 2)
    assert C.sizeof(vl.MapArchiveOptions) == 16 and vl.MapArchiveOptions.capacity_rows.offset == 8


def test_exports_defaults_and_the_refusals_without_a_device(vl):
    L = vl.lib()
    plain = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert re.search(r"(vloam_status|void)\s+%s\(" % sym, plain), sym
    o = vl.MapArchiveOptions(-1, -1)
    L.vloam_default_map_archive_options(C.byref(o))
    assert (o.struct_size, o.capacity_rows) == (16, 1 << 20)
    # launched outside the per-kernel profile table: ids and count are what they were
    L.vloam_profile_kernel_name.restype = C.c_char_p
    assert not any(L.vloam_profile_kernel_name(k).decode().startswith("k_map_archive") for k in range(L.vloam_profile_kernel_count()))

    def enable(opt):
        st = L.vloam_map_archive_enable(None, None if opt is None else C.byref(opt))
        msg = L.vloam_last_error()
        assert msg.startswith(b"vloam_map_archive_enable:"), msg
        return st, msg

    for ok in (vl.MapArchiveOptions(16, 1), vl.MapArchiveOptions(16, 1 << 26), o):
        st, msg = enable(ok)
        assert st == vl.ERR_INVALID and b"null handle" in msg, msg
    seen = set()
    for opt, text in ((None, b"null options"), (vl.MapArchiveOptions(12, 1 << 20), b"struct_size must be 16"), (vl.MapArchiveOptions(16, 0), b"capacity_rows must be 1 .. 67108864 rows, not 0"),
                      (vl.MapArchiveOptions(16, (1 << 26) + 1), b"capacity_rows must be 1 .. 67108864 rows, not 67108865"), (vl.MapArchiveOptions(16, -5), b"not -5")):
        st, msg = enable(opt)
        assert st == vl.ERR_INVALID and text in msg and b"null handle" not in msg, (text, msg)
        seen.add(msg)
    assert len(seen) == 5
    v, n, rows = np.zeros(4, np.int64), C.c_longlong(-1), np.zeros(2, vl.MAP_ARCHIVE_ROW_DTYPE)
    p, c = C.c_void_p(), C.c_void_p()
    for name, args in (("vloam_map_archive_info", (v.ctypes.data_as(C.c_void_p),)), ("vloam_map_archive_get", (rows.ctypes.data_as(C.c_void_p), C.c_longlong(2), C.byref(n), 0)),
                       ("vloam_map_archive_device_ptr", (C.byref(p), C.byref(c)))):
        st = getattr(L, name)(None, *args)
        msg = L.vloam_last_error()
        assert st == vl.ERR_INVALID and msg.startswith(name.encode() + b":") and b"null handle" in msg, (name, msg)
    for args, text in (((None, C.c_longlong(0), None, 0), b"null count"), ((None, C.c_longlong(3), C.byref(n), 0), b"3 rows at a null address"),
                       ((rows.ctypes.data_as(C.c_void_p), C.c_longlong(-1), C.byref(n), 0), b"-1 rows"), ((None, C.c_longlong(0), C.byref(n), 2), b"clear must be 0 or 1, not 2")):
        st = L.vloam_map_archive_get(None, *args)
        msg = L.vloam_last_error()
        assert st == vl.ERR_INVALID and text in msg and b"null handle" not in msg, (text, msg)
