"""CPU: the opt-in per-sweep diagnostics log — vloam_limits_ext::sweep_log, vloam_sweep_record and its two entry points, and the argument check
(before any device call).  The GPU side: tests/test_gpu_sweep_log.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(map_capacity_log2=12, max_points=4096)   # (the check is what is tested, not the arena)
PREVIOUS_SIZE = 20   # sizeof(vloam_limits) before sweep_log: still a valid struct_size, the new field then reads as 0


def header():
    return open(os.path.join(ROOT, "include", "vloam_hip", "c_api.h")).read()


def struct_fields(text, name):
    """[(C type, field, array length or None)] of a typedef'd struct of the header, comments stripped, `int a, b;` lists expanded."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    out = []
    for t, names in re.findall(r"\b(int|double|float)\s+([^;]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)):
        for n in names.split(","):
            m = re.match(r"\s*([a-zA-Z_0-9]+)\s*(?:\[(\d+)\])?\s*$", n)
            out.append((t, m.group(1), int(m.group(2)) if m.group(2) else None))
    return out


def test_limits_ext_field_and_exports(vl):
    """vloam_limits keeps its 20 bytes; sweep_log lies right behind it in vloam_limits_ext, where struct_size = 24 tells the library to read it."""
    text = header()
    ctype = {"int": C.c_int, "double": C.c_double, "float": C.c_float}
    assert [(n, ctype[t]) for t, n, _ in struct_fields(text, "vloam_limits")] == list(vl.Limits._fields_)
    assert C.sizeof(vl.Limits) == PREVIOUS_SIZE
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct vloam_limits_ext \{(.*?)\} vloam_limits_ext;", text, flags=re.S).group(1), flags=re.S)
    assert re.findall(r"\b(\w+)\s+(\w+);", body) == [("vloam_limits", "limits"), ("int", "sweep_log")]
    assert [n for n, _ in vl.LimitsExt._fields_] == ["limits", "sweep_log"]
    assert C.sizeof(vl.LimitsExt) == PREVIOUS_SIZE + 4 and vl.LimitsExt.sweep_log.offset == PREVIOUS_SIZE and vl.LimitsExt.limits.offset == 0
    ext = vl.default_limits_ext()
    assert ext.limits.struct_size == C.sizeof(vl.LimitsExt) and ext.sweep_log == 0
    base = vl.default_limits()
    assert base.struct_size == PREVIOUS_SIZE
    assert [getattr(ext.limits, n) for n, _ in vl.Limits._fields_[1:]] == [getattr(base, n) for n, _ in vl.Limits._fields_[1:]]
    L = vl.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert hasattr(L, "vloam_default_limits_ext") and re.search(r"void\s+vloam_default_limits_ext\(vloam_limits_ext\*", plain)
    for sym in ("vloam_get_sweep_log", "vloam_sweep_log_device_ptr"):
        assert hasattr(L, sym), sym
        assert re.search(r"vloam_status\s+%s\(vloam_handle\*\s*h," % sym, plain), sym


def test_record_is_192_bytes_and_the_dtype_mirrors_it(vl):
    text = header()
    assert re.search(r"static_assert\(sizeof\(vloam_sweep_record\) == 192", text)
    fields = struct_fields(text, "vloam_sweep_record")
    dt = vl.SWEEP_RECORD_DTYPE
    assert dt.itemsize == 192
    # the header's fields in order -> offsets as a C compiler lays them out (ints of 4, doubles of 8 aligned to 8)
    off, n_int, n_dbl = 0, 0, 0
    assert [n for _, n, _ in fields] == list(dt.names)
    for t, name, length in fields:
        size = 4 if t == "int" else 8
        off = (off + size - 1) // size * size
        sub, o = dt.fields[name][:2]
        assert o == off, (name, o, off)
        assert sub.base == np.dtype("<i4" if t == "int" else "<f8") and sub.shape == ((length,) if length else ()), name
        off += size * (length or 1)
        n_int += (length or 1) if t == "int" else 0
        n_dbl += (length or 1) if t == "double" else 0
    assert (n_int, n_dbl, off) == (32, 8, 192)
    assert [t for t, _, _ in fields] == ["int"] * fields.index(("double", "lo_initial_cost", 2)) + ["double"] * 4   # 32 ints, then the doubles
    assert dt.fields["frame"][1] == 0 and dt.fields["error_bits"][1] == 4 and dt.fields["flags"][1] == 8 and dt.fields["lo_initial_cost"][1] == 128
    # the public bit names, with the values the wrapper mirrors
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, val in [("EMPTY", 1), ("RING_TOO_LONG", 2), ("MAP_FULL", 4), ("MAP_RAW_CAPACITY", 8), ("STACK_FULL", 16), ("DS_TIMEOUT", 32), ("VO_DEGENERATE", 64)]:
        assert re.search(r"VLOAM_SWEEP_%s = %d\b" % (name, val), plain), name
        assert getattr(vl, "SWEEP_" + name) == val
    for name, val in [("FIRST", 1), ("MAP_SKIPPED", 2), ("MAP_NOT_OPTIMIZED", 4), ("LO_LESS_CORR_0", 8), ("LO_LESS_CORR_1", 16), ("SOLVE_DEGRADED", 32)]:
        assert re.search(r"VLOAM_SWEEP_FLAG_%s = %d\b" % (name, val), plain), name
        assert getattr(vl, "SWEEP_FLAG_" + name) == val


def _create(vl, lim, n_sessions=1, **cfg):
    L = vl.lib()
    h = C.c_void_p()
    st = L.vloam_create_with_limits(C.byref(vl.default_config(**dict(SMALL, **cfg))), None if lim is None else C.byref(lim), 0, n_sessions, C.byref(h))
    msg = L.vloam_last_error()
    if st == vl.VLOAM_OK:
        L.vloam_destroy(h)
    return st, msg


@pytest.mark.parametrize("n_sessions", [1, 2])
def test_argument_check(vl, n_sessions):
    """Accepted values answer what default creation answers here (without a GPU: VLOAM_ERR_NO_DEVICE, which comes after the check); refused
    ones VLOAM_ERR_INVALID."""
    expected, _ = _create(vl, None, n_sessions)
    assert expected in (vl.VLOAM_OK, vl.ERR_NO_DEVICE)
    for kw, cfg in [(dict(sweep_log=0), {}), (dict(sweep_log=1), {}), (dict(sweep_log=1), dict(with_mapping=0)), (dict(sweep_log=1, map_pub_number=2), {}),
                    (dict(sweep_log=1, max_surf_stack_points=32768), dict(max_points=32768))]:
        st, msg = _create(vl, vl.default_limits_ext(**kw), n_sessions, **cfg)
        assert st == expected, (kw, cfg, msg)
    for v in (2, -1, 7, 0x7fffffff):
        st, msg = _create(vl, vl.default_limits_ext(sweep_log=v), n_sessions)
        assert st == vl.ERR_INVALID and b"sweep_log" in msg and b"0 or 1" in msg, (v, msg)
    # the fields of vloam_limits inside are checked as ever
    assert _create(vl, vl.default_limits_ext(sweep_log=1, map_pub_number=-1), n_sessions)[0] == vl.ERR_INVALID


def ext(vl, size, sweep_log, *fields):
    return vl.LimitsExt(vl.Limits(size, *fields), sweep_log)


def test_struct_size_versions(vl):
    expected, _ = _create(vl, None)
    full = C.sizeof(vl.LimitsExt)
    # exactly vloam_limits_ext's size: sweep_log is read
    for size in (full,):
        assert _create(vl, ext(vl, size, 1, 0, 0, 0, 0))[0] == expected, size
        assert _create(vl, ext(vl, size, 2, 0, 0, 0, 0))[0] == vl.ERR_INVALID, size
        assert _create(vl, ext(vl, size, -1, 0, 0, 0, 0))[0] == vl.ERR_INVALID, size
    # 0 (= sizeof(vloam_limits)), 8, the previous size, a later header's: nothing behind vloam_limits is the library's to read
    for size in (0, 8, PREVIOUS_SIZE, PREVIOUS_SIZE + 3, full + 4, 64):
        for junk in (2, -1, 0x7fffffff):
            st, msg = _create(vl, ext(vl, size, junk, 0, 0, 0, 0))
            assert st == expected, (size, junk, msg)
    # ... while the previous size's own fields are still checked
    assert _create(vl, ext(vl, PREVIOUS_SIZE, 0, 0, -1, 0, 0))[0] == vl.ERR_INVALID
    assert _create(vl, ext(vl, PREVIOUS_SIZE, 0, 0, 0, 0, 2))[0] == vl.ERR_INVALID
    assert _create(vl, vl.Limits(PREVIOUS_SIZE, 0, 1, 0, 1))[0] == expected
    for size in (4, 12, 16, 19, -8):
        st, msg = _create(vl, ext(vl, size, 0, 0, 0, 0, 0))
        assert st == vl.ERR_INVALID and b"struct_size 0, 8 or >= 20" in msg, (size, msg)


def test_getters_refuse_a_null_handle(vl):
    L = vl.lib()
    p, b = C.c_void_p(), C.c_longlong(0)
    rows = np.zeros(1, dtype=vl.SWEEP_RECORD_DTYPE)
    assert L.vloam_get_sweep_log(None, 0, 1, rows.ctypes.data_as(C.c_void_p)) == vl.ERR_INVALID
    assert L.vloam_sweep_log_device_ptr(None, C.byref(p), C.byref(b)) == vl.ERR_INVALID
