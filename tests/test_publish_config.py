"""CPU: the opt-in published clouds of the mapping stream — vloam_limits::map_pub_number / max_published_map_points / publish_registered_cloud,
their entry points and the argument check (before any device call).  The GPU side: tests/test_gpu_publish.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FIELDS = ["map_pub_number", "max_published_map_points", "publish_registered_cloud"]
NEW_SYMBOLS = ["vloam_get_published_map", "vloam_get_published_cloud", "vloam_published_device_ptr"]
CAP_MIN, CAP_MAX, CAP_DEFAULT = 256, 16777216, 2097152
SMALL = dict(map_capacity_log2=12, max_points=4096)   # (the check is what is tested, not the arena)


def test_header_fields_and_exports(vl):
    text = open(os.path.join(ROOT, "include", "vloam_hip", "c_api.h")).read()
    body = re.search(r"typedef struct vloam_limits \{(.*?)\} vloam_limits;", text, flags=re.S).group(1)
    fields = re.findall(r"\b(int|double|float)\s+([a-zA-Z_0-9]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    ctype = {"int": C.c_int, "double": C.c_double, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(vl.Limits._fields_)
    assert [n for _, n in fields] == ["struct_size", "max_surf_stack_points"] + NEW_FIELDS
    assert C.sizeof(vl.Limits) == 20
    L = vl.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in NEW_SYMBOLS:
        assert hasattr(L, sym), sym
        assert re.search(r"vloam_status\s+%s\(vloam_handle\*\s*h," % sym, plain), sym
    # vloam_config did not grow: the header's fields are the 18 the wrapper mirrors, max_ring_points last, 80 bytes as compiled callers know it
    cbody = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct vloam_config \{(.*?)\} vloam_config;", text, flags=re.S).group(1), flags=re.S)
    cfields = re.findall(r"\b(?:int|double|float)\s+([a-zA-Z_0-9]+);", cbody)
    assert cfields == [f[0] for f in vl.Config._fields_] and len(cfields) == 18 and cfields[-1] == "max_ring_points"
    assert C.sizeof(vl.Config) == 80
    lim = vl.default_limits()
    assert lim.struct_size == 20 and lim.map_pub_number == 0 and lim.publish_registered_cloud == 0 and lim.max_published_map_points == CAP_DEFAULT


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
    ones VLOAM_ERR_INVALID with the allowed range in the message."""
    expected, _ = _create(vl, None, n_sessions)
    assert expected in (vl.VLOAM_OK, vl.ERR_NO_DEVICE)
    accepted = [dict(map_pub_number=1), dict(map_pub_number=20, max_published_map_points=0), dict(map_pub_number=1, max_published_map_points=CAP_MIN),
                dict(map_pub_number=3, max_published_map_points=65536), dict(publish_registered_cloud=1), dict(map_pub_number=2, publish_registered_cloud=1),
                dict(map_pub_number=0, max_published_map_points=5),        # the capacity is ignored while the map is not published
                dict(map_pub_number=0, max_published_map_points=-1)]
    for kw in accepted:
        st, msg = _create(vl, vl.default_limits(**kw), n_sessions)
        assert st == expected, (kw, msg)
    refused = [(dict(map_pub_number=-1), {}, [b"map_pub_number", b"0", b"1 .."]),
               (dict(map_pub_number=1, max_published_map_points=CAP_MIN - 1), {}, [b"256", b"16777216"]),
               (dict(map_pub_number=1, max_published_map_points=CAP_MAX + 1), {}, [b"256", b"16777216"]),
               (dict(map_pub_number=1, max_published_map_points=-5), {}, [b"256", b"16777216"]),
               (dict(publish_registered_cloud=2), {}, [b"publish_registered_cloud", b"0 or 1"]),
               (dict(publish_registered_cloud=-1), {}, [b"publish_registered_cloud", b"0 or 1"]),
               (dict(map_pub_number=1), dict(with_mapping=0), [b"with_mapping", b"map_pub_number", b"0 or 1"]),
               (dict(publish_registered_cloud=1), dict(with_mapping=0), [b"with_mapping", b"publish_registered_cloud", b"0 or 1"])]
    for kw, cfg, words in refused:
        st, msg = _create(vl, vl.default_limits(**kw), n_sessions, **cfg)
        assert st == vl.ERR_INVALID, (kw, cfg)
        assert all(w in msg for w in words), (kw, msg)
    # the products off on a handle without mapping: as before
    st, _ = _create(vl, vl.default_limits(), n_sessions, with_mapping=0)
    assert st == expected


def test_struct_size_versions(vl):
    expected, _ = _create(vl, None)
    # 0: this header's size, every field read
    st, _ = _create(vl, vl.Limits(0, 0, 1, 0, 1))
    assert st == expected
    st, _ = _create(vl, vl.Limits(0, 0, -1, 0, 0))
    assert st == vl.ERR_INVALID
    # 8: the first version of the struct; what lies behind max_surf_stack_points is not the caller's and is not read
    for junk in ((-1, -1, -1), (7, 3, 9), (0x7fffffff, 1, 2)):
        st, msg = _create(vl, vl.Limits(8, 0, *junk))
        assert st == expected, (junk, msg)
        st, _ = _create(vl, vl.Limits(8, 32768, *junk), max_points=32768)
        assert st == expected, junk
    st, _ = _create(vl, vl.Limits(8, 30000, 0, 0, 0))     # ... while its own field is still checked
    assert st == vl.ERR_INVALID
    # larger than this header's: a later version, the fields known here are read
    st, _ = _create(vl, vl.Limits(64, 0, 1, 0, 1))
    assert st == expected
    st, _ = _create(vl, vl.Limits(64, 0, 1, 5, 0))
    assert st == vl.ERR_INVALID
    # anything else is refused as it always was, with the same message
    for size in (4, 12, 16, 19, -8):
        st, msg = _create(vl, vl.Limits(size, 0, 0, 0, 0))
        assert st == vl.ERR_INVALID, size
        assert b"24576" in msg and b"131072" in msg and b"struct_size 0, 8 or >= 20" in msg, msg


def test_getters_refuse_a_null_handle(vl):
    L = vl.lib()
    n, nn, f, p = C.c_longlong(0), C.c_int(0), C.c_int(0), C.c_void_p()
    assert L.vloam_get_published_map(None, None, C.c_longlong(0), C.byref(n), C.byref(f)) == vl.ERR_INVALID
    assert L.vloam_get_published_cloud(None, None, 0, C.byref(nn), C.byref(f)) == vl.ERR_INVALID
    for which in (0, 1):
        assert L.vloam_published_device_ptr(None, which, C.byref(p), C.byref(n), C.byref(f)) == vl.ERR_INVALID
