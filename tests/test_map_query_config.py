"""CPU: map queries — vloam_map_query_options, the entry points, and the option check (before any device call, before the handle is looked
at: every refusal is made with a NULL handle).  The GPU side: tests/test_gpu_map_query.py."""
import ctypes as C
import re

import numpy as np

from test_sweep_log_config import header, struct_fields

SIZE = 20


def test_options_struct_and_exports(vl):
    text = header()
    ctype = {"int": C.c_int, "double": C.c_double, "float": C.c_float}
    assert [(n, ctype[t]) for t, n, _ in struct_fields(text, "vloam_map_query_options")] == list(vl.MapQueryOptions._fields_)
    assert C.sizeof(vl.MapQueryOptions) == SIZE and vl.MapQueryOptions.max_radius.offset == 16
    L = vl.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert hasattr(L, "vloam_default_map_query_options") and re.search(r"void\s+vloam_default_map_query_options\(vloam_map_query_options\*", plain)
    for sym in ("vloam_map_query", "vloam_map_query_device", "vloam_get_map_kind"):
        assert hasattr(L, sym), sym
        assert re.search(r"vloam_status\s+%s\(vloam_handle\*\s*h," % sym, plain), sym
    opt = vl.MapQueryOptions(-1, -1, -1, -1, -1.0)
    L.vloam_default_map_query_options(C.byref(opt))
    assert (opt.struct_size, opt.kind, opt.k, opt.reserved, opt.max_radius) == (SIZE, 2, 5, 0, 1.0)
    # the query kernel is launched outside the per-kernel profile table: ids and count are what they were
    L.vloam_profile_kernel_name.restype = C.c_char_p
    names = [L.vloam_profile_kernel_name(k).decode() for k in range(L.vloam_profile_kernel_count())]
    assert names[-2:] == ["k_pose_info_lo", "k_pose_info_map"] and "k_map_query" not in names


def test_every_option_refusal_with_a_null_handle(vl):
    L = vl.lib()
    q = np.zeros((4, 4), np.float32)
    out, d2, cnt = np.zeros((4, 8, 4), np.float32), np.zeros((4, 8), np.float32), np.zeros(4, np.int32)
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(fields, n=4, bufs=(q, out, d2, cnt)):
        opt = vl.MapQueryOptions(*fields)
        res = []
        for fn in (L.vloam_map_query, L.vloam_map_query_device):
            st = fn(None, C.byref(opt), P(bufs[0]), n, P(bufs[1]), P(bufs[2]), P(bufs[3]))
            res.append((st, L.vloam_last_error()))
        assert res[0][0] == res[1][0]
        assert res[0][1].split(b":", 1)[1] == res[1][1].split(b":", 1)[1], res   # same refusal, each under its own name
        assert res[0][1].startswith(b"vloam_map_query:") and res[1][1].startswith(b"vloam_map_query_device:")
        return res[0]

    # accepted options get as far as the (null) handle
    for ok in [(SIZE, 2, 5, 0, 1.0), (SIZE, 0, 1, 0, 1e-3), (SIZE, 1, 8, 0, 1e30)]:
        st, msg = call(ok)
        assert st == vl.ERR_INVALID and b"null handle" in msg, (ok, msg)
    st, msg = call((SIZE, 2, 5, 0, 1.0), n=0, bufs=(None, None, None, None))
    assert st == vl.ERR_INVALID and b"null handle" in msg, msg
    for size in (0, 16, 19, 24, -SIZE):
        st, msg = call((size, 2, 5, 0, 1.0))
        assert st == vl.ERR_INVALID and b"struct_size must be 20" in msg, (size, msg)
    for kind in (-1, 3, 1 << 30):
        st, msg = call((SIZE, kind, 5, 0, 1.0))
        assert st == vl.ERR_INVALID and b"kind must be" in msg, (kind, msg)
    for k in (0, -1, 9, 1 << 20):
        st, msg = call((SIZE, 2, k, 0, 1.0))
        assert st == vl.ERR_INVALID and b"k must be 1 .. 8" in msg, (k, msg)
    st, msg = call((SIZE, 2, 5, 1, 1.0))
    assert st == vl.ERR_INVALID and b"reserved" in msg, msg
    for r in (0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        st, msg = call((SIZE, 2, 5, 0, r))
        assert st == vl.ERR_INVALID and b"max_radius must be positive and finite" in msg, (r, msg)
    for missing in range(4):
        bufs = [q, out, d2, cnt]
        bufs[missing] = None
        st, msg = call((SIZE, 2, 5, 0, 1.0), bufs=bufs)
        assert st == vl.ERR_INVALID and b"null buffer" in msg, (missing, msg)
    st, msg = call((SIZE, 2, 5, 0, 1.0), n=-1)
    assert st == vl.ERR_INVALID and b"negative n" in msg, msg
    # the order of the checks: the first offence listed is the one reported
    st, msg = call((0, 7, 0, 1, -1.0), n=-1, bufs=(None, None, None, None))
    assert b"struct_size" in msg
    st, msg = call((SIZE, 7, 0, 1, -1.0), n=-1)
    assert b"kind must be" in msg
    st, msg = call((SIZE, 2, 0, 1, -1.0), n=-1)
    assert b"k must be" in msg
    st, msg = call((SIZE, 2, 5, 1, -1.0), n=-1)
    assert b"reserved" in msg
    st, msg = call((SIZE, 2, 5, 0, -1.0), n=-1)
    assert b"max_radius" in msg
    assert L.vloam_map_query(None, None, P(q), 4, P(out), P(d2), P(cnt)) == vl.ERR_INVALID and b"null options" in L.vloam_last_error()


def test_get_map_kind_refusals_need_no_device(vl):
    L = vl.lib()
    n = C.c_longlong(0)
    for kind in (-1, 2, 3):
        assert L.vloam_get_map_kind(None, kind, None, C.c_longlong(0), C.byref(n)) == vl.ERR_INVALID
        assert b"kind must be 0" in L.vloam_last_error()
    assert L.vloam_get_map_kind(None, 0, None, C.c_longlong(0), C.byref(n)) == vl.ERR_INVALID
