"""CPU: place recognition — the structs, the defaults, the exported entry points and every option refusal of c_api.h, each made with a NULL handle
(the options are checked before the handle is looked at, so no device is needed).  The GPU side: tests/test_gpu_place.py."""
import ctypes as C
import re

import numpy as np

import place_model as model
from test_sweep_log_config import header

P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
INF, NAN = float("inf"), float("nan")


def test_structs_defaults_and_exports(vl):
    assert C.sizeof(vl.PlaceOptions) == 36 and vl.PlaceOptions.min_range.offset == 16 and vl.PlaceOptions.reserved.offset == 32
    assert C.sizeof(vl.PlaceQueryOptions) == 16
    assert vl.PLACE_MATCH_DTYPE.itemsize == 32 and vl.PLACE_MATCH_DTYPE == model.MATCH_DTYPE
    L = vl.lib()
    plain = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for sym in ("vloam_place_enable", "vloam_place_describe", "vloam_place_describe_device", "vloam_place_add", "vloam_place_add_device", "vloam_place_count",
                "vloam_place_get", "vloam_place_load", "vloam_place_query", "vloam_place_query_device", "vloam_place_query_descriptor"):
        assert hasattr(L, sym), sym
        assert re.search(r"vloam_status\s+%s\(vloam_handle\*\s*h," % sym, plain), sym
    for sym in ("vloam_default_place_options", "vloam_default_place_query_options"):
        assert hasattr(L, sym) and re.search(r"void\s+%s\(" % sym, plain), sym
    for name, fields in (("vloam_place_options", "struct_size n_ring n_sector capacity min_range max_range z_min z_step reserved"),
                         ("vloam_place_query_options", "struct_size k exclude_last reserved")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), plain, flags=re.S).group(1)
        assert re.findall(r"\b([a-z_0-9]+)(?:\[\d+\])?;", body) == fields.split(), name
    o = vl.PlaceOptions(*([-1] * 4 + [-1.0] * 4 + [-1]))
    L.vloam_default_place_options(C.byref(o))
    assert (o.struct_size, o.n_ring, o.n_sector, o.capacity, o.reserved) == (36, 20, 60, 16384, 0)
    assert (o.min_range, o.max_range, o.z_min, o.z_step) == (0.0, 80.0, -3.0, float(np.float32(0.05)))
    q = vl.PlaceQueryOptions(-1, -1, -1, -1)
    L.vloam_default_place_query_options(C.byref(q))
    assert (q.struct_size, q.k, q.exclude_last, q.reserved) == (16, 1, 0, 0)
    # launched outside the per-kernel profile table: ids and count are what they were
    L.vloam_profile_kernel_name.restype = C.c_char_p
    names = [L.vloam_profile_kernel_name(k).decode() for k in range(L.vloam_profile_kernel_count())]
    assert not any(n.startswith("k_place") for n in names)


def popt(vl, **kw):
    o = vl.PlaceOptions()
    vl.lib().vloam_default_place_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_every_enable_refusal_with_a_null_handle(vl):
    L = vl.lib()

    def call(o):
        st = L.vloam_place_enable(None, None if o is None else C.byref(o))
        msg = L.vloam_last_error()
        assert msg.startswith(b"vloam_place_enable:"), msg
        return st, msg

    for ok in (popt(vl), popt(vl, n_ring=1, n_sector=1, capacity=1), popt(vl, n_ring=32, n_sector=120, capacity=1 << 20, min_range=1.0, max_range=1.5, z_min=-1e30, z_step=1e-30)):
        st, msg = call(ok)
        assert st == vl.ERR_INVALID and b"null handle" in msg, msg
    cases = [(None, b"null options"), (popt(vl, struct_size=32), b"struct_size must be 36"), (popt(vl, struct_size=40), b"struct_size must be 36"),
             (popt(vl, reserved=1), b"reserved must be 0"),
             (popt(vl, n_ring=0), b"n_ring must be 1 .. 32, not 0"), (popt(vl, n_ring=33), b"n_ring must be 1 .. 32, not 33"),
             (popt(vl, n_sector=0), b"n_sector must be 1 .. 120, not 0"), (popt(vl, n_sector=121), b"n_sector must be 1 .. 120, not 121"),
             (popt(vl, capacity=0), b"capacity must be 1 .. 1048576 rows, not 0"), (popt(vl, capacity=(1 << 20) + 1), b"capacity must be 1 .. 1048576 rows"),
             (popt(vl, max_range=0.0), b"max_range must be positive and finite"), (popt(vl, max_range=-1.0), b"max_range must be positive and finite"),
             (popt(vl, max_range=INF), b"max_range must be positive and finite"), (popt(vl, max_range=NAN), b"max_range must be positive and finite"),
             (popt(vl, z_step=0.0), b"z_step must be positive and finite"), (popt(vl, z_step=-0.05), b"z_step must be positive and finite"),
             (popt(vl, z_step=INF), b"z_step must be positive and finite"), (popt(vl, z_step=NAN), b"z_step must be positive and finite"),
             (popt(vl, z_min=NAN), b"z_min must be finite"), (popt(vl, z_min=-INF), b"z_min must be finite"),
             (popt(vl, min_range=-1.0), b"min_range must be finite and not negative"), (popt(vl, min_range=NAN), b"min_range must be finite and not negative"),
             (popt(vl, min_range=80.0), b"must be below max_range"), (popt(vl, min_range=90.0), b"must be below max_range")]
    for o, text in cases:
        st, msg = call(o)
        assert st == vl.ERR_INVALID and text in msg and b"null handle" not in msg, (text, msg)


def test_every_call_refusal_with_a_null_handle(vl):
    L = vl.lib()
    cloud, desc, info, tags = np.ones((5, 4), np.float32), np.zeros(300, np.uint32), np.zeros(2, np.int32), np.zeros(1, np.int32)
    out = np.zeros(8, vl.PLACE_MATCH_DTYPE)
    row, cnt = C.c_int(0), C.c_int(0)

    def qopt(size=16, k=1, exclude_last=0, reserved=0):
        return vl.PlaceQueryOptions(size, k, exclude_last, reserved)

    def run(name, *args):
        st = getattr(L, name)(None, *args)
        msg = L.vloam_last_error()
        assert msg.startswith(name.encode() + b":"), (name, msg)
        return st, msg

    # accepted arguments get as far as the (null) handle
    for name, args in (("vloam_place_describe", (P(cloud), 5, P(desc), P(info))), ("vloam_place_describe", (None, 0, P(desc), None)),
                       ("vloam_place_describe_device", (P(cloud), 5, P(desc), None)),
                       ("vloam_place_add", (P(cloud), 5, 7, C.byref(row))), ("vloam_place_add_device", (None, 0, 7, None)),
                       ("vloam_place_count", (C.byref(cnt),)), ("vloam_place_get", (0, 1, P(desc), None, None)), ("vloam_place_get", (0, 0, None, None, None)),
                       ("vloam_place_load", (P(desc), P(tags), 1)), ("vloam_place_load", (None, None, 0)),
                       ("vloam_place_query", (C.byref(qopt(k=8, exclude_last=1 << 30)), P(cloud), 5, P(out))),
                       ("vloam_place_query_device", (C.byref(qopt()), None, 0, P(out))),
                       ("vloam_place_query_descriptor", (C.byref(qopt()), P(desc), P(out)))):
        st, msg = run(name, *args)
        assert st == vl.ERR_INVALID and b"null handle" in msg, (name, msg)
    # the cloud, for every call that takes one
    for name, tail in (("vloam_place_describe", (P(desc), P(info))), ("vloam_place_describe_device", (P(desc), P(info))), ("vloam_place_add", (0, None)),
                       ("vloam_place_add_device", (0, None))):
        for n, ptr, text in ((-1, P(cloud), b"negative cloud size (-1 points)"), ((1 << 24) + 1, P(cloud), b"at most 16777216"), (5, None, b"null cloud with 5 points")):
            st, msg = run(name, ptr, n, *tail)
            assert st == vl.ERR_INVALID and text in msg, (name, msg)
    for name in ("vloam_place_query", "vloam_place_query_device"):
        for n, ptr, text in ((-1, P(cloud), b"negative cloud size"), ((1 << 24) + 1, P(cloud), b"at most 16777216"), (5, None, b"null cloud with 5 points")):
            st, msg = run(name, C.byref(qopt()), ptr, n, P(out))
            assert st == vl.ERR_INVALID and text in msg, (name, msg)
        st, msg = run(name, C.byref(qopt()), P(cloud), 5, None)
        assert st == vl.ERR_INVALID and b"null result" in msg, msg
    for name in ("vloam_place_describe", "vloam_place_describe_device"):
        st, msg = run(name, P(cloud), 5, None, P(info))
        assert st == vl.ERR_INVALID and b"null descriptor buffer" in msg, msg
    # the query options, for every form
    forms = (("vloam_place_query", (P(cloud), 5, P(out))), ("vloam_place_query_device", (P(cloud), 5, P(out))), ("vloam_place_query_descriptor", (P(desc), P(out))))
    for name, tail in forms:
        for o, text in ((None, b"null options"), (qopt(size=12), b"struct_size must be 16"), (qopt(reserved=2), b"reserved must be 0"),
                        (qopt(k=0), b"k must be 1 .. 8 matches, not 0"), (qopt(k=9), b"k must be 1 .. 8 matches, not 9"),
                        (qopt(exclude_last=-1), b"exclude_last must not be negative (-1)")):
            st, msg = run(name, None if o is None else C.byref(o), *tail)
            assert st == vl.ERR_INVALID and text in msg and b"null handle" not in msg, (name, msg)
    st, msg = run("vloam_place_query_descriptor", C.byref(qopt()), None, P(out))
    assert st == vl.ERR_INVALID and b"null descriptor" in msg, msg
    st, msg = run("vloam_place_query_descriptor", C.byref(qopt()), P(desc), None)
    assert st == vl.ERR_INVALID and b"null result" in msg, msg
    # count, get, load
    st, msg = run("vloam_place_count", None)
    assert st == vl.ERR_INVALID and b"null count" in msg, msg
    for first, count in ((-1, 1), (0, -1)):
        st, msg = run("vloam_place_get", first, count, P(desc), None, None)
        assert st == vl.ERR_INVALID and b"negative range" in msg, msg
    st, msg = run("vloam_place_get", 0, 1, None, P(tags), P(info))
    assert st == vl.ERR_INVALID and b"null descriptor buffer with 1 rows" in msg, msg
    st, msg = run("vloam_place_load", P(desc), P(tags), -1)
    assert st == vl.ERR_INVALID and b"negative row count (-1)" in msg, msg
    for d, t in ((None, P(tags)), (P(desc), None)):
        st, msg = run("vloam_place_load", d, t, 1)
        assert st == vl.ERR_INVALID and b"null buffer with 1 rows" in msg, msg
