"""CPU: map import — vloam_map_import_options / vloam_map_import_result, the entry points, and the option check (before any device call, before
the handle is looked at: every refusal is made with a NULL handle).  The GPU side: tests/test_gpu_map_import.py."""
import ctypes as C
import re

import numpy as np

from test_sweep_log_config import header

OPT_SIZE, RESULT_SIZE = 72, 88
N_MAX = 16777216


def fields_nd(text, name):
    """[(C type, field, shape tuple)] of a typedef'd struct of the header, comments stripped, `long long a[2], b[2];` lists expanded."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    out = []
    for t, names in re.findall(r"\b(long long|int|double|float)\s+([^;]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)):
        for n in names.split(","):
            m = re.match(r"\s*([a-zA-Z_0-9]+)((?:\s*\[\d+\])*)\s*$", n)
            out.append((t, m.group(1), tuple(int(d) for d in re.findall(r"\[(\d+)\]", m.group(2)))))
    return out


def test_structs_and_exports(vl):
    text = header()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert fields_nd(text, "vloam_map_import_options") == [("int", "struct_size", ()), ("int", "reserved", (3,)), ("double", "q_wmap_wodom", (4,)),
                                                           ("double", "t_wmap_wodom", (3,))]
    O = vl.MapImportOptions
    assert [n for n, _ in O._fields_] == ["struct_size", "reserved", "q_wmap_wodom", "t_wmap_wodom"]
    assert C.sizeof(O) == OPT_SIZE and (O.reserved.offset, O.q_wmap_wodom.offset, O.t_wmap_wodom.offset) == (4, 16, 48)
    # the result record against its numpy mirror: names, types, shapes in order; C layout rules give the offsets
    dt = vl.MAP_IMPORT_RESULT_DTYPE
    size = {"int": 4, "long long": 8}
    code = {"int": "<i4", "long long": "<i8"}
    off = 0
    decl = fields_nd(text, "vloam_map_import_result")
    assert [f[1] for f in decl] == list(dt.names)
    for t, n, shape in decl:
        off = (off + size[t] - 1) // size[t] * size[t]
        sub, o = dt.fields[n][0], dt.fields[n][1]
        assert o == off and sub.base == np.dtype(code[t]) and sub.shape == shape, (n, o, off, sub)
        off += size[t] * int(np.prod(shape, dtype=int))
    assert off == dt.itemsize == RESULT_SIZE
    assert dt.fields["max_per_voxel"][1] == 64 and dt.fields["center_cube"][1] == 72
    L = vl.lib()
    assert hasattr(L, "vloam_default_map_import_options") and re.search(r"void\s+vloam_default_map_import_options\(vloam_map_import_options\*", plain)
    for sym in ("vloam_map_import", "vloam_map_import_device"):
        assert hasattr(L, sym), sym
        assert re.search(r"vloam_status\s+%s\(vloam_handle\*\s*h," % sym, plain), sym
    opt = O(-1, (C.c_int * 3)(-1, -1, -1), (C.c_double * 4)(7, 7, 7, 7), (C.c_double * 3)(7, 7, 7))
    L.vloam_default_map_import_options(C.byref(opt))
    assert (opt.struct_size, list(opt.reserved), list(opt.q_wmap_wodom), list(opt.t_wmap_wodom)) == (OPT_SIZE, [0, 0, 0], [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0])
    # the import kernels are launched outside the per-kernel profile table: ids and count are what they were
    L.vloam_profile_kernel_name.restype = C.c_char_p
    names = [L.vloam_profile_kernel_name(k).decode() for k in range(L.vloam_profile_kernel_count())]
    assert names[-2:] == ["k_pose_info_lo", "k_pose_info_map"] and not [n for n in names if n.startswith("k_map_import")]


def test_every_option_refusal_with_a_null_handle(vl):
    L = vl.lib()
    corner, surf = np.ones((6, 4), np.float32), np.ones((9, 4), np.float32)
    out = np.zeros(1, vl.MAP_IMPORT_RESULT_DTYPE)
    q0, t0 = (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0)
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(size=OPT_SIZE, reserved=(0, 0, 0), q=q0, t=t0, c=corner, s=surf, nc=None, ns=None, res=out, host_only=False):
        opt = vl.MapImportOptions(size, (C.c_int * 3)(*reserved), (C.c_double * 4)(*q), (C.c_double * 3)(*t))
        nc = (0 if c is None else c.shape[0]) if nc is None else nc
        ns = (0 if s is None else s.shape[0]) if ns is None else ns
        got = []
        for fn in (L.vloam_map_import,) if host_only else (L.vloam_map_import, L.vloam_map_import_device):
            st = fn(None, C.byref(opt), P(c), C.c_longlong(nc), P(s), C.c_longlong(ns), P(res))
            got.append((st, L.vloam_last_error()))
        if not host_only:
            assert got[0][0] == got[1][0]
            assert got[0][1].split(b":", 1)[1] == got[1][1].split(b":", 1)[1], got   # same refusal, each under its own name
            assert got[1][1].startswith(b"vloam_map_import_device:")
        assert got[0][1].startswith(b"vloam_map_import:")
        return got[0]

    seen = set()

    def refused(what, **kw):
        st, msg = call(**kw)
        assert st == vl.ERR_INVALID and what in msg and b"null handle" not in msg, (kw, msg)
        seen.add(msg.split(b":", 1)[1].strip()[:20])
        return msg

    # accepted options get as far as the (null) handle: both clouds, one, none; a transform away from the origin; a count at the limit (the
    # device form only: it does not read the array)
    for kw in (dict(), dict(c=None), dict(s=None), dict(c=None, s=None), dict(nc=0, ns=0), dict(q=(0.0, 0.0, 0.6, 0.8), t=(730.0, -410.0, 60.0))):
        st, msg = call(**kw)
        assert st == vl.ERR_INVALID and b"null handle" in msg, (kw, msg)
    opt = vl.MapImportOptions(OPT_SIZE, (C.c_int * 3)(0, 0, 0), (C.c_double * 4)(*q0), (C.c_double * 3)(*t0))
    assert L.vloam_map_import_device(None, C.byref(opt), P(corner), C.c_longlong(N_MAX), P(surf), C.c_longlong(9), P(out)) == vl.ERR_INVALID
    assert b"null handle" in L.vloam_last_error()
    for size in (0, 16, 64, 80, -OPT_SIZE):
        refused(b"struct_size must be 72", size=size)
    for r in ((1, 0, 0), (0, -1, 0), (0, 0, 1 << 20)):
        refused(b"reserved must be 0", reserved=r)
    for bad in (float("nan"), float("inf"), float("-inf")):
        for k in range(7):
            q, t = list(q0), list(t0)
            (q if k < 4 else t)[k if k < 4 else k - 4] = bad
            msg = refused(b"is not finite", q=q, t=t)
            assert (b"q_wmap_wodom[%d]" % k if k < 4 else b"t_wmap_wodom[%d]" % (k - 4)) in msg
        for arr, which in ((corner, b"corner cloud, point 3"), (surf, b"surf cloud, point 3")):
            a = arr.copy()
            a[3, 2] = bad
            st, msg = call(host_only=True, **({"c": a} if arr is corner else {"s": a}))
            assert st == vl.ERR_INVALID and which in msg and b"not finite" in msg, msg
    seen.add(b"cloud not finite")
    for q in ((0.0, 0.0, 0.0, 1.0 + 2e-6), (0.0, 0.0, 0.0, 0.0), (0.5, 0.5, 0.5, 0.5 - 4e-6), (1.0, 1.0, 0.0, 0.0)):
        refused(b"within 1e-6 of 1", q=q)
    assert b"null handle" in call(q=(0.5, 0.5, 0.5, 0.5 + 1e-7))[1]   # inside the bound
    refused(b"negative cloud size", nc=-1)
    refused(b"negative cloud size", ns=-5)
    refused(b"at most 16777216 points of a kind", nc=N_MAX + 1)   # (refused by its count: the array is not read)
    refused(b"at most 16777216 points of a kind", ns=1 << 40)
    assert b"null corner cloud" in refused(b"with a positive point count", c=None, nc=3)
    assert b"null surf cloud" in refused(b"with a positive point count", s=None, ns=1)
    refused(b"null result", res=None)
    assert len(seen) >= 9, seen   # each kind of refusal has its own text
    # the order of the checks: the first offence listed is the one reported
    nanq = (float("nan"), 0.0, 0.0, 1.0)
    assert b"struct_size" in call(size=0, reserved=(1, 1, 1), q=nanq, nc=-1, c=None, res=None)[1]
    assert b"reserved" in call(reserved=(1, 1, 1), q=nanq, nc=-1, c=None, res=None)[1]
    assert b"not finite" in call(q=nanq, nc=-1, c=None, res=None)[1]
    assert b"within 1e-6" in call(q=(0.0, 0.0, 0.0, 2.0), nc=-1, c=None, res=None)[1]
    assert b"negative" in call(nc=-1, c=None, res=None)[1]
    assert b"at most" in call(nc=N_MAX + 1, c=None, res=None)[1]
    assert b"positive point count" in call(c=None, nc=2, res=None)[1]
    assert L.vloam_map_import(None, None, P(corner), C.c_longlong(6), P(surf), C.c_longlong(9), P(out)) == vl.ERR_INVALID and b"null options" in L.vloam_last_error()
