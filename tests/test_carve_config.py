"""CPU: map clean-up — vloam_carve_options / vloam_carve_result, the entry points, the defaults, and the option check (before any device call,
before the handle is looked at: every refusal is made with a NULL handle).  The GPU side: tests/test_gpu_carve.py."""
import ctypes as C
import re

import numpy as np

from test_sweep_log_config import header

OPT_SIZE, RESULT_SIZE = 48, 104


def struct_fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    out = []
    for t, names in re.findall(r"\b(int|float|double|long long)\s+([^;]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)):
        for n in names.split(","):
            m = re.match(r"\s*([a-zA-Z_0-9]+)((?:\s*\[\d+\])*)\s*$", n)
            out.append((t, m.group(1), tuple(int(d) for d in re.findall(r"\[(\d+)\]", m.group(2)))))
    return out


def test_structs_defaults_and_exports(vl):
    text = header()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = struct_fields(text, "vloam_carve_options")
    assert [f[1] for f in decl] == [n for n, _ in vl.CarveOptions._fields_]
    ctype = {"int": C.c_int, "float": C.c_float}
    assert [ctype[t] for t, _, _ in decl] == [c for _, c in vl.CarveOptions._fields_]
    assert C.sizeof(vl.CarveOptions) == OPT_SIZE
    dt = vl.CARVE_RESULT_DTYPE
    decl = struct_fields(text, "vloam_carve_result")
    assert [f[1] for f in decl] == list(dt.names) and all(t == "long long" for t, _, _ in decl)
    off = 0
    for _, n, shape in decl:
        sub, o = dt.fields[n][0], dt.fields[n][1]
        assert o == off and sub.base == np.dtype("<i8") and sub.shape == shape, n
        off += 8 * int(np.prod(shape, dtype=int))
    assert off == dt.itemsize == RESULT_SIZE
    L = vl.lib()
    assert hasattr(L, "vloam_default_carve_options") and re.search(r"void\s+vloam_default_carve_options\(vloam_carve_options\*", plain)
    for sym in ("vloam_map_carve", "vloam_map_carve_device"):
        assert hasattr(L, sym), sym
        assert re.search(r"vloam_status\s+%s\(vloam_handle\*\s*h," % sym, plain), sym
    opt = vl.CarveOptions(*([-1] * 12))
    L.vloam_default_carve_options(C.byref(opt))
    got = {n: getattr(opt, n) for n, _ in vl.CarveOptions._fields_}
    assert got == dict(struct_size=OPT_SIZE, kind_mask=3, rows=64, cols=1024, elev_min_deg=-25.0, elev_max_deg=3.0, min_range=2.0, max_range=80.0,
                       range_res=np.float32(0.05), margin=0.5, min_votes=1, apply=0)
    # the clean-up kernels are launched outside the per-kernel profile table: ids and count are what they were
    L.vloam_profile_kernel_name.restype = C.c_char_p
    names = [L.vloam_profile_kernel_name(k).decode() for k in range(L.vloam_profile_kernel_count())]
    assert names[-2:] == ["k_pose_info_lo", "k_pose_info_map"] and not [n for n in names if n.startswith("k_carve")]


def test_every_option_refusal_with_a_null_handle(vl):
    L = vl.lib()
    sweep = np.ones((8, 4), np.float32)
    removed = np.zeros((4, 4), np.float32)
    res = np.zeros(1, vl.CARVE_RESULT_DTYPE)
    pose = np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]])
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    NOARG = object()

    def call(n_sweeps=1, ns=NOARG, clouds=NOARG, poses=pose, out=removed, cap=4, result=res, **fields):
        opt = vl.CarveOptions()
        L.vloam_default_carve_options(C.byref(opt))
        for k, v in fields.items():
            setattr(opt, k, v)
        m = max(n_sweeps, 1)
        ptrs = (C.c_void_p * m)(*([sweep.ctypes.data] * m)) if clouds is NOARG else clouds
        n = (C.c_int * m)(*([8] * m)) if ns is NOARG else ns
        got = []
        for fn in (L.vloam_map_carve, L.vloam_map_carve_device):
            st = fn(None, C.byref(opt), ptrs, n, P(poses), n_sweeps, P(out), C.c_longlong(cap), P(result))
            got.append((st, L.vloam_last_error()))
        assert got[0][0] == got[1][0] and got[0][1].split(b":", 1)[1] == got[1][1].split(b":", 1)[1], got
        assert got[0][1].startswith(b"vloam_map_carve:") and got[1][1].startswith(b"vloam_map_carve_device:")
        return got[0]

    seen = set()

    def refused(what, **kw):
        st, msg = call(**kw)
        assert st == vl.ERR_INVALID and what in msg and b"null handle" not in msg, (kw, msg)
        seen.add(msg.split(b":", 1)[1].strip()[:20])

    # accepted arguments get as far as the (null) handle
    poses16 = np.tile(pose, (16, 1))
    for kw in (dict(), dict(poses=None), dict(n_sweeps=16, poses=poses16), dict(rows=1, cols=4), dict(rows=1024, cols=1024), dict(out=None, cap=0),
               dict(ns=(C.c_int * 1)(0), clouds=(C.c_void_p * 1)(None)), dict(kind_mask=1, apply=1, min_votes=16), dict(ns=(C.c_int * 1)(262144))):
        st, msg = call(**kw)
        assert st == vl.ERR_INVALID and b"null handle" in msg, (kw, msg)
    for size in (0, 44, 52, -OPT_SIZE):
        refused(b"struct_size must be 48", struct_size=size)
    for km in (0, 4, -1):
        refused(b"kind_mask must be", kind_mask=km)
    for rc in ((0, 1024), (64, 3), (1025, 1024), (2048, 1024), (-1, 8)):
        refused(b"rows * cols > 2^20", rows=rc[0], cols=rc[1])
    for e in ((float("nan"), 3.0), (-25.0, float("inf")), (-91.0, 3.0), (-25.0, 91.0), (3.0, 3.0), (3.0, -25.0)):
        refused(b"elevations", elev_min_deg=e[0], elev_max_deg=e[1])
    for r in ((0.0, 80.0), (-1.0, 80.0), (80.0, 80.0), (2.0, float("inf")), (float("nan"), 80.0)):
        refused(b"0 < min_range < max_range", min_range=r[0], max_range=r[1])
    for rr in (0.0, -0.05, float("nan"), float("inf"), 1e-9):
        refused(b"range_res", range_res=rr)
    for mg in (-0.1, float("nan"), float("inf"), 1e9):
        refused(b"margin", margin=mg)
    for mv in (0, 17, -1):
        refused(b"min_votes must be 1 .. 16", min_votes=mv)
    for ap in (-1, 2):
        refused(b"apply must be 0", apply=ap)
    for ns in (0, 17, -1):
        refused(b"n_sweeps must be 1 .. 16", n_sweeps=ns, poses=np.tile(pose, (17, 1)))
    refused(b"null array", clouds=None)
    refused(b"null array", ns=None)
    refused(b"0 .. 262144", ns=(C.c_int * 1)(262145))
    refused(b"0 .. 262144", ns=(C.c_int * 1)(-1))
    refused(b"null sweep pointer 1", n_sweeps=2, clouds=(C.c_void_p * 2)(sweep.ctypes.data, None), poses=np.tile(pose, (2, 1)))
    refused(b"with n_sweeps == 1 only", n_sweeps=2, poses=None)
    for bad in (float("nan"), float("inf")):
        for k in range(7):
            p = np.tile(pose, (2, 1))
            p[1, k] = bad
            refused(b"pose 1, component %d is not finite" % k, n_sweeps=2, poses=p)
    for q in ([0.0, 0.0, 0.0, 1.0 + 2e-6], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0]):
        refused(b"within 1e-6 of 1", poses=np.array([q + [0.0, 0.0, 0.0]]))
    refused(b"a list of -1 points", cap=-1)
    refused(b"a list of 4 points at a null address", out=None)
    refused(b"null result", result=None)
    assert len(seen) >= 17, seen   # each kind of refusal has its own text
    # the first offence listed is the one reported
    assert b"struct_size" in call(struct_size=0, kind_mask=0, rows=0, n_sweeps=0, result=None)[1]
    assert b"kind_mask" in call(kind_mask=0, rows=0, n_sweeps=0, result=None)[1]
    assert b"rows" in call(rows=0, min_votes=0, n_sweeps=0, result=None)[1]
    assert b"min_votes" in call(min_votes=0, n_sweeps=0, result=None)[1]
    assert b"n_sweeps" in call(n_sweeps=0, result=None)[1]
    assert L.vloam_map_carve(None, None, None, None, None, 1, None, C.c_longlong(0), None) == vl.ERR_INVALID and b"null options" in L.vloam_last_error()
