"""CPU: localisation — vloam_localize_options / vloam_localize_result, the entry points, and the option check (before any device call,
before the handle is looked at: every refusal is made with a NULL handle).  The GPU side: tests/test_gpu_localize.py."""
import ctypes as C
import re

import numpy as np

from test_sweep_log_config import header

OPT_SIZE, RESULT_SIZE = 16, 216
N_CORNER_MAX = 7680


def fields_nd(text, name):
    """[(C type, field, shape tuple)] of a typedef'd struct of the header, comments stripped, `int a[2], b[2][2];` lists expanded."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    out = []
    for t, names in re.findall(r"\b(int|double|float)\s+([^;]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)):
        for n in names.split(","):
            m = re.match(r"\s*([a-zA-Z_0-9]+)((?:\s*\[\d+\])*)\s*$", n)
            out.append((t, m.group(1), tuple(int(d) for d in re.findall(r"\[(\d+)\]", m.group(2)))))
    return out


def test_structs_and_exports(vl):
    text = header()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert fields_nd(text, "vloam_localize_options") == [("int", "struct_size", ()), ("int", "pose_frame", ()), ("int", "reserved", (2,))]
    assert [n for n, _ in vl.LocalizeOptions._fields_] == ["struct_size", "pose_frame", "reserved"]
    assert C.sizeof(vl.LocalizeOptions) == OPT_SIZE and vl.LocalizeOptions.reserved.offset == 8
    # the result record against its numpy mirror: names, types, shapes in order; C layout rules give the offsets
    dt = vl.LOCALIZE_RESULT_DTYPE
    size = {"int": 4, "double": 8}
    code = {"int": "<i4", "double": "<f8"}
    off = 0
    decl = fields_nd(text, "vloam_localize_result")
    assert [f[1] for f in decl] == list(dt.names)
    for t, n, shape in decl:
        off = (off + size[t] - 1) // size[t] * size[t]
        sub, o = dt.fields[n][0], dt.fields[n][1]
        assert o == off and sub.base == np.dtype(code[t]) and sub.shape == shape, (n, o, off, sub)
        off += size[t] * int(np.prod(shape, dtype=int))
    assert off == dt.itemsize == RESULT_SIZE
    assert dt.fields["q_guess"][1] == 72 and dt.fields["final_cost"][1] == 200
    # ints first, then doubles
    kinds = [t for t, _, _ in decl]
    assert kinds == sorted(kinds, key=lambda k: k != "int")
    assert (vl.LOC_SOLVED, vl.LOC_NOT_OPTIMIZED, vl.LOC_WOULD_ROLL, vl.LOC_DEGRADED) == (1, 2, 4, 8)
    for name, val in (("SOLVED", 1), ("NOT_OPTIMIZED", 2), ("WOULD_ROLL", 4), ("DEGRADED", 8)):
        assert re.search(r"VLOAM_LOC_%s\s*=\s*%d\b" % (name, val), plain), name
    L = vl.lib()
    assert hasattr(L, "vloam_default_localize_options") and re.search(r"void\s+vloam_default_localize_options\(vloam_localize_options\*", plain)
    for sym in ("vloam_map_localize", "vloam_map_localize_device"):
        assert hasattr(L, sym), sym
        assert re.search(r"vloam_status\s+%s\(vloam_handle\*\s*h," % sym, plain), sym
    opt = vl.LocalizeOptions(-1, -1, (C.c_int * 2)(-1, -1))
    L.vloam_default_localize_options(C.byref(opt))
    assert (opt.struct_size, opt.pose_frame, list(opt.reserved)) == (OPT_SIZE, 0, [0, 0])
    # the localisation kernels are launched outside the per-kernel profile table: ids and count are what they were
    L.vloam_profile_kernel_name.restype = C.c_char_p
    names = [L.vloam_profile_kernel_name(k).decode() for k in range(L.vloam_profile_kernel_count())]
    assert names[-2:] == ["k_pose_info_lo", "k_pose_info_map"] and not [n for n in names if n.startswith("k_map_loc")]


def test_every_option_refusal_with_a_null_handle(vl):
    L = vl.lib()
    corner, surf = np.ones((6, 4), np.float32), np.ones((9, 4), np.float32)
    out = np.zeros(1, vl.LOCALIZE_RESULT_DTYPE)
    q0, t0 = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(fields=(OPT_SIZE, 0, 0, 0), c=corner, s=surf, nc=None, ns=None, q=q0, t=t0, res=out, host_only=False):
        opt = vl.LocalizeOptions(fields[0], fields[1], (C.c_int * 2)(fields[2], fields[3]))
        nc = (0 if c is None else c.shape[0]) if nc is None else nc
        ns = (0 if s is None else s.shape[0]) if ns is None else ns
        got = []
        for fn in (L.vloam_map_localize,) if host_only else (L.vloam_map_localize, L.vloam_map_localize_device):
            st = fn(None, C.byref(opt), P(c), nc, P(s), ns, P(q), P(t), P(res))
            got.append((st, L.vloam_last_error()))
        if not host_only:
            assert got[0][0] == got[1][0]
            assert got[0][1].split(b":", 1)[1] == got[1][1].split(b":", 1)[1], got   # same refusal, each under its own name
            assert got[1][1].startswith(b"vloam_map_localize_device:")
        assert got[0][1].startswith(b"vloam_map_localize:")
        return got[0]

    seen = set()

    def refused(what, **kw):
        st, msg = call(**kw)
        assert st == vl.ERR_INVALID and what in msg and b"null handle" not in msg, (kw, msg)
        seen.add(msg.split(b":", 1)[1].strip()[:24])
        return msg

    # accepted options get as far as the (null) handle: foreign clouds in both pose frames, the sweep in progress with and without a pose
    for kw in (dict(), dict(fields=(OPT_SIZE, 1, 0, 0)), dict(c=None, s=None), dict(c=None, s=None, q=None, t=None),
               dict(nc=0, ns=0), dict(c=np.ones((N_CORNER_MAX, 4), np.float32))):
        st, msg = call(**kw)
        assert st == vl.ERR_INVALID and b"null handle" in msg, (kw, msg)
    for size in (0, 8, 12, 20, -OPT_SIZE):
        refused(b"struct_size must be 16", fields=(size, 0, 0, 0))
    for pf in (-1, 2, 1 << 30):
        refused(b"pose_frame must be 0", fields=(OPT_SIZE, pf, 0, 0))
    refused(b"reserved must be 0", fields=(OPT_SIZE, 0, 1, 0))
    refused(b"reserved must be 0", fields=(OPT_SIZE, 0, 0, -1))
    refused(b"corner AND surf", c=None)
    refused(b"corner AND surf", s=None)
    refused(b"q AND t", q=None)
    refused(b"q AND t", t=None)
    refused(b"null pose goes with null clouds", q=None, t=None)
    refused(b"negative cloud size", nc=-1)
    refused(b"negative cloud size", ns=-5)
    big = np.ones((N_CORNER_MAX + 1, 4), np.float32)
    refused(b"the corner cloud takes 7680", c=big)
    refused(b"the corner cloud takes 7680", ns=(1 << 24) + 1)   # (refused by its count: the array is not read)
    refused(b"null result", res=None)
    for bad in (float("nan"), float("inf"), float("-inf")):
        for arr, which in ((corner, b"corner cloud, point 3"), (surf, b"surf cloud, point 3")):
            a = arr.copy()
            a[3, 2] = bad
            st, msg = call(host_only=True, **({"c": a} if arr is corner else {"s": a}))
            assert st == vl.ERR_INVALID and which in msg and b"not finite" in msg, msg
        for k in range(7):
            q, t = q0.copy(), t0.copy()
            (q if k < 4 else t)[k % 4 if k < 4 else k - 4] = bad
            refused(b"is not finite", q=q, t=t)
            refused(b"is not finite", q=q, t=t, c=None, s=None)
    seen.add(b"cloud not finite")
    for q in ([0.0, 0.0, 0.0, 1.0 + 2e-6], [0.0, 0.0, 0.0, 0.0], [0.5, 0.5, 0.5, 0.5 - 4e-6], [1.0, 1.0, 0.0, 0.0]):
        refused(b"within 1e-6 of 1", q=np.array(q))
    st, msg = call(q=np.array([0.5, 0.5, 0.5, 0.5 + 1e-7]))   # inside the bound
    assert b"null handle" in msg
    assert len(seen) >= 11, seen   # each kind of refusal has its own text
    # the order of the checks: the first offence listed is the one reported
    assert b"struct_size" in call(fields=(0, 7, 1, 1), c=None, nc=-1, q=None, res=None)[1]
    assert b"pose_frame" in call(fields=(OPT_SIZE, 7, 1, 1), c=None, nc=-1, q=None, res=None)[1]
    assert b"reserved" in call(fields=(OPT_SIZE, 0, 1, 1), c=None, nc=-1, q=None, res=None)[1]
    assert b"corner AND surf" in call(c=None, nc=-1, q=None, res=None)[1]
    assert b"q AND t" in call(nc=-1, q=None, res=None)[1]
    assert b"negative" in call(nc=-1, res=None)[1]
    assert b"null result" in call(res=None, q=np.array([0.0, 0.0, 0.0, 2.0]))[1]
    assert L.vloam_map_localize(None, None, P(corner), 6, P(surf), 9, P(q0), P(t0), P(out)) == vl.ERR_INVALID and b"null options" in L.vloam_last_error()
