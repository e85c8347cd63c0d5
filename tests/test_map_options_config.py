"""CPU: the opt-in growable voxel map — vloam_map_options, vloam_create_with_options and its argument check (before any device call).
The GPU side: tests/test_gpu_map_growth.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(map_capacity_log2=12, max_points=4096)   # (the check is what is tested, not the arena)


def header():
    return open(os.path.join(ROOT, "include", "vloam_hip", "c_api.h")).read()


def _create(vl, opt, lim=None, n_sessions=1, with_options=True, **cfg):
    L = vl.lib()
    h = C.c_void_p()
    c = vl.default_config(**dict(SMALL, **cfg))
    lim_p = None if lim is None else C.byref(lim)
    if with_options:
        st = L.vloam_create_with_options(C.byref(c), lim_p, None if opt is None else C.byref(opt), 0, n_sessions, C.byref(h))
    else:
        st = L.vloam_create_with_limits(C.byref(c), lim_p, 0, n_sessions, C.byref(h))
    msg = L.vloam_last_error()
    if st == vl.VLOAM_OK:
        L.vloam_destroy(h)
    return st, msg


def test_struct_size_defaults_and_exports(vl):
    text = header()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct vloam_map_options \{(.*?)\} vloam_map_options;", text, flags=re.S).group(1), flags=re.S)
    assert re.findall(r"\b(\w+)\s+(\w+);", body) == [("int", "struct_size"), ("int", "grow"), ("int", "max_capacity_log2")]
    assert [(n, t) for n, t in vl.MapOptions._fields_] == [("struct_size", C.c_int), ("grow", C.c_int), ("max_capacity_log2", C.c_int)]
    assert C.sizeof(vl.MapOptions) == 12
    opt = vl.default_map_options()
    assert (opt.struct_size, opt.grow, opt.max_capacity_log2) == (12, 0, 28)
    L = vl.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert hasattr(L, "vloam_default_map_options") and re.search(r"void\s+vloam_default_map_options\(vloam_map_options\*", plain)
    assert hasattr(L, "vloam_create_with_options")
    assert re.search(r"vloam_status\s+vloam_create_with_options\(const vloam_config\*\s*\w*,\s*const vloam_limits\*\s*\w*,\s*const vloam_map_options\*", plain)
    # vloam_limits and its extension are what they were: the option did not go into another vloam_limits* size
    assert C.sizeof(vl.Limits) == 20 and C.sizeof(vl.LimitsExt) == 24


@pytest.mark.parametrize("n_sessions", [1, 2])
def test_null_options_and_grow_0_are_create_with_limits(vl, n_sessions):
    """Accepted forms answer what vloam_create_with_limits answers here (without a GPU: VLOAM_ERR_NO_DEVICE, which comes after the check)."""
    expected, _ = _create(vl, None, n_sessions=n_sessions, with_options=False)
    assert expected in (vl.VLOAM_OK, vl.ERR_NO_DEVICE)
    for lim in (None, vl.default_limits(), vl.default_limits(map_pub_number=2), vl.default_limits_ext(sweep_log=1).limits):
        assert _create(vl, None, lim, n_sessions)[0] == expected
        assert _create(vl, vl.default_map_options(), lim, n_sessions)[0] == expected
        assert _create(vl, vl.default_map_options(grow=0, max_capacity_log2=0), lim, n_sessions)[0] == expected
        assert _create(vl, vl.default_map_options(grow=0, max_capacity_log2=12), lim, n_sessions)[0] == expected
    # grow = 0 with with_mapping == 0 is an ordinary handle too
    assert _create(vl, vl.default_map_options(), n_sessions=n_sessions, with_mapping=0)[0] == _create(vl, None, n_sessions=n_sessions, with_options=False, with_mapping=0)[0]
    # the limits inside are checked as ever
    assert _create(vl, vl.default_map_options(), vl.default_limits(map_pub_number=-1), n_sessions)[0] == vl.ERR_INVALID


def test_accepted_growable_forms(vl):
    expected, _ = _create(vl, None, with_options=False)
    for kw, cfg in [(dict(grow=1), {}), (dict(grow=1, max_capacity_log2=0), {}), (dict(grow=1, max_capacity_log2=12), {}), (dict(grow=1, max_capacity_log2=28), {}),
                    (dict(grow=1, max_capacity_log2=10), dict(map_capacity_log2=3)),      # the start size is clamped to 10 first
                    (dict(grow=1, max_capacity_log2=28), dict(map_capacity_log2=40))]:    # ... and to 28
        st, msg = _create(vl, vl.default_map_options(**kw), **cfg)
        assert st == expected, (kw, cfg, msg)
    st, msg = _create(vl, vl.default_map_options(grow=1, max_capacity_log2=20), vl.default_limits(map_pub_number=5, publish_registered_cloud=1))
    assert st == expected, msg


def test_refusals_each_with_its_own_message(vl):
    for size in (0, 8, 11, 16, 20, -12):
        st, msg = _create(vl, vl.MapOptions(size, 0, 0))
        assert st == vl.ERR_INVALID and b"vloam_map_options" in msg and b"struct_size must be 12" in msg, (size, msg)
    for grow in (2, -1, 0x7fffffff):
        st, msg = _create(vl, vl.default_map_options(grow=grow))
        assert st == vl.ERR_INVALID and b"grow must be 0 or 1" in msg, (grow, msg)
    for cap in (11, 9, 1, -1, 29, 64):   # below the start size (SMALL: 12), or beyond 28
        for grow in (0, 1):
            st, msg = _create(vl, vl.default_map_options(grow=grow, max_capacity_log2=cap))
            assert st == vl.ERR_INVALID and b"max_capacity_log2" in msg and b"(12) .. 28" in msg, (cap, msg)
    st, msg = _create(vl, vl.default_map_options(grow=1, max_capacity_log2=27), map_capacity_log2=40)   # the start size clamps to 28
    assert st == vl.ERR_INVALID and b"(28) .. 28" in msg, msg
    for n_sessions, cfg in [(2, {}), (8, {}), (1, dict(with_mapping=0)), (3, dict(with_mapping=0))]:
        st, msg = _create(vl, vl.default_map_options(grow=1), n_sessions=n_sessions, **cfg)
        assert st == vl.ERR_INVALID and b"grow = 1 needs a single-sequence handle" in msg and b"with_mapping" in msg, (n_sessions, cfg, msg)
    # the three messages are three texts
    texts = {_create(vl, vl.MapOptions(8, 0, 0))[1], _create(vl, vl.default_map_options(grow=2))[1], _create(vl, vl.default_map_options(grow=1), n_sessions=2)[1]}
    assert len(texts) == 3
    # null arguments as ever
    L = vl.lib()
    assert L.vloam_create_with_options(None, None, None, 0, 1, C.byref(C.c_void_p())) == vl.ERR_INVALID


def test_wrapper_passes_the_options(vl):
    with pytest.raises(vl.VloamError) as e:
        vl.Handle(0, n_sessions=2, map_grow=1, **SMALL)
    assert e.value.status == vl.ERR_INVALID and "grow = 1" in str(e.value)
    with pytest.raises(vl.VloamError) as e:
        vl.Handle(0, map_grow=1, map_max_capacity_log2=11, **SMALL)
    assert e.value.status == vl.ERR_INVALID and "max_capacity_log2" in str(e.value)
