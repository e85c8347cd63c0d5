"""CPU: the opt-in surf stack capacity vloam_limits::max_surf_stack_points (large stack tier), its entry point and argument check, and the
inputs the GPU tests of the tier run on (tests/test_gpu_surf_stack.py): a 64-line street drive at a 0.2 m plane leaf."""
import ctypes as C
import os
import re

import pytest

import surf_stack_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT, TOP = 24576, 131072


def test_header_declares_and_library_exports_the_limits(vl):
    text = open(os.path.join(ROOT, "include", "vloam_hip", "c_api.h")).read()
    body = re.search(r"typedef struct vloam_limits \{(.*?)\} vloam_limits;", text, flags=re.S).group(1)
    fields = re.findall(r"\b(int|double|float)\s+([a-zA-Z_0-9]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    ctype = {"int": C.c_int, "double": C.c_double, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(vl.Limits._fields_)
    assert fields[0][1] == "struct_size" and fields[1][1] == "max_surf_stack_points"
    assert re.search(r"void\s+vloam_default_limits\(vloam_limits\*\s*lim\);", text)
    assert re.search(r"vloam_status\s+vloam_create_with_limits\(const vloam_config\*\s*cfg,\s*const vloam_limits\*\s*lim,\s*int device,\s*int n_sessions,\s*vloam_handle\*\*\s*out\);", text)
    L = vl.lib()
    for sym in ("vloam_default_limits", "vloam_create_with_limits"):
        assert hasattr(L, sym), sym
    # vloam_config did not grow
    assert vl.Config._fields_[-1][0] == "max_ring_points"


def test_default_limits(vl):
    lim = vl.default_limits()
    assert lim.max_surf_stack_points == DEFAULT == vl.K_STACK_CAP_SURF
    assert lim.struct_size == C.sizeof(vl.Limits)


def _create(vl, lim, n_sessions, **cfg):
    L = vl.lib()
    h = C.c_void_p()
    st = L.vloam_create_with_limits(C.byref(vl.default_config(**cfg)), None if lim is None else C.byref(lim), 0, n_sessions, C.byref(h))
    return st, h, L.vloam_last_error()


@pytest.mark.parametrize("n_sessions", [1, 2])
def test_max_surf_stack_points_argument_check(vl, n_sessions):
    """0 (= 24576), 24576 and multiples of 8192 up to 131072 pass the check (without a GPU: VLOAM_ERR_NO_DEVICE, which comes after it);
    anything else is refused before any device call, with both ends of the range in the message."""
    L = vl.lib()
    # (a small voxel table: the check is what is tested, not the arena)
    small = dict(map_capacity_log2=12, max_points=TOP)
    # with a device or without one: what the library's own default creation answers (the HIP runtime decides, whatever other frameworks see)
    expected, h, _ = _create(vl, None, n_sessions, **small)
    assert expected in (vl.VLOAM_OK, vl.ERR_NO_DEVICE)
    if expected == vl.VLOAM_OK:
        L.vloam_destroy(h)
    for v in (0, DEFAULT, 32768, 65536, TOP):
        st, h, _ = _create(vl, vl.default_limits(max_surf_stack_points=v), n_sessions, **small)
        assert st == expected, v
        if st == vl.VLOAM_OK:
            L.vloam_destroy(h)
    refused = [(vl.default_limits(max_surf_stack_points=v), small) for v in (-1, 1, DEFAULT - 1, 30000, TOP + 8192)]
    refused.append((vl.default_limits(max_surf_stack_points=65536), dict(map_capacity_log2=12, max_points=40000)))
    refused.append((vl.default_limits(struct_size=4), small))
    for lim, cfg in refused:
        st, _, msg = _create(vl, lim, n_sessions, **cfg)
        assert st == vl.ERR_INVALID, (lim.struct_size, lim.max_surf_stack_points, cfg)
        assert b"24576" in msg and b"131072" in msg, msg
    # the default capacity holds on a handle with fewer max_points than that, as it always has (only a LARGER capacity is tied to max_points)
    for lim in (None, vl.default_limits(), vl.default_limits(max_surf_stack_points=0)):
        st, h, _ = _create(vl, lim, n_sessions, map_capacity_log2=12, max_points=1024)
        assert st == expected
        if st == vl.VLOAM_OK:
            L.vloam_destroy(h)
    # struct_size 0 (a zero-initialised vloam_limits with one field set) is this header's size
    st, h, _ = _create(vl, vl.Limits(0, 32768), n_sessions, **small)
    assert st == expected
    if st == vl.VLOAM_OK:
        L.vloam_destroy(h)


@pytest.mark.parametrize("n_sessions", [1, 2])
def test_null_limits_behave_like_create_batch(vl, n_sessions):
    L = vl.lib()
    h = C.c_void_p()
    for cfg in (dict(), dict(max_ring_points=5), dict(scan_line=48)):
        a = L.vloam_create_batch(C.byref(vl.default_config(map_capacity_log2=12, **cfg)), 0, n_sessions, C.byref(h))
        msg_a = L.vloam_last_error()
        if a == vl.VLOAM_OK:
            L.vloam_destroy(h)
        b, h2, msg_b = _create(vl, None, n_sessions, map_capacity_log2=12, **cfg)
        if b == vl.VLOAM_OK:
            L.vloam_destroy(h2)
        assert a == b and msg_a == msg_b, cfg
        c, h3, _ = _create(vl, vl.default_limits(), n_sessions, map_capacity_log2=12, **cfg)
        if c == vl.VLOAM_OK:
            L.vloam_destroy(h3)
        assert c == a, cfg


def test_street_drive_at_a_20_cm_leaf_is_beyond_the_default_stack(synth, orc):
    """Oracle only.  The default 64 x 2048 street drive under a 0.2 / 0.2 m leaf: every sweep's surf stack lies in (24576, 32768] (measured:
    27 244 - 27 510), every corner stack below 8192 (measured: ~5 400 - 5 550) — the input of tests/test_gpu_surf_stack.py."""
    seq = synth.SynthSequence(**cases.STREET)
    o = orc.Oracle(line_res=cases.LEAF, plane_res=cases.LEAF)
    for k in range(6):
        assert o.process(seq.sweep(k)) == 0
        ns, nc = o.cloud(8).shape[0], o.cloud(7).shape[0]
        print("sweep %d: surf stack %d, corner stack %d" % (k, ns, nc))
        assert DEFAULT < ns <= 32768, (k, ns)
        assert nc < 8192, (k, nc)


def test_ground_lattice_is_one_point_per_voxel_and_gives_plane_factors(synth, orc):
    """Oracle only.  The constructed laserCloudSurfLast of the exact-capacity case: VoxelGrid(0.2) keeps every one of its 65 536 (65 537)
    points, and mapped after two ordinary sweeps the first outer round accepts at least 1 000 plane factors (measured: 5 978)."""
    rings, n_az = cases.LATTICE_SHAPE
    seq = synth.SynthSequence(n_rings=rings, n_azimuth=n_az, n_sweeps=40)
    G = cases.ground_lattice(synth, seq, 65536)
    assert orc.voxel_grid(G, cases.LEAF).shape[0] == 65536
    assert orc.voxel_grid(cases.ground_lattice(synth, seq, 65537), cases.LEAF).shape[0] == 65537
    o = orc.Oracle(line_res=cases.LEAF, plane_res=cases.LEAF)
    for k in range(cases.LATTICE_SWEEP):
        assert o.process(seq.sweep(k)) == 0
    assert o.stage_sr(seq.sweep(cases.LATTICE_SWEEP)) == 0
    o.stage_lo()
    assert o.stage_map(surf=G) == 0
    assert o.cloud(8).shape[0] == 65536 and o.map_num_outer() == 2
    n_plane = o.map_factors(0)[2].size
    print("plane factors accepted in outer round 0:", n_plane)
    assert n_plane >= 1000
