"""CPU: the opt-in ring capacity vloam_config::max_ring_points (long ring tier), its argument check, and the hdl64e sensor model of synth."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_config_and_field_order(vl):
    assert vl.default_config().max_ring_points == 4096
    assert vl.Config._fields_[-1][0] == "max_ring_points"
    text = open(os.path.join(ROOT, "include", "vloam_hip", "c_api.h")).read()
    body = re.search(r"typedef struct vloam_config \{(.*?)\} vloam_config;", text, flags=re.S).group(1)
    fields = re.findall(r"\b(?:int|double|float)\s+([a-zA-Z_0-9]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields[-1] == "max_ring_points"


def test_max_ring_points_argument_check(vl):
    """0 (= 4096), 4096 .. 16384 pass the check (without a GPU: VLOAM_ERR_NO_DEVICE, which comes after it); anything else is refused
    before any device call, with the accepted range in the message."""
    import torch
    L = vl.lib()
    h = C.c_void_p()
    for v in (0, 4096, 8192, 16384):
        st = L.vloam_create(C.byref(vl.default_config(max_ring_points=v)), 0, C.byref(h))
        if torch.cuda.is_available():
            assert st == vl.VLOAM_OK, v
            L.vloam_destroy(h)
        else:
            assert st == vl.ERR_NO_DEVICE, v
    for v in (4095, 1, -1, 16385):
        assert L.vloam_create(C.byref(vl.default_config(max_ring_points=v)), 0, C.byref(h)) == vl.ERR_INVALID, v
        assert b"4096" in L.vloam_last_error() and b"16384" in L.vloam_last_error()
        assert L.vloam_create_batch(C.byref(vl.default_config(max_ring_points=v)), 0, 2, C.byref(h)) == vl.ERR_INVALID, v


def test_profile_names_the_long_tier(vl):
    L = vl.lib()
    L.vloam_profile_kernel_name.restype = C.c_char_p
    names = [L.vloam_profile_kernel_name(k).decode() for k in range(L.vloam_profile_kernel_count())]
    assert "k_sr_ring_long" in names


def test_hdl64e_sweeps_have_scan_lines_beyond_4096_points(synth, orc):
    """Under the oracle's own binning (atan(z / r) of the point, scan_registration.cpp:215-223) the default hdl64e head puts two lasers into
    a scan line twice, on every sweep: lines of 4 166 points."""
    seq = synth.SynthSequence(n_sweeps=3, sensor="hdl64e")
    assert seq.n_azimuth == synth.HDL64E_FIRINGS == 2083
    el, dz = synth.hdl64e_beams()
    nominal = np.concatenate([2.0 - np.arange(32) / 3.0, -8.83 - np.arange(32) / 2.0])
    assert np.all(np.abs(el - nominal) <= 0.15) and np.all(dz[:32] == 0.1) and np.all(dz[32:] == -0.1)
    o = orc.Oracle(with_mapping=False)
    for k in (0, 2):
        assert o.scan_registration(seq.sweep(k)) == 0
        per_line = np.bincount(o.cloud(0)[:, 3].astype(np.int64), minlength=64)
        assert np.count_nonzero(per_line > 4096) >= 2, per_line


def test_default_synthetic_sweeps_are_unchanged(synth):
    """The default sensor's sweeps stay bit for bit what the golden and parity tests were written against."""
    for case in json.load(open(os.path.join(ROOT, "tests", "golden", "synth_default_sweeps_sha256.json"))):
        seq = synth.SynthSequence(**case["kwargs"])
        got = [hashlib.sha256(seq.sweep(k).tobytes()).hexdigest() for k in range(case["kwargs"]["n_sweeps"])]
        assert got == case["sha256"], case["kwargs"]
