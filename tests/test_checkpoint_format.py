"""CPU: checkpoint and restore (vloam_checkpoint_size / _save / _load, include/vloam_hip/c_api.h) — the exports, the refusals of a buffer that
is no checkpoint (they come back before any device call, so without a GPU too, and before the handle is looked at), and the parser of
csrc/ckpt_format.h under AddressSanitizer / UBSan in a stand-alone program (tests/cpp/ckpt_format_check.cpp): every truncation and every
single-byte corruption of the header and its section table, from buffers allocated exactly.  The GPU side: tests/test_gpu_checkpoint.py."""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vloam-cmu-16833_amd", "csrc")
MAGIC = b"VLOAMCKP"


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vloam_hip", "c_api.h")).read(), flags=re.S)


def header_bytes():
    """sizeof(CkptHeader), read from what the library says about a buffer of magic + version only."""
    return 8 + 4 + 4 + 8 * 4 + 6 * 4 + 2 * 4 + 8 + 4 * 4 + 4 * 8 + 6 * 4 + 2 * 4 + 11 * 24 + 8 + 8


def load(vl, h, data, n=None):
    L = vl.lib()
    buf = None if data is None else C.create_string_buffer(bytes(data), max(len(data), 1))
    st = L.vloam_checkpoint_load(h, buf, C.c_longlong(len(data) if n is None else n))
    return st, L.vloam_last_error().decode()


def test_the_three_symbols_exist(vl):
    L, text = vl.lib(), header_text()
    for name, args in (("vloam_checkpoint_size", r"vloam_handle\*\s*\w*,\s*long long\*"), ("vloam_checkpoint_save", r"vloam_handle\*\s*\w*,\s*void\*\s*\w*,\s*long long\s*\w*,\s*long long\*"),
                       ("vloam_checkpoint_load", r"vloam_handle\*\s*\w*,\s*const void\*\s*\w*,\s*long long")):
        assert hasattr(L, name), name
        assert re.search(r"vloam_status\s+%s\(%s" % (name, args), text), name
    assert hasattr(vl.Handle, "checkpoint") and hasattr(vl.Handle, "restore")
    compat = open(os.path.join(ROOT, "include", "vloam_hip", "compat.hpp")).read()
    assert "checkpoint()" in compat and "void restore(" in compat and "const vloam_map_options& opt" in compat


def test_null_arguments(vl):
    L = vl.lib()
    n = C.c_longlong(0)
    assert L.vloam_checkpoint_size(None, C.byref(n)) == vl.ERR_INVALID
    assert L.vloam_checkpoint_save(None, None, C.c_longlong(0), C.byref(n)) == vl.ERR_INVALID
    st, msg = load(vl, None, None, 100)
    assert st == vl.ERR_INVALID and "null buffer" in msg


@pytest.mark.parametrize("with_handle", [False, True])
def test_refusals_of_a_buffer_that_is_no_checkpoint(vl, with_handle):
    """Each with its own message, the same with and without a handle: the format is checked first.  With a handle the "expected status" pattern
    of tests/test_map_options_config.py: where no handle can be created (no GPU) that half has nothing to run on."""
    L = vl.lib()
    h = C.c_void_p()
    if with_handle:
        cfg = vl.default_config(map_capacity_log2=12, max_points=4096)
        st = L.vloam_create(C.byref(cfg), 0, C.byref(h))
        assert st in (vl.VLOAM_OK, vl.ERR_NO_DEVICE)
        if st != vl.VLOAM_OK:
            return
    HB = header_bytes()
    try:
        cases = [(b"", "shorter than its header"), (MAGIC, "shorter than its header"), (MAGIC + bytes(HB - 9), "shorter than its header"),
                 (b"VLOAMCKQ" + bytes(HB - 8), "bad magic"), (bytes(HB + 64), "bad magic"),
                 (MAGIC + struct.pack("<i", 2) + bytes(HB - 12), "format version"), (MAGIC + struct.pack("<i", 0) + bytes(HB - 12), "format version"),
                 (MAGIC + struct.pack("<ii", 1, HB + 8) + bytes(HB - 16), "header struct size"),
                 (MAGIC + struct.pack("<ii", 1, HB) + bytes(HB - 16), "device struct size"),
                 (MAGIC + struct.pack("<ii", 1, HB) + struct.pack("<8i", 1, 2, 32, 4, 192, 9702, 0, 0) + bytes(HB - 48), "device struct size")]
        texts = set()
        for data, want in cases:
            st, msg = load(vl, h if with_handle else None, data)
            assert st == vl.ERR_INVALID and want in msg and "vloam_checkpoint_load" in msg, (len(data), want, msg)
            texts.add(want)
        assert len(texts) == 5
        if with_handle:   # the handle is still fresh and usable
            n = C.c_int(-1)
            assert L.vloam_frame_count(h, C.byref(n)) == vl.VLOAM_OK and n.value == 0
    finally:
        if with_handle:
            L.vloam_destroy(h)


def test_header_size_matches_the_library(vl):
    """A buffer one byte shorter than the header is "shorter than its header", one of the header's size is not."""
    HB = header_bytes()
    assert "shorter" in load(vl, None, MAGIC + bytes(HB - 9))[1]
    assert "shorter" not in load(vl, None, MAGIC + bytes(HB - 8))[1]


def test_parser_under_sanitizers(tmp_path):
    src = open(os.path.join(ROOT, "tests", "cpp", "ckpt_format_check.cpp")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["ckpt_format.h"]
    fmt = open(os.path.join(CSRC, "ckpt_format.h")).read()
    assert "hip" not in " ".join(re.findall(r"#include\s+\S+", fmt)).lower() and "vloam_handle" not in fmt
    exe = str(tmp_path / "ckpt_format_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "ckpt_format_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (r.stdout, r.stderr[-2000:])
    total, cases = (int(x) for x in r.stdout.split()[1:3])
    assert cases > total + 4 * header_bytes()
