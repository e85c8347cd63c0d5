"""csrc/fdlibm_f32.h (the atanf / atan2f the device's scan registration calls) against the C library's atanf / atan2f, bit for bit.

The reference computes a return's scan line and relative time from glibc's float atan / atan2 (scan_registration.cpp:166-167,192,234); the
header restates glibc's (fdlibm's) algorithm so that the device produces the same bits.  Compiled here for the host with g++
-ffp-contract=off (the flag the device translation unit is built with) and run over 2^24 arguments per generator: random bit patterns of
every binade, the arguments LiDAR returns produce, break points, signed zeros, infinities, NaN.  No GPU involved; the GPU side of the same
claim is tests/test_gpu_dev_probe.py (the device build of the header against this host build, bit for bit on 2^20 arguments per function,
through vloam_debug_probe) and, at the arguments a drive produces, tests/test_gpu_scan_registration.py (intensity and startOri / endOri bit
for bit against the oracle, which calls the C library).
The check is meaningful on a glibc that still builds atanf / atan2f from the fdlibm float sources (<= 2.40; this image: 2.35)."""
import os
import platform
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_atanf_atan2f_equal_the_c_library(tmp_path):
    libc = platform.libc_ver()
    if libc[0] == "glibc" and tuple(int(v) for v in libc[1].split(".")[:2]) >= (2, 41):
        pytest.skip("glibc %s computes atanf / atan2f with the correctly-rounded CORE-MATH routines, not fdlibm's" % libc[1])
    exe = str(tmp_path / "fdlibm_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "vloam-cmu-16833_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "fdlibm_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(1 << 24)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    rows = dict((ln.split()[0], [int(v) for v in ln.split()[1:]]) for ln in r.stdout.strip().splitlines()[-2:])
    assert rows["atanf"][0] > (1 << 25) and rows["atanf"][1] == 0
    assert rows["atan2f"][0] > (1 << 25) and rows["atan2f"][1] == 0


def test_numpy_statement_equals_the_c_library():
    """tests/fdlibm_np.py (used by the literal Python transcription of scan registration) against the C library through ctypes."""
    import ctypes
    import ctypes.util

    import numpy as np

    import fdlibm_np as fd
    libc = platform.libc_ver()
    if libc[0] == "glibc" and tuple(int(v) for v in libc[1].split(".")[:2]) >= (2, 41):
        pytest.skip("glibc %s: correctly-rounded atanf / atan2f" % libc[1])
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.atanf.restype = ctypes.c_float
    libm.atanf.argtypes = [ctypes.c_float]
    libm.atan2f.restype = ctypes.c_float
    libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
    rng = np.random.default_rng(1)
    xs = np.concatenate([rng.integers(0, 2 ** 32, 8000, dtype=np.uint64).astype(np.uint32).view(np.float32), rng.uniform(-0.6, 0.6, 8000).astype(np.float32),
                         np.array([0.4375, 0.6875, 1.1875, 2.4375, 0.0, -0.0, 1, -1, np.inf, -np.inf, 33554432.0], np.float32)])
    with np.errstate(all="ignore"):
        for x in xs:
            a, b = np.float32(libm.atanf(float(x))), np.float32(fd.atanf(x))
            assert (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32), float(x)
        for y, x in zip(rng.uniform(-120, 120, 8000).astype(np.float32), rng.uniform(-120, 120, 8000).astype(np.float32)):
            assert np.float32(libm.atan2f(float(y), float(x))).view(np.uint32) == np.float32(fd.atan2f(y, x)).view(np.uint32), (float(y), float(x))
        for y in (0.0, -0.0, 1.0, -1.0, np.inf, -np.inf):
            for x in (0.0, -0.0, 1.0, -1.0, np.inf, -np.inf):
                assert np.float32(libm.atan2f(y, x)).view(np.uint32) == np.float32(fd.atan2f(y, x)).view(np.uint32), (y, x)
