"""GPU: the device build of the shared primitives against their host statement, bit for bit, through vloam_debug_probe (csrc/dev_probe.hip).

Every test feeds the same 2^20 arguments (tests/dev_probe_cases.py) to the probe kernel and to the host statement and compares raw bits — "both
NaN, or equal bits", as tests/test_fdlibm_f32.py does, because a NaN's payload may differ:
  fd_atanf, fd_atan2f, the elevation expression, tf_set_rotation / tf_get_rotation / tf_mul / tf_inverse
      tests/cpp/dev_probe_host.cpp, the same headers compiled by g++ -ffp-contract=off (tied to fdlibm_np, kitti_io's tf2 model and an
      np.longdouble evaluation in tests/test_dev_probe_host.py)
  associate_to_map, dquat_mul, dquat_rot (__device__-only)     NumPy f64 in the order of map_device.h (dev_probe_cases.np_*)
  block_bitonic_sort_u64 at every (P2, workgroup size) its callers use     np.sort of each problem
Both sides evaluate the same text with IEEE operations and contraction off, so there is no tolerance: the comparison asserts that the device
build does not contract, that its f32 divide / sqrtf and f64 sqrt are correctly rounded and that it does not flush f32 denormals.  The
explicit rows of each test are single arguments that would move under one of those changes."""
import faulthandler
import os
import subprocess

import numpy as np
import pytest

import dev_probe_cases as dc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def time_limit():
    """A probe is milliseconds of GPU time and a few seconds with the generator and the host side: a test still running after a minute hangs,
    and the process ends there with a traceback instead of waiting on the device."""
    faulthandler.dump_traceback_later(60, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """run(probe, array) -> the host program's raw output bytes (the program of tests/test_dev_probe_host.py)."""
    d = tmp_path_factory.mktemp("dev_probe_host")
    exe = str(d / "dev_probe_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "vloam-cmu-16833_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "dev_probe_host.cpp"), "-o", exe], check=True, timeout=300)

    def run(probe, a):
        fin, fout = str(d / (probe + ".in")), str(d / (probe + ".out"))
        np.ascontiguousarray(a).tofile(fin)
        r = subprocess.run([exe, probe, fin, fout], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return np.fromfile(fout, dtype=np.uint8)
    return run


def _mismatch(dev, ref, dtype, per_element):
    """Indices of the elements whose output differs in any word that is not NaN on both sides."""
    a, b = dev.view(dtype), ref.view(dtype)
    assert a.size == b.size
    u = np.uint32 if dtype == np.float32 else np.uint64
    same = (np.isnan(a) & np.isnan(b)) | (a.view(u) == b.view(u))
    return np.nonzero(~same.reshape(-1, per_element).all(1))[0]


def _assert_equal(dev, ref, dtype, per_element, cases, what):
    bad = _mismatch(dev, ref, dtype, per_element)
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%s: %d of %d elements differ; first at %d: in %r device %r host %r" % (
            what, bad.size, cases.shape[0], i, cases[i].tolist(), dev.view(dtype).reshape(-1, per_element)[i].tolist(),
            ref.view(dtype).reshape(-1, per_element)[i].tolist()))


def test_atanf(vl, host):
    x = dc.gen_atanf()
    dev = vl.debug_probe(vl.PROBE_ATANF, x)
    _assert_equal(dev, host("atanf", x), np.float32, 1, x, "fd_atanf")
    # explicit rows: a denormal comes back as it is (a flushing device returns 0); 2^-29 is the first argument that takes the polynomial
    rows = np.array([1e-45, -1e-45, 1.1754942e-38, 2.0 ** -29, 0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 25], np.float32)
    got = vl.debug_probe(vl.PROBE_ATANF, rows).view(np.float32)
    assert np.array_equal(got[:3].view(np.uint32), rows[:3].view(np.uint32))
    assert np.array_equal(got.view(np.uint32), host("atanf", rows).view(np.uint32))


def test_atan2f(vl, host):
    yx = dc.gen_atan2f()
    dev = vl.debug_probe(vl.PROBE_ATAN2F, yx)
    _assert_equal(dev, host("atan2f", yx), np.float32, 1, yx, "fd_atan2f")


def test_elevation(vl, host):
    p = dc.gen_elev()
    dev = vl.debug_probe(vl.PROBE_ELEV, p)
    _assert_equal(dev, host("elev", p), np.float32, 1, p, "fd_atanf(z / sqrtf(x * x + y * y))")


def test_tf_get_rotation(vl, host):
    m, _ = dc.gen_tf_getrot()
    dev = vl.debug_probe(vl.PROBE_TF_GETROT, m)
    _assert_equal(dev, host("tf_getrot", m), np.float64, 4, m, "tf_get_rotation")


def test_tf_roundtrip(vl, host):
    q = dc.gen_tf_roundtrip()
    dev = vl.debug_probe(vl.PROBE_TF_ROUNDTRIP, q)
    _assert_equal(dev, host("tf_roundtrip", q), np.float64, 13, q, "tf_set_rotation + tf_get_rotation")
    assert (q[0] == 0).all() and np.isnan(dev.view(np.float64)[:13]).all()      # the zero quaternion: NaN on both sides


def test_tf_chain(vl, host):
    c = dc.gen_tf_chain()
    dev = vl.debug_probe(vl.PROBE_TF_CHAIN, c)
    _assert_equal(dev, host("tf_chain", c), np.float64, 12, c, "tf_mul(a, tf_inverse(b))")


def test_associate_to_map(vl):
    c = dc.gen_assoc()
    dev = vl.debug_probe(vl.PROBE_ASSOC, c)
    ref = dc.np_associate_to_map(c)
    bad = _mismatch(dev, np.ascontiguousarray(ref).view(np.uint8).ravel(), np.float32, 4)
    assert bad.size == 0, ("associate_to_map", bad.size, c[bad[:3]].tolist(), dev.view(np.float32).reshape(-1, 4)[bad[:3]].tolist(), ref[bad[:3]].tolist())


def test_dquat(vl):
    c = dc.gen_quat()
    dev = vl.debug_probe(vl.PROBE_QUAT, c)
    ref = np.ascontiguousarray(dc.np_dquat(c)).view(np.uint8).ravel()
    _assert_equal(dev, ref, np.float64, 7, c, "dquat_mul / dquat_rot")


@pytest.mark.parametrize("p2,t", [pytest.param(p2, t, id="P2=%d-T=%d" % (p2, t)) for p2, t in dc.SORT_PAIRS])
def test_block_bitonic_sort(vl, p2, t):
    keys = dc.gen_sort(p2)
    dev = vl.debug_probe(vl.probe_sort(p2, t), keys).view(np.uint64).reshape(keys.shape)
    want = np.sort(keys, axis=1)
    bad = np.nonzero((dev != want).any(1))[0]
    assert bad.size == 0, ("problems", bad.tolist(), "first differing index", int(np.nonzero(dev[bad[0]] != want[bad[0]])[0][0]))


def test_sort_pairs_are_the_librarys(vl):
    assert tuple(dc.SORT_PAIRS) == tuple(vl.PROBE_SORT_PAIRS)


def test_bad_arguments_are_refused_and_the_next_call_works(vl):
    import ctypes as C
    L = vl.lib()
    x = np.array([1.0, 0.5], np.float32)
    out = np.zeros(2, np.float32)

    def call(which, n, out_bytes):
        return L.vloam_debug_probe(C.c_int(0), C.c_int(which), x.ctypes.data_as(C.c_void_p), C.c_longlong(n), out.ctypes.data_as(C.c_void_p),
                                   C.c_longlong(out_bytes))
    assert call(0, 2, 8) == vl.ERR_INVALID and b"unknown probe" in L.vloam_last_error()
    assert call(99, 2, 8) == vl.ERR_INVALID
    assert call(vl.probe_sort(128, 256), 2, 8) == vl.ERR_INVALID           # a (P2, T) pair nobody uses
    assert call(vl.probe_sort(8192, 256), 2, 8) == vl.ERR_INVALID
    assert call(vl.PROBE_ATANF, -1, 8) == vl.ERR_INVALID
    assert call(vl.PROBE_ATANF, 2, 4) == vl.ERR_INVALID and b"out_bytes" in L.vloam_last_error()   # short
    assert call(vl.PROBE_ATANF, 2, 12) == vl.ERR_INVALID
    assert call(vl.probe_sort(256, 256), 2, 16) == vl.ERR_INVALID          # no whole problem
    assert np.array_equal(out, np.zeros(2, np.float32))                     # nothing was written
    assert call(vl.PROBE_ATANF, 2, 8) == vl.VLOAM_OK
    import fdlibm_np as fd
    assert out[0].view(np.uint32) == fd.atanf(x[0]).view(np.uint32) and out[1].view(np.uint32) == fd.atanf(x[1]).view(np.uint32)
