"""CPU: the host statement of the device probes (tests/cpp/dev_probe_host.cpp: csrc/fdlibm_f32.h and csrc/tf_dev.h compiled by g++ with
-ffp-contract=off) against statements that are already tied to something else, on the generators of tests/dev_probe_cases.py —
tests/test_gpu_dev_probe.py then holds the device to this program bit for bit.

  atanf / atan2f / elevation   tests/fdlibm_np.py, bit for bit (that transcription is held to the C library in tests/test_fdlibm_f32.py).  The
                               transcription is scalar Python, so this runs the generators at N_CPU elements: every constructed edge case and
                               fewer random ones.
  tf_get_rotation              kitti_io.tf2_rotation_of, bit for bit: the ONE operation of kitti_io's tf2 model (tests/test_kitti_io.py) with the
                               operation order of tf2.  kitti_io.make_T (s * (y*y + z*z) instead of y * (y * s) + ...) and inv_T / `@` (NumPy's
                               matrix product) round differently from Matrix3x3::setRotation, Transform::inverse and operator*, so
  tf_set_rotation, tf_mul, tf_inverse   are held to an np.longdouble evaluation at bounds derived below, like
  the quaternion of tf_get_rotation     which reproduces its input rotation to 4 ulp of f64 per matrix entry with unit norm to 4 ulp, in each of
                               the four branches and on each tie.
The branch census of the tf_get_rotation generator is computed here from the inputs alone."""
import os
import subprocess

import numpy as np
import pytest

import dev_probe_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -52      # of f64 at 1


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """run(probe, array) -> the host program's raw output bytes."""
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


def same_bits_f32(a, b):
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.uint32) == b.view(np.uint32))


def same_bits_f64(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.uint64) == b.view(np.uint64))


def test_atanf_equals_the_numpy_transcription(host):
    import fdlibm_np as fd
    x = dc.gen_atanf(dc.N_CPU)
    got = host("atanf", x).view(np.float32)
    with np.errstate(all="ignore"):
        want = np.array([fd.atanf(v) for v in x], np.float32)
    ok = same_bits_f32(got, want)
    assert ok.all(), ("atanf", [float(v) for v in x[~ok][:5]])
    den = (np.abs(x) < 2.0 ** -126) & (x != 0)
    assert den.sum() > 500 and np.array_equal(got[den].view(np.uint32), x[den].view(np.uint32))   # a denormal is returned as it is


def test_atan2f_equals_the_numpy_transcription(host):
    import fdlibm_np as fd
    yx = dc.gen_atan2f(dc.N_CPU)
    got = host("atan2f", yx).view(np.float32)
    with np.errstate(all="ignore"):
        want = np.array([fd.atan2f(y, x) for y, x in yx], np.float32)
    ok = same_bits_f32(got, want)
    assert ok.all(), ("atan2f", yx[~ok][:5].tolist())


def test_elevation_equals_the_numpy_transcription(host):
    import fdlibm_np as fd
    p = dc.gen_elev(dc.N_CPU)
    got = host("elev", p).view(np.float32)
    with np.errstate(all="ignore"):
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        arg = (z / np.sqrt((x * x + y * y).astype(np.float32))).astype(np.float32)    # f32 throughout, each operation rounded once
        want = np.array([fd.atanf(v) for v in arg], np.float32)
    ok = same_bits_f32(got, want)
    assert ok.all(), ("elev", p[~ok][:5].tolist())
    h2 = (x.astype(np.float64) ** 2 + y.astype(np.float64) ** 2)
    assert ((h2 > 0) & (h2 < 2.0 ** -126)).sum() >= 64 and (h2 == 0).sum() >= 64 and (h2 > 3.5e38).sum() >= 64 and (z == 0).sum() >= 256


def test_getrot_generator_census():
    m, is_rot = dc.gen_tf_getrot(dc.N_GPU)
    branch, ties = dc.getrot_census(m)
    for b in range(4):
        assert ((branch == b) & is_rot).sum() >= 1000, (b, int(((branch == b) & is_rot).sum()))
    for name in dc.TIE_NAMES:
        assert (ties[name] & is_rot).sum() >= 1, name
    assert ties["trace==0"].sum() >= 300
    # the quaternion generator of the round trip reaches them through tf_set_rotation: census of the matrices of an np.longdouble evaluation
    q = dc.gen_tf_roundtrip(dc.N_CPU)
    fin = np.isfinite(q).all(1) & (np.abs(q).max(1) > 0)
    branch_q, _ = dc.getrot_census(dc.rotation_ld(q[fin]).astype(np.float64))
    for b in range(4):
        assert (branch_q == b).sum() >= 1000, (b, int((branch_q == b).sum()))


def test_getrot_equals_the_tf2_model_of_kitti_io(host, vl):
    """kitti_io.tf2_rotation_of is Matrix3x3::getRotation in tf2's operation order: bit for bit, NaN for NaN."""
    from importlib import import_module
    kio = import_module(vl.__name__ + ".kitti_io")
    m, _ = dc.gen_tf_getrot(dc.N_CPU)
    got = host("tf_getrot", m).view(np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        want = np.array([kio.tf2_rotation_of(r.reshape(3, 3)) for r in m])
    ok = same_bits_f64(got, want).reshape(-1, 4).all(1)
    assert ok.all(), m[~ok][:3].tolist()
    # ... and the second half of the round trip is the same function
    q = dc.gen_tf_roundtrip(dc.N_CPU)
    rt = host("tf_roundtrip", q).view(np.float64).reshape(-1, 13)
    with np.errstate(all="ignore"):
        want = np.array([kio.tf2_rotation_of(r.reshape(3, 3)) for r in rt[:, :9]])
    ok = same_bits_f64(rt[:, 9:], want).reshape(-1, 4).all(1)
    assert ok.all(), q[~ok][:3].tolist()


def _check_quaternion(q_out, rot_in, what):
    """q_out reproduces the rotation rot_in (rows of nine, longdouble) to 4 ulp per entry and has unit norm to 4 ulp."""
    q = np.asarray(q_out, dc.LD)
    norm = np.sqrt((q * q).sum(1))
    err_n = np.abs(norm - 1).max()
    err_r = np.abs(dc.rotation_ld(q_out) - rot_in).max()
    print("%s: |norm - 1| max %.3g ulp, rotation entry max %.3g ulp" % (what, float(err_n / ULP), float(err_r / ULP)))
    assert err_n <= 4 * ULP, what
    assert err_r <= 4 * ULP, what


def test_getrot_against_longdouble(host):
    m, is_rot = dc.gen_tf_getrot(dc.N_GPU)
    got = host("tf_getrot", m).view(np.float64).reshape(-1, 4)
    branch, ties = dc.getrot_census(m)
    for b in range(4):
        sel = is_rot & (branch == b)
        _check_quaternion(got[sel], m[sel].astype(dc.LD), "branch %d" % b)
    for name in dc.TIE_NAMES:
        sel = is_rot & ties[name]
        _check_quaternion(got[sel], m[sel].astype(dc.LD), name)


def test_roundtrip_against_longdouble(host):
    """tf_set_rotation of any non-zero finite quaternion is the rotation of q / |q|: every entry is 1 - (a + b) or a +- b of products
    u * (v * s), s = 2 / d, d a sum of four squares.  d carries 3 roundings and s one more, each product two more: every product is within
    (1 + e)^6 of its exact value, e = 2^-53, its absolute value at most 1 (|2 u v / d| <= 1), so at most 6 e + O(e^2) off; the sum or difference of
    two adds e * 2 at most (|a +- b| <= 2), the subtraction from 1 another e: (6 + 6 + 2 + 1) e = 7.5 ulp as the bound for a diagonal entry,
    7 ulp for the others — asserted as 7.5 ulp.  The quaternion read back then reproduces THAT matrix' rotation ... to the 4 ulp of the
    issue plus the matrix' own distance from a rotation, the 7.5 ulp above: 11.5 ulp against the input's rotation, unit norm to 4 ulp."""
    q = dc.gen_tf_roundtrip(dc.N_GPU)
    rt = host("tf_roundtrip", q).view(np.float64).reshape(-1, 13)
    fin = np.isfinite(q).all(1) & (np.abs(q).max(1) > 0) & (np.abs(q).max(1) < 1e160) & (np.abs(q).max(1) > 1e-160)
    assert fin.sum() > q.shape[0] - 16
    want = dc.rotation_ld(q[fin])
    err_m = np.abs(rt[fin, :9].astype(dc.LD) - want).max()
    qo = rt[fin, 9:]
    norm = np.sqrt((qo.astype(dc.LD) ** 2).sum(1))
    err_n = np.abs(norm - 1).max()
    err_r = np.abs(dc.rotation_ld(qo) - want).max()
    print("round trip: matrix entry max %.3g ulp, |norm - 1| max %.3g ulp, rotation entry max %.3g ulp" % (float(err_m / ULP), float(err_n / ULP), float(err_r / ULP)))
    assert err_m <= 7.5 * ULP
    assert err_n <= 4 * ULP
    assert err_r <= 11.5 * ULP
    # the zero quaternion: s = 2 / 0 = inf, every product 0 * inf = NaN — thirteen NaNs, on every platform
    assert (q[0] == 0).all() and np.isnan(rt[0]).all()


def test_chain_against_longdouble(host):
    """tf_mul(a, tf_inverse(b)): the basis is a^m b.m^T, three products and two sums per entry of factors <= 1 in magnitude — 3 * 0.5 + 2 * 1 half-ulps
    of values <= ~1, asserted as 2 ulp(1); the origin is a.o - (a.m b.m^T) b.o evaluated as a.m (b.m^T (-b.o)) + a.o: with S = |b.o|_1 (an upper
    bound of every partial sum of the inner product) and |a.m| <= 1 row sums <= sqrt 3, each of the two nested 3-term products adds at most
    (3 * 0.5 + 2) ulp of a value <= sqrt(3) S, the final sum one ulp of <= |a.o| + sqrt(3) S: bounded by 8 * 2^-52 * (sqrt(3) S + |a.o|_inf)."""
    c = dc.gen_tf_chain(1 << 16)
    got = host("tf_chain", c).view(np.float64).reshape(-1, 12)
    a_m, a_o, b_m, b_o = (c[:, 0:9].reshape(-1, 3, 3).astype(dc.LD), c[:, 9:12].astype(dc.LD), c[:, 12:21].reshape(-1, 3, 3).astype(dc.LD),
                          c[:, 21:24].astype(dc.LD))
    bt = np.swapaxes(b_m, 1, 2)
    m = np.einsum("nij,njk->nik", a_m, bt)
    o = np.einsum("nij,nj->ni", a_m, np.einsum("nij,nj->ni", bt, -b_o)) + a_o
    err_m = np.abs(got[:, :9].astype(dc.LD) - m.reshape(-1, 9)).max()
    scale = np.sqrt(dc.LD(3)) * np.abs(b_o).sum(1) + np.abs(a_o).max(1)
    err_o = (np.abs(got[:, 9:].astype(dc.LD) - o).max(1) / np.maximum(scale, dc.LD(1e-300))).max()
    print("chain: basis entry max %.3g ulp, origin max %.3g ulp of its scale" % (float(err_m / ULP), float(err_o / ULP)))
    assert err_m <= 2 * ULP
    assert err_o <= 8 * ULP
    same = (c[:, :12] == c[:, 12:]).all(1)
    assert same.sum() > 1000 and np.abs(got[same, :9] - np.eye(3).ravel()).max() < 1e-15
