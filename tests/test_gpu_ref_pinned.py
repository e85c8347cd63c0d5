"""-m gpu: HIP scan registration through the C ABI against the output of the REFERENCE'S OWN scan_registration.cpp — not against the oracle.

Always: the committed recordings tests/golden/ref_sr_*.npz (written by tests/golden/make_golden.py from oracle/_ref/libref.so, which is the
reference's file compiled unmodified; tests/test_ref_scan_registration.py regenerates and re-checks them wherever the reference exists).
Additionally, when oracle/_ref/libref.so is present next to the tests (a build product; it is there only if the tree came from a machine
that has the reference): the 64 x 2048, 64 x 512 and hdl64e sweeps live through that library.

Compared bit for bit, all four floats of every point, and the order of the points: laserCloud, cornerPointsSharp, cornerPointsLessSharp,
surfPointsFlat as the reference wrote them; surfPointsLessFlat against the reference run with the stand-in VoxelGrid in the canonical
within-voxel order (PCL's std::sort leaves that order unspecified and the f32 centroid sums depend on it; the device computes the canonical
one — same convention as tests/test_gpu_scan_registration.py).  None of these cases holds bit-identical neighbouring returns, so std::sort's
unspecified order among EQUAL curvatures (scan_registration.cpp:323) does not come into play; that is
test_gpu_scan_registration.py::test_equal_curvatures_are_picked_in_the_canonical_order's subject.
"""
import glob
import os

import numpy as np
import pytest

import ref_cases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "ref_sr_*.npz")))
NAMES = ["laserCloud", "cornerPointsSharp", "cornerPointsLessSharp", "surfPointsFlat", "surfPointsLessFlat"]


def assert_device_equals(h, clouds, less_flat_canonical, what):
    want = list(clouds[:4]) + [less_flat_canonical]
    for w, name in enumerate(NAMES):
        dev, ref = h.features(w), want[w]
        assert dev.shape == ref.shape, "%s %s: %d points on the device, %d in the reference" % (what, name, dev.shape[0], ref.shape[0])
        same = (dev.view(np.uint32) == ref.view(np.uint32)).all(axis=1)
        assert same.all(), "%s %s: %d of %d points differ, first at row %d: %r vs %r" % (
            what, name, np.count_nonzero(~same), same.size, int(np.argmin(same)), dev[np.argmin(same)], ref[np.argmin(same)])


def test_the_recordings_are_all_here():
    assert sorted(os.path.basename(p)[7:-4] for p in GOLDEN) == sorted(ref_cases.small_cases())


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[7:-4] for p in GOLDEN])
def test_device_against_the_reference_binarys_recorded_output(vl, path):
    scan_line, minimum_range, sweeps, results = ref_cases.load_golden(path)
    kw = {}
    if max(ref_cases.longest_ring(r[0]) for r in results) > 4096:     # beyond the default tier: the opt-in long ring tier, sized for its limit
        kw = dict(max_ring_points=16384, max_points=max(max(c.shape[0] for c in sweeps), 1024))
    h = vl.Handle(0, scan_line=scan_line, minimum_range=minimum_range, with_mapping=0, **kw)
    for k, c in enumerate(sweeps):     # several sweeps: one handle, like the one ScanRegistration object of the recording
        h.reset_frame()
        h.scan_registration(c)
        clouds, canonical = results[k]
        assert clouds[0].shape[0] > 0
        assert_device_equals(h, clouds, canonical, "%s sweep %d" % (os.path.basename(path), k))


def _live():
    import ref
    return ref if os.path.exists(os.path.join(ref.REF_OUT, "libref.so")) else None


@pytest.mark.parametrize("name", ["64x2048", "64x512", "hdl64e"])
def test_device_against_the_reference_binary_live(vl, name):
    ref = _live()
    if ref is None:
        pytest.skip("oracle/_ref/libref.so (the reference's scan_registration.cpp, compiled where the reference exists) did not travel with this tree")
    scan_line, minimum_range, sweeps = ref_cases.large_cases()[name]
    lit = ref.ScanRegistration(scan_line, minimum_range, voxel_stable=False)
    can = ref.ScanRegistration(scan_line, minimum_range, voxel_stable=True)
    kw = dict(max_ring_points=8192) if name == "hdl64e" else {}     # two lasers share a scan line there: 4 166 points in a ring (long ring tier)
    h = vl.Handle(0, scan_line=scan_line, minimum_range=minimum_range, with_mapping=0, max_points=max(max(c.shape[0] for c in sweeps), 1024), **kw)
    for k, c in enumerate(sweeps):
        assert lit.run(c) == 0 and can.run(c) == 0
        h.reset_frame()
        h.scan_registration(c)
        assert_device_equals(h, lit.clouds(), can.cloud(4), "%s sweep %d (live)" % (name, k))
