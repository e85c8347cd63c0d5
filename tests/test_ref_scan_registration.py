"""CPU: the oracle's scan registration against the REFERENCE'S OWN scan_registration.cpp, compiled unmodified (oracle/_ref/libref.so through
oracle/ref.py; stand-in headers for PCL / ROS in oracle/ref_shim/) — all five clouds, all four floats of every point, bit for bit, and the
order of the points.

Bit equality is the derived tolerance: both sides run the same f32 / f64 operations under the same compiler flags (-O3 -ffp-contract=off
-fno-fast-math) against the same libm, so any difference is a difference in program text — which is what this file exists to find.

std::sort (scan_registration.cpp:323, and PCL's VoxelGrid) leaves equal keys in an unspecified order.  liborc_stdsort.so calls std::sort on
the same ranges with the same comparator and is compared on EVERY case; liborc.so (the canonical order the device computes: stable) is
compared too, with the stand-in VoxelGrid switched to input order within a voxel, on every case whose sweeps contain no bit-identical
neighbouring returns (the fuzz generator plants such repeats on purpose: equal curvatures).

What is pinned: control flow, constants, index arithmetic, overload resolution and evaluation order of scan_registration.cpp:131-449.
What is not: pcl::VoxelGrid and removeNaNFromPointCloud are stand-ins (a second restatement each, sharing no code with the oracle's).

Skips: only when neither the reference checkout nor a built oracle/_ref/libref.so exists; where the reference exists a failed build fails.
"""
import os

import numpy as np
import pytest

import ref_cases

import ref   # oracle/ref.py, a module of this repository (conftest puts oracle/ on the path): if it does not import, that is an error, not a skip

pytestmark = pytest.mark.skipif(not ref.available(), reason=ref.SKIP_REASON)

NAMES = ["laserCloud", "cornerPointsSharp", "cornerPointsLessSharp", "surfPointsFlat", "surfPointsLessFlat"]


def assert_same_clouds(got, want, what):
    for w, (a, b) in enumerate(zip(got, want)):
        name = NAMES[w] if len(got) == 5 else ""
        assert a.shape == b.shape, "%s %s: %d vs %d points" % (what, name, a.shape[0], b.shape[0])
        same = a.view(np.uint32) == b.view(np.uint32)
        assert same.all(), "%s %s: %d of %d points differ, first at row %d: %r vs %r" % (
            what, name, np.count_nonzero(~same.all(axis=1)), a.shape[0], int(np.argmin(same.all(axis=1))), a[np.argmin(same.all(axis=1))], b[np.argmin(same.all(axis=1))])


def run_reference_and_oracle(orc, scan_line, minimum_range, sweeps, canonical, what):
    """The sweeps through ONE reference object and ONE oracle session, compared after every sweep; returns the last reference clouds."""
    r = ref.ScanRegistration(scan_line, minimum_range, voxel_stable=canonical)
    o = orc.Oracle(scan_line=scan_line, minimum_range=minimum_range, with_mapping=False, variant="liborc.so" if canonical else "liborc_stdsort.so")
    out = None
    for k, c in enumerate(sweeps):
        assert r.run(c) == 0 and o.stage_sr(c) == 0
        out = r.clouds()
        assert_same_clouds([o.cloud(w) for w in range(5)], out, "%s sweep %d (%s order)" % (what, k, "canonical" if canonical else "std::sort"))
    return out


def test_the_reference_build_resolves_atan_and_sqrt_of_floats_to_the_float_overloads():
    """orc_loam.cpp restates scan_registration.cpp:192 with atanf / sqrtf, and csrc/fdlibm_f32.h reproduces glibc's atanf bit for bit on that
    assumption.  Here the compiler answers: in the reference's translation unit, built with the include the real tf header has (<math.h>),
    the unqualified atan(float) / sqrt(float) are the float overloads; without that include they are the C library's double functions."""
    assert ref.math_overloads_are_float("libref.so") is True
    assert ref.math_overloads_are_float("libref_cmath_only.so") is False


SMALL = ref_cases.small_cases()
LARGE_NAMES = ["64x2048", "64x512", "hdl64e"]
_large = {}


def large(name):
    if not _large:
        _large.update(ref_cases.large_cases())
    return _large[name]


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_cases(orc, name, canonical):
    scan_line, minimum_range, sweeps = SMALL[name]
    run_reference_and_oracle(orc, scan_line, minimum_range, sweeps, canonical, name)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("name", LARGE_NAMES + ["16x1024", "32x1024"])
def test_synthetic_sweeps(orc, name, canonical):
    if name in LARGE_NAMES:
        scan_line, minimum_range, sweeps = large(name)
    else:
        scan_line = int(name.split("x")[0])
        minimum_range, sweeps = 5.0, [ref_cases.synth_sweep(scan_line, 1024, 1), ref_cases.synth_sweep(scan_line, 1024, 2)]
    out = run_reference_and_oracle(orc, scan_line, minimum_range, sweeps, canonical, name)
    assert out[1].shape[0] > 0 and out[3].shape[0] > 0 and out[4].shape[0] > 0


@pytest.mark.parametrize("rings,n_az,seed", ref_cases.FUZZ)
def test_random_range_images(orc, rings, n_az, seed):
    """tests/test_gpu_fuzz.py's generator: ragged rings, dropouts (NaN / inf / zero), returns inside minimum_range, repeats (equal
    curvatures: std::sort order only), rings too short for a sector, any start azimuth, 0.3 - 1.04 turns."""
    c = ref_cases.fuzz_cloud(rings, n_az, seed)
    out = run_reference_and_oracle(orc, rings, 5.0, [c], False, "fuzz %d" % seed)
    assert out[1].shape[0] > 0 and out[3].shape[0] > 0


@pytest.mark.parametrize("scan_line", [16, 32, 64])
def test_bin_edge_case_straddles_every_edge_as_closely_as_f32_allows(scan_line):
    """The edge cases are what they claim to be.  `angle` = f32(f64(f32(atanf(.) * 180)) / pi) (:192): near an edge e the arc tangent steps
    through the f32 values a around e * pi / 180, so only the values f32(f64(f32(a * 180)) / pi) of those a are ATTAINABLE — a grid coarser
    than f32's own around e (180 / pi = 57.3 is not a power of two), which is why "within one ulp" is stated on that grid.  For every edge the sweep must hold a return on
    the nearest attainable angle below the edge, one on the nearest above it, and one on the edge itself where f32 can represent it."""
    cloud, masks = ref_cases.bin_edge_sweep(scan_line)
    edges = ref_cases.bin_edges_deg(scan_line)
    for name, m in masks.items():
        e = edges[name]
        ang = ref_cases.elevation_f32(cloud[m]).astype(np.float64)
        grid = [np.float32(e * np.pi / 180.0)]
        for _ in range(4):
            grid = [np.nextafter(grid[0], np.float32(-np.inf))] + grid + [np.nextafter(grid[-1], np.float32(np.inf))]
        attainable = np.array([np.float32(np.float64(np.float32(g * np.float32(180))) / np.pi) for g in grid], dtype=np.float64)
        lo, hi = attainable[attainable < e].max(), attainable[attainable > e].min()
        print("%s: %d returns; nearest attainable angles %.9g | %.9g, held by %d | %d returns, %d on the edge itself" % (
            name, ang.size, lo, hi, np.count_nonzero(ang == lo), np.count_nonzero(ang == hi), np.count_nonzero(ang == e)))
        assert np.count_nonzero(ang == lo) > 0 and np.count_nonzero(ang == hi) > 0, name
        if np.any(attainable == e):
            assert np.count_nonzero(ang == e) > 0, name


def test_start_azimuth_cases_take_every_correction():
    """The INPUTS of the `start_a` / `start_b` cases are placed where intended: by this test's own f64 arithmetic on the first / last point
    and on every point's azimuth, the sweeps cover each outcome of :169-176 (endOri - startOri > 3 pi, < pi, neither) and both wraps of
    :235-262.  That says where the inputs lie, NOT which branch the reference binary took — nothing here observes that, apart from the
    sanity check that its relTime fractions stay in [0, 1.06].  What pins the branches is the bit-for-bit comparison of the same sweeps in
    test_small_cases[start_a / start_b]: an oracle that took another branch on any of them would differ in every intensity."""
    seen = set()
    for i, (yaw0, turn) in enumerate(ref_cases.START_AZIMUTHS):
        c = ref_cases.start_sweeps()[i]
        s = -np.arctan2(c[0, 1], c[0, 0])
        e = -np.arctan2(c[-1, 1], c[-1, 0]) + 2 * np.pi
        seen.add("> 3 pi" if e - s > 3 * np.pi else "< pi" if e - s < np.pi else "neither")
        ori = -np.arctan2(c[:, 1], c[:, 0])
        if np.any(ori < s - np.pi / 2):
            seen.add("ori += 2 pi")
        if np.any(ori > s + 1.5 * np.pi):
            seen.add("ori -= 2 pi")
        r = ref.ScanRegistration(64, 5.0)
        assert r.run(c) == 0
        frac = (r.cloud(0)[:, 3].astype(np.float64) % 1.0) / 0.1
        assert frac.min() >= -1e-6 and frac.max() <= 1.06, (yaw0, turn, frac.min(), frac.max())
    assert seen == {"> 3 pi", "< pi", "neither", "ori += 2 pi", "ori -= 2 pi"}, seen


def test_ring_length_case_has_the_rings_it_claims():
    """:314 skips a ring when scanEndInd - scanStartInd < 6, i.e. (see ref_cases.ring_length_sweep) when it holds fewer than 17 points: the
    reference binary takes features from the rings of 17 and from none of the rings of 16, 13, 12, 11, 5 or 1."""
    r = ref.ScanRegistration(64, 5.0)
    assert r.run(ref_cases.ring_length_sweep()) == 0
    n = np.bincount(r.cloud(0)[:, 3].astype(np.int64), minlength=64)
    assert [int(n[k]) for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 33, 34, 35)] == [0, 1, 5, 11, 12, 13, 17, 0, 12, 16, 17, 0, 3]
    feature_rings = set(np.concatenate([r.cloud(w)[:, 3] for w in (1, 2, 3, 4)]).astype(np.int64))
    assert 6 in feature_rings and 33 in feature_rings
    assert not feature_rings & {1, 2, 3, 4, 5, 8, 9, 35}


def test_no_surviving_point_is_reported_by_both(orc):
    """All NaN, or everything inside minimum_range: the reference would read points[0] of an empty vector (:166, undefined behaviour), so
    the harness does not call it; the oracle reports the empty sweep."""
    c = np.full((64, 4), np.nan, dtype=np.float32)
    assert ref.ScanRegistration(64, 5.0).run(c) == -1
    assert orc.Oracle(with_mapping=False).stage_sr(c) == -1
    c = np.ones((64, 4), dtype=np.float32)
    assert ref.ScanRegistration(64, 5.0).run(c) == -1
    assert orc.Oracle(with_mapping=False).stage_sr(c) == -1


def test_dense_flag_with_nan_input_is_a_stated_deviation(orc):
    """removeNaNFromPointCloud looks at no coordinate when the cloud says is_dense = true (:157; PCL filter.hpp).  The C ABI has no such flag:
    the oracle and the device ALWAYS remove non-finite points (branch table: stated deviation).  What the reference
    binary does with NaN-bearing input flagged dense, recorded here:
      * finite input: the flag changes nothing;
      * NaN points in the interior: they pass both filters (every comparison with NaN is false), their `angle` is NaN, int(NaN) is
        INT_MIN on x86-64 (formally undefined), scanID < 0, dropped at :198-224 — the same five clouds as with the flag cleared;
      * a NaN before the first or after the last return that survives minimum_range: it IS the first / last point, startOri / endOri = NaN, every relTime is NaN, every intensity is NaN — garbage the oracle does not reproduce."""
    base = ref_cases.synth_sweep(64, 256, 1)
    base = base[np.isfinite(base[:, :3]).all(axis=1)]   # (the generator marks a missing return with NaN)
    a, b = ref.ScanRegistration(64, 5.0), ref.ScanRegistration(64, 5.0)
    assert a.run(base, is_dense=True) == 0 and b.run(base, is_dense=False) == 0
    assert_same_clouds(a.clouds(), b.clouds(), "finite input, dense vs non-dense")
    c = base.copy()
    far = np.flatnonzero(np.linalg.norm(base[:, :3], axis=1) >= 5.0)
    # between the first and the last return that survives minimum_range (a NaN passes that filter too: outside them it would BE the first / last point)
    c[np.random.default_rng(3).permutation(far[-1] - far[0] - 2)[:300] + far[0] + 1, :3] = np.nan
    o = orc.Oracle(with_mapping=False, variant="liborc_stdsort.so")
    assert a.run(c, is_dense=True) == 0 and o.stage_sr(c) == 0
    assert_same_clouds(a.clouds(), [o.cloud(w) for w in range(5)], "interior NaN flagged dense vs the oracle (which removes them)")
    c[far[-1] + 1, :3] = np.nan   # inside minimum_range until now, removed; as NaN it stays and becomes the LAST point
    assert a.run(c, is_dense=True) == 0 and o.stage_sr(c) == 0
    full = a.cloud(0)
    assert np.isnan(full[:, 3]).all(), "a NaN last point flagged dense poisons every intensity in the reference"
    assert np.isfinite(o.cloud(0)).all(), "the oracle removed it (stated deviation)"


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", sorted(SMALL))
def test_committed_recordings_are_what_the_reference_binary_computes(name):
    """tests/golden/ref_sr_<name>.npz (what the GPU tests compare the device with, on a machine without the reference) regenerated from the
    reference binary: same inputs, same five clouds, same canonical surfPointsLessFlat, bit for bit."""
    scan_line, minimum_range, sweeps = SMALL[name]
    g_line, g_range, g_sweeps, g_results = ref_cases.load_golden(os.path.join(GOLDEN, "ref_sr_%s.npz" % name))
    assert (g_line, g_range, len(g_sweeps)) == (scan_line, minimum_range, len(sweeps))
    lit = ref.ScanRegistration(scan_line, minimum_range, voxel_stable=False)
    can = ref.ScanRegistration(scan_line, minimum_range, voxel_stable=True)
    for k, c in enumerate(sweeps):
        assert np.array_equal(c[:, :3].view(np.uint32), g_sweeps[k][:, :3].view(np.uint32)), "%s sweep %d: the committed input is not what ref_cases builds" % (name, k)
        assert lit.run(c) == 0 and can.run(c) == 0
        assert_same_clouds(g_results[k][0], lit.clouds(), "%s sweep %d, committed vs regenerated" % (name, k))
        assert_same_clouds([g_results[k][1]], [can.cloud(4)], "%s sweep %d canonical surfPointsLessFlat, committed vs regenerated" % (name, k))
    assert os.path.getsize(os.path.join(GOLDEN, "ref_sr_%s.npz" % name)) < os.path.getsize(os.path.join(GOLDEN, "vloam_64x256_5frames.npz"))


def overload_sensitivity():
    """Every sweep of this file through libref.so and libref_cmath_only.so: (points, points whose scan line differs or that exist in one output
    only, points with the same scan line but other intensity bits).  DESIGN.md section 2 quotes the totals."""
    rows = []
    cases = dict(SMALL)
    cases.update(ref_cases.large_cases())
    for rings, n_az, seed in ref_cases.FUZZ:
        cases["fuzz%d" % seed] = (rings, 5.0, [ref_cases.fuzz_cloud(rings, n_az, seed)])
    for name in sorted(cases):
        scan_line, minimum_range, sweeps = cases[name]
        a, b = ref.ScanRegistration(scan_line, minimum_range), ref.ScanRegistration(scan_line, minimum_range, variant="libref_cmath_only.so")
        for c in sweeps:
            assert a.run(c) == 0 and b.run(c) == 0
            A, B = a.cloud(0), b.cloud(0)
            ka = {p[:3].tobytes(): p[3] for p in A}
            moved = bits = 0
            seen = 0
            for p in B:
                v = ka.get(p[:3].tobytes())
                if v is None or int(v) != int(p[3]):
                    moved += 1
                elif np.float32(v).view(np.uint32) != np.float32(p[3]).view(np.uint32):
                    bits += 1
                seen += v is not None
            moved += A.shape[0] - seen
            rows.append((name, A.shape[0], moved, bits))
    return rows


def test_cmath_only_build_sizes_the_overload_assumption():
    """The counter-factual build (double atan / sqrt at :192) over the same sweeps.  On sensor-like sweeps the two builds agree on every scan
    line: a return must lie within ~1e-7 relative of a bin edge for the f64 elevation to truncate differently.  On the bin-edge cases, which
    put returns exactly there, they must differ — otherwise this comparison could not see the difference it is there to size."""
    rows = overload_sensitivity()
    for r in rows:
        print("%-10s %7d points, %4d change scan line / appear / vanish, %4d change intensity bits only" % r)
    total = sum(r[1] for r in rows)
    moved = sum(r[2] for r in rows)
    edge_moved = sum(r[2] for r in rows if r[0].startswith("edges"))
    print("total %d points, %d moved (%d of them in the bin-edge cases)" % (total, moved, edge_moved))
    assert edge_moved > 0
    assert moved - edge_moved <= 1e-4 * total, "ordinary sweeps: the two overload sets should almost never disagree about a scan line"
