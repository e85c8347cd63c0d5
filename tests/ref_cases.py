"""Input sweeps for the tests that pin scan registration to the REFERENCE'S OWN program (oracle/_ref/libref.so = scan_registration.cpp
compiled unmodified, oracle/ref_harness.cpp): shared by tests/test_ref_scan_registration.py (CPU: reference binary vs oracle),
tests/golden/make_golden.py (records the reference binary's outputs for the small cases) and tests/test_gpu_ref_pinned.py (device vs
those recordings).  Every case is (scan_line, minimum_range, [sweep, ...]) — the sweeps of one case go through ONE ScanRegistration
object in order.  Each builder names the branch of scan_registration.cpp:131-449 it is there to reach.
"""
import numpy as np

import conftest

_F = np.float32


def _polar(rad, el_deg, az):
    c = np.zeros(np.broadcast(rad, el_deg, az).shape + (4,), dtype=_F)
    el = np.deg2rad(el_deg)
    c[..., 0] = rad * np.cos(el) * np.cos(az)
    c[..., 1] = rad * np.cos(el) * np.sin(az)
    c[..., 2] = rad * np.sin(el)
    return c


def synth_sweep(n_rings, n_az, k, sensor="default"):
    synth = conftest.load_synth()
    kw = dict(n_rings=n_rings, n_sweeps=k + 1, sensor=sensor)
    if n_az is not None:
        kw["n_azimuth"] = n_az
    return synth.SynthSequence(**kw).sweep(k)


# ---------------------------------------------------------------- scan-line bin edges (:192-226)
def bin_edges_deg(scan_line):
    """Elevations [deg] at which the reference's scan-line formulas change their answer: {name: angle}."""
    if scan_line == 16:    # :197 scanID = int((angle + 15) / 2 + 0.5), kept for 0 <= scanID <= 15; int() truncates towards zero, so scan line 0
        #                    reaches down to angle > -18 (the expression > -1)
        return {"16: -18 (scanID -1 | 0)": -18.0, "16: -14 (0 | 1)": -14.0, "16: 2 (8 | 9)": 2.0, "16: 14 (14 | 15)": 14.0, "16: 16 (15 | 16 dropped)": 16.0}
    if scan_line == 32:    # :206 scanID = int((angle + 92/3) * 3/4), kept for 0 <= scanID <= 31; scan line 0 reaches down to angle > -32
        return {"32: -32 (scanID -1 | 0)": -32.0, "32: -88/3 (0 | 1)": -88.0 / 3.0, "32: -28/3 (15 | 16)": -28.0 / 3.0, "32: 32/3 (30 | 31)": 32.0 / 3.0,
                "32: 12 (31 | 32 dropped)": 12.0}
    if scan_line == 64:    # :215-221 two formulas switching at -8.83; dropped above 2, below -24.33 and for scanID > 50
        return {"64: 2 (kept | dropped)": 2.0, "64: 2 - 0.5/3 (0 | 1)": 2.0 - 0.5 / 3.0, "64: 2 - 9.5/3 (9 | 10)": 2.0 - 9.5 / 3.0,
                "64: -8.83 (upper | lower formula)": -8.83,
                # the two formulas agree around -8.83 itself (both give 32); they part where the upper one WOULD step to 33, inside the lower one's range:
                # a switch constant moved below that elevation shows here and nowhere else
                "64: 2 - 32.5/3 (32 either side, by the lower formula only)": 2.0 - 32.5 / 3.0, "64: -8.83 - 0.25 (32 | 33)": -8.83 - 0.25, "64: -18.08 (scanID 50 | 51 dropped)": -18.08,
                "64: -24.33 (dropped on both sides: scanID 63 > 50 already)": -24.33}
    raise ValueError(scan_line)


def elevation_f32(c):
    """The reference's `angle` of every point in its own f32 / f64 steps (:192), atanf modelled by tests/fdlibm_np.py.  Used to show where a
    case's candidates lie relative to an edge, never as an expected value."""
    import fdlibm_np
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    a = np.array([fdlibm_np.atanf(v) for v in (z / np.sqrt(x * x + y * y, dtype=_F)).astype(_F)], dtype=_F)   # (scalar model)
    return ((a * _F(180)).astype(_F).astype(np.float64) / np.pi).astype(_F)


def bin_edge_sweep(scan_line, n_az=360, seed=5):
    """One ring of returns per edge of bin_edges_deg(scan_line): column j of a ring has its z moved by (j % 15) - 7 ulps off the edge
    elevation, so the f32 `angle` of the ring's points steps through the representable values right below, at and right above the edge.
    Firing order (all rings of a column, then the next column), one turn starting at azimuth 0.  Returns (cloud, {edge name: row mask})."""
    rng = np.random.default_rng(seed)
    edges = bin_edges_deg(scan_line)
    az = -2.0 * np.pi * (np.arange(n_az) + rng.uniform(-0.3, 0.3, n_az)) / n_az
    rings, names = [], []
    for name, e in edges.items():
        rad = rng.uniform(9.0, 30.0) + 2.0 * np.sin(3 * az + rng.uniform(0, 6)) + 0.01 * rng.standard_normal(n_az)
        rad[(np.arange(n_az) // 31) % 2 == 1] += 1.5      # range steps: corner candidates
        p = _polar(rad, e, az)
        steps = (np.arange(n_az) % 15) - 7
        z = p[:, 2].copy()
        for k in range(1, 8):
            up = steps >= k
            dn = steps <= -k
            z[up] = np.nextafter(z[up], _F(np.inf))
            z[dn] = np.nextafter(z[dn], _F(-np.inf))
        p[:, 2] = z
        xs = (np.arange(n_az) // 15) % 3 - 1        # ... and x by -1 / 0 / +1 ulp, which moves the angle by a fraction of its own ulp
        p[xs > 0, 0] = np.nextafter(p[xs > 0, 0], _F(np.inf))
        p[xs < 0, 0] = np.nextafter(p[xs < 0, 0], _F(-np.inf))
        rings.append(p)
        names.append(name)
    # two ordinary rings well inside a scan line, so that every sweep also has ordinary features
    mid = {16: (-5.0, 5.0), 32: (-10.0, 2.0), 64: (-3.0, -12.08)}[scan_line]
    for e in mid:
        rad = 15.0 + 3.0 * np.sin(2 * az) + 0.01 * rng.standard_normal(n_az)
        rad[(np.arange(n_az) // 23) % 2 == 1] += 1.0
        rings.append(_polar(rad, e, az))
        names.append(None)
    allp = np.stack(rings, 1)                       # [n_az, n_rings, 4]: firing order
    ring_of = np.broadcast_to(np.arange(len(rings))[None, :], allp.shape[:2]).reshape(-1)
    cloud = np.ascontiguousarray(allp.reshape(-1, 4))
    return cloud, {n: ring_of == i for i, n in enumerate(names) if n is not None}


# ---------------------------------------------------------------- start azimuths (:166-176, :234-262)
def start_azimuth_sweep(scan_line, yaw0, turn, n_az=300, seed=9):
    """A sweep whose first column points at azimuth yaw0 [rad] and whose columns cover `turn` of a revolution (clockwise, so that
    ori = -atan2(y, x) increases).  startOri = -yaw0; endOri - startOri = 2 pi (1 - turn) + 2 pi before the corrections of :169-176:
    a turn below ~1/2 makes the first fire (> 3 pi), a turn slightly above 1 the second (< pi)."""
    synth = conftest.load_synth()
    rng = np.random.default_rng(seed)
    el = synth.beam_elevations_deg(scan_line)
    el = el[(el > -24.0)] if scan_line == 64 else el
    az = yaw0 - 2.0 * np.pi * turn * (np.arange(n_az) + rng.uniform(-0.3, 0.3, n_az)) / n_az
    rad = 14.0 + 3.0 * np.sin(3 * az)[:, None] + 0.3 * np.arange(el.size)[None, :] + 0.01 * rng.standard_normal((n_az, el.size))
    rad[(np.arange(n_az) // 29) % 2 == 1, :] += 1.2
    return np.ascontiguousarray(_polar(rad, el[None, :], az[:, None]).reshape(-1, 4))


START_AZIMUTHS = [(0.0, 1.0), (3.0, 1.0), (-3.0, 1.0), (1.6, 1.0), (-1.6, 1.0), (2.0, 0.45), (-2.5, 0.3), (0.5, 1.03), (-1.0, 1.04), (3.1, 0.97),
                  (-3.1, 0.93), (1.0, 0.55)]


def start_sweeps():
    return [start_azimuth_sweep(64, y, t, n_az=80, seed=20 + i) for i, (y, t) in enumerate(START_AZIMUTHS)]


# ---------------------------------------------------------------- ring lengths (:276-281, :314)
def ring_length_sweep(seed=13):
    """64-line sweep in firing order whose scan lines hold 0, 1, 5, 11, 12, 13, 16, 17 and 50+ points.  scanStartInd = first + 5 and
    scanEndInd = last - 5 (:278-280), so `scanEndInd - scanStartInd < 6` (:314) skips every ring of fewer than 17 points — rings of 11, 12,
    13 and 16 among them —; a ring of exactly 17 has six one-point sectors; empty rings leave start > end."""
    synth = conftest.load_synth()
    rng = np.random.default_rng(seed)
    el = synth.beam_elevations_deg(64)
    n_az = 64
    counts = {0: 0, 1: 1, 2: 5, 3: 11, 4: 12, 5: 13, 6: 17, 7: 0, 8: 12, 9: 16, 33: 17, 34: 0, 35: 3}
    az = -2.0 * np.pi * 0.06 * (np.arange(n_az) + rng.uniform(-0.3, 0.3, n_az)) / n_az   # 6 cm between neighbours: flat and sharp candidates
    rows = []
    for j in range(n_az):
        for r in range(51):
            keep = counts.get(r, n_az - (r % 7))
            if j >= keep:
                continue
            rad = 12.0 + 0.2 * r + 2.0 * np.sin(2 * az[j] + r) + 0.002 * rng.standard_normal() + (1.0 if (j // 9) % 2 else 0.0)
            rows.append(_polar(rad, el[r], az[j]))
    return np.ascontiguousarray(np.stack(rows))


# ---------------------------------------------------------------- input filters (:157-158)
def range_and_nan_sweep(minimum_range=5.0, seed=17):
    """64 x 256 synthetic sweep with returns inside minimum_range, ON it within an ulp either way (x^2 + y^2 + z^2 < thres^2 in f32 drops,
    equality keeps: :114-117), NaN / +-inf coordinates (removed only when the cloud is flagged non-dense: :157), and the first and last
    rows among the removed ones (startOri / endOri come from the first / last SURVIVING point: :166-167)."""
    rng = np.random.default_rng(seed)
    c = synth_sweep(64, 256, 1).copy()
    n = c.shape[0]
    idx = rng.permutation(n)
    close, on, bad = idx[:400], idx[400:420], idx[700:1000]
    c[close, :3] *= (rng.uniform(0.02, 0.9, 400)[:, None] * minimum_range / np.linalg.norm(c[close, :3], axis=1)[:, None]).astype(_F)
    # on the threshold: axis-aligned returns at exactly minimum_range (square == thres * thres bit for bit) and one ulp below / above
    m = _F(minimum_range)
    vals = np.array([np.nextafter(m, _F(0)), m, np.nextafter(m, _F(np.inf))], dtype=_F)
    # (20 distinct points: a return repeated bit for bit next to itself would tie curvatures, which is another test's subject)
    axis = [(sx * v, 0.0) if ax == 0 else (0.0, sx * v) for v in vals for ax in (0, 1) for sx in (-1.0, 1.0)]
    pyth = [(sx * a, sy * b) for a, b in ((3.0, 4.0), (4.0, 3.0)) for sx in (-1.0, 1.0) for sy in (-1.0, 1.0)]   # 9 + 16 == 25 exactly: kept
    c[on, :2] = np.array(axis + pyth, dtype=_F)
    c[on, 2] = 0
    kinds = np.arange(300) % 4
    c[bad[kinds == 0], 0] = np.nan
    c[bad[kinds == 1], 1] = np.inf
    c[bad[kinds == 2], 2] = -np.inf
    c[bad[kinds == 3], :3] = np.nan
    c[:7, :3] = np.nan
    c[-5:, 1] = np.inf
    c[7:9, :3] *= _F(0.01)
    return c


def fuzz_cloud(rings, n_az, seed):
    """tests/test_gpu_fuzz.py's random range images (ragged rings, dropouts, repeats = equal curvatures, close returns, any start azimuth)."""
    import test_gpu_fuzz
    return test_gpu_fuzz.random_cloud(conftest.load_synth(), rings, n_az, seed)


FUZZ = [(64, 600, 103), (32, 1500, 105), (16, 257, 107), (64, 2048, 927), (16, 1800, 908), (32, 2000, 945), (64, 1500, 940), (64, 2000, 1013), (16, 1900, 1014)]


def small_cases():
    """{name: (scan_line, minimum_range, [sweeps])} — the cases whose reference outputs are committed (tests/golden/ref_sr_<name>.npz)."""
    cases = {
        "64x256": (64, 5.0, [synth_sweep(64, 256, 1)]),
        "16x256": (16, 5.0, [synth_sweep(16, 256, 1)]),
        "twice": (16, 5.0, [synth_sweep(16, 256, 2), synth_sweep(16, 200, 0)]),     # two sweeps through ONE object: the member arrays persist (:288-307)
        "32x256": (32, 5.0, [synth_sweep(32, 256, 2)]),
        "edges16": (16, 5.0, [bin_edge_sweep(16)[0]]),
        "edges32": (32, 5.0, [bin_edge_sweep(32)[0]]),
        "edges64": (64, 5.0, [bin_edge_sweep(64)[0]]),
        "rings": (64, 5.0, [ring_length_sweep()]),
        "filters": (64, 5.0, [range_and_nan_sweep(5.0)]),
        "start_a": (64, 5.0, start_sweeps()[:6]),
        "start_b": (64, 5.0, start_sweeps()[6:]),
    }
    return cases


def large_cases():
    """Cases compared live only (reference binary vs oracle on the CPU; vs the device when oracle/_ref/ travelled)."""
    return {
        "64x2048": (64, 5.0, [synth_sweep(64, 2048, 1)]),
        "64x512": (64, 5.0, [synth_sweep(64, 512, 3)]),
        "hdl64e": (64, 5.0, [synth_sweep(64, None, 1, sensor="hdl64e")]),
    }


# ---------------------------------------------------------------- committed recordings of the reference binary (tests/golden/ref_sr_*.npz)
def _rows_index(rows, table):
    """Index into `table` of a row with the same bits, for every row of `rows` (rows with equal bits are interchangeable)."""
    key = {r.tobytes(): i for i, r in enumerate(table)}
    return np.array([key[r.tobytes()] for r in rows], dtype=np.int32).reshape(-1)


def pack_golden(scan_line, minimum_range, sweeps, results):
    """results[k] = (the five clouds with VoxelGrid sorting as PCL does, surfPointsLessFlat with the canonical within-voxel order).
    Stored without redundancy, losslessly: laserCloud is a selection of input rows plus an intensity (s<k>_full_src, s<k>_full_intensity);
    the three picked clouds are copies of laserCloud points (:338-388), stored as indices into it (s<k>_idx<which>); only VoxelGrid's
    centroids are new floats (s<k>_c4, s<k>_c4_canonical)."""
    d = {"scan_line": np.int32(scan_line), "minimum_range": np.float64(minimum_range), "n_sweeps": np.int32(len(sweeps))}
    for k, (c, (clouds, less_flat_canonical)) in enumerate(zip(sweeps, results)):
        xyz = np.ascontiguousarray(c[:, :3])
        d["in_%d" % k] = xyz
        full = clouds[0]
        d["s%d_full_src" % k] = _rows_index(np.ascontiguousarray(full[:, :3]), xyz)
        d["s%d_full_intensity" % k] = full[:, 3].copy()
        for w in (1, 2, 3):
            d["s%d_idx%d" % (k, w)] = _rows_index(clouds[w], full)
        d["s%d_c4" % k] = clouds[4]
        d["s%d_c4_canonical" % k] = less_flat_canonical
    return d


def load_golden(path):
    """(scan_line, minimum_range, [input sweep [n, 4]], [(five clouds, canonical surfPointsLessFlat)]) of one ref_sr_*.npz."""
    z = np.load(path)
    sweeps, results = [], []
    for k in range(int(z["n_sweeps"])):
        xyz = z["in_%d" % k]
        c = np.zeros((xyz.shape[0], 4), dtype=_F)
        c[:, :3] = xyz
        full = np.zeros((z["s%d_full_src" % k].shape[0], 4), dtype=_F)
        full[:, :3] = xyz[z["s%d_full_src" % k]]
        full[:, 3] = z["s%d_full_intensity" % k]
        clouds = [full] + [full[z["s%d_idx%d" % (k, w)]].reshape(-1, 4) for w in (1, 2, 3)] + [z["s%d_c4" % k]]
        sweeps.append(c)
        results.append((clouds, z["s%d_c4_canonical" % k]))
    return int(z["scan_line"]), float(z["minimum_range"]), sweeps, results
