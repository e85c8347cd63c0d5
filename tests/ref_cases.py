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


def long_ring_sweep(n_long=16384, seed=23):
    """A scan line of exactly n_long returns (the top of the opt-in long ring tier, max_ring_points = 16 384) next to two ordinary scan
    lines of 256, in firing order by azimuth, one turn."""
    rng = np.random.default_rng(seed)
    parts = []
    for el, n in ((-10.43, n_long), (-3.0, 256), (-15.08, 256)):
        az = -2.0 * np.pi * (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / n
        rad = 20.0 + 3.0 * np.sin(3 * az) + 0.02 * rng.standard_normal(n)
        rad[(np.arange(n) * 64 // n) % 2 == 1] += 1.0      # range steps: corner candidates
        parts.append((az, _polar(rad, el, az)))
    az = np.concatenate([a for a, _ in parts])
    pts = np.concatenate([p for _, p in parts])
    return np.ascontiguousarray(pts[np.argsort(-az, kind="stable")])


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
        "ring16384": (64, 5.0, [long_ring_sweep()]),       # handles need max_ring_points = 16384 for it (longest_ring)
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


def longest_ring(clouds):
    """Points of the fullest scan line of a recorded laserCloud: what a handle's max_ring_points has to cover."""
    full = clouds[0]
    return int(np.bincount(full[:, 3].astype(np.int64)).max()) if full.shape[0] else 0


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


# ---------------------------------------------------------------- sequences for laser odometry and mapping (tests/test_ref_laser_*.py)
def synth_sequence(n_rings, n_az, n, sensor="default", **kw):
    synth = conftest.load_synth()
    args = dict(n_rings=n_rings, n_sweeps=n + 1, sensor=sensor)
    if n_az is not None:
        args["n_azimuth"] = n_az
    args.update(kw)
    seq = synth.SynthSequence(**args)
    return [np.ascontiguousarray(seq.sweep(k), dtype=_F) for k in range(n)]


def moving_fuzz_sequence(rings, n_az, seed, n=4, step=0.3):
    """One random range image of the fuzz generator seen from a sensor that advances `step` metres per sweep along x: ragged rings,
    dropouts and repeats, with real scan-to-scan correspondences."""
    base = fuzz_cloud(rings, n_az, seed)
    out = []
    for k in range(n):
        c = base.copy()
        c[:, 0] -= _F(step * k)
        out.append(c)
    return out


def nearby_scan_clouds():
    """(corner tree, surf tree, sharp query, flat query, expected corner triple, expected plane quadruple): candidates exactly 2 and 3 scan
    lines above the closest point, the one 3 lines away NEARER — `> closestPointScanID + NEARBY_SCAN` (2.5) ends the walk before it
    (laser_odometry.cpp:286, :371), so the point 2 lines away is paired; a bound of 3.5 would pair the other, 1.5 none.  Below the closest
    point the same two distances are occupied by farther points, so the upward side decides."""
    def P(x, y, z, ring):
        return [x, y, z, ring]
    corner = np.array([P(10, 0, -0.9, 7), P(10, 0, -1.2, 8), P(10, 0, 0, 10), P(10, 0, 1.0, 12), P(10, 0, 0.5, 13)], _F)
    surf = np.array([P(11, 0, -0.9, 7), P(11, 0, -1.2, 8), P(10, 0, 0, 10), P(10, 1, 0, 10), P(11, 0, 1.0, 12), P(11, 0, 0.5, 13)], _F)
    sharp = np.array([P(10, 0.01, 0, 10)], _F)
    flat = np.array([P(10, 0.3, 0.01, 10)], _F)
    return corner, surf, sharp, flat, (0, 2, 3), (0, 2, 3, 4)


def vo_priors(n, seed=4):
    """A non-trivial velo_last_VOT_velo_curr per sweep: a few centimetres and milliradians off the true motion's scale."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        v = rng.normal(0, 0.01, 3)
        q = np.array([v[0], v[1], v[2], 1.0])
        out.append((q / np.linalg.norm(q), np.array([0.4, 0.0, 0.0]) + rng.normal(0, 0.05, 3)))
    return out


def loam_sequences():
    """{name: (parameters of the session, sweeps, what to hand LaserMapping::input instead of the odometry pose or None, VO priors or None)}"""
    import branch_cases
    import degenerate_cases
    import test_gpu_launch_configs as lc
    synth = conftest.load_synth()
    cases = {
        "64x256": (dict(), synth_sequence(64, 256, 8), None, None),
        "64x512": (dict(), synth_sequence(64, 512, 6), None, None),
        "64x2048": (dict(), synth_sequence(64, 2048, 3), None, None),
        "hdl64e": (dict(), synth_sequence(64, None, 3, sensor="hdl64e"), None, None),
        "fuzz": (dict(), moving_fuzz_sequence(64, 600, 103), None, None),
        "no_correspondence": (dict(), degenerate_cases.lo_sequence(synth, n=6, far_at=(3,)), None, None),
        "fewer_than_ten": (dict(), degenerate_cases.lo_sequence(synth, n=6, far_at=(), wedge_at=(3,)), None, None),
        "small_map": (dict(scan_line=16), degenerate_cases.sparse_map_sequence(synth, n=6), None, None),
        "skip2": (dict(mapping_skip_frame=2), synth_sequence(64, 256, 7), None, None),
        "skip5": (dict(mapping_skip_frame=5), synth_sequence(64, 256, 11), None, None),
        "ground_only": (dict(), branch_cases.ground_only_sequence(synth, n=5), None, None),
        "repeated_sweep": (dict(), branch_cases.repeated_sweep_sequence(synth, n=5), None, None),
        "vo_prior": (dict(detach_vo_lo=False), synth_sequence(64, 256, 6), None, vo_priors(6)),
        "vo_prior_skip2": (dict(detach_vo_lo=False, mapping_skip_frame=2), synth_sequence(64, 256, 6), None, vo_priors(6, seed=8)),
    }
    for name, (rings, az, p) in lc.LAUNCH.items():
        cases[name] = (dict(scan_line=rings, minimum_range=p["minimum_range"], line_res=p["mapping_line_resolution"], plane_res=p["mapping_plane_resolution"],
                            mapping_skip_frame=p["mapping_skip_frame"]), lc.sequence(synth, name, 4, 2.0), None, None)
    # a full turn on the spot-ish: the drive of 64 x 256 with the sensor yawed 0.11 rad more every sweep (tests/test_gpu_turns.py), 60 sweeps = 6.6 rad
    import test_gpu_turns
    cases["full_turn"] = (dict(), [test_gpu_turns.spun(c, 0.11 * k) for k, c in enumerate(synth_sequence(64, 256, 60))], None, None)
    walk = branch_cases.six_way_walk()
    cases["six_way_walk"] = (dict(), synth_sequence(64, 256, len(walk) - 1 + 1)[:len(walk)], walk, None)
    return cases


# ---------------------------------------------------------------- committed recordings of laser odometry / mapping (tests/golden/ref_lo_*.npz, ref_map_*.npz)
def loam_golden_cases():
    """{file stem: (session parameters, sweeps, VO priors or None, with mapping)} — small on purpose: each file holds its input sweeps."""
    return {
        "ref_lo_64x128": (dict(), synth_sequence(64, 128, 3), None, False),
        "ref_lo_16x256_prior_skip2": (dict(scan_line=16, detach_vo_lo=False, mapping_skip_frame=2), synth_sequence(16, 256, 5), vo_priors(5, seed=11), False),
        "ref_map_16x256": (dict(scan_line=16), synth_sequence(16, 256, 5), None, True),
        "ref_map_64x128": (dict(), synth_sequence(64, 128, 3), None, True),
        "ref_map_16x256_skip2": (dict(scan_line=16, mapping_skip_frame=2), synth_sequence(16, 256, 6), None, True),
    }


def _unique_index(points_f64, table, what):
    key = {}
    for i, r in enumerate(np.ascontiguousarray(table[:, :3])):
        assert r.tobytes() not in key, "%s: the cloud holds a point twice, indices would not be unique" % what
        key[r.tobytes()] = i
    return np.array([key[r.tobytes()] for r in np.ascontiguousarray(points_f64, dtype=_F)], dtype=np.int32)


def record_loam(ref, params, sweeps, priors, with_mapping):
    """The sweeps through the reference binary (ref.Loam, canonical VoxelGrid order: what the device computes); everything the CPU tests
    compare with the oracle, as plain arrays.  Correspondences are stored as indices into the sweep's own clouds (recovered from the
    functors' points, which must be unique there)."""
    r = ref.Loam(**params)
    d = {"n_sweeps": np.int32(len(sweeps)), "with_mapping": np.int32(with_mapping), "has_prior": np.int32(priors is not None)}
    for k, v in dict(scan_line=64, minimum_range=5.0, line_res=0.4, plane_res=0.8, mapping_skip_frame=1, detach_vo_lo=True).items():
        d["p_" + k] = np.float64(params.get(k, v))
    tree_c = tree_s = np.zeros((0, 4), _F)
    for k, c in enumerate(sweeps):
        d["in_%d" % k] = np.ascontiguousarray(c[:, :3])
        if priors is not None:
            q, t = r.set_vo_prior(*priors[k])
            d["prior_%d" % k] = np.concatenate([q, t])
        assert r.stage_sr(c) == 0
        cl = [r.cloud(i) for i in range(5)]
        assert r.stage_lo() == 0
        n = r.num_solves(r.ODOMETRY)
        d["lo%d_n" % k] = np.int32(n)
        for o in range(n):
            s = r.solve(r.ODOMETRY, o)
            nc = int(np.count_nonzero(s["types"] == 0))
            pc, pp = s["payload"][:nc], s["payload"][nc:]
            w = "sweep %d round %d" % (k, o)
            d["lo%d_%d_corner" % (k, o)] = np.stack([_unique_index(pc[:, 0:3], cl[1], w), _unique_index(pc[:, 3:6], tree_c, w), _unique_index(pc[:, 6:9], tree_c, w)], 1).reshape(-1, 3)
            d["lo%d_%d_plane" % (k, o)] = np.stack([_unique_index(pp[:, 0:3], cl[3], w)] + [_unique_index(pp[:, 3 * j:3 * j + 3], tree_s, w) for j in (1, 2, 3)], 1).reshape(-1, 4)
            d["lo%d_%d_res0" % (k, o)] = s["residuals0"]
            d["lo%d_%d_x" % (k, o)] = np.concatenate([s["q_in"], s["t_in"], s["q_out"], s["t_out"]])
        d["lo%d_pose" % k] = np.concatenate(r.lo_pose())
        d["lo%d_skip" % k] = np.int32(r.skip_frame())
        if not with_mapping:     # (the mapping recordings leave the hand-over clouds to the odometry recordings: file size)
            d["lo%d_c2" % k], d["lo%d_c4" % k] = cl[2], cl[4]
            # laserCloudFullRes is a selection of input rows plus an intensity, stored that way (as pack_golden does)
            xyz = np.ascontiguousarray(c[:, :3])
            d["lo%d_full_src" % k] = _rows_index(np.ascontiguousarray(cl[0][:, :3]), xyz)
            d["lo%d_full_intensity" % k] = cl[0][:, 3].copy()
            if not r.skip_frame():
                assert np.array_equal(r.cloud(7).view(np.uint32), cl[0].view(np.uint32)) and np.array_equal(r.cloud(5).view(np.uint32), cl[2].view(np.uint32))
        tree_c, tree_s = cl[2], cl[4]
        if not with_mapping:
            continue
        assert r.stage_map() == 0
        n = r.num_solves(r.MAPPING)
        d["map%d_n" % k] = np.int32(n)
        d["map%d_pub" % k] = np.concatenate(r.published_pose(1))
        if r.skip_frame():
            continue
        d["map%d_stacks" % k] = r.map_filter_log()[:2, 1].astype(np.int32)
        for o in range(n):
            s = r.solve(r.MAPPING, o)
            ne = int(np.count_nonzero(s["types"] == 0))
            assert np.all(s["types"][:ne] == 0) and np.all(s["types"][ne:] == 2)
            d["map%d_%d_ne" % (k, o)] = np.int32(ne)
            d["map%d_%d_curr" % (k, o)] = s["payload"][:, 0:3].astype(_F)
            d["map%d_%d_cab" % (k, o)] = s["payload"][:ne, 3:9]
            d["map%d_%d_spl" % (k, o)] = s["payload"][ne:, 3:7]
            d["map%d_%d_res0" % (k, o)] = s["residuals0"]
            d["map%d_%d_x" % (k, o)] = np.concatenate([s["q_in"], s["t_in"], s["q_out"], s["t_out"]])
        d["map%d_counts" % k] = r.map_cube_counts().astype(np.int32)
    if with_mapping:
        d["map_cloud"] = r.cloud(8)
    return d


def loam_golden_params(z):
    return dict(scan_line=int(z["p_scan_line"]), minimum_range=float(z["p_minimum_range"]), line_res=float(z["p_line_res"]), plane_res=float(z["p_plane_res"]),
                mapping_skip_frame=int(z["p_mapping_skip_frame"]), detach_vo_lo=bool(z["p_detach_vo_lo"]))


def loam_golden_full(z, k):
    """laserCloudFullRes of sweep k of a ref_lo_* recording."""
    xyz = z["in_%d" % k]
    full = np.zeros((z["lo%d_full_src" % k].shape[0], 4), dtype=_F)
    full[:, :3] = xyz[z["lo%d_full_src" % k]]
    full[:, 3] = z["lo%d_full_intensity" % k]
    return full


def loam_golden_sweep(z, k):
    xyz = z["in_%d" % k]
    c = np.zeros((xyz.shape[0], 4), dtype=_F)
    c[:, :3] = xyz
    return c
