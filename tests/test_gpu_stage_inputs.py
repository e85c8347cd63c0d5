"""-m gpu: clouds and poses EDITED between the façade's stages.

The reference hands clouds and the odometry pose from stage to stage by value and every stage deep-copies what it is given
(LaserOdometry::input laser_odometry.cpp:135-146, LaserMapping::input laser_mapping.cpp:167-196): a caller may thin, filter or replace them
in between.  Here the stages exchange their results on the device; vloam_set_odometry_input / vloam_set_mapping_input upload what the caller
changed.  Oracle: the same stage-by-stage sequence with the same edits (orc_stage_sr / orc_set_sr_cloud / orc_stage_lo / orc_stage_map).
Rounds 1 - 5 refused a substituted cloud (std::invalid_argument from compat.hpp)."""
import zlib

import numpy as np
import pytest

from test_gpu_laser_mapping import lexsort_rows, oracle_map_points, qdist

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-8


def edited(clouds5, k):
    """The caller's edit of scan registration's five clouds for sweep k (order-preserving, as a filter would)."""
    full, sharp, less_sharp, flat, less_flat = [c.copy() for c in clouds5]
    out = [None] * 5
    if k % 3 == 1:    # a thinning filter on the two less-clouds + a few features dropped
        out[2] = less_sharp[np.arange(less_sharp.shape[0]) % 7 != 3]
        out[4] = less_flat[np.arange(less_flat.shape[0]) % 5 != 0]
        out[1] = sharp[2:]
    elif k % 3 == 2:  # an object mask: everything within 6 m in front is removed from all five; the flat features nudged
        def keep(c):
            return c[~((c[:, 0] > 0) & (np.abs(c[:, 1]) < 3.0) & (c[:, 0] < 12.0))]
        out = [keep(full), keep(sharp), keep(less_sharp), keep(flat), keep(less_flat)]
        out[3] = out[3].copy()
        out[3][:, 2] += np.float32(0.003)
    return out


def test_edited_clouds_between_scan_registration_and_odometry(vl, orc, sweeps):
    n, shape = 9, (64, 512)
    h = vl.Handle(0, with_mapping=1, debug=1)
    o = orc.Oracle(with_mapping=True)
    n_edits = 0
    for k in range(n):
        cloud = sweeps(shape[0], shape[1], k)
        h.reset_frame()
        h.scan_registration(cloud)
        assert o.stage_sr(cloud) == 0
        five = [h.features(w) for w in range(5)]
        for w in range(5):   # all four floats (intensity = scan line + 0.1 relTime goes through atan2f: the device computes it the way glibc does)
            assert np.array_equal(np.ascontiguousarray(five[w][:, :4]).view(np.uint32), np.ascontiguousarray(o.cloud(w)[:, :4]).view(np.uint32))
        ed = edited(five, k)
        if any(e is not None for e in ed):
            n_edits += 1
            h.set_odometry_input(*ed)
            for w in range(5):
                if ed[w] is not None:
                    o.set_sr_cloud(w, ed[w])
                    assert np.array_equal(h.features(w).view(np.uint32), np.ascontiguousarray(ed[w]).view(np.uint32)), "the device holds the edited cloud %d" % w
        qw, tw, _, _ = h.laser_odometry()
        o.stage_lo()
        oq, ot, _, _ = o.lo_pose()
        assert qdist(qw, oq) < POSE_TOL and np.linalg.norm(tw - ot) < POSE_TOL, "odometry pose, sweep %d" % k
        if k > 0:
            for outer in range(2):
                d = h.lo_debug(outer)
                oc, op = o.lo_corr(outer)
                assert np.array_equal(d["corner"], oc) and np.array_equal(d["plane"], op), "correspondences, sweep %d round %d" % (k, outer)
        # LaserOdometry::output hands the (edited) less-clouds on as CornerLast / SurfLast
        for which in (5, 6):
            assert np.array_equal(h.features(which)[:, :4].view(np.uint32), o.cloud(which)[:, :4].view(np.uint32))
        qm, tm = h.laser_mapping()
        assert o.stage_map() == 0
        for which in (7, 8):
            assert np.array_equal(h.features(which)[:, :4].view(np.uint32), o.cloud(which)[:, :4].view(np.uint32)), "stack %d, sweep %d" % (which, k)
        oq, ot, _, _ = o.map_pose()
        assert qdist(qm, oq) < POSE_TOL and np.linalg.norm(tm - ot) < POSE_TOL, "map pose, sweep %d" % k
    assert n_edits >= 5
    for kind in (0, 1):
        _, pts = h.map_dump(kind)
        ref = oracle_map_points(o, kind)
        assert pts.shape == ref.shape and np.array_equal(lexsort_rows(pts)[:, :4].view(np.uint32), lexsort_rows(ref)[:, :4].view(np.uint32))
    h.close()


@pytest.mark.parametrize("skip", [1, 2])
def test_edited_inputs_between_odometry_and_mapping(vl, orc, sweeps, skip):
    """LaserMapping::input with thinned clouds and a nudged odometry pose: this sweep's mapping works on them, the odometry's own CornerLast /
    SurfLast (next sweep's search clouds) do not change — separate copies in the reference."""
    n, shape = 8, (64, 512)
    h = vl.Handle(0, with_mapping=1, mapping_skip_frame=skip)
    o = orc.Oracle(with_mapping=True, mapping_skip_frame=skip)
    for k in range(n):
        cloud = sweeps(shape[0], shape[1], k)
        h.reset_frame()
        h.scan_registration(cloud)
        qw, tw, _, _ = h.laser_odometry()
        assert o.stage_sr(cloud) == 0
        o.stage_lo()
        oq, ot, _, _ = o.lo_pose()
        assert qdist(qw, oq) < POSE_TOL and np.linalg.norm(tw - ot) < POSE_TOL, "odometry pose, sweep %d" % k
        dq, dt = h.odometry_pose()
        assert np.array_equal(dq, qw) and np.array_equal(dt, tw)
        corner, surf, full = h.features(5), h.features(6), h.features(0)
        kw, okw = {}, {}
        if k % 2 == 1:
            c2, s2, f2 = corner[::2].copy(), surf[np.arange(surf.shape[0]) % 3 != 1].copy(), full[: full.shape[0] // 2].copy()
            kw.update(laserCloudCornerLast=c2, laserCloudSurfLast=s2, laserCloudFullRes=f2)
            okw.update(corner=c2, surf=s2, full=f2)
        if k in (2, 3, 6):
            # a UNIT quaternion, like every Eigen::Quaterniond an odometry hands on: the solver's closed-form Jacobians (d lp / d delta =
            # -2 [R p]x) are those of a rotation; with |q|^2 = 1 + 5e-6 the reference's autodiff and they part at that relative size and the
            # poses after 2 x 4 iterations by 1e-9 (measured) — stated in c_api.h
            q2 = qw + np.array([1e-3, -2e-3, 5e-4, 0.0])
            q2 = q2 / np.linalg.norm(q2)
            t2 = tw + np.array([0.02, -0.01, 0.005])
            kw.update(q_wodom_curr=q2, t_wodom_curr=t2)
            okw.update(q=q2, t=t2)
        if kw:
            h.set_mapping_input(**kw)
        qm, tm = h.laser_mapping()
        assert o.stage_map(**okw) == 0
        oq, ot = o.map_published_pose()
        assert qdist(qm, oq) < POSE_TOL and np.linalg.norm(tm - ot) < POSE_TOL, "map pose, sweep %d" % k
        skipped = ((k + 1) % skip) != 0
        if "laserCloudFullRes" in kw and not skipped:   # /velodyne_cloud_registered is the full-resolution cloud as handed in (laser_mapping.cpp:795-799)
            reg, ref = h.features(11), o.cloud(11)
            assert reg.shape == ref.shape and np.allclose(reg[:, :3], ref[:, :3], rtol=0, atol=1e-5)
        # the odometry's clouds are untouched
        assert np.array_equal(h.features(5).view(np.uint32), corner.view(np.uint32)) and np.array_equal(h.features(6).view(np.uint32), surf.view(np.uint32))
    tj = h.trajectory()
    assert tj.shape[0] == n
    for kind in (0, 1):
        _, pts = h.map_dump(kind)
        ref = oracle_map_points(o, kind)
        assert pts.shape == ref.shape and np.array_equal(lexsort_rows(pts)[:, :4].view(np.uint32), lexsort_rows(ref)[:, :4].view(np.uint32))
    h.close()


def test_stage_input_call_order_and_capacity(vl, sweeps):
    h = vl.Handle(0, with_mapping=1)
    c = sweeps(64, 512, 0)
    with pytest.raises(vl.VloamError) as e:
        h.set_odometry_input(cornerPointsSharp=c[:10])
    assert e.value.status == vl.ERR_ORDER
    h.reset_frame()
    h.scan_registration(c)
    with pytest.raises(vl.VloamError) as e:
        h.set_mapping_input(laserCloudCornerLast=c[:10])
    assert e.value.status == vl.ERR_ORDER
    with pytest.raises(vl.VloamError) as e:
        h.set_odometry_input(cornerPointsSharp=np.zeros((769, 4), np.float32))
    assert e.value.status == vl.ERR_CAPACITY
    h.set_odometry_input(cornerPointsSharp=np.zeros((0, 4), np.float32))   # an EMPTY substituted cloud is a cloud
    assert h.features(1).shape[0] == 0
    h.laser_odometry()
    h.laser_mapping()
    hb = vl.Handle(0, n_sessions=2, with_mapping=1)
    with pytest.raises(vl.VloamError) as e:
        hb.set_odometry_input(cornerPointsSharp=c[:10])
    assert e.value.status == vl.ERR_INVALID
    hb.close()
    h.close()


# ---- edits the reference accepts, at the edges of the rule vloam_set_odometry_input enforces (c_api.h, csrc/stage_input_check.h)
ODO_NAMES = ("laserCloud", "cornerPointsSharp", "cornerPointsLessSharp", "surfPointsFlat", "surfPointsLessFlat")
WALKED = (2, 4)   # the two less-clouds: the next sweep's CornerLast / SurfLast, walked by scan line


def _lines(c):
    return np.trunc(c[:, 3].astype(np.float64)).astype(np.int64)


def _interior(n, step=37):
    return np.arange(1, max(n - 1, 1), step)


def admissible_edit(kind, five, rng):
    """The caller's edit of scan registration's five clouds (None = keep the device's)."""
    out = [None] * 5
    if kind == "shuffle_within_lines":      # a seeded shuffle inside every run of equal int(intensity)
        for w in WALKED:
            L = _lines(five[w])
            out[w] = five[w][np.lexsort((rng.random(L.size), L))]
    elif kind == "windows_of_three":        # lines reversed in windows of three: the largest inversion is exactly 2 (every walk then breaks
        # at once in the reference, no correspondence at all: the device must find none either)
        for w in WALKED:
            L = _lines(five[w])
            out[w] = five[w][np.lexsort((np.arange(L.size), 2 - L % 3, L // 3))]
    elif kind == "one_window_reversed":     # lines 30, 31, 32 reversed, the rest in order: walks from around them run across the inversion
        for w in WALKED:
            L = _lines(five[w])
            key = np.where((L >= 30) & (L <= 32), 62 - L, L)
            out[w] = five[w][np.lexsort((np.arange(L.size), key))]
    elif kind == "line_jitter":             # int(intensity) r -> r - 1 on interior points (the jitter scan registration produces)
        for w in WALKED:
            c = five[w].copy()
            i = _interior(c.shape[0])
            i = i[_lines(c)[i] >= 1]
            c[i, 3] = (_lines(c)[i] - np.float32(0.02)).astype(np.float32)
            out[w] = c
    elif kind == "reltime":                 # fractional intensity (relTime) of the sharp / flat points only (DISTORTION is false in the
        # reference: TransformToStart does not read it, and the result must not move either)
        for w in (1, 3):
            c = five[w].copy()
            L = _lines(c).astype(np.float32)
            c[:, 3] = L + (c[:, 3] - L) * np.float32(0.5)
            out[w] = c
    elif kind == "xyz_nudge":               # interior points moved, sizes kept, in all five clouds
        for w in range(5):
            c = five[w].copy()
            c[_interior(c.shape[0], 29), 2] += np.float32(0.02)
            out[w] = c
    elif kind == "empty":
        out[2], out[4] = five[2][:0], five[4][:0]
    elif kind == "single":
        out[2], out[4] = five[2][five[2].shape[0] // 2:][:1], five[4][five[4].shape[0] // 2:][:1]
    elif kind == "lines_0_63":              # only the lowest and the highest line (lines 0 / 63 and their r - 1 jitter)
        for w in WALKED:
            L = _lines(five[w])
            out[w] = five[w][(L <= 0) | (L >= 62)]
    elif kind == "missing_lines":           # a run of missing lines in the middle
        for w in WALKED:
            L = _lines(five[w])
            out[w] = five[w][(L < 20) | (L > 29)]
    return out


def _compare_sweep(h, o, k, with_corr=True):
    qw, tw, _, _ = h.laser_odometry()
    o.stage_lo()
    oq, ot, _, _ = o.lo_pose()
    assert qdist(qw, oq) < POSE_TOL and np.linalg.norm(tw - ot) < POSE_TOL, "odometry pose, sweep %d" % k
    n_corr = 0
    if k > 0 and with_corr:
        for outer in range(2):
            d = h.lo_debug(outer)
            oc, op = o.lo_corr(outer)
            assert np.array_equal(d["corner"], oc) and np.array_equal(d["plane"], op), "correspondences, sweep %d round %d" % (k, outer)
            n_corr += oc.shape[0] + op.shape[0]
    for which in (5, 6):
        assert np.array_equal(h.features(which)[:, :4].view(np.uint32), o.cloud(which)[:, :4].view(np.uint32)), "cloud %d, sweep %d" % (which, k)
    qm, tm = h.laser_mapping()
    assert o.stage_map() == 0
    for which in (7, 8):
        assert np.array_equal(h.features(which)[:, :4].view(np.uint32), o.cloud(which)[:, :4].view(np.uint32)), "stack %d, sweep %d" % (which, k)
    oq, ot, _, _ = o.map_pose()
    assert qdist(qm, oq) < POSE_TOL and np.linalg.norm(tm - ot) < POSE_TOL, "map pose, sweep %d" % k
    return n_corr


def _compare_maps(h, o):
    for kind in (0, 1):
        _, pts = h.map_dump(kind)
        ref = oracle_map_points(o, kind)
        assert pts.shape == ref.shape and np.array_equal(lexsort_rows(pts)[:, :4].view(np.uint32), lexsort_rows(ref)[:, :4].view(np.uint32))


@pytest.mark.parametrize("kind", ["shuffle_within_lines", "windows_of_three", "one_window_reversed", "line_jitter", "reltime", "xyz_nudge", "empty", "single",
                                  "lines_0_63", "missing_lines"])
def test_admissible_edits_through_the_c_abi(vl, orc, sweeps, kind):
    """Edits the rule admits, at sweeps 1 and 2; the next sweep walks the edited less-clouds as CornerLast / SurfLast, so its correspondence
    triples (and both rounds of every later sweep) must equal the oracle's with the same edits, the stacks and the map bit for bit."""
    import stage_walk_model as wm
    n, shape, edit_at = 5, (64, 512), (1, 2)
    rng = np.random.default_rng(zlib.crc32(kind.encode()))
    h = vl.Handle(0, with_mapping=1, debug=1)
    o = orc.Oracle(with_mapping=True)
    for k in range(n):
        cloud = sweeps(shape[0], shape[1], k)
        h.reset_frame()
        h.scan_registration(cloud)
        assert o.stage_sr(cloud) == 0
        if k in edit_at:
            five = [h.features(w) for w in range(5)]
            ed = admissible_edit(kind, five, rng)
            for w in range(5):
                if ed[w] is not None:
                    assert wm.rule_fault(ed[w], w in WALKED) == (0, -1), (kind, w)
                    if kind in ("windows_of_three", "one_window_reversed", "line_jitter", "shuffle_within_lines") and w in WALKED:
                        assert not np.array_equal(ed[w], five[w]), "the edit changes cloud %d" % w
            h.set_odometry_input(**{ODO_NAMES[w]: ed[w] for w in range(5) if ed[w] is not None})
            for w in range(5):
                if ed[w] is not None:
                    o.set_sr_cloud(w, ed[w])
                    assert np.array_equal(h.features(w).view(np.uint32), np.ascontiguousarray(ed[w]).view(np.uint32)), "the device holds cloud %d" % w
        _compare_sweep(h, o, k)
    _compare_maps(h, o)
    h.close()


def _with_point(c, i, col, value):
    c = c.copy()
    c[i, col] = np.float32(value)
    return c


def refused_edits(five):
    """(cloud index, edited cloud, point, rule) of edits the rule refuses: a NaN in each of the five clouds; in each less-cloud one point 3
    lines below an earlier line, a line of 64, a line of -1."""
    cases = []
    for w in range(5):
        i = five[w].shape[0] // 2
        cases.append((w, _with_point(five[w], i, w % 4, np.nan), i, 1))
    for w in WALKED:
        c, L = five[w], _lines(five[w])
        i = int(np.nonzero(L >= L.max() // 2)[0][0]) + 3   # a point whose earlier lines reach 3 above the line it is given
        top = int(L[:i].max())
        cases.append((w, _with_point(c, i, 3, top - 3 + 0.04), i, 3))
        cases.append((w, _with_point(c, i, 3, 64.02), i, 2))
        cases.append((w, _with_point(c, i, 3, -1.05), i, 2))
    return cases


def test_refused_edits_leave_the_sweep_unedited(vl, orc, sweeps):
    """Every refused edit returns VLOAM_ERR_INVALID naming the point, uploads nothing (not even the admissible clouds of the same call), and
    the sweep — this one and the next, which walks CornerLast / SurfLast — equals the oracle's unedited run.  Each refused order is one the
    device would really walk differently: the reference's literal walk from that point breaks elsewhere than the device's stop tables."""
    import stage_walk_model as wm
    n, shape = 4, (64, 512)
    h = vl.Handle(0, with_mapping=1, debug=1)
    o = orc.Oracle(with_mapping=True)
    names = ("laserCloudCornerLast", "laserCloudSurfLast", "laserCloudFullRes")
    n_refused = 0
    for k in range(n):
        cloud = sweeps(shape[0], shape[1], k)
        h.reset_frame()
        h.scan_registration(cloud)
        assert o.stage_sr(cloud) == 0
        five = [h.features(w) for w in range(5)]
        if k in (1, 2):
            for w, c, i, rule in refused_edits(five):
                assert wm.rule_fault(c, w in WALKED) == (rule, i)
                if rule == 3:
                    assert i in wm.walk_mismatches(_lines(c), indices=[i]), "the device's stops and the literal walk part at point %d" % i
                args = {ODO_NAMES[w]: c}
                if w != 1:   # an admissible edit in the same call is not uploaded either
                    args["cornerPointsSharp"] = five[1][2:]
                with pytest.raises(vl.VloamError) as e:
                    h.set_odometry_input(**args)
                assert e.value.status == vl.ERR_INVALID and ("point %d:" % i) in str(e.value) and ODO_NAMES[w] in str(e.value), str(e.value)
                n_refused += 1
            for w in range(5):
                assert np.array_equal(h.features(w).view(np.uint32), five[w].view(np.uint32)), "cloud %d untouched" % w
        if k in (1, 2):
            qw, tw, _, _ = h.laser_odometry()
            o.stage_lo()
            oq, ot, _, _ = o.lo_pose()
            assert qdist(qw, oq) < POSE_TOL and np.linalg.norm(tw - ot) < POSE_TOL, "odometry pose, sweep %d" % k
            for outer in range(2):
                d = h.lo_debug(outer)
                oc, op = o.lo_corr(outer)
                assert np.array_equal(d["corner"], oc) and np.array_equal(d["plane"], op), "correspondences, sweep %d round %d" % (k, outer)
            own = [h.features(5), h.features(6), h.features(0)]
            for j in range(3):
                i = own[j].shape[0] // 2
                with pytest.raises(vl.VloamError) as e:
                    h.set_mapping_input(**{names[j]: _with_point(own[j], i, j, np.inf if j == 1 else np.nan)})
                assert e.value.status == vl.ERR_INVALID and ("point %d:" % i) in str(e.value) and names[j] in str(e.value), str(e.value)
                n_refused += 1
            qm, tm = h.laser_mapping()
            assert o.stage_map() == 0
            for which in (7, 8):
                assert np.array_equal(h.features(which)[:, :4].view(np.uint32), o.cloud(which)[:, :4].view(np.uint32)), "stack %d, sweep %d" % (which, k)
            oq, ot, _, _ = o.map_pose()
            assert qdist(qm, oq) < POSE_TOL and np.linalg.norm(tm - ot) < POSE_TOL, "map pose, sweep %d" % k
        else:
            _compare_sweep(h, o, k)
    assert n_refused == 2 * (5 + 6 + 3)
    _compare_maps(h, o)
    h.close()


def test_python_mirror_uploads_same_size_edits(vl, orc, sweeps):
    """vl.LidarOdometryMapping's stage objects with input() calls that carry same-size edits: an intensity-only edit of the first point of
    cornerPointsLessSharp, an interior nudge of surfPointsFlat, a nudged laserCloudSurfLast before LaserMapping.input.  Unedited clouds are
    handed back too (nothing to upload).  Poses, CornerLast / SurfLast and the map equal the oracle's with the same edits."""
    n, shape = 5, (64, 512)
    loam = vl.LidarOdometryMapping(0, with_mapping=1)
    o = orc.Oracle(with_mapping=True)
    for k in range(n):
        cloud = sweeps(shape[0], shape[1], k)
        loam.reset()
        loam.scan_registration.input(cloud)
        assert o.stage_sr(cloud) == 0
        five = list(loam.scan_registration.output())
        if k in (1, 3):
            ls = five[2].copy()
            ls[0, 3] += np.float32(0.03125)
            fl = five[3].copy()
            fl[fl.shape[0] // 2, 2] += np.float32(0.05)
            five[2], five[3] = ls, fl
            o.set_sr_cloud(2, ls)
            o.set_sr_cloud(3, fl)
        loam.laser_odometry.input(*five)
        for w in (2, 3):
            assert np.array_equal(loam.hd.features(w).view(np.uint32), np.ascontiguousarray(five[w]).view(np.uint32))
        loam.laser_odometry.solveLO()
        o.stage_lo()
        q, t, corner, surf, full, skip = loam.laser_odometry.output()
        oq, ot, _, _ = o.lo_pose()
        assert qdist(q, oq) < POSE_TOL and np.linalg.norm(t - ot) < POSE_TOL, "odometry pose, sweep %d" % k
        for which, c in ((5, corner), (6, surf)):
            assert np.array_equal(c.view(np.uint32), o.cloud(which).view(np.uint32))
        kw = {}
        if k in (2, 3):
            surf = surf.copy()
            surf[surf.shape[0] // 2, 2] += np.float32(0.05)
            kw["surf"] = surf
        loam.laser_mapping.input(corner, surf, full, q, t, skip)
        loam.laser_mapping.solveMapping()
        assert o.stage_map(**kw) == 0
        qm, tm = loam.laser_mapping.q_w_curr, loam.laser_mapping.t_w_curr
        oq, ot = o.map_published_pose()
        assert qdist(qm, oq) < POSE_TOL and np.linalg.norm(tm - ot) < POSE_TOL, "map pose, sweep %d" % k
    _compare_maps(loam.hd, o)
    loam.hd.close()
