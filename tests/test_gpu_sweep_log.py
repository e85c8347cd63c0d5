"""-m gpu: the opt-in per-sweep diagnostics log (vloam_limits_ext::sweep_log, vloam_get_sweep_log) against the unmodified CPU oracle.

One vloam_sweep_record per sweep, written by the stage streams themselves: the counts the reference keeps per frame (feature picks,
corner_correspondence / plane_correspondence, laserCloudCornerFromMapNum ...), the summaries of the four solves, "less correspondence"
(laser_odometry.cpp:452-455), "Map corner and surf num are not enough" (laser_mapping.cpp:448) and the error bits of THAT sweep."""
import numpy as np
import pytest

from degenerate_cases import lo_sequence
from test_gpu_batch import same_poses, sequences
from test_gpu_long_rings import one_ring

pytestmark = pytest.mark.gpu

INT_FIELDS = ["frame", "error_bits", "flags", "n_in", "n_cloud", "n_sharp", "n_less_sharp", "n_flat", "n_less_flat", "lo_corner_factors", "lo_plane_factors",
              "lo_iterations", "lo_termination", "n_corner_stack", "n_surf_stack", "n_map_corner", "n_map_surf", "map_corner_factors", "map_surf_factors",
              "map_iterations", "map_termination", "reserved"]
COST_FIELDS = ["lo_initial_cost", "lo_final_cost", "map_initial_cost", "map_final_cost"]


def oracle_rows(vl, o, clouds, skip=1, with_mapping=True):
    """What the oracle says about every sweep, in the record's layout."""
    rows = np.zeros(len(clouds), dtype=vl.SWEEP_RECORD_DTYPE)
    for k, cloud in enumerate(clouds):
        assert o.process(cloud) == 0
        r = rows[k]
        r["frame"], r["n_in"], r["n_cloud"] = k, cloud.shape[0], o.cloud(0).shape[0]
        r["n_sharp"], r["n_less_sharp"], r["n_flat"], r["n_less_flat"] = [o.cloud(w).shape[0] for w in (1, 2, 3, 4)]
        flags = 0
        if k == 0:
            assert o.lo_num_outer() == 0
            flags |= vl.SWEEP_FLAG_FIRST
        else:
            assert o.lo_num_outer() == 2
            for outer in range(2):
                c, p = o.lo_corr(outer)
                s = o.lo_solve(outer)
                r["lo_corner_factors"][outer], r["lo_plane_factors"][outer] = c.shape[0], p.shape[0]
                r["lo_iterations"][outer], r["lo_termination"][outer] = s["trace"].shape[0], s["termination"]
                r["lo_initial_cost"][outer], r["lo_final_cost"][outer] = s["initial_cost"], s["final_cost"]
                if c.shape[0] + p.shape[0] < 10:
                    flags |= (vl.SWEEP_FLAG_LO_LESS_CORR_0, vl.SWEEP_FLAG_LO_LESS_CORR_1)[outer]
        if with_mapping and (k + 1) % skip != 0:
            flags |= vl.SWEEP_FLAG_MAP_SKIPPED
        elif with_mapping:
            r["n_corner_stack"], r["n_surf_stack"], r["n_map_corner"], r["n_map_surf"] = [o.cloud(w).shape[0] for w in (7, 8, 9, 10)]
            if o.map_num_outer() == 0:   # the oracle's do_optimize
                flags |= vl.SWEEP_FLAG_MAP_NOT_OPTIMIZED
            else:
                assert o.map_num_outer() == 2
                for outer in range(2):
                    s = o.map_solve(outer)
                    r["map_corner_factors"][outer], r["map_surf_factors"][outer] = s["corner_num"], s["surf_num"]
                    r["map_iterations"][outer], r["map_termination"][outer] = s["trace"].shape[0], s["termination"]
                    r["map_initial_cost"][outer], r["map_final_cost"][outer] = s["initial_cost"], s["final_cost"]
        r["flags"] = flags
    return rows


def assert_ints(got, want, what=""):
    assert got.shape == want.shape, what
    for f in INT_FIELDS:
        assert np.array_equal(got[f], want[f]), "%s %s: %s, expected %s" % (what, f, got[f].tolist(), want[f].tolist())


def assert_costs(got, want, what=""):
    """The bars of tests/test_gpu_laser_odometry.py::compare_outer for residual-derived quantities: the initial cost to 1e-10 (1 + cost), a
    cost of the iteration trace (the final cost is the best of them) to rtol 1e-8 / atol 1e-12."""
    for f in ("lo_initial_cost", "map_initial_cost"):
        print(what, f, "max |dev - oracle| / (1 + oracle) =", float(np.max(np.abs(got[f] - want[f]) / (1 + want[f]))))
        assert np.all(np.abs(got[f] - want[f]) < 1e-10 * (1 + want[f])), (what, f)
    for f in ("lo_final_cost", "map_final_cost"):
        print(what, f, "max rel =", float(np.max(np.abs(got[f] - want[f]) / np.maximum(want[f], 1e-300))))
        assert np.allclose(got[f], want[f], rtol=1e-8, atol=1e-12), (what, f)


def run(vl, clouds, **kw):
    h = vl.Handle(0, **kw)
    for c in clouds:
        h.process_scan(c)
    return h


@pytest.mark.parametrize("shape", [(16, 512), (64, 512)])
def test_parity_with_the_oracle(vl, orc, sweeps, shape):
    clouds = [sweeps(shape[0], shape[1], k) for k in range(8)]
    h = run(vl, clouds, scan_line=shape[0], sweep_log=1)
    h.sync()
    got = h.sweep_log()
    want = oracle_rows(vl, orc.Oracle(scan_line=shape[0]), clouds)
    assert_ints(got, want, "%d x %d" % shape)
    assert_costs(got, want, "%d x %d" % shape)
    assert got["flags"][0] == vl.SWEEP_FLAG_FIRST | vl.SWEEP_FLAG_MAP_NOT_OPTIMIZED and not np.any(got["flags"][1:] & vl.SWEEP_FLAG_FIRST)
    assert np.all(got["error_bits"] == 0) and np.all(got["lo_iterations"][1:] > 0) and np.all(got["map_corner_factors"][1:] > 0)
    p, nbytes = h.sweep_log_device_ptr()
    assert p and nbytes == h.cfg.max_frames * 192


def test_error_bits_belong_to_the_sweep_that_raised_them(vl, sweeps):
    good = [sweeps(64, 512, k) for k in range(7)]
    # a scan line of 4 100 points on a default handle (ring capacity 4 096): dropped, loudly, in sweep 3 only
    clouds = good[:6]
    clouds[3] = one_ring(4100, noise=0.05)
    h = run(vl, clouds, sweep_log=1)
    with pytest.raises(vl.VloamError) as ei:
        h.sync()
    assert ei.value.status == vl.ERR_CAPACITY
    assert "a ring held more than 4096 points (dropped) in at least one sweep since the last vloam_sync" in str(ei.value)
    h.sync()   # reported once, as ever
    rows = h.sweep_log()
    assert rows["frame"].tolist() == list(range(6)) and rows["n_in"][3] == 4100
    assert (rows["error_bits"] & vl.SWEEP_RING_TOO_LONG).tolist() == [0, 0, 0, vl.SWEEP_RING_TOO_LONG, 0, 0]
    assert not np.any(rows["error_bits"] & vl.SWEEP_EMPTY)
    # a separate run with one sweep whose points all lie inside minimum_range (5 m)
    clouds = good[:7]
    clouds[4] = one_ring(2000, radius=1.0)
    h = run(vl, clouds, sweep_log=1)
    with pytest.raises(vl.VloamError) as ei:
        h.sync()
    assert ei.value.status == vl.ERR_EMPTY
    rows = h.sweep_log()
    assert rows["frame"].tolist() == list(range(7)) and rows["n_cloud"][4] == 0
    assert (rows["error_bits"] & vl.SWEEP_EMPTY).tolist() == [0, 0, 0, 0, vl.SWEEP_EMPTY, 0, 0]
    assert not np.any(rows["error_bits"] & vl.SWEEP_RING_TOO_LONG)


def test_skipped_mapping_sweeps(vl, orc, sweeps):
    clouds = [sweeps(64, 512, k) for k in range(8)]
    h = run(vl, clouds, sweep_log=1, mapping_skip_frame=2)
    h.sync()
    got = h.sweep_log()
    o = orc.Oracle(mapping_skip_frame=2)
    want = oracle_rows(vl, o, clouds, skip=2)
    assert_ints(got, want, "skip 2")
    assert_costs(got, want, "skip 2")
    skipped = (got["flags"] & vl.SWEEP_FLAG_MAP_SKIPPED) != 0
    assert skipped.tolist() == [(k + 1) % 2 != 0 for k in range(8)]
    for f in ("map_corner_factors", "map_surf_factors", "map_iterations", "map_termination", "map_initial_cost", "map_final_cost"):
        assert not np.any(got[f][skipped]), f
    t = h.trajectory()
    qw, tw, _, _ = o.lo_pose()
    qm, tm = o.map_published_pose()
    assert same_poses(t[-1:, :7], np.concatenate([qw, tw])[None, :], 1e-8) and same_poses(t[-1:, 7:], np.concatenate([qm, tm])[None, :], 1e-8)


def test_less_correspondence(vl, orc, synth):
    """An open-field sweep (tests/degenerate_cases.py): sweep 3 finds nothing of sweep 2 within 5 m, sweep 4 nothing of sweep 3; sweep 5 is a wedge
    with a handful of correspondences."""
    clouds = lo_sequence(synth, n=7, far_at=(3,), wedge_at=(5,))
    h = run(vl, clouds, sweep_log=1, with_mapping=0)
    h.sync()
    got = h.sweep_log()
    want = oracle_rows(vl, orc.Oracle(with_mapping=False), clouds, with_mapping=False)
    assert_ints(got, want, "open field")
    less = vl.SWEEP_FLAG_LO_LESS_CORR_0 | vl.SWEEP_FLAG_LO_LESS_CORR_1
    n = want["lo_corner_factors"] + want["lo_plane_factors"]
    assert np.any(n[1:] < 10) and np.any(n[1:] >= 10)
    for k in range(1, 7):
        expect = (vl.SWEEP_FLAG_LO_LESS_CORR_0 if n[k, 0] < 10 else 0) | (vl.SWEEP_FLAG_LO_LESS_CORR_1 if n[k, 1] < 10 else 0)
        assert got["flags"][k] & less == expect, (k, n[k].tolist(), int(got["flags"][k]))
    # without a mapping stage the odometry completes the row and the mapping fields stay 0
    assert got["frame"].tolist() == list(range(7)) and not np.any(got["n_corner_stack"]) and not np.any(got["flags"] & vl.SWEEP_FLAG_MAP_SKIPPED)


def test_batched_sessions_log_what_the_sequences_log_alone(vl, synth):
    n = 8
    seqs = sequences(synth, 2, n)
    hb = vl.Handle(0, n_sessions=2, sweep_log=1)
    for k in range(n):
        hb.batch_process_scan([seqs[b][k] for b in range(2)])
    hb.sync()
    rows = []
    for b in range(2):
        hs = run(vl, seqs[b], sweep_log=1)
        hs.sync()
        rows.append(hb.select(b).sweep_log())
        assert_ints(rows[b], hs.sweep_log(), "session %d" % b)
    assert not np.array_equal(rows[0]["n_cloud"], rows[1]["n_cloud"]), "the sessions are different sequences"


def test_rows_can_be_read_while_the_pipeline_runs(vl, sweeps):
    clouds = [sweeps(64, 512, k) for k in range(16)]
    ref = run(vl, clouds, sweep_log=1)
    ref.sync()
    want = ref.sweep_log()
    h = run(vl, clouds[:12], sweep_log=1)   # no vloam_sync
    first = h.sweep_log(0, 4)
    assert first["frame"].tolist() == [0, 1, 2, 3]
    assert_ints(first, want[:4], "rows 0-3 read behind 12 enqueued sweeps")
    for c in clouds[12:]:
        h.process_scan(c)
    h.sync()
    got = h.sweep_log()
    assert got.shape == (16,)
    assert_ints(got, want, "all 16")
    with pytest.raises(vl.VloamError) as ei:
        h.sweep_log(10, 7)
    assert ei.value.status == vl.ERR_INVALID


def test_off_by_default_and_no_change_to_results_when_on(vl, sweeps):
    clouds = [sweeps(64, 512, k) for k in range(8)]
    off = run(vl, clouds)
    on = run(vl, clouds, sweep_log=1)
    off.sync(); on.sync()
    for call in (off.sweep_log, off.sweep_log_device_ptr):
        with pytest.raises(vl.VloamError) as ei:
            call()
        assert ei.value.status == vl.ERR_ORDER and "sweep_log" in str(ei.value)
    a, b = off.trajectory(), on.trajectory()
    assert a.shape == (8, 14) and np.array_equal(a, b)
    for which in range(5):
        fa, fb = off.features(which), on.features(which)
        assert fa.shape == fb.shape and fa.shape[0] > 0 and np.array_equal(fa.view(np.uint32), fb.view(np.uint32)), which
