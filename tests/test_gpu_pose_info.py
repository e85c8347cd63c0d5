"""-m gpu: per-sweep pose information matrices and degeneracy flags (vloam_pose_info_enable, c_api.h) against the CPU oracle.

For every sweep and LiDAR stage the device's record holds J^T J (after the loss corrector, tangent space of EigenQuaternionParameterization) of
the LAST outer round's problem at the pose that round returned.  The oracle's counterpart: its own factor set of that round
(tests/pose_info_cases.py) handed to orc_solve, started at the DEVICE's pose, whose H0 / initial cost are that matrix and cost.  Bound: the
one the project uses for LMRecord::H0 (tests/test_gpu_laser_odometry.py:34-35), max |dH| / sqrt(diag x diag) < 1e-9; costs to the same
relative bound.  Eigenvalues against numpy.linalg.eigvalsh of the device's own matrix: cyclic Jacobi is backward stable with an absolute
error of order n eps |H| per sweep; n = 6 and at most a dozen sweeps give ~4e-14 lambda_max, asserted at 1e-12 lambda_max.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import degenerate_cases as G
import pose_info_cases as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H_TOL = 1e-9          # tests/test_gpu_laser_odometry.py:35
EIG_TOL = 1e-12       # x lambda_max (module docstring)
COST_VS_LOG = 1e-12   # the same sum at the same point in another order


def drive(vl, clouds, stagewise=False, pose_info=True, thr=(0.0, 0.0), want_map=False, **kw):
    """One device run.  stagewise: the façade stage by stage (keeps what the odometry / mapping calls return), else vloam_process_scan."""
    h = vl.Handle(0, **kw)
    if pose_info:
        h.enable_pose_info(*thr)
    lo_ret, map_ret = [], []
    for c in clouds:
        if stagewise:
            h.reset_frame()
            h.scan_registration(c)
            _, _, ql, tl = h.laser_odometry()
            lo_ret.append(np.concatenate([ql, tl]))
            q, t = h.laser_mapping()
            map_ret.append(np.concatenate([q, t]))
        else:
            h.process_scan(c)
    h.sync()
    out = dict(rows=h.pose_info() if pose_info else None, traj=h.trajectory(), lo_ret=lo_ret, map_ret=map_ret,
               log=h.sweep_log() if kw.get("sweep_log") else None, map=h.get_map() if want_map else None)
    h.close()
    return out


def H6(row, stage):
    return row[stage + "_H"].reshape(6, 6)


def valid(vl, row, stage):
    return bool(row["flags"] & (vl.POSE_INFO_LO_VALID if stage == "lo" else vl.POSE_INFO_MAP_VALID))


def half_is_zero(row, stage):
    return all(not np.any(row[stage + "_" + f]) for f in ("x", "cost", "H", "eig", "factors"))


def check_eigenvalues(vl, rows):
    for r in rows:
        for stage in ("lo", "map"):
            if not valid(vl, r, stage):
                assert half_is_zero(r, stage)
                continue
            H, ev = H6(r, stage), r[stage + "_eig"]
            assert np.array_equal(H, H.T), "H is symmetric"
            assert np.all(np.diff(ev) >= 0), "ascending"
            ref = np.linalg.eigvalsh(H)
            assert np.max(np.abs(ev - ref)) <= EIG_TOL * max(abs(ref[-1]), abs(ref[0])), (stage, int(r["frame"]), ev, ref)


def check_flags_against_thresholds(vl, rows, thr):
    for r in rows:
        for stage, t, bit in (("lo", thr[0], vl.POSE_INFO_LO_DEGENERATE), ("map", thr[1], vl.POSE_INFO_MAP_DEGENERATE)):
            want = valid(vl, r, stage) and t > 0 and r[stage + "_eig"][0] < t
            assert bool(r["flags"] & bit) == bool(want), (stage, int(r["frame"]), r[stage + "_eig"][0], t)


def rows_close(vl, a, b):
    """Two device runs of the same sequence whose solves add in another order (batch, stack tier, restored handle): the test-1 bound."""
    assert a.shape == b.shape
    for ra, rb in zip(a, b):
        assert ra["frame"] == rb["frame"] and ra["flags"] == rb["flags"]
        assert np.array_equal(ra["lo_factors"], rb["lo_factors"]) and np.array_equal(ra["map_factors"], rb["map_factors"])
        for stage in ("lo", "map"):
            if not valid(vl, ra, stage):
                assert half_is_zero(ra, stage) and half_is_zero(rb, stage)
                continue
            assert P.rel_err(H6(ra, stage), H6(rb, stage)) < H_TOL, (stage, int(ra["frame"]))
            assert abs(ra[stage + "_cost"] - rb[stage + "_cost"]) <= H_TOL * (1e-300 + abs(rb[stage + "_cost"])) + 1e-18
            assert np.max(np.abs(ra[stage + "_x"] - rb[stage + "_x"])) < H_TOL
            assert np.max(np.abs(ra[stage + "_eig"] - rb[stage + "_eig"])) <= H_TOL * abs(rb[stage + "_eig"][-1])


_runs = {}


def street_run(vl, orc, sweeps, shape, n):
    """Device (stage-wise, sweep log on) and oracle through the same sweeps, once per shape."""
    key = (shape, n)
    if key not in _runs:
        clouds = [sweeps(shape[0], shape[1], k) for k in range(n)]
        d = drive(vl, clouds, stagewise=True, scan_line=shape[0], sweep_log=1)
        o = P.OracleRun(orc, scan_line=shape[0])
        for c in clouds:
            o.process(c)
        _runs[key] = (d, o)
    return _runs[key]


SHAPES = [((16, 256), 5), ((64, 256), 4), ((64, 2048), 2)]


@pytest.mark.parametrize("shape,n", SHAPES)
def test_matrix_cost_and_counts_vs_the_oracle(vl, orc, sweeps, shape, n):
    d, o = street_run(vl, orc, sweeps, shape, n)
    rows = d["rows"]
    assert rows.shape[0] == n and np.array_equal(rows["frame"], np.arange(n))
    solved = 0
    for k, r in enumerate(rows):
        for stage, oracle_rows, ret in (("lo", o.lo_rows[k], d["lo_ret"][k]), ("map", o.map_rows[k], d["traj"][k, 7:14])):
            assert valid(vl, r, stage) == (oracle_rows is not None), (stage, k)
            if oracle_rows is None:
                assert half_is_zero(r, stage)
                continue
            x = r[stage + "_x"]
            assert np.array_equal(x, ret), "%s_x of sweep %d is the pose the stage returned, bit for bit" % (stage, k)
            if stage == "map":
                assert np.array_equal(x, d["map_ret"][k])
            H_orc, cost_orc = o.matrix(oracle_rows, x)   # started at the DEVICE's pose
            err = P.rel_err(H6(r, stage), H_orc)
            cerr = abs(r[stage + "_cost"] - cost_orc) / cost_orc
            print("%s sweep %d: factors %s, H err %.3g, cost err %.3g" % (stage, k, r[stage + "_factors"], err, cerr))
            assert err < H_TOL, (stage, k, err)
            assert cerr < H_TOL, (stage, k, r[stage + "_cost"], cost_orc)
            assert list(r[stage + "_factors"]) == [oracle_rows[1], oracle_rows[2]], (stage, k)
            solved += 1
    assert solved >= 2 * (n - 1) - 1


@pytest.mark.parametrize("shape,n", SHAPES)
def test_cost_and_counts_equal_the_sweep_log(vl, orc, sweeps, shape, n):
    d, _ = street_run(vl, orc, sweeps, shape, n)
    for r, lg in zip(d["rows"], d["log"]):
        assert valid(vl, r, "lo") == (not lg["flags"] & vl.SWEEP_FLAG_FIRST)
        assert valid(vl, r, "map") == (not lg["flags"] & (vl.SWEEP_FLAG_MAP_SKIPPED | vl.SWEEP_FLAG_MAP_NOT_OPTIMIZED))
        for stage, kinds in (("lo", ("lo_corner_factors", "lo_plane_factors")), ("map", ("map_corner_factors", "map_surf_factors"))):
            if not valid(vl, r, stage):
                continue
            final = lg[stage + "_final_cost"][1]
            assert abs(r[stage + "_cost"] - final) <= COST_VS_LOG * final, (stage, int(r["frame"]), r[stage + "_cost"], final)
            assert list(r[stage + "_factors"]) == [lg[kinds[0]][1], lg[kinds[1]][1]]


@pytest.mark.parametrize("shape,n", SHAPES)
def test_eigenvalues_vs_numpy(vl, orc, sweeps, shape, n):
    d, _ = street_run(vl, orc, sweeps, shape, n)
    check_eigenvalues(vl, d["rows"])


def test_degeneracy_flags(vl, orc, synth, sweeps):
    """A sweep that sees almost nothing of the sweep before (tests/degenerate_cases.py: wedge_sweep, a handful of correspondences): the odometry
    problem has three unobservable directions.  Asserted on the oracle's matrix first; thresholds from it; the street sequence stays clear.
    (The ground-only sequence of tests/branch_cases.py does not qualify: its noise edge features give lambda_4 / lambda_3 = 400 - 450 in the
    odometry and 80 - 230 in the mapping on the oracle, the rotation / translation scale gap every street sweep has too; the wedge sweep gives
    1.9e4 with three correspondences.)"""
    clouds = G.lo_sequence(synth, n=5, shape=(64, 256), far_at=(), wedge_at=(3,))
    o = P.OracleRun(orc, scan_line=64)
    for c in clouds:
        o.process(c)
    H, _ = o.matrix(o.lo_rows[3], o.lo_x[3])
    ev = np.linalg.eigvalsh(H)
    assert ev[2] > 0 and ev[3] / ev[2] >= 1e3, ev
    t = float(np.sqrt(ev[2] * ev[3]))
    thr = (t, t)
    rows = drive(vl, clouds, thr=thr, scan_line=64)["rows"]
    assert rows[3]["flags"] & vl.POSE_INFO_LO_VALID and rows[3]["flags"] & vl.POSE_INFO_LO_DEGENERATE, (rows[3]["flags"], rows[3]["lo_eig"])
    check_flags_against_thresholds(vl, rows, thr)
    check_eigenvalues(vl, rows)
    street = drive(vl, [sweeps(64, 256, k) for k in range(4)], thr=thr, scan_line=64)["rows"]
    assert not np.any(street["flags"] & (vl.POSE_INFO_LO_DEGENERATE | vl.POSE_INFO_MAP_DEGENERATE)), (street["flags"], street["lo_eig"][:, 0], street["map_eig"][:, 0])
    assert np.all(street["flags"][1:] & vl.POSE_INFO_LO_VALID) and np.all(street["flags"][1:] & vl.POSE_INFO_MAP_VALID)
    check_flags_against_thresholds(vl, street, thr)


def test_validity_flags(vl, orc, synth, sweeps):
    LO, MAP = vl.POSE_INFO_LO_VALID, vl.POSE_INFO_MAP_VALID
    clouds = [sweeps(16, 256, k) for k in range(4)]
    # the first sweep: no odometry solve, an empty map
    d, _ = street_run(vl, orc, sweeps, (16, 256), 5)
    r0 = d["rows"][0]
    assert r0["frame"] == 0 and r0["flags"] == 0 and half_is_zero(r0, "lo") and half_is_zero(r0, "map")
    # mapping_skip_frame = 2: sweeps 0 and 2 are not mapped, sweep 1 meets an empty map
    s = drive(vl, clouds, scan_line=16, mapping_skip_frame=2, sweep_log=1)
    rows, log = s["rows"], s["log"]
    assert np.array_equal(rows["frame"], np.arange(4))
    assert [bool(f & MAP) for f in rows["flags"]] == [False, False, False, True] and [bool(f & LO) for f in rows["flags"]] == [False, True, True, True]
    assert log[0]["flags"] & vl.SWEEP_FLAG_MAP_SKIPPED and log[2]["flags"] & vl.SWEEP_FLAG_MAP_SKIPPED and log[1]["flags"] & vl.SWEEP_FLAG_MAP_NOT_OPTIMIZED
    for k in (0, 1, 2):
        assert half_is_zero(rows[k], "map")
    check_eigenvalues(vl, rows)
    # no mapping stage: the odometry stamps the row
    rows = drive(vl, clouds, scan_line=16, with_mapping=0)["rows"]
    assert np.array_equal(rows["frame"], np.arange(4)) and not np.any(rows["flags"] & MAP) and all(half_is_zero(r, "map") for r in rows)
    assert [bool(f & LO) for f in rows["flags"]] == [False, True, True, True]
    # "Map corner and surf num are not enough" on mapped sweeps with a NON-empty map (tests/degenerate_cases.py); no plane factor at all in the odometry
    s = drive(vl, G.sparse_map_sequence(synth, n=5), scan_line=16, sweep_log=1)
    rows, log = s["rows"], s["log"]
    assert [bool(f & MAP) for f in rows["flags"]] == [False, False, False, True, True]
    assert all(log[k]["flags"] & vl.SWEEP_FLAG_MAP_NOT_OPTIMIZED for k in (0, 1, 2)) and log[1]["n_map_surf"] > 0
    assert all(half_is_zero(rows[k], "map") for k in (0, 1, 2))
    assert all(r["lo_factors"][0] > 0 and r["lo_factors"][1] == 0 for r in rows[1:]), rows["lo_factors"]
    for r, lg in zip(rows[1:], log[1:]):
        assert abs(r["lo_cost"] - lg["lo_final_cost"][1]) <= COST_VS_LOG * lg["lo_final_cost"][1]
    # stage-wise driving: a sweep whose mapping the caller left out is never completed
    h = vl.Handle(0, scan_line=16)
    h.enable_pose_info()
    for k, c in enumerate(clouds[:3]):
        h.scan_registration(c); h.laser_odometry()   # (no vloam_reset_frame: the next sweep's scan registration closes a sweep that ended after its odometry)
        if k != 1:
            h.laser_mapping()
    rows = h.pose_info()
    assert list(rows["frame"]) == [0, -1, 2] and rows[1]["flags"] == LO and half_is_zero(rows[1], "map")
    h.close()


def test_batch_sessions_equal_single_runs(vl, synth):
    seqs = [synth.SynthSequence(n_rings=64, n_azimuth=256, n_sweeps=8, seed_scene=s) for s in (11, 12, 13)]
    clouds = [[np.ascontiguousarray(q.sweep(k), dtype=np.float32) for k in range(4)] for q in seqs]
    h = vl.Handle(0, n_sessions=3, scan_line=64)
    h.enable_pose_info()
    for k in range(4):
        h.batch_process_scan([clouds[b][k] for b in range(3)])
    h.sync()
    batch = [h.select(b).pose_info().copy() for b in range(3)]
    h.close()
    assert not np.array_equal(batch[0]["lo_H"], batch[1]["lo_H"]) and not np.array_equal(batch[1]["map_H"], batch[2]["map_H"]), "select picks the rows"
    for b in range(3):
        alone = drive(vl, clouds[b], scan_line=64)["rows"]
        assert np.any(alone["flags"] == (vl.POSE_INFO_LO_VALID | vl.POSE_INFO_MAP_VALID))
        rows_close(vl, batch[b], alone)
        check_eigenvalues(vl, batch[b])


def test_large_stack_tier(vl, orc, sweeps):
    """max_surf_stack_points = 32768: the mapping table has 8192 + 32768 slots and the capacity reaches the kernel at run time."""
    d, _ = street_run(vl, orc, sweeps, (64, 256), 4)
    tier = drive(vl, [sweeps(64, 256, k) for k in range(4)], stagewise=True, scan_line=64, max_surf_stack_points=32768)["rows"]
    rows_close(vl, tier, d["rows"])
    check_eigenvalues(vl, tier)


def test_determinism_and_non_interference(vl, sweeps):
    clouds = [sweeps(64, 256, k) for k in range(5)]
    a = drive(vl, clouds, scan_line=64, want_map=True)
    b = drive(vl, clouds, scan_line=64, want_map=True)
    assert a["rows"].tobytes() == b["rows"].tobytes(), "two runs, byte-identical rows"
    off = drive(vl, clouds, pose_info=False, scan_line=64, want_map=True)
    assert a["traj"].tobytes() == off["traj"].tobytes() and a["map"].shape == off["map"].shape and a["map"].tobytes() == off["map"].tobytes()


def test_lifecycle_and_checkpoint(vl, orc, sweeps):
    clouds = [sweeps(16, 256, k) for k in range(5)]
    whole = drive(vl, clouds, scan_line=16)["rows"]
    h = vl.Handle(0, scan_line=16)
    rows1 = np.zeros(1, dtype=vl.POSE_INFO_DTYPE)
    assert h.L.vloam_get_pose_info(h.h, 0, 0, C.c_void_p(rows1.ctypes.data)) == vl.ERR_ORDER, "getter on a handle without the product"
    with pytest.raises(vl.VloamError) as e:
        h.pose_info_device_ptr()
    assert e.value.status == vl.ERR_ORDER
    h.process_scan(clouds[0])
    with pytest.raises(vl.VloamError) as e:
        h.enable_pose_info()
    assert e.value.status == vl.ERR_ORDER, "enable after the first sweep"
    h.close()
    h = vl.Handle(0, scan_line=16)
    h.enable_pose_info()
    with pytest.raises(vl.VloamError) as e:
        h.enable_pose_info()
    assert e.value.status == vl.ERR_ORDER, "enabled once"
    for c in clouds[:3]:
        h.process_scan(c)
    for first, count in ((0, 4), (3, 1), (-1, 1)):
        with pytest.raises(vl.VloamError) as e:
            h.pose_info(first, count)
        assert e.value.status == vl.ERR_INVALID, "a range beyond vloam_frame_count"
    assert np.array_equal(h.pose_info(1, 2)["frame"], [1, 2])
    p, nbytes = h.pose_info_device_ptr()
    assert p and nbytes == 832 * h.cfg.max_frames
    data = h.checkpoint()
    h.close()
    # rows do not travel in a checkpoint: restored sweeps read frame == -1, later sweeps are written normally
    plain = vl.Handle(0, scan_line=16)
    for c in clouds[:3]:
        plain.process_scan(c)
    assert len(plain.checkpoint()) == len(data), "checkpoint sizes do not depend on the product"
    plain.close()
    h = vl.Handle(0, scan_line=16)
    h.enable_pose_info()
    h.restore(data)
    assert h.frame_count() == 3 and np.array_equal(h.pose_info()["frame"], [-1, -1, -1]) and not np.any(h.pose_info()["flags"])
    for c in clouds[3:]:
        h.process_scan(c)
    h.sync()
    rows = h.pose_info()
    h.close()
    assert list(rows["frame"]) == [-1, -1, -1, 3, 4]
    rows_close(vl, rows[3:], whole[3:])


def test_run_sequence_tool(tmp_path):
    """tools/run_sequence.py --pose-info adds four metrics per frame; without the flag the keys are what they were."""
    tool = [sys.executable, os.path.join(ROOT, "tools", "run_sequence.py"), "--azimuth", "512", "--mapping-skip-frame", "1"]
    new = {"lo_min_eig", "map_min_eig", "lo_degenerate", "map_degenerate"}

    def run(n, *extra):
        m = tmp_path / ("m%d%d.jsonl" % (n, len(extra)))
        r = subprocess.run(tool + ["--synthetic", str(n), "--out", str(tmp_path / "out"), "--metrics", str(m)] + list(extra), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return [json.loads(line) for line in open(m)]

    on = run(6, "--pose-info", "--lo-min-eig", "1e9")
    assert len(on) == 6 and all(new <= set(rec) for rec in on)
    assert on[0]["lo_min_eig"] is None and on[0]["map_min_eig"] is None and not on[0]["lo_degenerate"]
    assert all(rec["lo_min_eig"] > 0 and rec["map_min_eig"] > 0 and rec["lo_degenerate"] and not rec["map_degenerate"] for rec in on[1:])
    off = run(2)
    assert [set(rec) for rec in off] == [set(rec) - new for rec in on[:2]]
