"""-m gpu: per-sweep pose covariance rows (vloam_pose_cov_enable, c_api.h): eigenvectors, covariances and the VO solve's matrix.

Bounds.  The eigen-decomposition is checked against the device's own H (the pose information row; vo_H for the VO) with the bound
tests/test_gpu_pose_info.py applies to Jacobi eigenvalues: EIG_TOL = 1e-12, times lambda_max for the residual H V - V diag(eig) and for the
eigenvalues, as it stands for the dimensionless V^T V - I.  The covariance against numpy (eigh of the same H, the same truncation rule, the same
sigma^2 formula) within EIG_TOL x kappa x max |cov|, kappa = the condition number of the kept spectrum: the first-order perturbation of an
inverse, d(H^+) = H^+ dH H^+, |dH| <= EIG_TOL lambda_max, |H^+| = 1 / lambda_min.  An eigenvector against numpy's within
EIG_TOL lambda_max / gap (the first-order perturbation of an eigenvector).  The VO matrix against the oracle within the project's H_TOL = 1e-9.
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
from test_gpu_pose_info import EIG_TOL, H_TOL, H6, half_is_zero as info_half_is_zero, valid as info_valid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
STAGES = ("lo", "map", "vo")
SHAPES = [(16, 256), (64, 256)]
N_SWEEPS = 5


def cov_valid(vl, row, stage):
    return bool(row["flags"] & {"lo": vl.POSE_COV_LO_VALID, "map": vl.POSE_COV_MAP_VALID, "vo": vl.POSE_COV_VO_VALID}[stage])


def truncated(vl, row, stage):
    return bool(row["flags"] & {"lo": vl.POSE_COV_LO_TRUNCATED, "map": vl.POSE_COV_MAP_TRUNCATED, "vo": vl.POSE_COV_VO_TRUNCATED}[stage])


def half_is_zero(vl, row, stage):
    k = STAGES.index(stage)
    fields = ("eig", "V", "cov") + (("x", "cost", "H", "factors") if stage == "vo" else ())
    return all(not np.any(row[stage + "_" + f]) for f in fields) and row["rank"][k] == 0 and row["sigma2"][k] == 0 and \
        not cov_valid(vl, row, stage) and not truncated(vl, row, stage)


def problem(info, row, stage):
    """(H, cost, residual rows) of a stage as the device recorded them."""
    if stage == "vo":
        return row["vo_H"].reshape(6, 6), float(row["vo_cost"]), 2 * int(row["vo_factors"][0]) + int(row["vo_factors"][1])
    cnt = info[stage + "_factors"]
    return H6(info, stage), float(info[stage + "_cost"]), 3 * int(cnt[0]) + int(cnt[1])


def check_decomposition(vl, info, row, stage):
    H, _, _ = problem(info, row, stage)
    ev, V = row[stage + "_eig"], row[stage + "_V"].reshape(6, 6)
    ref = np.linalg.eigvalsh(H)
    lmax = max(abs(ref[-1]), abs(ref[0]))
    res = np.max(np.abs(H @ V - V * ev[None, :]))
    orth = np.max(np.abs(V.T @ V - np.eye(6)))
    derr = np.max(np.abs(ev - ref))
    print("%s sweep %d: |HV - VD| %.3g, |VtV - I| %.3g, |eig - numpy| %.3g (lambda_max %.3g)" % (stage, int(row["frame"]), res, orth, derr, lmax))
    assert res <= EIG_TOL * lmax and orth <= EIG_TOL and derr <= EIG_TOL * lmax, (stage, int(row["frame"]), res, orth, derr, lmax)
    assert np.all(np.diff(ev) >= 0), "ascending"
    for i in range(6):   # the component of largest magnitude of every column is positive, ties go to the lowest row (argmax: the first)
        assert V[np.argmax(np.abs(V[:, i])), i] > 0, (stage, i, V[:, i])


def check_covariance(vl, info, row, stage, thr=0.0):
    """rank, sigma2, cov and the flags against numpy on the device's own H, cost and counts.  Returns (eigenvalues, eigenvectors, kept) of numpy."""
    k = STAGES.index(stage)
    H, cost, res_rows = problem(info, row, stage)
    ev, V = np.linalg.eigh(H)
    keep = (ev >= max(thr, 1e-12 * ev[-1])) & (ev > 0)
    rank = int(keep.sum())
    assert row["rank"][k] == rank, (stage, int(row["frame"]), row["rank"], ev, thr)
    assert truncated(vl, row, stage) == (rank < 6)
    dof = res_rows - rank
    cov = row[stage + "_cov"].reshape(6, 6)
    assert cov_valid(vl, row, stage) == (dof > 0)
    if dof <= 0:
        assert row["sigma2"][k] == 0 and not np.any(cov)
        return ev, V, keep
    sigma2 = 2.0 * cost / dof
    assert abs(row["sigma2"][k] - sigma2) <= 4 * np.finfo(float).eps * sigma2, (row["sigma2"][k], sigma2)
    cov_ref = sigma2 * (V[:, keep] / ev[keep]) @ V[:, keep].T
    kappa = ev[keep][-1] / ev[keep][0]
    err = np.max(np.abs(cov - cov_ref))
    print("%s sweep %d: rank %d, sigma2 %.3g, kappa %.3g, |cov - numpy| / max |cov| %.3g" % (stage, int(row["frame"]), rank, sigma2, kappa, err / np.max(np.abs(cov_ref))))
    assert err <= EIG_TOL * kappa * np.max(np.abs(cov_ref)), (stage, int(row["frame"]), err, kappa)
    assert np.array_equal(cov, cov.T)
    return ev, V, keep


def drive(vl, clouds, info=True, cov=True, thr=(0.0, 0.0, 0.0), profile=False, **kw):
    h = vl.Handle(0, **kw)
    if info:
        h.enable_pose_info()
    if cov:
        h.pose_cov_enable(*thr)
    if profile:
        h.profile_kernel("*", 4096)
    for c in clouds:
        h.process_scan(c)
    h.sync()
    out = dict(info=h.pose_info() if info else None, cov=h.get_pose_cov() if cov else None, traj=h.trajectory(), map=h.get_map(), counts=h.counts(),
               table=h.profile_table() if profile else None)
    h.close()
    return out


_runs = {}


def street(vl, sweeps, shape, **kw):
    key = (shape, tuple(sorted(kw.items())))
    if key not in _runs:
        _runs[key] = drive(vl, [sweeps(shape[0], shape[1], k) for k in range(N_SWEEPS)], scan_line=shape[0], **kw)
    return _runs[key]


# ---------------------------------------------------------------------------------------------- 1. nothing else moves
@pytest.mark.parametrize("shape", SHAPES)
def test_poses_map_and_pose_info_rows_do_not_move(vl, sweeps, shape):
    on, ref = street(vl, sweeps, shape), street(vl, sweeps, shape, cov=False)
    assert on["traj"].tobytes() == ref["traj"].tobytes() and on["map"].shape == ref["map"].shape and on["map"].tobytes() == ref["map"].tobytes()
    assert on["info"].tobytes() == ref["info"].tobytes(), "the 832-byte rows, byte for byte"
    assert np.array_equal(on["cov"]["frame"], np.arange(N_SWEEPS))
    off = street(vl, sweeps, shape, info=False, cov=False)
    assert on["traj"].tobytes() == off["traj"].tobytes() and on["map"].tobytes() == off["map"].tobytes()


def test_batched_handle_does_not_move(vl, synth):
    seqs = [synth.SynthSequence(n_rings=64, n_azimuth=256, n_sweeps=8, seed_scene=s) for s in (11, 12, 13)]
    clouds = [[np.ascontiguousarray(q.sweep(k), dtype=np.float32) for k in range(N_SWEEPS)] for q in seqs]
    out = {}
    for cov in (False, True):
        h = vl.Handle(0, n_sessions=3, scan_line=64)
        h.enable_pose_info()
        if cov:
            h.pose_cov_enable()
        for k in range(N_SWEEPS):
            h.batch_process_scan([clouds[b][k] for b in range(3)])
        h.sync()
        out[cov] = [(h.select(b).pose_info().copy(), h.select(b).trajectory().copy(), h.select(b).get_map().copy(),
                     h.select(b).get_pose_cov().copy() if cov else None) for b in range(3)]
        h.close()
    for b in range(3):
        for a, r in zip(out[True][b][:3], out[False][b][:3]):
            assert a.shape == r.shape and a.tobytes() == r.tobytes(), b
        info, rows = out[True][b][0], out[True][b][3]
        assert np.array_equal(rows["frame"], np.arange(N_SWEEPS))
        for i, r in zip(info, rows):
            for stage in ("lo", "map"):
                if info_valid(vl, i, stage):
                    check_decomposition(vl, i, r, stage)
                    check_covariance(vl, i, r, stage)
                else:
                    assert half_is_zero(vl, r, stage)
    assert not np.array_equal(out[True][0][3]["lo_V"], out[True][1][3]["lo_V"]), "select picks the rows"


def test_a_handle_with_neither_product_launches_nothing_new(vl, sweeps):
    shape = SHAPES[1]
    plain = street(vl, sweeps, shape, info=False, cov=False, profile=True)
    both = street(vl, sweeps, shape, profile=True)
    vl.lib().vloam_profile_kernel_name.restype = C.c_char_p
    names = [vl.lib().vloam_profile_kernel_name(k) for k in range(vl.lib().vloam_profile_kernel_count())]
    assert names[-1] == b"k_pose_info_map" and not any(b"pose_cov" in n for n in names), "the event timer's table is what it was"
    launches = lambda t: {k: v[1] for k, v in t.items() if v[1]}   # noqa: E731
    assert not any("pose_" in k for k in launches(plain["table"]))
    assert {k: v for k, v in launches(both["table"]).items() if "pose_info" not in k} == launches(plain["table"])
    assert plain["counts"] == both["counts"]


# ---------------------------------------------------------------------------------------------- 2. + 3. decomposition and covariance of the LiDAR stages
@pytest.mark.parametrize("shape", SHAPES)
def test_eigen_decomposition_and_covariance(vl, sweeps, shape):
    d = street(vl, sweeps, shape)
    solved = 0
    for info, row in zip(d["info"], d["cov"]):
        assert half_is_zero(vl, row, "vo"), "sweeps driven by vloam_process_scan have no VO half"
        for stage in ("lo", "map"):
            if not info_valid(vl, info, stage):
                assert info_half_is_zero(info, stage) and half_is_zero(vl, row, stage)
                continue
            check_decomposition(vl, info, row, stage)
            check_covariance(vl, info, row, stage)
            # thresholds at 0 on the street scene: nothing is cut
            assert cov_valid(vl, row, stage) and not truncated(vl, row, stage) and row["rank"][STAGES.index(stage)] == 6
            solved += 1
    assert solved >= 2 * (N_SWEEPS - 1) - 1
    again = drive(vl, [sweeps(shape[0], shape[1], k) for k in range(N_SWEEPS)], scan_line=shape[0])
    assert again["cov"].tobytes() == d["cov"].tobytes(), "two runs, byte-identical rows"


def test_truncated_covariance_of_a_degenerate_sweep(vl, orc, synth):
    """The sweep tests/test_gpu_pose_info.py uses for LO_DEGENERATE (tests/degenerate_cases.py: wedge_sweep at sweep 3; two edge and one plane
    correspondence, so J has five independent rows and lambda_0 = 0 up to rounding).  On the oracle's matrix first: the gap between lambda_0 and
    lambda_1 must be wide enough for v_0 to be defined to better than 1e-4 under a perturbation of EIG_TOL lambda_max."""
    clouds = G.lo_sequence(synth, n=5, shape=(64, 256), far_at=(), wedge_at=(3,))
    o = P.OracleRun(orc, scan_line=64)
    for c in clouds:
        o.process(c)
    Ho, _ = o.matrix(o.lo_rows[3], o.lo_x[3])
    evo = np.linalg.eigvalsh(Ho)
    assert 3 * o.lo_rows[3][1] + o.lo_rows[3][2] > 5, "residual rows beyond the rank: sigma2 is defined"
    assert abs(evo[0]) < 1e-9 * evo[-1] and EIG_TOL * evo[-1] / (evo[1] - evo[0]) < 1e-4, evo
    thr = 0.5 * evo[1]   # above the smallest eigenvalue, below the next
    d = drive(vl, clouds, thr=(thr, 0.0, 0.0), scan_line=64)
    info, row = d["info"][3], d["cov"][3]
    assert info_valid(vl, info, "lo")
    check_decomposition(vl, info, row, "lo")
    ev, V, keep = check_covariance(vl, info, row, "lo", thr)
    assert row["rank"][0] == 5 and truncated(vl, row, "lo") and cov_valid(vl, row, "lo") and list(keep) == [False] + [True] * 5
    cov = row["lo_cov"].reshape(6, 6)
    kappa = ev[5] / ev[1]
    assert np.max(np.abs(cov @ V[:, 0])) <= EIG_TOL * kappa * np.max(np.abs(cov)), "the unobserved direction carries no covariance"
    v0 = V[:, 0] * (1.0 if V[np.argmax(np.abs(V[:, 0])), 0] > 0 else -1.0)   # numpy's, in the device's sign convention
    tol = EIG_TOL * ev[5] / (ev[1] - ev[0])
    print("v0 device", row["lo_V"].reshape(6, 6)[:, 0], "numpy", v0, "tol", tol)
    assert np.max(np.abs(row["lo_V"].reshape(6, 6)[:, 0] - v0)) <= tol
    for i, r in zip(d["info"], d["cov"]):   # the other sweeps of the run under the same threshold
        for stage in ("lo", "map"):
            if info_valid(vl, i, stage):
                check_decomposition(vl, i, r, stage)
                check_covariance(vl, i, r, stage, thr if stage == "lo" else 0.0)


# ---------------------------------------------------------------------------------------------- 4. the VO matrix against the oracle
def test_vo_matrix_vs_the_oracle_on_the_golden_frames(vl, orc, sweeps):
    g = np.load(os.path.join(HERE, "golden", "vloam_64x256_5frames.npz"))
    h = vl.Handle(0, with_mapping=1, detach_VO_LO=0)
    h.enable_pose_info()
    h.pose_cov_enable()
    h.vo_set_calib(g["cam_T_velo"], g["rect0_T_cam"], g["P_rect0"])
    h.set_extrinsics(g["base_T_cam0"], g["velo_T_cam0"])
    o = orc.VOOracle(g["cam_T_velo"], g["rect0_T_cam"], g["P_rect0"], remove_outlier=100)
    for k in range(5):
        c = np.zeros((g["in_%d" % k].shape[0], 4), dtype=np.float32)
        c[:, :3] = g["in_%d" % k]
        o.reset()
        o.process_point_cloud(c)
        if k == 0:
            h.process_frame(c)
            row = h.get_pose_cov(0, 1)[0]
            assert row["frame"] == 0 and half_is_zero(vl, row, "vo"), "the first frame has no VO solve"
            continue
        h.process_frame(c, g["prev_uv_%d" % k], g["curr_uv_%d" % k])
        r = h.vo_result()
        row, info = h.get_pose_cov(k, 1)[0], h.pose_info(k, 1)[0]
        assert row["frame"] == k
        assert np.array_equal(row["vo_x"], np.concatenate([r["angles"], r["t"]])), "vo_x is what vloam_get_vo_result returns"
        ro = o.solve(g["prev_uv_%d" % k], g["curr_uv_%d" % k], np.zeros(3), np.zeros(3))   # (the residual blocks do not depend on the start)
        rows = [[3, *m[2:7]] if m[0] == 32 else [4, *m[2:6]] for m in ro["match_debug"] if m[0] in (32, 22)]
        assert list(row["vo_factors"]) == [ro["counter32"], ro["counter22"]] and len(rows) == ro["counter32"] + ro["counter22"]
        s = orc.solve(rows, row["vo_x"][:3], row["vo_x"][3:], quaternion=False, huber_a=0.1, max_iters=0)
        err = P.rel_err(row["vo_H"].reshape(6, 6), s["H0"])
        cerr = abs(row["vo_cost"] - s["initial_cost"]) / s["initial_cost"]
        print("frame %d: factors %s, H err %.3g, cost err %.3g" % (k, row["vo_factors"], err, cerr))
        assert err < H_TOL and cerr < H_TOL, (k, err, cerr)
        check_decomposition(vl, info, row, "vo")
        check_covariance(vl, info, row, "vo")
        assert cov_valid(vl, row, "vo")
        for stage in ("lo", "map"):   # the LiDAR halves of a coupled frame
            if info_valid(vl, info, stage):
                check_decomposition(vl, info, row, stage)
                check_covariance(vl, info, row, stage)
    # a scan-driven sweep behind the frames: its VO half stays zero
    h.process_scan(sweeps(64, 256, 5))
    h.sync()
    rows = h.get_pose_cov()
    assert list(rows["frame"]) == list(range(6)) and half_is_zero(vl, rows[5], "vo") and not half_is_zero(vl, rows[4], "vo")
    h.close()


# ---------------------------------------------------------------------------------------------- 5. order and range refusals, checkpoints
def test_order_and_range_refusals_and_checkpoint(vl, sweeps):
    clouds = [sweeps(16, 256, k) for k in range(5)]
    h = vl.Handle(0, scan_line=16)
    rows1 = np.zeros(1, dtype=vl.POSE_COV_DTYPE)
    assert h.L.vloam_get_pose_cov(h.h, 0, 0, C.c_void_p(rows1.ctypes.data)) == vl.ERR_ORDER, "getter on a handle without the product"
    with pytest.raises(vl.VloamError) as e:
        h.pose_cov_device_ptr()
    assert e.value.status == vl.ERR_ORDER
    with pytest.raises(vl.VloamError) as e:
        h.pose_cov_enable()
    assert e.value.status == vl.ERR_ORDER and "vloam_pose_info_enable first" in str(e.value), "enable without pose information"
    h.enable_pose_info()
    h.process_scan(clouds[0])
    with pytest.raises(vl.VloamError) as e:
        h.pose_cov_enable()
    assert e.value.status == vl.ERR_ORDER, "enable after the first sweep"
    assert np.array_equal(h.pose_info()["frame"], [0]), "the pose information product goes on"
    h.close()
    h = vl.Handle(0, scan_line=16)
    h.enable_pose_info()
    h.pose_cov_enable()
    with pytest.raises(vl.VloamError) as e:
        h.pose_cov_enable()
    assert e.value.status == vl.ERR_ORDER and "already enabled" in str(e.value), "enabled once"
    for c in clouds[:3]:
        h.process_scan(c)
    for first, count in ((0, 4), (3, 1), (-1, 1)):
        with pytest.raises(vl.VloamError) as e:
            h.get_pose_cov(first, count)
        assert e.value.status == vl.ERR_INVALID, "a range beyond vloam_frame_count"
    assert np.array_equal(h.get_pose_cov(1, 2)["frame"], [1, 2])
    p, nbytes = h.pose_cov_device_ptr()
    assert p and nbytes == 2288 * h.cfg.max_frames
    whole3 = h.get_pose_cov().copy()
    data = h.checkpoint()
    h.close()
    # rows do not travel in a checkpoint: restored sweeps read frame == -1, later sweeps are written
    h = vl.Handle(0, scan_line=16)
    h.enable_pose_info()
    h.pose_cov_enable()
    h.restore(data)
    assert h.frame_count() == 3 and np.array_equal(h.get_pose_cov()["frame"], [-1, -1, -1]) and not np.any(h.get_pose_cov()["flags"])
    for c in clouds[3:]:
        h.process_scan(c)
    h.sync()
    rows, info = h.get_pose_cov(), h.pose_info()
    h.close()
    assert list(rows["frame"]) == [-1, -1, -1, 3, 4] and list(whole3["frame"]) == [0, 1, 2]
    for i, r in zip(info[3:], rows[3:]):
        for stage in ("lo", "map"):
            assert info_valid(vl, i, stage)
            check_decomposition(vl, i, r, stage)
            check_covariance(vl, i, r, stage)


# ---------------------------------------------------------------------------------------------- 6. tools/run_sequence.py --pose-cov
def test_run_sequence_tool(tmp_path):
    tool = [sys.executable, os.path.join(ROOT, "tools", "run_sequence.py"), "--azimuth", "512", "--mapping-skip-frame", "1"]
    new = {s + f for s in ("lo", "map", "vo") for f in ("_rank", "_sigma_t", "_sigma_r")}
    info_keys = {"lo_min_eig", "map_min_eig", "lo_degenerate", "map_degenerate"}

    def run(n, *extra):
        m = tmp_path / ("m%d%d.jsonl" % (n, len(extra)))
        r = subprocess.run(tool + ["--synthetic", str(n), "--out", str(tmp_path / "out"), "--metrics", str(m)] + list(extra), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return [json.loads(line) for line in open(m)]

    on = run(6, "--pose-cov")
    assert len(on) == 6 and all(new | info_keys <= set(rec) for rec in on), "--pose-cov implies --pose-info"
    assert all(on[0][k] is None for k in new)
    for rec in on[1:]:
        assert rec["lo_rank"] == 6 and rec["map_rank"] == 6 and rec["vo_rank"] is None and rec["vo_sigma_t"] is None and rec["vo_sigma_r"] is None
        assert all(0 < rec[s + f] < 1 for s in ("lo", "map") for f in ("_sigma_t", "_sigma_r")), rec
    off = run(2)
    assert [set(rec) for rec in off] == [set(rec) - new - info_keys for rec in on[:2]]
