"""CPU: the oracle's coupled frame loop (oracle/orc_vloam.py over orc.py) and the transform arithmetic of kitti_io.VloamTF against the
REFERENCE'S OWN vloam_tf.cpp and lidar_odometry_mapping.cpp, compiled unmodified next to scan registration, laser odometry, laser mapping
and the visual odometry (oracle/_ref/libref_vloam.so through oracle/ref.py; harness oracle/ref_vloam_harness.cpp, which restates the 25
lines of vloam_main_node.cpp's callback()).  One VloamTF is shared by both halves, so the cycle solveNlsAll -> VO2VeloAndBase -> solveLO
(both outer rounds) -> LaserOdometry::publish -> the next frame's solveNlsAll start runs on the reference's text.

Bit for bit: the five scan-registration clouds, the VO rows (kind, depth0, observations) and counters, the odometry's correspondences of
both outer rounds (compare_odometry of tests/test_ref_laser_odometry.py), the parameters both rounds start from (velo_last_VOT_velo_curr
as tf2 reads it back in combined mode, the previous result in detached mode), skip_frame and the hand-over clouds, the row text.
To the existing bars: every transform of VloamTF and the LO / mapping poses to POSE_TOL = 1e-8 (x frame index for accumulated poses) of
tests/test_ref_laser_odometry.py / test_ref_laser_mapping.py, frame 1 included; the VO solve to POSE_TOL of
tests/test_ref_visual_odometry.py; the VO's START from the prior to POSE_TOL, at frame 1 — and for nothing else — to the 1e-7 that
tests/test_oracle_vloam.py documents (2 acos(w) next to w = 1).
The oracle's odometry is handed the prior as the reference reads it back out of its tf2 transform (< 1e-15 from
what was stored) AFTER the oracle's own velo_last_VOT_velo_curr has been compared with it, so that the rounds start from the same bits.
NaN is compared by position.

What the degenerate scenario records (nothing assumed): see test_degenerate_frames.

Skips: only when neither the reference checkout nor a built oracle/_ref/libref_vloam.so exists.
"""
import os

import numpy as np
import pytest

import ref_vloam_cases as cases
from test_ref_laser_odometry import POSE_TOL, compare_odometry, qdist, same_cloud

import ref

pytestmark = pytest.mark.skipif(not ref.vloam_available(), reason=ref.SKIP_REASON)

HERE = os.path.dirname(os.path.abspath(__file__))
STEMS = {"combined": "ref_vloam_combined", "detached": "ref_vloam_detached", "degenerate": "ref_vloam_degenerate", "extrinsics": "ref_vloam_extrinsics"}
FRAME1_START = 1e-7     # tests/test_oracle_vloam.py::test_coupling_carries_the_motion_both_ways
MAXIMA = {}


def note(key, v):
    MAXIMA[key] = max(MAXIMA.get(key, 0.0), float(v))


def tf_err(row12, T):
    """max |difference| between a recorded transform (basis row-major, origin) and an oracle TF / 4 x 4; NaN must sit at the same places."""
    m, o = (T.m, T.o) if hasattr(T, "m") else (T[:3, :3], T[:3, 3])
    got = np.concatenate([np.asarray(m).reshape(-1), np.asarray(o)])
    assert np.array_equal(np.isnan(got), np.isnan(row12)), "NaN at other places: %s vs %s" % (got, row12)
    ok = ~np.isnan(got)
    return float(np.max(np.abs(got[ok] - row12[ok]), initial=0.0))


class LoamView:
    """ref.Vloam seen through the calls compare_odometry makes on ref.Loam."""
    ODOMETRY, MAPPING = 1, 2

    def __init__(self, r, ov):
        self.r, self.ov = r, ov
        self.s = r.solves()

    def num_solves(self, stage):
        return sum(1 for s in self.s if s["stage"] == stage)

    def solve(self, stage, k):
        s = [s for s in self.s if s["stage"] == stage][k]
        return dict(s, q_in=s["x_in"][:4], t_in=s["x_in"][4:], q_out=s["x_out"][:4], t_out=s["x_out"][4:])

    def lo_pose(self):
        return self.r.lo_pose()

    def published_pose(self, topic):
        return self.r.published_pose(topic)

    def tf(self, which):
        row = self.r.tfs()[{0: 16, 1: 12, 2: 18}[which]]
        return self.ov.quat_from_basis(row[:9].reshape(3, 3)), row[9:]


def run_against_oracle(orc, ov, kitti_io, sc, opts, what):
    """The scenario through the reference binary and the oracle in lock-step.  Returns (recording, per-frame LO world translations)."""
    TF = ref.TF_NAMES.index
    st = [kitti_io.make_T(q, t) for q, t in sc["statics"]]
    ktf = kitti_io.VloamTF(st[0], st[1], st[2])
    o = ov.VloamOracle(*sc["calib"], ktf.base_T_cam0, ktf.velo_T_cam0, detach_VO_LO=bool(opts["detach_VO_LO"]), reset_VO_to_identity=bool(opts["reset_VO_to_identity"]),
                       remove_VO_outlier=opts["remove_VO_outlier"], scan_line=opts["scan_line"], with_mapping=True, mapping_skip_frame=opts["mapping_skip_frame"])
    state = {}
    own_set = o.lidar.set_vo_prior

    def hand_over(q, t):     # the oracle's own prior is compared in per_frame; its odometry starts from the reference's read-back bits
        state["own_prior"] = (np.array(q), np.array(t))
        own_set(*state["ref_prior"])
    o.lidar.set_vo_prior = hand_over
    lo_t = []

    def per_frame(r, k, status, cl, tree_c, tree_s):
        w = "%s frame %d" % (what, k)
        tfs = r.tfs()
        m = sc["matches"][k]
        state["ref_prior"] = (r.tf_rotation(8), tfs[TF("velo_last_VOT_velo_curr"), 9:].copy())
        if status == -5:     # the oracle restates laser_mapping.cpp:207 too: like the reference it must not be handed the NaN position
            whole = o.lidar.process
            o.lidar.process = lambda c: o.lidar.stage_sr(c) or o.lidar.stage_lo()
        assert o.process(sc["frames"][k], *(m if m is not None else (None, None))) == 0
        if status == -5:
            o.lidar.process = whole
        if k == 0:   # processStaticTransform against kitti_io's composition
            for name, T in (("imu_T_velo", st[0]), ("imu_T_cam0", st[1]), ("base_T_imu", st[2]), ("base_T_cam0", ktf.base_T_cam0), ("velo_T_cam0", ktf.velo_T_cam0)):
                e = tf_err(tfs[TF(name)], T)
                note("static transforms", e)
                assert e < POSE_TOL, "%s: %s" % (w, name)
            es = r.eigen_statics()     # imu_eigen_T_velo / imu_eigen_T_cam0: through the message's quaternion and Eigen's toRotationMatrix, then f32
            for got, T in ((es[0], st[0]), (es[1], st[1])):
                assert np.array_equal(got, kitti_io.transform_to_eigen_f32(T)), "%s: imu_eigen_T_*" % w
                assert np.array_equal(got[3], [0, 0, 0, 1])
        # ---- scan registration: bit for bit
        for i in range(5):
            assert same_cloud(cl[i], o.lidar.cloud(i)), "%s scan registration cloud %d" % (w, i)
        # ---- VO
        v = r.vo(0 if m is None else m[0].shape[0])
        assert (v is None) == (k == 0) and (o.vo_result is None) == (k == 0)
        if v is not None:
            ovr, rows = o.vo_result, v["match_rows"]
            md = ovr["match_debug"]
            assert np.array_equal(md[:, 0], rows[:, 0]), "%s: kinds" % w
            assert np.array_equal(md[:, 1].astype(np.float32).view(np.uint32), rows[:, 1].astype(np.float32).view(np.uint32)), "%s: depth0" % w
            assert np.array_equal(md[:, 2:], rows[:, 2:7]), "%s: observations" % w
            assert (ovr["counter32"], ovr["counter22"]) == (v["counter32"], v["counter22"]), "%s: counters" % w
            e_start = max(np.max(np.abs(ovr["init_angles"] - v["x_in"][:3])), np.max(np.abs(ovr["init_t"] - v["x_in"][3:])))
            note("VO start, frame 1" if k == 1 else "VO start, later frames", e_start)
            assert e_start < (FRAME1_START if k == 1 else POSE_TOL), "%s: the start from cam0_curr_LOT_cam0_prev: %.3e" % (w, e_start)
            if opts["reset_VO_to_identity"]:
                assert not v["x_in"].any(), "%s: reset_VO_to_identity" % w
            e = max(np.linalg.norm(ovr["angles"] - v["x_out"][:3]), np.linalg.norm(ovr["t"] - v["x_out"][3:]))
            note("VO solve, frame 1" if k == 1 else "VO solve, later frames", e)
            assert e < POSE_TOL, "%s: the VO solve: %.3e" % (w, e)
            if v["counter32"] + v["counter22"] == 0:
                assert np.array_equal(v["x_in"], v["x_out"])
        # ---- VloamTF after VO2VeloAndBase
        tol = POSE_TOL * (k + 1)     # (FRAME1_START is for the VO's start alone)
        for name, T in (("VO.cam0_curr_T_cam0_last", o.cam0_curr_T_cam0_last), ("velo_last_VOT_velo_curr", o.velo_last_VOT_velo_curr),
                        ("base_last_VOT_base_curr", o.base_last_VOT_base_curr), ("world_VOT_base_last", o.world_VOT_base_last),
                        ("cam0_curr_LOT_cam0_prev", o.cam0_curr_LOT_cam0_prev)):
            e = tf_err(tfs[TF(name)], T)
            note(name, e)
            assert e < tol, "%s: %s differs by %.3e" % (w, name, e)
        own_q, own_t = state["own_prior"]
        rq, rt = state["ref_prior"]
        if not np.any(np.isnan(rq)):
            assert qdist(own_q, rq) < tol and np.linalg.norm(own_t - rt) < tol, "%s: the oracle's own velo_last_VOT_velo_curr" % w
            stored = ov.quat_from_basis(tfs[TF("velo_last_VOT_velo_curr"), :9].reshape(3, 3))
            assert qdist(stored, rq) < 1e-15
        else:
            assert np.array_equal(np.isnan(own_q), np.isnan(rq)) and np.array_equal(np.isnan(own_t), np.isnan(rt)), "%s: NaN prior" % w
        # ---- odometry: both rounds
        view = LoamView(r, ov)
        nan_prior = bool(np.any(np.isnan(rq)))
        if not nan_prior and not np.any(np.isnan(r.lo_pose()[0])):
            compare_odometry(view, o.lidar, k, cl[1], cl[3], tree_c, tree_s, (rq, rt) if (k > 0 and not opts["detach_VO_LO"]) else None, w)
        rounds = [view.solve(view.ODOMETRY, i) for i in range(view.num_solves(view.ODOMETRY))]
        assert len(rounds) == (0 if k == 0 else 2)
        if k > 0 and opts["detach_VO_LO"] and "prev_out" in state:
            assert np.array_equal(rounds[0]["x_in"], state["prev_out"]), "%s: detached, round 0 starts from the previous result" % w
            assert np.array_equal(rounds[1]["x_in"], rounds[0]["x_out"]), "%s: detached, round 1 starts from round 0's result" % w
        if k > 0 and not opts["detach_VO_LO"]:
            for s in rounds:
                assert np.array_equal(s["x_in"], np.concatenate([rq, rt]), equal_nan=True), "%s: combined, both rounds start from the prior" % w
        if rounds:
            state["prev_out"] = rounds[1]["x_out"]
        stages = [s["stage"] for s in view.s]
        assert stages == sorted(stages) and stages[:1] == ([0] if k else stages[:1]), "%s: the stages report in callback() order: %s" % (w, stages)
        # ---- hand-over, poses
        want_skip = (k + 1) % opts["mapping_skip_frame"] != 0
        assert r.skip_frame() == want_skip, "%s skip_frame" % w
        if not want_skip:
            assert same_cloud(r.cloud(5), cl[2]) and same_cloud(r.cloud(6), cl[4]) and same_cloud(r.cloud(7), cl[0]), "%s hand-over clouds" % w
        qw, tw = r.lo_pose()
        oqw, otw, _, _ = o.lidar.lo_pose()
        assert np.array_equal(np.isnan(np.concatenate([qw, tw])), np.isnan(np.concatenate([oqw, otw]))), "%s: NaN in the LO world pose" % w
        lo_t.append(tw.copy())
        if not np.any(np.isnan(qw)):
            e = max(qdist(qw, oqw), np.linalg.norm(tw - otw))
            note("LO world pose / (k + 1)", e / (k + 1))
            assert e < POSE_TOL * (k + 1), "%s LO world pose" % w
            e = tf_err(tfs[TF("world_LOT_base_last")], ov.TF.from_qt(oqw, otw))
            assert e < POSE_TOL * (k + 1), "%s world_LOT_base_last" % w
        if status == 0:
            assert r.map_ran() == (not want_skip)
            pq, pt = r.published_pose(1)
            oq, ot = o.lidar.map_published_pose()
            assert np.array_equal(np.isnan(np.concatenate([pq, pt])), np.isnan(np.concatenate([oq, ot]))), "%s: NaN in the map pose" % w
            if not np.any(np.isnan(pq)):
                e = max(qdist(pq, oq), np.linalg.norm(pt - ot))
                note("map pose / (k + 1)", e / (k + 1))
                assert e < POSE_TOL * (k + 1), "%s published map pose" % w
                assert tf_err(tfs[TF("world_MOT_base_last")], ov.TF.from_qt(oq, ot)) < POSE_TOL * (k + 1), "%s world_MOT_base_last" % w
                if not want_skip:
                    assert sum(1 for s in stages if s == 2) == o.lidar.map_num_outer(), "%s: mapping rounds" % w
                else:
                    assert 2 not in stages, "%s: a skipped frame solved a mapping problem" % w
        # ---- trajectory rows: kitti_io.VloamTF fed with the ORACLE'S poses, row text against the reference's bytes
        state.setdefault("ktf", ktf)
        ktf.world_VOT_base_last = np.eye(4)
        ktf.world_VOT_base_last[:3, :3], ktf.world_VOT_base_last[:3, 3] = o.world_VOT_base_last.m, o.world_VOT_base_last.o
        c = k - opts["start_frame"]
        want = ["", "", ""]
        if status == 0 and opts["save_traj"] and opts["start_frame"] <= k <= opts["end_frame"]:
            oq, ot = o.lidar.map_published_pose()
            want = [kitti_io.format_pose_row(ktf.VO2Cam0StartFrame(c)), kitti_io.format_pose_row(ktf.LO2Cam0StartFrame(oqw, otw, c)),
                    kitti_io.format_pose_row(ktf.MO2Cam0StartFrame(oq, ot, c))]
        state.setdefault("want_rows", []).append(want)

    d = cases.record_session(ref, sc, opts, "", per_frame)
    d["n_frames"] = np.int32(len(sc["frames"]))
    return d, lo_t, state


@pytest.fixture(scope="module")
def scenarios():
    """What runs against the oracle: A and B with 5 frames, C with 6 (the recordings hold the first 4 of each)."""
    return cases.scenarios(live=True)


@pytest.fixture(scope="module")
def mods(orc):
    import orc_vloam as ov
    import conftest
    conftest.load_pkg()
    from vloam_amd import kitti_io
    return orc, ov, kitti_io


@pytest.fixture(scope="module")
def runs(scenarios, mods):
    out = {}
    for name in ("combined", "detached", "extrinsics"):
        out[name] = run_against_oracle(*mods, scenarios[name], scenarios[name]["opts"], name)
    print("measured maxima:", {k: "%.3e" % v for k, v in sorted(MAXIMA.items())})
    return out


def check_rows(d, state, opts, what):
    """Scenario E on the reference's bytes: no row before start_frame, the identity at start_frame, and kitti_io's text for every row."""
    import io
    for which in range(3):
        per = cases.rows_per_frame(d, which)
        for k, text in per.items():
            inside = opts["start_frame"] <= k <= opts["end_frame"]
            assert (text != "") == inside, "%s file %d frame %d" % (what, which, k)
            if k == opts["start_frame"]:
                assert text == "1.000000 0.000000 0.000000 0.000000 0.000000 1.000000 0.000000 0.000000 0.000000 0.000000 1.000000 0.000000\n", text
            assert text == state["want_rows"][k][which], "%s file %d frame %d:\nreference %r\nkitti_io  %r" % (what, which, k, text, state["want_rows"][k][which])
    return per


def test_combined_mode(runs, scenarios, mods, tmp_path):
    d, lo_t, state = runs["combined"]
    opts = scenarios["combined"]["opts"]
    assert int(d["n_run"]) == 5 and all(int(d["f%d_status" % k]) == 0 for k in range(5))
    check_rows(d, state, opts, "combined")
    kitti_io = mods[2]
    for which, name in enumerate(("VO", "LO", "MO")):     # the reference's files parse with kitti_io's reader; rows are relative to the start frame
        p = tmp_path / (name + "0.txt")
        p.write_bytes(bytes(d["rows_" + name]))
        T = kitti_io.read_trajectory(str(p))
        assert T.shape == (3, 4, 4) and np.array_equal(T[0], np.eye(4)) and np.linalg.norm(T[1, :3, 3]) > 0.5
        assert np.linalg.norm(T[2, :3, 3]) > 1.5 * np.linalg.norm(T[1, :3, 3]), "rows are relative to the start frame, not to the previous row"
    print("measured maxima:", {k: "%.3e" % v for k, v in sorted(MAXIMA.items())})


def test_detached_mode_computes_the_prior_and_ignores_it(runs):
    (a, ta, _), (b, tb, _) = runs["combined"], runs["detached"]
    # frames 0 and 1 see the same VO start in both modes, so the prior is the same bits; later the VO starts from each mode's own LO result
    # and the priors differ legitimately (that each is the right one is checked against the oracle in run_against_oracle)
    for k in range(5):
        if k < 2:
            assert np.array_equal(a["f%d_tfs" % k][8], b["f%d_tfs" % k][8]), "frame %d: velo_last_VOT_velo_curr is computed in both modes" % k
        assert np.all(np.isfinite(b["f%d_tfs" % k][8]))
    assert np.linalg.norm(b["f1_tfs"][8, 9:]) > 0.3, "the detached session still computes the prior"
    assert all(not np.array_equal(ta[k], tb[k]) for k in range(1, 5)), "the LO poses of the two modes must differ"


def test_extrinsics_that_tell_mistakes_apart(runs, scenarios, mods):
    d, _, state = runs["extrinsics"]
    B, V = d["base_T_cam0"], d["velo_T_cam0"]
    inv = mods[2].inv_T
    for X, name in ((B, "base_T_cam0"), (V, "velo_T_cam0")):
        assert np.max(np.abs(X - inv(X))) > 0.3, "%s is too close to its own inverse" % name
    assert np.max(np.abs(B - V)) > 0.3 and np.max(np.abs(B - inv(V))) > 0.3
    assert np.max(np.abs(V - inv(B))) > 0.3
    for X, name in ((B, "base_T_cam0"), (V, "velo_T_cam0")):
        a = cases.angle_to_nearest_axis_permutation(X[:3, :3])
        print("%s: %.3f rad from the nearest axis permutation" % (name, a))
        assert a > 0.3, "%s is %.3f rad from an axis permutation" % (name, a)
    for q, t in scenarios["extrinsics"]["statics"][::2]:
        assert 0.3 <= 2 * np.arccos(abs(q[3])) <= 1.2
    lens = sorted(float(np.linalg.norm(t)) for _, t in scenarios["extrinsics"]["statics"])
    assert lens[1] - lens[0] > 0.1 and lens[2] - lens[1] > 0.1, "translations of different lengths: %s" % lens
    check_rows(d, state, scenarios["extrinsics"]["opts"], "extrinsics")


def test_degenerate_frames(scenarios, mods):
    """What the reference does, recorded: a frame whose matches are all gated out, or that has none, leaves the problem without a block;
    reset_VO_to_identity has zeroed the parameters, so visual_odometry.cpp:427-430 divides 0 by 0: cam0_curr_T_cam0_last, velo_last_VOT_velo_curr
    and base_last_VOT_base_curr are NaN, the gate of vloam_tf.cpp:69-72 closes and world_VOT_base_last keeps its value.
    COMBINED mode: both odometry rounds start from the NaN prior, find no correspondence, and q_w_curr / t_w_curr are NaN from then on —
    for good, since they are accumulated; the next MAPPED frame would convert the NaN position to int (laser_mapping.cpp:207), which is
    undefined: the harness stops there (-5).  DETACHED mode: the odometry never reads the prior, nothing else is affected: the LO and map poses stay finite, frames 3 and 5 are mapped, and the VO world pose resumes at frame 4."""
    sc = scenarios["degenerate"]
    d, lo_t, _ = run_against_oracle(*mods, sc, sc["opts"], "degenerate")
    nan = lambda row: bool(np.any(np.isnan(row)))
    assert [int(d["f%d_status" % k]) for k in range(4)] == [0, 0, 0, -5] and int(d["n_run"]) == 4
    assert tuple(d["f2_vo_counters"]) == (0, 0) and not d["f2_vo_x"].any()
    for name in ("velo_last_VOT_velo_curr", "base_last_VOT_base_curr", "VO.cam0_curr_T_cam0_last"):
        assert nan(d["f2_tfs"][ref.TF_NAMES.index(name)]) and not nan(d["f1_tfs"][ref.TF_NAMES.index(name)])
    W = ref.TF_NAMES.index("world_VOT_base_last")
    assert np.array_equal(d["f2_tfs"][W], d["f1_tfs"][W]) and np.array_equal(d["f3_tfs"][W], d["f1_tfs"][W]), "the gate is closed at frames 2 and 3"
    assert not np.array_equal(d["f1_tfs"][W], d["f0_tfs"][W])
    for k in (2, 3):
        assert nan(d["f%d_lo0_x" % k]) and d["f%d_lo0_corner" % k].shape[0] == 0 and d["f%d_lo1_plane" % k].shape[0] == 0 and nan(d["f%d_lo_pose" % k])
    assert not nan(d["f1_lo_pose"]) and d["f1_lo1_corner"].shape[0] > 10 and int(d["f2_skip"]) == 1 and int(d["f3_skip"]) == 0
    t = sc["twin"]
    e, lo_e, _ = run_against_oracle(*mods, sc, t, "degenerate detached")
    assert [int(e["f%d_status" % k]) for k in range(6)] == [0] * 6
    assert tuple(e["f3_vo_counters"]) == (0, 0) and e["f3_vo_kind"].size == 0 and tuple(e["f2_vo_counters"]) == (0, 0) and e["f2_vo_kind"].size == 400
    for k in (2, 3):
        assert nan(e["f%d_tfs" % k][8]) and np.array_equal(e["f%d_tfs" % k][W], e["f1_tfs"][W])
    for k in (4, 5):
        assert not nan(e["f%d_tfs" % k][8]) and not np.array_equal(e["f%d_tfs" % k][W], e["f%d_tfs" % (k - 1)][W]), "the VO world pose resumes at frame %d" % k
    assert not any(nan(e["f%d_lo_pose" % k]) or nan(e["f%d_map_pub" % k]) for k in range(6))
    assert [int(e["f%d_skip" % k]) for k in range(6)] == [1, 0] * 3 and int(e["f3_map_n"]) + int(e["f5_map_n"]) > 0, "mapped frames follow the NaN frames"


@pytest.mark.parametrize("name", sorted(STEMS))
def test_the_committed_recording_is_what_the_reference_binary_gives(name):
    d, z = cases.record(ref, cases.scenarios()[name]), np.load(os.path.join(HERE, "golden", STEMS[name] + ".npz"))
    assert sorted(d) == sorted(z.files)
    for key in sorted(d):
        a, b = np.asarray(d[key]), z[key]
        assert a.shape == b.shape and a.dtype == b.dtype, key
        if a.dtype.kind == "f" and (key.endswith("_x") or key.endswith("tfs") or key.endswith("pose") or key.endswith("map_pub") or key.endswith("prior")):
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.max(np.abs(a - b)[~np.isnan(a)], initial=0) < POSE_TOL * 8, key
        else:
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), key
    assert os.path.getsize(os.path.join(HERE, "golden", STEMS[name] + ".npz")) <= os.path.getsize(os.path.join(HERE, "golden", "vloam_64x256_5frames.npz"))
