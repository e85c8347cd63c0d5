"""Inputs of the coupled-frame-loop pin (tests/test_ref_vloam.py, tests/golden/make_golden.py) and the layout of its recordings
tests/golden/ref_vloam_*.npz (read by tests/test_gpu_ref_pinned_vloam.py, which needs nothing else).

A scenario is a calibration, the three static transforms tf's lookups return (imu_T_velo, imu_T_cam0, base_T_imu as (q xyzw, t)), the
node's options, the sweeps and per frame the integer pixel pairs the image front-end would have left (None for the first frame).

  combined    A: 64 x 256, synth_matches (400 pairs), mapping on, KITTI-like statics; rows written from frame 2 on (scenario E: start_frame
              = 2, end_frame = 4).  5 frames against the oracle; the recording holds the first 4 (a fifth does not fit a fixture's size).
  detached    B: the same sweeps and matches with detach_VO_LO = 1.
  degenerate  C: the sweeps of A (at 16 x 256, 64 x 128 or 32 x 256 the depth map is too sparse for a single depth factor, every VO solve stays
              at zero and the very first one is degenerate), mapping_skip_frame = 2, reset_VO_to_identity = 1, combined mode.  Frame 2 has
              matches of which none is usable (every pair is farther apart than remove_VO_outlier), frame 3 has no match at all.  6 frames
              against the oracle, the first 4 in the recording.
  degenerate_detached  C again with detach_VO_LO = 1: the combined session cannot get past its first mapped frame after the NaN (see
              test_ref_vloam.py), the detached one sees both degenerate frames.  Stored inside ref_vloam_degenerate.npz (prefix d_).
  extrinsics  D: 64 x 256, 4 frames, combined mode: a camera turned and tilted against the KITTI-like one (telling_calib, with matches
              generated for it) and random imu_T_velo / base_T_imu, so that base_T_cam0 AND velo_T_cam0 are far from each other, from their
              inverses and from every axis permutation.
The recordings' frames and match counts are as small as the 1 MB bound on a fixture needs; no case was dropped for it.
"""
import numpy as np

import conftest

NBX, NBY = 249, 75
_F = np.float32
OPT_KEYS = ("scan_line", "mapping_skip_frame", "detach_VO_LO", "reset_VO_to_identity", "remove_VO_outlier", "save_traj", "start_frame", "end_frame")


def quat_of(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([a * np.sin(0.5 * angle), [np.cos(0.5 * angle)]])


def kitti_like_statics(synth):
    """The statics synth.kitti_like_extrinsics() composes, as (q, t) pairs: imu_T_velo, imu_T_cam0, base_T_imu."""
    cam_T_velo = synth.kitti_like_calib()[0].astype(np.float64)
    imu_T_velo = np.eye(4)
    imu_T_velo[:3, 3] = [0.81, -0.32, 0.80]
    imu_T_velo[:3, :3] = synth._rot_zyx(0.0148, -0.0021, 0.0009)
    imu_T_cam0 = imu_T_velo @ np.linalg.inv(cam_T_velo)
    return [(synth.rot_to_quat_xyzw(imu_T_velo[:3, :3]), imu_T_velo[:3, 3].copy()), (synth.rot_to_quat_xyzw(imu_T_cam0[:3, :3]), imu_T_cam0[:3, 3].copy()),
            (np.array([0.0, 0.0, 0.0, 1.0]), np.array([-1.405, 0.32, 0.93]))]


def telling_calib(synth, seed=7):
    """Scenario D's calibration: the KITTI-like camera turned by 0.3 - 1.2 rad about the velodyne's z axis (the sweep covers 360 degrees, so
    the image still sees the scene) and tilted by 0.3 - 0.5 rad about the new viewing direction (a roll: it keeps the scene in the image).
    cam_T_velo = kitti_cam_T_velo * turn^-1, stored as f32 like every calibration."""
    rng = np.random.default_rng(seed)
    cam_T_velo, rect0_T_cam, P = synth.kitti_like_calib()
    yaw, roll = rng.uniform(0.3, 1.2), rng.uniform(0.3, 0.5)
    turn = np.eye(4)
    turn[:3, :3] = synth._rot_zyx(yaw, 0.0, 0.0) @ synth._rot_zyx(0.0, 0.0, roll)
    turn[:3, 3] = rng.uniform(-0.3, 0.3, 3)
    return (cam_T_velo.astype(np.float64) @ np.linalg.inv(turn)).astype(_F), rect0_T_cam, P


def telling_statics(synth, calib, seed=7):
    """Scenario D.  imu_T_velo and base_T_imu are random: angles in [0.3, 1.2] rad about the x and the z axis (each axis tilted at random by
    at most 0.2), translations of 0.5 and 2.5 m in random directions.  imu_T_cam0 = imu_T_velo * cam_T_velo^-1 with the turned camera of
    telling_calib, so that the scene is consistent (a VO motion conjugated by velo_T_cam0 is the velodyne's motion) and velo_T_cam0 =
    cam_T_velo^-1 is itself 0.3 rad or more from every axis permutation."""
    from vloam_amd import kitti_io
    rng = np.random.default_rng(seed + 1)
    out = []
    for k, length in ((0, 0.5), (2, 2.5)):
        axis = np.eye(3)[k] + rng.uniform(-0.2, 0.2, 3)
        q = quat_of(axis, rng.uniform(0.3, 1.2))
        d = rng.normal(size=3)
        out.append((q, length * d / np.linalg.norm(d)))
    imu_T_cam0 = kitti_io.make_T(*out[0]) @ np.linalg.inv(calib[0].astype(np.float64))
    R = imu_T_cam0[:3, :3]
    u, _, vt = np.linalg.svd(R)          # the f32 calibration's rotation is orthonormal to 1e-7 only: the quaternion is taken of the nearest rotation
    return [out[0], (synth.rot_to_quat_xyzw(u @ vt), imu_T_cam0[:3, 3].copy()), out[1]]


def angle_to_nearest_axis_permutation(R):
    """The smallest rotation angle between R and one of the 24 proper signed axis permutations."""
    import itertools
    best = np.pi
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            Pm = np.zeros((3, 3))
            for r in range(3):
                Pm[r, perm[r]] = signs[r]
            if np.linalg.det(Pm) > 0:
                best = min(best, float(np.arccos(np.clip((np.trace(Pm.T @ R) - 1.0) / 2.0, -1.0, 1.0))))
    return best


def matches_for(synth, seq, k, calib, n_match, pixel_noise=0.5, seed=99):
    """synth.synth_matches for a calibration of the caller's: pixel pairs (frame k - 1 -> frame k) of scene points visible in both images."""
    K = calib[2][:, :3].astype(np.float64)
    Tcv = calib[0].astype(np.float64)
    rng = np.random.default_rng(seed + k)
    prev = seq.sweep(k - 1)[:, :3].astype(np.float64)
    prev = prev[np.isfinite(prev[:, 0])]
    q, t = seq.gt_relative(k)
    curr = (prev - t[None, :]) @ synth.quat_to_rot(q)

    def proj(pts):
        pc = pts @ Tcv[:3, :3].T + Tcv[:3, 3]
        uv = pc @ K.T
        with np.errstate(divide="ignore", invalid="ignore"):
            return uv[:, :2] / uv[:, 2:3], pc[:, 2]
    uv0, z0 = proj(prev)
    uv1, z1 = proj(curr)
    ok = (z0 > 1.0) & (z1 > 1.0) & (uv0[:, 0] > 2) & (uv0[:, 0] < 1239) & (uv0[:, 1] > 2) & (uv0[:, 1] < 372) & \
         (uv1[:, 0] > 2) & (uv1[:, 0] < 1239) & (uv1[:, 1] > 2) & (uv1[:, 1] < 372)
    idx = np.nonzero(ok)[0]
    idx = rng.choice(idx, size=min(n_match, idx.size), replace=False)
    a = uv0[idx] + rng.normal(0, pixel_noise, (idx.size, 2))
    b = uv1[idx] + rng.normal(0, pixel_noise, (idx.size, 2))
    return a.astype(_F).astype(np.int32), b.astype(_F).astype(np.int32)


def _frames(synth, rings, n_az, n, n_match, calib=None):
    seq = synth.SynthSequence(n_rings=rings, n_azimuth=n_az, n_sweeps=n + 1)
    sweeps = [np.ascontiguousarray(seq.sweep(k), dtype=_F) for k in range(n)]
    if calib is None:
        matches = [None] + [synth.synth_matches(seq, k, n_match=n_match) for k in range(1, n)]
    else:
        matches = [None] + [matches_for(synth, seq, k, calib, n_match) for k in range(1, n)]
    return sweeps, matches


BASE_OPTS = dict(scan_line=64, mapping_skip_frame=1, detach_VO_LO=0, reset_VO_to_identity=0, remove_VO_outlier=100, save_traj=1, start_frame=2, end_frame=4)


def extrinsics_scenario(n_az=256, n=4, n_match=400):
    """Scenario D at a size of the caller's (the recording: 64 x 256; the live device re-check: 64 x 512)."""
    synth = conftest.load_synth()
    calib = telling_calib(synth)
    sweeps, matches = _frames(synth, 64, n_az, n, n_match, calib)
    return dict(calib=calib, statics=telling_statics(synth, calib), opts=dict(BASE_OPTS, start_frame=1, end_frame=3), frames=sweeps, matches=matches)


def scenarios(live=False):
    """live = False: what the recordings hold (4 frames each: the bound on a fixture's size).  live = True: what tests/test_ref_vloam.py runs
    against the oracle: A and B with 5 frames (two rows after the identity row), C with 6 (two frames after the degenerate ones)."""
    synth = conftest.load_synth()
    calib = synth.kitti_like_calib()
    ks = kitti_like_statics(synth)
    base = dict(BASE_OPTS)
    sa, ma = _frames(synth, 64, 256, 5 if live else 4, 400)
    sc_, mc = _frames(synth, 64, 256, 6 if live else 4, 400)
    far = mc[2][0].copy()
    far[:, 0] = np.where(far[:, 0] < 621, far[:, 0] + 400, far[:, 0] - 400)     # every pair 400 px apart: none passes the gate of 100
    mc[2] = (far, mc[2][1])
    mc[3] = (np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32))
    copt = dict(base, mapping_skip_frame=2, reset_VO_to_identity=1, start_frame=1, end_frame=3)
    return {
        "combined": dict(calib=calib, statics=ks, opts=base, frames=sa, matches=ma),
        "detached": dict(calib=calib, statics=ks, opts=dict(base, detach_VO_LO=1), frames=sa, matches=ma),
        "degenerate": dict(calib=calib, statics=ks, opts=copt, frames=sc_, matches=mc, twin=dict(copt, detach_VO_LO=1)),
        "extrinsics": extrinsics_scenario(),
    }


def new_session(ref, sc, opts):
    o = dict(opts)
    return ref.Vloam(*sc["calib"], sc["statics"], scan_line=o["scan_line"], mapping_skip_frame=o["mapping_skip_frame"], detach_VO_LO=o["detach_VO_LO"],
                     reset_VO_to_identity=o["reset_VO_to_identity"], remove_VO_outlier=o["remove_VO_outlier"], save_traj=o["save_traj"],
                     start_frame=o["start_frame"], end_frame=o["end_frame"])


def T4(row12):
    T = np.eye(4)
    T[:3, :3] = row12[:9].reshape(3, 3)
    T[:3, 3] = row12[9:]
    return T


def sparse(b):
    bx, by, bd, bc = b
    idx = np.nonzero(bc)[0].astype(np.int32)
    return idx, bx[idx], by[idx], bd[idx], bc[idx].astype(np.int16)


def dense(z, pre):
    bx, by, bd = [np.zeros(NBX * NBY, dtype=_F) for _ in range(3)]
    bc = np.zeros(NBX * NBY, dtype=np.int32)
    idx = z[pre + "bidx"]
    bx[idx], by[idx], bd[idx], bc[idx] = z[pre + "bx"], z[pre + "by"], z[pre + "bd"], z[pre + "bc"]
    return bx, by, bd, bc


def _unique_index(points_f64, table, what):
    key = {}
    for i, r in enumerate(np.ascontiguousarray(table[:, :3])):
        assert r.tobytes() not in key, "%s: the cloud holds a point twice, indices would not be unique" % what
        key[r.tobytes()] = i
    return np.array([key[r.tobytes()] for r in np.ascontiguousarray(points_f64, dtype=_F)], dtype=np.int32)


def record_session(ref, sc, opts, prefix="", per_frame=None):
    """One session through the reference binary; the arrays of its recording.  per_frame(r, k, status, clouds, tree_c, tree_s) sees the live session."""
    r = new_session(ref, sc, opts)
    d = {prefix + "opts": np.array([opts[k] for k in OPT_KEYS], dtype=np.int32), prefix + "statics": np.array([np.concatenate(s) for s in sc["statics"]])}
    tree_c = tree_s = np.zeros((0, 4), _F)
    n_run = 0
    for k, c in enumerate(sc["frames"]):
        m = sc["matches"][k]
        pre = "%sf%d_" % (prefix, k)
        status = r.frame(c, *(m if m is not None else (None, None)))
        d[pre + "status"] = np.int32(status)
        if status == -3:
            break
        n_run = k + 1
        tfs = r.tfs()
        d[pre + "tfs"] = tfs
        d[pre + "prior"] = np.concatenate([r.tf_rotation(8), tfs[8, 9:]])
        if k == 0:
            d[prefix + "base_T_cam0"], d[prefix + "velo_T_cam0"] = T4(tfs[3]), T4(tfs[4])
            d[prefix + "eigen_statics"] = r.eigen_statics()
        if not prefix:     # (a twin session sees the same sweeps: the same depth maps)
            d[pre + "bidx"], d[pre + "bx"], d[pre + "by"], d[pre + "bd"], d[pre + "bc"] = sparse(r.buckets())
        v = r.vo(0 if m is None else m[0].shape[0])
        if v is not None:
            rows = v["match_rows"]
            d[pre + "vo_x"] = np.concatenate([v["x_in"], v["x_out"]])
            d[pre + "vo_counters"] = np.array([v["counter32"], v["counter22"]], dtype=np.int32)
            d[pre + "vo_kind"], d[pre + "vo_depth0"], d[pre + "vo_obs"] = rows[:, 0].astype(np.int8), rows[:, 1].astype(_F), rows[:, 2:7].copy()
            assert np.array_equal(rows[:, 7:9], m[0]) and np.array_equal(rows[:, 9:11], m[1])
        cl = [r.cloud(i) for i in range(5)]
        solves = r.solves()
        d[pre + "stages"] = np.array([s["stage"] for s in solves], dtype=np.int32)
        lo = [s for s in solves if s["stage"] == r.ODOMETRY]
        for o, s in enumerate(lo):
            nc = int(np.count_nonzero(s["types"] == 0))
            pc, pp = s["payload"][:nc], s["payload"][nc:]
            w = "frame %d round %d" % (k, o)
            d["%slo%d_corner" % (pre, o)] = np.stack([_unique_index(pc[:, 0:3], cl[1], w), _unique_index(pc[:, 3:6], tree_c, w), _unique_index(pc[:, 6:9], tree_c, w)], 1).reshape(-1, 3).astype(np.int16)
            d["%slo%d_plane" % (pre, o)] = np.stack([_unique_index(pp[:, 0:3], cl[3], w)] + [_unique_index(pp[:, 3 * j:3 * j + 3], tree_s, w) for j in (1, 2, 3)], 1).reshape(-1, 4).astype(np.int16)
            d["%slo%d_x" % (pre, o)] = np.concatenate([s["x_in"], s["x_out"]])
        d[pre + "lo_pose"] = np.concatenate(r.lo_pose())
        d[pre + "skip"] = np.int32(r.skip_frame())
        if status == 0:
            d[pre + "map_pub"] = np.concatenate(r.published_pose(1))
            d[pre + "map_n"] = np.int32(sum(1 for s in solves if s["stage"] == r.MAPPING))
        if per_frame is not None:
            per_frame(r, k, status, cl, tree_c, tree_s)
        tree_c, tree_s = cl[2], cl[4]
        d[pre + "rows_len"] = np.array([len(r.rows_text(w) or b"") for w in range(3)], dtype=np.int32)
    d[prefix + "n_run"] = np.int32(n_run)
    for w, name in enumerate(("VO", "LO", "MO")):
        d[prefix + "rows_" + name] = np.frombuffer(r.rows_text(w) or b"", dtype=np.uint8).copy()
    return d


def record(ref, sc, per_frame=None, per_frame_twin=None):
    """A scenario's recording: the inputs once, then the session (and, for the degenerate scenario, its detached twin under the prefix d_)."""
    d = dict(cam_T_velo=sc["calib"][0], rect0_T_cam=sc["calib"][1], P_rect0=sc["calib"][2], n_frames=np.int32(len(sc["frames"])))
    for k, c in enumerate(sc["frames"]):
        d["f%d_cloud" % k] = np.ascontiguousarray(c[:, :3])
        if sc["matches"][k] is not None:
            d["f%d_prev_uv" % k], d["f%d_curr_uv" % k] = (np.ascontiguousarray(a, dtype=np.int16) for a in sc["matches"][k])
    d.update(record_session(ref, sc, sc["opts"], "", per_frame))
    if "twin" in sc:
        d.update(record_session(ref, sc, sc["twin"], "d_", per_frame_twin))
    return d


# ---------------------------------------------------------------- reading a recording
def cloud_of(z, k):
    c = np.zeros((z["f%d_cloud" % k].shape[0], 4), dtype=_F)
    c[:, :3] = z["f%d_cloud" % k]
    return c


def matches_of(z, k):
    if "f%d_prev_uv" % k not in z:
        return None, None
    return z["f%d_prev_uv" % k].astype(np.int32), z["f%d_curr_uv" % k].astype(np.int32)


def opts_of(z, prefix=""):
    return dict(zip(OPT_KEYS, (int(v) for v in z[prefix + "opts"])))


def rows_per_frame(z, which, prefix=""):
    """{frame: the text that frame appended to file which (0 VO, 1 LO, 2 MO)}."""
    text = bytes(z[prefix + "rows_" + ("VO", "LO", "MO")[which]]).decode()
    out, at = {}, 0
    for k in range(int(z[prefix + "n_run"])):
        end = int(z["%sf%d_rows_len" % (prefix, k)][which])
        out[k] = text[at:end]
        at = end
    return out
