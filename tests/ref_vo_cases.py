"""Inputs of the visual-odometry pin (tests/test_ref_visual_odometry.py, tests/golden/make_golden.py) and the layout of its recordings
tests/golden/ref_vo_*.npz (read by tests/test_gpu_ref_pinned_vo.py, which needs nothing else).

A scenario is a calibration, a few sweeps ("frames") and sessions.  A session is one VisualOdometry object with its options
(remove_VO_outlier, reset_VO_to_identity, optical_flow_match) that sees every frame and runs solveNlsAll at the frames it has a run for.
A run is what the OpenCV front-end would have left in the public containers: keypoints + (queryIdx, trainIdx) or the two optical-flow
point lists + status, and optionally the prior cam0_curr_LOT_cam0_prev.
"""
import numpy as np

import conftest

W, H, GRID = 1242, 375, 5
NBX, NBY = 249, 75


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def back_project(calib, u, v, z):
    """Velodyne points [n, 4] f32 whose projection through calib (in exact arithmetic) is pixel (u, v) at depth z."""
    T, P = calib[0].astype(np.float64), calib[2].astype(np.float64)
    K = P[:, :3]
    cam = np.linalg.solve(K, np.stack([u * z, v * z, z]))            # [3, n]
    velo = T[:3, :3].T @ (cam - T[:3, 3:4])
    out = np.zeros((velo.shape[1], 4), dtype=np.float32)
    out[:, :3] = velo.T
    return out


def edge_calib(synth):
    """kitti_like_calib with the depth row's translation set to zero: the projected depth of a point is then its velodyne x exactly
    (((x * 1 + y * 0) + z * 0) + 1 * 0 in f32), so depths of 0.1f and its two neighbours can be placed."""
    cam_T_velo, rect0_T_cam, P = synth.kitti_like_calib()
    cam_T_velo = cam_T_velo.copy()
    cam_T_velo[2, 3] = 0.0
    return cam_T_velo, rect0_T_cam, P


def perturbed_calib(synth, seed):
    """_perturbed_calib of tests/test_gpu_fuzz.py."""
    rng = np.random.default_rng(seed)
    cam_T_velo, rect0_T_cam, P = synth.kitti_like_calib()
    w = rng.uniform(-0.03, 0.03, 3)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    dR = np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx
    T = cam_T_velo.astype(np.float64)
    T[:3, :3] = dR @ T[:3, :3]
    T[:3, 3] += rng.uniform(-0.05, 0.05, 3)
    P = P.astype(np.float64)
    P[0, 0] *= rng.uniform(0.9, 1.1); P[1, 1] = P[0, 0]
    P[0, 2] += rng.uniform(-20, 20); P[1, 2] += rng.uniform(-10, 10)
    return T.astype(np.float32), rect0_T_cam, P.astype(np.float32)


CLUSTERS = {(50, 30): 1, (60, 30): 2, (70, 30): 40}     # bucket -> points it receives


def bucket_cloud(calib, seed, fill=0.42, edges=True):
    """A sweep of a few thousand points built in the image: about `fill` x 249 x 75 points, each in a bucket drawn WITH replacement
    (so most filled buckets hold one point, some two to four, and 25-bucket neighbourhoods hold from none to more than ten), at depths
    4 .. 40 m.  With edges: the three CLUSTERS buckets receive exactly 1, 2 and 40 points; points at depth 0.1f and its two f32
    neighbours (edge_calib); points that project to u or v in (-5, 0), [1240, 1245), [1245, 1250), [370, 375), [375, 380).  The rows
    are shuffled, so the order-dependent fold sees the points of a bucket at scattered positions."""
    rng = np.random.default_rng(seed)
    n = int(fill * NBX * NBY)
    bx, by = rng.integers(0, NBX, n), rng.integers(0, NBY, n)
    if edges:
        keep = np.array([(int(a), int(b)) not in CLUSTERS for a, b in zip(bx, by)])
        bx, by = bx[keep], by[keep]
        for (cx, cy), cnt in CLUSTERS.items():
            bx, by = np.concatenate([bx, np.full(cnt, cx)]), np.concatenate([by, np.full(cnt, cy)])
    u = GRID * bx + rng.uniform(0.3, 4.7, bx.size)
    v = GRID * by + rng.uniform(0.3, 4.7, bx.size)
    z = rng.uniform(4.0, 40.0, bx.size)
    parts = [back_project(calib, u, v, z)]
    if edges:
        ue = np.array([-2.5, -4.8, -0.2, 300.0, 301.0, -3.0, 1240.4, 1244.6, 1245.5, 1249.0, 700.0, 701.0, 702.0, 1243.0, 1247.0, -2.0])
        ve = np.array([100.0, 101.0, 102.0, -2.5, -4.8, -3.0, 200.0, 201.0, 202.0, 203.0, 370.4, 374.6, 375.5, 372.0, 377.0, 373.0])
        parts.append(back_project(calib, ue, ve, np.full(ue.size, 10.0)))
        tenth = np.float32(0.1)
        near = np.zeros((3, 4), dtype=np.float32)
        near[:, 0] = [np.nextafter(tenth, np.float32(0)), tenth, np.nextafter(tenth, np.float32(1))]
        parts.append(near)
    cloud = np.concatenate(parts)
    return cloud[rng.permutation(cloud.shape[0])]


def lattice_pixels():
    """Every pixel of the 5-px lattice, the four corners and the four edge mid-points."""
    xs, ys = np.meshgrid(np.arange(0, W, GRID), np.arange(0, H, GRID), indexing="ij")
    extra = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2)]
    return f32(np.concatenate([np.stack([xs.ravel(), ys.ravel()], axis=1), np.array(extra)]))


def orb_run(kp_prev, kp_curr, rng, prior=None):
    """Scatter the two keypoint lists independently; (queryIdx, trainIdx) put the pairs together again."""
    n = kp_prev.shape[0]
    pa, pb = rng.permutation(n), rng.permutation(n)
    a, b = np.zeros_like(kp_prev), np.zeros_like(kp_curr)
    a[pa], b[pb] = kp_prev, kp_curr
    r = dict(kp_prev=f32(a), kp_curr=f32(b), query_idx=pa.astype(np.int32), train_idx=pb.astype(np.int32))
    if prior is not None:
        r["prior_q"], r["prior_t"] = prior
    return r


def keypoint_pairs(rng, n, spread):
    """n keypoint pairs with fractional coordinates inside the image; the second of a pair `spread` pixels (sigma) from the first."""
    a = np.stack([rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)], axis=1)
    b = a + rng.normal(0, spread, (n, 2))
    b[:, 0], b[:, 1] = np.clip(b[:, 0], 0, W - 1), np.clip(b[:, 1], 0, H - 1)
    return f32(a), f32(b)


def gate_pairs():
    """Pairs whose INTEGER pixel distance squared is 100^2 exactly (60, 80), one pixel more and one less, with fractional parts that a
    rounding conversion would move to the next integer."""
    a = np.array([[200.3, 100.7], [400.9, 120.99], [640.5, 150.5], [900.99, 90.01]] * 3)
    d = np.array([[60, 80]] * 4 + [[60, 81]] * 4 + [[60, 79]] * 4)
    b = np.floor(a) + d + np.array([[0.9, 0.2], [0.5, 0.5], [0.99, 0.99], [0.0, 0.6]] * 3)
    return f32(a), f32(b)


def quat_of(aa):
    aa = np.asarray(aa, dtype=np.float64)
    th = np.linalg.norm(aa)
    return np.concatenate([aa / th * np.sin(th / 2), [np.cos(th / 2)]])


def scenarios():
    """{file stem: dict(calib, frames, queries, sessions)}."""
    synth = conftest.load_synth()
    out = {}
    # ---- plain and perturbed calibration: three frames of the 64 x 256 synthetic sweep, synth_matches
    seq = synth.SynthSequence(n_rings=64, n_azimuth=256, n_sweeps=4)
    frames = [seq.sweep(k) for k in range(3)]
    for stem, calib, seed, nf in (("ref_vo_64x256_3frames", synth.kitti_like_calib(), 1, 3), ("ref_vo_64x256_perturbed", perturbed_calib(synth, 7), 2, 2)):
        rng = np.random.default_rng(seed)
        runs, queries = {}, {}
        for k in range(nf):
            pu, cu = synth.synth_matches(seq, max(k, 1), n_match=300)
            queries[k] = f32(np.concatenate([cu, np.stack([rng.uniform(0, W - 1, 300), rng.uniform(0, H - 1, 300)], axis=1)]))
            if k > 0:
                n = pu.shape[0]
                runs[k] = dict(kp_prev=f32(pu), kp_curr=f32(cu), query_idx=np.arange(n, dtype=np.int32), train_idx=np.arange(n, dtype=np.int32))
        out[stem] = dict(calib=calib, frames=frames[:nf], queries=queries,
                         sessions=[dict(remove_outlier=100, reset_to_identity=True, optical_flow_match=False, runs=runs)])
    # ---- projection and queryDepth edges: two bucket clouds; the lattice is queried in both depth maps, and a share of it goes through
    # the match loop (previous pixel = current pixel), which is how the device's C ABI reaches queryDepth
    calib = edge_calib(synth)
    frames = [bucket_cloud(calib, 11), bucket_cloud(calib, 12)]
    lat = lattice_pixels()
    sub = np.concatenate([lat[:NBX * NBY:47], lat[NBX * NBY:]])
    n = sub.shape[0]
    out["ref_vo_edges"] = dict(calib=calib, frames=frames, queries={0: lat, 1: lat}, sessions=[dict(
        remove_outlier=100, reset_to_identity=True, optical_flow_match=False,
        runs={1: dict(kp_prev=sub, kp_curr=sub, query_idx=np.arange(n, dtype=np.int32), train_idx=np.arange(n, dtype=np.int32))})])
    # ---- match loop
    calib = synth.kitti_like_calib()
    frames = [bucket_cloud(calib, 21, edges=False), bucket_cloud(calib, 22, edges=False)]
    rng = np.random.default_rng(23)
    a, b = keypoint_pairs(rng, 300, 3.0)
    ga, gb = gate_pairs()
    near_a, near_b = np.concatenate([a, ga]), np.concatenate([b, gb])
    far_a, _ = keypoint_pairs(rng, 200, 1.0)
    far_b, _ = keypoint_pairs(rng, 200, 1.0)
    fa, fb = keypoint_pairs(rng, 300, 3.0)
    status = rng.choice(np.array([0, 1, 1, 1, 2], dtype=np.uint8), fa.shape[0])
    off_a = f32(np.stack([rng.uniform(0, 500, 60), rng.uniform(0, H - 1, 60)], axis=1))
    off_b = off_a + np.float32(300.0)
    off_b[:, 1] = off_a[:, 1]
    prior = (quat_of([0.01, -0.02, 0.015]), np.array([0.02, -0.01, 0.8]))
    ident = (np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3))
    S = lambda remove, reset, flow, run: dict(remove_outlier=remove, reset_to_identity=reset, optical_flow_match=flow, runs={1: run})
    out["ref_vo_match_loop"] = dict(calib=calib, frames=frames, queries={}, sessions=[
        S(100, True, False, orb_run(near_a, near_b, rng)),                    # fractional keypoints, permuted indices, the gate's boundary
        S(0, True, False, orb_run(far_a, far_b, rng)),                        # remove_VO_outlier = 0: the gate is off
        S(100, True, True, dict(kp_prev=fa, kp_curr=fb, status=status)),      # optical flow, status 0 / 1 / 2 mixed
        S(100, False, False, orb_run(near_a, near_b, rng, prior=ident)),      # reset_VO_to_identity false, identity prior
        S(100, False, False, orb_run(near_a, near_b, rng, prior=prior)),      # ... a prior that is not the identity
        S(100, False, False, orb_run(off_a, off_b, rng, prior=prior)),        # no usable match: every pair fails the gate
    ])
    return out


# ---------------------------------------------------------------- recording (needs oracle/ref.py's library) and its layout
def sparse(b):
    """Bucket matrices -> (indices of the non-empty buckets, x, y, depth, count)."""
    bx, by, bd, bc = b
    idx = np.nonzero(bc)[0].astype(np.int32)
    assert not bx[bc == 0].any() and not by[bc == 0].any() and not bd[bc == 0].any(), "an empty bucket holds a value"
    return idx, bx[idx], by[idx], bd[idx], bc[idx]


def dense(z, k):
    bx, by, bd = [np.zeros(NBX * NBY, dtype=np.float32) for _ in range(3)]
    bc = np.zeros(NBX * NBY, dtype=np.int32)
    idx = z["f%d_bidx" % k]
    bx[idx], by[idx], bd[idx], bc[idx] = z["f%d_bx" % k], z["f%d_by" % k], z["f%d_bd" % k], z["f%d_bc" % k]
    return bx, by, bd, bc


def new_session(ref, calib, s):
    return ref.VO(*calib, remove_outlier=s["remove_outlier"], reset_to_identity=s["reset_to_identity"], optical_flow_match=s["optical_flow_match"])


def solve_run(r, run):
    return r.solve(run["kp_prev"], run["kp_curr"], run.get("query_idx"), run.get("train_idx"), run.get("status"), run.get("prior_q"), run.get("prior_t"))


def record(ref, sc):
    """Run the reference binary on a scenario; the arrays of its recording (inputs and outputs)."""
    d = dict(cam_T_velo=sc["calib"][0], rect0_T_cam=sc["calib"][1], P_rect0=sc["calib"][2], n_frames=np.int32(len(sc["frames"])),
             n_sessions=np.int32(len(sc["sessions"])))
    for si, s in enumerate(sc["sessions"]):
        r = new_session(ref, sc["calib"], s)
        d["s%d_opts" % si] = np.array([s["remove_outlier"], s["reset_to_identity"], s["optical_flow_match"]], dtype=np.int32)
        d["s%d_run_frames" % si] = np.array(sorted(s["runs"]), dtype=np.int32)
        for k, c in enumerate(sc["frames"]):
            r.frame(c)
            if si == 0:
                d["f%d_cloud" % k] = f32(c[:, :3])
                d["f%d_p2d" % k] = r.points2d()
                d["f%d_dnsp" % k] = r.dnsp()
                d["f%d_bidx" % k], d["f%d_bx" % k], d["f%d_by" % k], d["f%d_bd" % k], d["f%d_bc" % k] = sparse(r.buckets(0))
                if k in sc["queries"]:
                    d["f%d_qxy" % k] = sc["queries"][k]
                    d["f%d_qdepth" % k], tie = r.query_depth(0, sc["queries"][k])
                    d["f%d_qtie" % k] = tie.astype(np.uint8)
            if k in s["runs"]:
                run = s["runs"][k]
                res = solve_run(r, run)
                pre = "s%d_r%d_" % (si, k)
                for key, v in run.items():
                    d[pre + "in_" + key] = v
                d[pre + "rows"] = res["match_rows"]
                d[pre + "x_in"] = np.concatenate([res["angles_in"], res["t_in"]])
                d[pre + "x_out"] = np.concatenate([res["angles"], res["t"]])
                d[pre + "counters"] = np.array([res["counter32"], res["counter22"]], dtype=np.int32)
    return d


def tie_share(d):
    """(ties, queries) over every query list of a recording."""
    t = [d[k] for k in d if k.endswith("_qtie")]
    return int(sum(int(a.sum()) for a in t)), int(sum(a.size for a in t))
