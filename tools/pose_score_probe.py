#!/usr/bin/env python3
"""Pose scores, measured (profiles/r12_pose_score.txt): on the 64 x 2048 bench map after N sweeps, M poses x (512 corner + 2048 surf points) at
radius 1.0 through

  score:  vloam_map_score_poses_device, one call
  query:  the only way to get the same hit counts without it — the M * N points transformed with torch (f64, rounded to f32), two
          vloam_map_query_device calls with k = 1 (corner points against the corner map, surf points against the surf map), hits summed from `count`

Each timed with a host clock around `repeats` calls that end in a synchronise of the handle and of torch, after a warm-up call; the two routes
alternate.  The hit counts of the two routes are compared.  Where the score's time goes, by poses that switch parts of the kernel off: poses
2e7 m away are not searched at all (transform, LDS staging, reductions and atomics remain); poses 500 m away are searched in empty space (the
piece tables are built and every occupancy block of the box is probed, no voxel record is read); the poses themselves read records too.
Then vloam_map_relocalize on the 9 x 9 x 1 x 9 grid, top_k 4.  Usage: python tools/pose_score_probe.py [--sweeps 200] [--poses 4096]"""
import argparse
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
_seq = None


def _sweep(k):
    global _seq
    import conftest
    synth = conftest.load_synth()
    if _seq is None:
        _seq = synth.SynthSequence(n_rings=64, n_azimuth=2048, n_sweeps=int(os.environ["SCORE_PROBE_T"]) + 1)
    return _seq.sweep(k)


def thin(cloud, n):
    return np.ascontiguousarray(cloud[::max(1, cloud.shape[0] // n)][:n], dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--poses", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    os.environ["SCORE_PROBE_T"] = str(a.sweeps)
    with ProcessPoolExecutor(16) as ex:   # before HIP exists in this process
        clouds = list(ex.map(_sweep, range(a.sweeps), chunksize=4))
    import torch
    torch.zeros(1).cuda()
    import conftest
    vl = conftest.load_pkg()
    n_pts = max(c.shape[0] for c in clouds)
    h = vl.Handle(0, with_mapping=1, max_points=n_pts, max_frames=a.sweeps + 8)
    for c in clouds:
        h.process_scan(c)
    h.sync()
    src = vl.Handle(0, with_mapping=0, max_points=n_pts, max_frames=4)
    src.scan_registration(clouds[-1])
    corner, surf = thin(src.features(2), 512), thin(src.features(4), 2048)
    src.close()
    true = h.trajectory()[a.sweeps - 1, 7:14].copy()
    true[:4] /= np.linalg.norm(true[:4])
    rng = np.random.default_rng(5)
    M = a.poses
    ang = np.deg2rad(rng.uniform(-10, 10, M)) / 2.0
    qy = np.stack([np.zeros(M), np.zeros(M), np.sin(ang), np.cos(ang)], axis=1)
    x1, y1, z1, w1 = qy.T
    x2, y2, z2, w2 = true[:4]
    q = np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2,
                  w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], axis=1)
    t = true[4:] + rng.uniform(-2, 2, (M, 3)) * np.array([1.0, 1.0, 0.0])
    poses = np.ascontiguousarray(np.concatenate([q, t], axis=1))
    print("map: %d sweeps, %d corner + %d surf map points; %d poses x (%d corner + %d surf) points, radius 1.0" %
          (a.sweeps, h.get_map_kind(0).shape[0], h.get_map_kind(1).shape[0], M, corner.shape[0], surf.shape[0]), flush=True)

    d_c, d_s = torch.from_numpy(corner).cuda(), torch.from_numpy(surf).cuda()
    out = torch.zeros(M * vl.POSE_SCORE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")

    def score(p):
        h.map_score_poses_device(d_c, d_s, p, out)
        h.sync()

    nq = [M * corner.shape[0], M * surf.shape[0]]
    qbuf = [torch.zeros((n, 4), dtype=torch.float32, device="cuda") for n in nq]
    xyzi = [torch.zeros((n, 4), dtype=torch.float32, device="cuda") for n in nq]
    d2 = [torch.zeros(n, dtype=torch.float32, device="cuda") for n in nq]
    cnt = [torch.zeros(n, dtype=torch.int32, device="cuda") for n in nq]
    hits_q = [None, None]

    def query(p):
        u, w, tt = p[:, None, 0:3], p[:, None, 3:4], p[:, None, 4:7]
        for kind, pts in enumerate((d_c, d_s)):
            v = pts[None, :, :3].double()
            c = torch.cross(u.expand(-1, v.shape[1], -1), v.expand(p.shape[0], -1, -1), dim=2)
            c = c + c
            qbuf[kind].view(p.shape[0], -1, 4)[:, :, :3] = ((v + w * c) + torch.cross(u.expand_as(c), c, dim=2) + tt).float()
        torch.cuda.synchronize()
        for kind in (0, 1):
            h.map_query_device(qbuf[kind].data_ptr(), nq[kind], xyzi[kind].data_ptr(), d2[kind].data_ptr(), cnt[kind].data_ptr(), k=1, max_radius=1.0, kind=kind)
        h.sync()
        for kind in (0, 1):
            hits_q[kind] = cnt[kind].view(p.shape[0], -1).sum(dim=1)
        torch.cuda.synchronize()

    def timed(fn, arg):
        t0 = time.perf_counter()
        for _ in range(a.repeats):
            fn(arg)
        return 1e3 * (time.perf_counter() - t0) / a.repeats

    d_p = torch.from_numpy(poses).cuda()
    score(d_p)
    query(d_p)
    rec = out.cpu().numpy().view(vl.POSE_SCORE_DTYPE)
    same = all(np.array_equal(rec["n_hit"][:, k], hits_q[k].cpu().numpy()) for k in (0, 1))
    print("hit counts of the two routes equal: %s (hits per pose, mean: %.1f corner, %.1f surf)" % (same, rec["n_hit"][:, 0].mean(), rec["n_hit"][:, 1].mean()), flush=True)
    ts, tq = [], []
    for r in range(3):   # alternating
        ts.append(timed(score, d_p))
        tq.append(timed(query, d_p))
        print("pass %d: score %.3f ms per call, query route %.3f ms per call" % (r, ts[-1], tq[-1]), flush=True)
    print("score %.3f ms (min of 3 passes of %d calls), query route %.3f ms: ratio query / score %.2f" % (min(ts), a.repeats, min(tq), min(tq) / min(ts)))
    parts = {}
    for name, shift in (("poses 2e7 m away (no search)", [0.0, 2.0e7, 0.0]), ("poses 500 m away (empty space)", [500.0, 0.0, 0.0])):
        far = poses.copy()
        far[:, 4:] += shift
        d_f = torch.from_numpy(far).cuda()
        score(d_f)
        assert not out.cpu().numpy().view(vl.POSE_SCORE_DTYPE)["n_hit"].any()
        parts[name] = min(timed(score, d_f) for _ in range(3))
        print("score, %s: %.3f ms per call" % (name, parts[name]), flush=True)
    full, none, empty = min(ts), parts["poses 2e7 m away (no search)"], parts["poses 500 m away (empty space)"]
    print("share of the score call that is the table walk: %.0f %% (piece tables + block probes %.0f %%, voxel records %.0f %%); launch, transform, staging, "
          "reductions and atomics %.0f %%" % (100 * (full - none) / full, 100 * (empty - none) / full, 100 * (full - empty) / full, 100 * none / full))
    qc, tc = true[:4], true[4:] + np.array([1.5, -1.0, 0.0])
    h.map_relocalize(corner, surf, qc, tc)
    tr = []
    for _ in range(5):
        t0 = time.perf_counter()
        r = h.map_relocalize(corner, surf, qc, tc)
        tr.append(1e3 * (time.perf_counter() - t0))
    print("vloam_map_relocalize, 9 x 9 x 1 x 9 candidates, top_k 4, %d + %d points: %.2f ms wall (median of 5; %.2f - %.2f); refined[best] %.3f m from the true pose"
          % (corner.shape[0], surf.shape[0], float(np.median(tr)), min(tr), max(tr), float(np.linalg.norm(r["refined"][r["best"]]["t_map"] - true[4:]))))
    h.close()


if __name__ == "__main__":
    main()
