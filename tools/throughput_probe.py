#!/usr/bin/env python3
"""Quick steady-state throughput probe (seconds, not minutes): one sequence and B batched sequences of 64 x 2048 sweeps with mapping,
after a short warm-up.  For A/B-ing a kernel change; bench.py remains the measurement of record.
  python tools/throughput_probe.py [--sessions 8] [--warm 60] [--steps 120] [--table]
  python tools/throughput_probe.py --no-batch --steps 200 --map-pub-number 20 --publish-registered-cloud --publish-ab 3
      the single sequence with the published clouds of the mapping stream (vloam_limits) off and on, alternately, in one process
  python tools/throughput_probe.py --no-batch --steps 200 --pose-info-ab 3 [--table]
      the single sequence with the pose information product (vloam_pose_info_enable) off and on, alternately
  python tools/throughput_probe.py --no-batch --steps 200 --pose-cov-ab 3
      the single sequence with neither product, with pose information, and with pose information + covariance rows (vloam_pose_cov_enable), alternately
  python tools/throughput_probe.py --no-batch --steps 2000 --map-log2 20 --map-grow-ab 3
      the single sequence on a fixed handle and on a growable one (vloam_map_options::grow) of the same size, alternately
  python tools/throughput_probe.py --no-batch --steps 200 --map-archive-ab 3
      the single sequence without and with the map archive (vloam_map_archive_enable), alternately
  python tools/throughput_probe.py --grow-step 18,21
      one forced growth step of both tables from 2^18 and from 2^21 slots with the warm-up's map in them (for a kernel trace: --procs 1)"""
import argparse
import multiprocessing as mp
import os
import sys
import time

# the stage streams of a handle (+ torch's) must not share hardware queues (the runtime's default is 4); before the HIP runtime loads
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sessions", type=int, default=8)
ap.add_argument("--warm", type=int, default=60)
ap.add_argument("--steps", type=int, default=120)
ap.add_argument("--sweeps", type=int, default=48)
ap.add_argument("--table", action="store_true", help="per-kernel HIP-event table of the batched run")
ap.add_argument("--no-single", action="store_true")
ap.add_argument("--no-batch", action="store_true")
ap.add_argument("--map-pub-number", type=int, default=0, help="vloam_limits::map_pub_number of the handles")
ap.add_argument("--publish-registered-cloud", action="store_true", help="vloam_limits::publish_registered_cloud of the handles")
ap.add_argument("--publish-ab", type=int, default=0, help="that many off / on pairs of single-sequence runs, products off first; replaces the normal run")
ap.add_argument("--sweep-log-ab", type=int, default=0, help="that many off / on pairs of single-sequence runs (then of --sessions batches unless --no-batch), "
                                                         "vloam_limits_ext::sweep_log off first; replaces the normal run")
ap.add_argument("--pose-info-ab", type=int, default=0, help="that many off / on pairs of single-sequence runs (then of --sessions batches unless --no-batch), the pose "
                                                         "information product (vloam_pose_info_enable) off first; replaces the normal run")
ap.add_argument("--pose-cov-ab", type=int, default=0, help="that many off / pose information / pose information + covariance rows (vloam_pose_cov_enable) triples of "
                                                        "single-sequence runs (then of --sessions batches unless --no-batch); replaces the normal run")
ap.add_argument("--map-grow-ab", type=int, default=0, help="that many fixed / growable pairs of single-sequence runs at --map-log2, fixed first; replaces the normal run")
ap.add_argument("--map-archive-ab", type=int, default=0, help="that many off / on pairs of single-sequence runs, the map archive (vloam_map_archive_enable) off first; replaces the normal run")
ap.add_argument("--grow-step", default="", help="comma-separated log2 sizes: a growable handle of that size, --warm sweeps, one forced growth step, timed on the host; replaces the normal run")
ap.add_argument("--map-log2", type=int, default=22, help="map_capacity_log2 of the handles (voxel table slots)")
ap.add_argument("--procs", type=int, default=32, help="worker processes for the synthesis (1 under rocprofv3: it follows forked children)")
ap.add_argument("--from-idle", default="", help="comma-separated sweep counts: time that many sweeps of ONE sequence from a drained pipeline (5 repeats each) "
                "and fit time = fill + period x sweeps; replaces the normal run")
a = ap.parse_args()
synth = conftest.load_synth()
_SEQ = synth.SynthSequence(n_rings=64, n_azimuth=2048, n_sweeps=a.sweeps + 1)


def _w(k):
    return _SEQ.sweep(k)


if a.procs > 1:
    with mp.get_context("fork").Pool(min(a.procs, os.cpu_count() or 1)) as pool:   # before the HIP runtime loads
        host = np.stack(pool.map(_w, range(a.sweeps), chunksize=2))
else:
    host = np.stack([_w(k) for k in range(a.sweeps)])
vl = conftest.load_pkg()
import torch  # noqa: E402

d = torch.from_numpy(host).cuda()
npts = host.shape[1]
ptr = lambda k: d.data_ptr() + (k % a.sweeps) * npts * 16   # noqa: E731  (the sequence wraps: a jump back every a.sweeps, same for every variant)


PUB = dict(map_pub_number=a.map_pub_number, publish_registered_cloud=int(a.publish_registered_cloud))


def run(B, pub=PUB):
    pub = dict(pub)
    pose_info = pub.pop("pose_info", 0)
    pose_cov = pub.pop("pose_cov", 0)
    map_archive = pub.pop("map_archive", 0)
    h = vl.Handle(0, n_sessions=B, with_mapping=1, max_frames=a.warm + a.steps + 8, map_capacity_log2=a.map_log2, **pub)
    if pose_info:
        h.enable_pose_info()
    if pose_cov:
        h.pose_cov_enable()
    if map_archive:
        h.map_archive_enable()
    step = (lambda k: h.process_scan_device(ptr(k), npts)) if B == 1 else (lambda k: h.batch_process_scan_device([ptr(k)] * B, [npts] * B))
    for k in range(a.warm):
        step(k)
    h.sync()
    if a.table:
        h.profile_kernel("*", 16384)
    t0 = time.perf_counter()
    for k in range(a.warm, a.warm + a.steps):
        step(k)
    h.sync()
    dt = time.perf_counter() - t0
    note = "   sweep_log 1" if pub.get("sweep_log") else ""
    note += "   pose_info 1" if pose_info else ""
    note += "   pose_cov 1" if pose_cov else ""
    note += "   map_archive 1 %s" % (h.map_archive_info(),) if map_archive else ""
    if pub.get("map_pub_number") or pub.get("publish_registered_cloud"):
        note += "   published: map every %d, registered cloud %d" % (pub["map_pub_number"], pub["publish_registered_cloud"])
    print("B = %2d: %8.0f scans/s   (%.1f us per step)%s" % (B, B * a.steps / dt, 1e6 * dt / a.steps, note), flush=True)
    if a.table:
        rows = h.profile_table()
        tot = sum(ms for ms, _ in rows.values())
        for name, (ms, cnt) in sorted(rows.items(), key=lambda kv: -kv[1][0])[:14]:
            print("   %-20s %6.1f us x %5d  (%4.1f %%)" % (name, 1e3 * ms / max(cnt, 1), cnt, 100 * ms / tot))
        for name in ("k_lm_solve", "k_pose_info_lo", "k_pose_info_map"):
            if pose_info and name in rows:
                print("   %-20s %6.1f us x %5d  (new kernels next to one solve launch)" % (name, 1e3 * rows[name][0] / max(rows[name][1], 1), rows[name][1]))
    if pub.get("map_grow"):
        print("         growable: %s" % (h.health(),), flush=True)
    tr = h.trajectory(0, a.warm + a.steps)
    h.close()
    return tr


def grow_step(sizes):
    for lg in sizes:
        h = vl.Handle(0, with_mapping=1, max_frames=a.warm + 8, map_capacity_log2=lg, map_grow=1)
        for k in range(a.warm):
            h.process_scan_device(ptr(k), npts)
            if k % 4 == 3:
                h.sync()
        h.sync()
        before, keys = h.health(), h.map_health()["keys"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.map_force_grow()
        h.sync()
        dt = time.perf_counter() - t0
        print("start 2^%d: tables %s with %s keys -> %s: %.3f ms on the host for both steps (allocation, memsets, k_map_grow, sync); growth steps before: %d"
              % (lg, before["map_log2"], keys, h.health()["map_log2"], 1e3 * dt, before["map_growth_steps"]), flush=True)
        h.close()


def from_idle(counts):
    h = vl.Handle(0, with_mapping=1, max_frames=a.warm + 6 * sum(counts) + 64)
    k = 0
    for _ in range(a.warm):
        h.process_scan_device(ptr(k), npts); k += 1
    h.sync()
    xs, ys = [], []
    for n in counts:
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                h.process_scan_device(ptr(k), npts); k += 1
            h.sync()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        print("%4d sweeps from idle: median %.3f ms (min %.3f)  -> %6.0f scans/s" % (n, 1e3 * ts[2], 1e3 * ts[0], n / ts[2]), flush=True)
        xs.append(n); ys.append(ts[2])
    if len(xs) >= 2:
        b, c = np.polyfit(xs, ys, 1)
        print("fit: fill %.3f ms + %.1f us per sweep" % (1e3 * c, 1e6 * b))
    h.close()


if a.from_idle:
    from_idle([int(v) for v in a.from_idle.split(",")])
    sys.exit(0)
if a.grow_step:
    grow_step([int(v) for v in a.grow_step.split(",")])
    sys.exit(0)
if a.map_grow_ab:
    for _ in range(a.map_grow_ab):
        run(1, dict())
        run(1, dict(map_grow=1))
    sys.exit(0)
if a.publish_ab:
    for _ in range(a.publish_ab):
        run(1, dict(map_pub_number=0, publish_registered_cloud=0))
        run(1)
    sys.exit(0)
if a.pose_info_ab:
    for B in [1] + ([] if a.no_batch else [a.sessions]):
        for _ in range(a.pose_info_ab):
            run(B, dict(pose_info=0))
            run(B, dict(pose_info=1))
    sys.exit(0)
if a.pose_cov_ab:
    for B in [1] + ([] if a.no_batch else [a.sessions]):
        for _ in range(a.pose_cov_ab):
            run(B, dict(pose_info=0))
            run(B, dict(pose_info=1))
            run(B, dict(pose_info=1, pose_cov=1))
    sys.exit(0)
if a.map_archive_ab:
    for _ in range(a.map_archive_ab):
        run(1, dict(map_archive=0))
        run(1, dict(map_archive=1))
    sys.exit(0)
if a.sweep_log_ab:
    for B in [1] + ([] if a.no_batch else [a.sessions]):
        for _ in range(a.sweep_log_ab):
            run(B, dict(sweep_log=0))
            run(B, dict(sweep_log=1))
    sys.exit(0)
t1 = None if a.no_single else run(1)
if a.no_batch:
    sys.exit(0)
tb = run(a.sessions)
if t1 is not None:
    print("batched session 0 identical to the single sequence:", bool(np.array_equal(t1, tb)))
