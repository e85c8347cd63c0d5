#!/usr/bin/env python3
"""bench.py — scans/s of the MI355X-native VLOAM per-scan odometry hot path on synthetic HDL-64E sweeps.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W``; for N > 1 launched through
``python -m torch.distributed.run --nproc-per-node N …`` (one rank per GPU, RCCL).  A *step* is one
sweep (64 rings x 2048 azimuth steps = 131 072 points) through the façade
reset -> scanRegistration -> laserOdometry -> laserMapping (lidar_odometry_mapping.cpp:73-154) on inputs
already resident in HBM.  The default workload is BASELINE.json's configs[2] — the configuration the metric
("scans/s END-TO-END odometry", SURVEY.md §8d: SR -> LO -> laserMapping) is quoted on: before the W warm-up
steps the sequence's first ``--map-warmup`` (200) sweeps are streamed through the same handle, untimed, so
that the voxel-hash local map is at its steady-state size ("~200 scans") when the K timed sweeps run.
``--workload lo`` is configs[1] (no mapping); a ``--full`` run reports it as the extra leg ``configs1``.
Rank r drives its own independent sequence (different scene / trajectory / noise seeds): the path
shards one-sequence-per-GPU with no data-path collective; the only collective is an
all-gather of the trajectories after the timed region.  Rank 0 prints ONE JSON line.

A plain run does only what the headline needs: it synthesises the sweeps, warms up, times the K steps,
writes the outputs if ``--dump-outputs DIR`` is given and prints the line.  Everything else — the
per-kernel replay and the roofline, the extra legs (configs[1], batched sessions, latency, sustained
streaming, host input, the VO / image stages), the CPU baseline and the parity check against the
oracle — runs only with ``--full`` (``--no-kernel-timer``, ``--no-extras``, ``--no-cpu-baseline``
switch single parts of it off again).

``--dump-outputs DIR`` writes, after the timed region, what a caller of the timed path holds after its
last step (rank 0): the trajectory rows of the K timed sweeps (float64), the last sweep's scan-registration
clouds, its registered full-resolution cloud and the published map (float32 x, y, z, intensity), as
DIR/<name>.npy.  The inputs are synthesised from fixed seeds, so the same arguments give the same inputs.

PyTorch is plumbing only here (device buffers for the inputs, torch.distributed barrier / gather).
The CPU oracle (oracle/) is used only for the ``cpu_baseline`` leg and the parity numbers — never
inside the timed region.
"""
import argparse
import glob
import json
import multiprocessing as mp
import os
import sys
import time

# the three stage streams of a handle (+ torch's) should not share hardware queues; must be set before the HIP runtime loads
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6.3 TB/s achievable

WORKLOADS = {
    "lo": "configs[1]: scanRegistration + scan-to-scan laserOdometry ICP, synthetic HDL-64E 64x2048",
    "map": "configs[2]: scanRegistration + laserOdometry + laserMapping scan-to-map ICP (voxel-hash local map, ~200 scans), synthetic HDL-64E 64x2048",
}

# the reference's per-substage timers -> the kernels that do that work here
REFERENCE_TIMERS = {
    "scan registration: prepare + sort q time + seperate points (scan_registration.cpp:285,430-432)":
        ["k_sr_first_last", "k_sr_label", "k_sr_scatter", "k_sr_ring", "k_sr_compact"],
    "laser odometry: data association (laser_odometry.cpp:453)": ["k_lo_assoc"],
    "laser odometry / mapping: solver time (laser_odometry.cpp:465, laser_mapping.cpp:618)": ["k_lm_compact", "k_lm_solve"],
    "laser odometry: build tree -> NN grids (laser_odometry.cpp:525-526)": ["k_lo_grid_count", "k_lo_grid_scan", "k_lo_grid_scatter"],
    "laser mapping: filter time (laser_mapping.cpp:432-446)": ["k_map_ds_bin", "k_map_ds_reduce"],
    "laser mapping: shift + build tree (laser_mapping.cpp:422,453) -> none needed: persistent voxel hash": ["k_map_prepare"],
    "laser mapping: mapping data assosiation (laser_mapping.cpp:606)": ["k_map_assoc", "k_map_fit"],
    "laser mapping: add points + filter (laser_mapping.cpp:686,705)": ["k_map_insert", "k_map_finalize"],
}


# the per-unit figure behind algorithmic_bytes() for the kernels a roofline object is usually built for
ALGORITHMIC_UNIT = {
    "k_lm_solve": "64 B per factor and residual/Jacobian evaluation (SURVEY.md §8d: curr + <= 3 matched points); units per launch = (F E_o + K_m E_m) / 4 of counts_last_sweep",
    "k_lo_assoc": "16 B per feature + 16 B per point of CornerLast / SurfLast (read once) + 76 B per factor record written",
    "k_map_assoc": "(16 + 5 x 32 + 20) B per stack point: the point, five 32-byte voxel records, five slot ids",
    "k_sr_ring": "16 B per point in + 16 B per lessFlat point out + 4 B per pick",
    "k_map_ds_reduce": "8 B per key + 16 B per point in, 16 B per occupied cell out",
    "k_map_ds_bin": "16 B per point in + 8 B per sort key out",
}


def algorithmic_bytes(kernel, c):
    """ALGORITHMIC (compulsory) bytes one launch of `kernel` moves, from the measured counts of the run."""
    n_feat = c["n_sharp"] + c["n_flat"]
    F = c["F_corner"] + c["F_plane"]
    nn = c["n_c"] + c["n_s"]
    n_less = c["n_lessSharp"] + c["n_lessFlat"]
    if kernel in ("k_lo_assoc", "k_lo_assoc_fast"):  # features + both candidate clouds read once, one 76-byte factor record written per factor
        return 16 * n_feat + 16 * (c["C"] + c["S"]) + 76 * F
    if kernel == "k_lm_solve":
        # every residual / Jacobian evaluation reads curr + <= 3 matched points = 64 B per factor; a launch is one solve, the
        # units of a launch are its factor-evaluations — averaged over the solves of a sweep (2 odometry + 2 mapping): (F E_o + K_m E_m) / 4
        if c["K_m"] > 0:
            return 64 * (F * c["E_o"] + c["K_m"] * c["E_m"]) / 4.0
        return 64 * F * max(c["E_o"], 2) / 2.0
    if kernel == "k_lm_compact":
        return 2 * 76 * c["K_m"]
    if kernel == "k_sr_ring":   # ring-ordered cloud in, per-ring voxel centroids + picks out
        return 16 * c["N2"] + 16 * c["n_lessFlat"] + 4 * (c["n_sharp"] + c["n_lessSharp"] + c["n_flat"])
    if kernel == "k_sr_first_last":   # sixteen walkers (eight per end) look at one 4 096-point trip each on an ordinary sweep
        return 16 * min(c["N_in"], 16 * 4096)
    if kernel == "k_sr_label":
        return 16 * c["N_in"] + 5 * c["N_in"]
    if kernel == "k_sr_scatter":
        return 16 * c["N_in"] + 5 * c["N_in"] + 16 * c["N2"]
    if kernel == "k_sr_compact":
        return 32 * (c["n_sharp"] + c["n_lessSharp"] + c["n_flat"] + c["n_lessFlat"])
    if kernel in ("k_lo_grid_count", "k_lo_grid_scatter"):  # the two less-clouds in; scatter also writes the bucket-ordered copies (2 levels)
        return 16 * n_less + (2 * 16 * n_less if kernel == "k_lo_grid_scatter" else 0)
    if kernel == "k_map_ds_bin":      # the two less-clouds in, one 8-byte sort key (cell index | point index) per point out
        return 16 * n_less + 8 * n_less
    if kernel == "k_map_ds_reduce":   # the keys back in, every point fetched once, one centroid per occupied cell out
        return 8 * n_less + 16 * n_less + 16 * nn
    if kernel == "k_map_assoc":   # stack point in, 5 neighbour voxels (32-byte records) looked at, 5 slot ids out
        return nn * (16 + 5 * 32 + 20)
    if kernel == "k_map_fit":     # 5 neighbours in, one 76-byte factor record out
        return nn * (16 + 5 * 32) + 76 * c["K_m"]
    if kernel == "k_map_insert":  # stack point in, map-frame point out, one voxel record touched
        return nn * (16 + 16 + 32)
    if kernel == "k_map_finalize":
        return nn * (16 + 2 * 32)
    return 0


def pmc_traffic(workload, kernel):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 --pmc passes (FETCH_SIZE and WRITE_SIZE collected in
    separate runs, FETCH_SIZE doubled per the gfx950 note of MI355X_MICROARCH.md; tools/pmc_summary.py wrote the table).
    A PMC pass cannot run inside this process, so the number is read from profiles/ (latest round) — None when missing, and None when
    the table was measured on OTHER kernel sources than the ones being timed: the table's header carries the content hash of csrc/
    (tools/pmc_summary.py: csrc_sha256) and a table without a matching hash is named as stale instead of being quoted."""
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_%s_hbm_traffic.txt" % workload)))
    if not cands:
        return None, None
    path = cands[-1]
    rel = os.path.relpath(path, ROOT)
    tot, cnt, sha = 0.0, 0, None
    try:
        for line in open(path):
            if line.startswith("# csrc_sha256:"):
                sha = line.split(":", 1)[1].strip()
            name = line.split("<")[0].split()[:1]
            f = line.split()
            if name and name[0] == kernel and len(f) >= 5:  # every instantiation of the kernel, weighted by its launches
                tot += float(f[-1]) * int(f[-4])
                cnt += int(f[-4])
    except (OSError, ValueError):
        return None, None
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pmc_summary
    now = pmc_summary.csrc_sha256(ROOT)
    if sha != now:
        return None, "%s is STALE (measured on csrc %s, timing csrc %s): not quoted" % (rel, sha or "without a hash", now)
    if cnt == 0:
        return None, None
    return tot / cnt, rel


def _matching_profile(pattern):
    """Latest profiles/ table of that name whose header carries the content hash of the kernel sources being timed; (lines, relative path) or (None, why)."""
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)))
    if not cands:
        return None, None
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pmc_summary
    now = pmc_summary.csrc_sha256(ROOT)
    path = cands[-1]
    rel = os.path.relpath(path, ROOT)
    try:
        lines = open(path).read().split("\n")
    except OSError:
        return None, None
    sha = next((l.split(":", 1)[1].strip() for l in lines if l.startswith("# csrc_sha256:")), None)
    if sha != now:
        return None, "%s is STALE (measured on csrc %s, timing csrc %s): not quoted" % (rel, sha or "without a hash", now)
    return lines, rel


def rocprof_avg_us(workload, kernel):
    """Average duration of `kernel` in the committed rocprofv3 --kernel-trace --stats summary of the same command (all instantiations, weighted
    by calls) — only when that summary was measured on the kernel sources being timed."""
    lines, src = _matching_profile("r[0-9][0-9]_%s_kernel_stats.txt" % workload)
    if lines is None:
        return None, src
    tot, calls = 0.0, 0
    for l in lines:
        f = l.split()
        if len(f) >= 5 and not l.startswith("#") and l.split("<")[0].split()[0] == kernel:
            try:
                calls += int(f[-4]); tot += float(f[-3])
            except ValueError:
                pass
    return (tot / calls if calls else None), src


def sq_wait_pct(kernel):
    """Share of its wave cycles `kernel` spends waiting (SQ_WAIT_ANY / SQ_WAVE_CYCLES, single-sequence run), from the committed SQ-counter
    table when it was measured on the kernel sources being timed."""
    lines, src = _matching_profile("r[0-9][0-9]_batch1_sq_counters.txt")
    if lines is None:
        return None, src
    num, den = 0.0, 0.0
    for l in lines:
        f = l.split()
        if len(f) >= 7 and not l.startswith("#") and l.split("<")[0].split()[0] == kernel:
            try:
                w = float(f[-5]) * int(f[-6]); num += float(f[-2]) * w; den += w
            except ValueError:
                pass
    return (num / den if den else None), src


def sweep_bytes(c, with_mapping):
    """B_SR + B_LO (+ B_MAP) per sweep from measured counts."""
    n_feat_all = c["n_sharp"] + c["n_lessSharp"] + c["n_flat"] + c["n_lessFlat"]
    b_sr = 16 * c["N_in"] + 16 * c["N2"] + 16 * n_feat_all
    F_o = c["F_corner"] + c["F_plane"]
    b_lo = 2 * (16 * (c["n_sharp"] + c["n_flat"]) + 16 * (c["C"] + c["S"])) + c["E_o"] * F_o * 64 + 16 * (c["n_lessSharp"] + c["n_lessFlat"])
    b_map = 0
    if with_mapping:
        nn = c["n_c"] + c["n_s"]
        b_map = 16 * (c["C"] + c["S"]) + 16 * c["M"] + 2 * nn * (16 + 5 * 16) + c["E_m"] * c["K_m"] * 64 + 16 * nn + 2 * 16 * c["M"]
    return b_sr, b_lo, b_map


DUMP_LIMIT_BYTES = 64 << 20
SCAN_CLOUDS = ((0, "laserCloud"), (1, "cornerPointsSharp"), (2, "cornerPointsLessSharp"), (3, "surfPointsFlat"), (4, "surfPointsLessFlat"))


def timed_outputs(h, traj, first, with_mapping):
    """What a caller of the timed path holds after its last step (c_api.h): the trajectory rows of the timed sweeps (f64: laser-odometry
    world pose + mapping pose), the last sweep's scan-registration clouds and, with mapping, its full-resolution cloud registered in the
    map frame and the published map (f32 x, y, z, intensity)."""
    out = {"trajectory": traj[first:]}
    for which, name in SCAN_CLOUDS:
        out[name] = h.features(which)
    if with_mapping:
        out["laserCloudRegistered"] = h.features(11)
        out["laserCloudMap"] = h.get_map()
    return out


def dump_outputs(path, arrays):
    """DIR/<name>.npy per array in its own dtype; an array larger than its share of DUMP_LIMIT_BYTES is replaced by a fixed, seeded sample
    of its rows, kept in order."""
    os.makedirs(path, exist_ok=True)
    share = DUMP_LIMIT_BYTES // len(arrays)
    for name, a in arrays.items():
        if a.nbytes > share:
            keep = np.random.default_rng(0).choice(a.shape[0], share // (a.nbytes // a.shape[0]), replace=False)
            a = a[np.sort(keep)]
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))


# ---------------------------------------------------------------------------------------------------- host-side helpers
_SEQS = []
_SYNTH = None


def _synth_worker(job):
    what, s, k = job
    if what == "sweep":
        return _SEQS[s].sweep(k)
    if what == "image":
        return _SYNTH.render_image(_SEQS[s], k)
    return _SYNTH.synth_matches(_SEQS[s], k)   # "match"


def synthesise(synth, jobs, seqs, procs):
    """Run the ray-casting / rendering / matching jobs [(what, sequence, frame)] in worker processes (forked BEFORE the HIP runtime loads)."""
    global _SEQS, _SYNTH
    _SEQS, _SYNTH = seqs, synth
    if procs > 1 and len(jobs) > 1:
        with mp.get_context("fork").Pool(min(procs, len(jobs))) as pool:
            return pool.map(_synth_worker, jobs, chunksize=2)
    return [_synth_worker(j) for j in jobs]


def _oracle_worker(args):
    """One CPU-oracle session over sweeps [0, n) in its own process (the "N sequences on N cores" figure)."""
    rings, with_mapping, n, path = args
    import orc
    host = np.load(path, mmap_mode="r")
    o = orc.Oracle(scan_line=rings, with_mapping=with_mapping)
    t0 = time.perf_counter()
    for k in range(n):
        o.process(np.asarray(host[k]))
    return time.perf_counter() - t0


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def pose_err(row, q_lo, t_lo, q_map, t_map, with_mapping):
    dt = float(np.linalg.norm(row[4:7] - t_lo))
    dq = float(min(np.linalg.norm(row[0:4] - q_lo), np.linalg.norm(row[0:4] + q_lo)))
    if with_mapping:
        dt = max(dt, float(np.linalg.norm(row[11:14] - t_map)))
        dq = max(dq, float(min(np.linalg.norm(row[7:11] - q_map), np.linalg.norm(row[7:11] + q_map))))
    return dt, dq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default=os.environ.get("VLOAM_BENCH_WORKLOAD", "map"))
    ap.add_argument("--map-warmup", type=int, default=int(os.environ.get("VLOAM_BENCH_MAP_WARMUP", "200")),
                    help="configs[2]: sweeps streamed (untimed) before the warm-up steps so that the local map is at steady state")
    ap.add_argument("--kernel", default=os.environ.get("VLOAM_BENCH_KERNEL", ""), help="kernel the roofline object is computed for (default: the one with the largest share of GPU time in this run)")
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--azimuth", type=int, default=2048)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-cores-leg", type=int, default=24, help="sweeps per process of the 'N sequences on N cores' CPU figure (0 = skip)")
    ap.add_argument("--no-kernel-timer", action="store_true", help="skip the HIP-event replay (per-kernel table + roofline kernel; for profiler runs)")
    ap.add_argument("--no-extras", action="store_true", help="skip the extra legs (latency, configs[1], multi-session, VO stage)")
    ap.add_argument("--vo-frames", type=int, default=20, help="extra leg: frames of the coupled VLOAM loop (configs[3] analogue) to time (0 = skip)")
    ap.add_argument("--image-frames", type=int, default=24, help="extra leg: frames of the coupled loop driven from raw images (rendered on the host before the GPU work starts; 0 = skip)")
    ap.add_argument("--sessions", type=int, default=int(os.environ.get("VLOAM_BENCH_SESSIONS", "8")),
                    help="extra leg: batched execution, this many independent sequences per launch chain on ONE GPU (vloam_create_batch); 0 = skip")
    ap.add_argument("--map-capacity-log2", type=int, default=0, help="voxel-hash slots per feature kind = 2^n (0: the library's default, 22); A/B runs of the table footprint")
    ap.add_argument("--sustain-seconds", type=float, default=float(os.environ.get("VLOAM_BENCH_SUSTAIN_S", "6")),
                    help="extra leg: stream the headline workload for about this long (sweeps replayed back and forth; 0 = skip)")
    ap.add_argument("--no-host-input", action="store_true", help="skip the host-input leg (vloam_process_scan from pinned / pageable memory)")
    ap.add_argument("--synth-procs", type=int, default=0, help="worker processes for the synthetic ray casting (0 = min(cores, 16))")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beside the headline: per-kernel replay + roofline, the extra legs, CPU baseline + parity vs the oracle")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="write what the timed path computed in its last step as DIR/<name>.npy")
    args = ap.parse_args()
    if not args.full:   # a plain run: set-up, warm-up, the timed steps, the outputs and the line
        args.no_cpu_baseline = args.no_kernel_timer = args.no_extras = True

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    K, W = args.steps, args.warmup
    with_mapping = args.workload == "map"
    M0 = max(args.map_warmup, 0) if with_mapping else 0
    T = M0 + W + K

    # ---- synthetic input first (forks worker processes: must happen before torch / the HIP runtime are loaded)
    import conftest
    import importlib
    vl = conftest.load_pkg()
    synth = conftest.load_synth()
    multi = importlib.import_module("vloam_amd.multi")
    # N > 1: this rank's enqueue thread and its ray-casting workers stay on the NUMA node of its GPU (an even slice of it per rank)
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    affinity = multi.pin_host_threads(local_rank, local_world)
    cores = os.cpu_count() or 1
    g0 = time.perf_counter()
    # Sequence 0 is this rank's headline sequence; the batched legs drive B DIFFERENT sequences (sessions 1 .. B - 1 get sequences of their
    # own: other scenes, trajectories and noise, multi.rank_sequence_seeds), so that no two sessions share a cache line of input or map
    extras_ok = world == 1 and not args.no_extras
    n_seq = max(args.sessions, 1) if extras_ok else 1
    seqs = [synth.SynthSequence(n_rings=args.rings, n_azimuth=args.azimuth, n_sweeps=T, **multi.rank_sequence_seeds(rank if b == 0 else 1000 + b))
            for b in range(n_seq)]
    n_img = 0 if (not extras_ok or args.rings != 64) else min(max(args.image_frames, 0), T - 1)
    n_img_seq = min(n_seq, 4) if n_img >= 2 else 0
    n_vo = min(max(args.vo_frames, 2), K) if (extras_ok and args.vo_frames > 0) else 0
    jobs = [("sweep", b, k) for b in range(n_seq) for k in range(T)]
    jobs += [("image", b, k) for b in range(n_img_seq) for k in range(T - n_img, T)]
    jobs += [("match", b, k) for b in range(n_seq if n_vo else 0) for k in range(T - n_vo, T)]
    procs = args.synth_procs or max(1, min(affinity["cpus"] if world > 1 else cores, 16 if n_seq == 1 else 48))
    res = synthesise(synth, jobs, seqs, procs)
    hosts = np.stack(res[:n_seq * T]).reshape(n_seq, T, -1, 4)
    off = n_seq * T
    images_all = np.stack(res[off:off + n_img_seq * n_img]).reshape(n_img_seq, n_img, *res[off].shape) if n_img_seq else None
    off += n_img_seq * n_img
    matches_all = {(b, k): res[off + b * n_vo + (k - (T - n_vo))] for b in range(n_seq if n_vo else 0) for k in range(T - n_vo, T)}
    del res
    seq, host = seqs[0], hosts[0]
    images = images_all[0] if images_all is not None else None
    synth_s = time.perf_counter() - g0
    n_pts = host.shape[1]

    # the "N sequences on N cores" CPU leg also forks: run it now, before HIP exists in this process
    cpu_cores_leg = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline and args.cpu_cores_leg > 0 and cores > 1:
        import tempfile
        import orc
        orc.build()  # once, in the parent (the workers only dlopen it)
        nproc = min(cores, 64)
        ns = min(args.cpu_cores_leg, T)
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "sweeps.npy")
            np.save(path, host[:ns])
            c0 = time.perf_counter()
            with mp.get_context("fork").Pool(nproc) as pool:
                per = pool.map(_oracle_worker, [(args.rings, with_mapping, ns, path)] * nproc)
            c1 = time.perf_counter()
        cpu_cores_leg = {"processes": nproc, "value": nproc * ns / (c1 - c0), "unit": "scans/s",
                         "per_process_scans_per_s": ns / (sum(per) / len(per)),
                         "sample": "%d independent oracle sessions (one per host core) x the first %d sweeps, %.1f s wall" % (nproc, ns, c1 - c0)}

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU fallback)")
    local_rank = local_rank % torch.cuda.device_count()  # identity on a full node; lets the gloo path share one GPU in tests
    torch.cuda.set_device(local_rank)
    dist = None
    # VLOAM_BENCH_FORCE_DIST=1: take the N > 1 path with WORLD_SIZE 1 as well (tests/test_gpu_bench_multi.py initialises RCCL — process group,
    # device binding, barrier, the all_gather of the trajectory, the MAX all-reduce — on a single GPU, before the first 8-GPU run does)
    if world > 1 or os.environ.get("VLOAM_BENCH_FORCE_DIST") == "1":
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("VLOAM_BENCH_BACKEND", "nccl")  # "nccl" == RCCL; "gloo" only to exercise this path on a 1-GPU box
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend=backend)
    coll_dev = "cuda" if os.environ.get("VLOAM_BENCH_BACKEND", "nccl") == "nccl" else "cpu"

    # ---- one independent sequence per rank, resident in HBM before the timed region
    d_clouds = torch.from_numpy(hosts).to(torch.device("cuda", local_rank))
    base_ptr, stride = d_clouds.data_ptr(), n_pts * 16
    seq_ptr = [base_ptr + b * T * stride for b in range(n_seq)]   # sequence b's sweeps (b = 0: the headline sequence)

    cap_kw = {"map_capacity_log2": args.map_capacity_log2} if args.map_capacity_log2 > 0 else {}

    def new_handle(mapping=with_mapping, frames=T + 8):
        return vl.Handle(local_rank, scan_line=args.rings, with_mapping=int(mapping), max_points=max(n_pts, 1024), max_frames=frames, **cap_kw)

    def stream(hh, lo, hi):
        for kk in range(lo, hi):
            hh.process_scan_device(base_ptr + kk * stride, n_pts)

    def barrier():
        if dist is not None:
            dist.barrier()

    h = new_handle()
    stream(h, 0, M0 + W)   # map warm-up (configs[2]) + the W warm-up steps, untimed
    h.sync()

    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stream(h, M0 + W, T)
    h.sync()
    torch.cuda.synchronize()
    barrier()
    t1 = time.perf_counter()

    elapsed = t1 - t0
    per_rank_s = [elapsed]
    if dist is not None:
        per_rank_s = multi.gather_seconds(dist, elapsed, device=coll_dev)
        elapsed = multi.max_over_ranks(dist, elapsed, device=coll_dev)
    counts = h.counts()
    traj = h.trajectory()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, timed_outputs(h, traj, M0 + W, with_mapping))
    h.close()

    # ---- per-kernel leg: every kernel's launch duration, HIP events on the kernel's own stream.  A separate replay of the same
    # sweeps on a fresh session, so that the event records (marker packets around every launch) do not sit in the timed region.
    ktable = {}
    if not args.no_kernel_timer:
        hk = new_handle()
        stream(hk, 0, M0 + W)
        hk.sync()
        hk.profile_kernel("*", 48 * K + 64)
        stream(hk, M0 + W, T)
        hk.sync()
        ktable = hk.profile_table()
        hk.close()

    # the one collective of the path: gather the per-sequence trajectories
    trajectories = [traj]
    if dist is not None:
        trajectories = multi.gather_trajectories(dist, traj, T + 8, device=coll_dev)

    extras = world == 1 and not args.no_extras
    # ---- extra leg: configs[1] (no mapping) on the same K sweeps
    configs1 = None
    if extras and with_mapping:
        h1 = new_handle(mapping=False)
        stream(h1, M0, M0 + W)
        h1.sync()
        torch.cuda.synchronize()
        a0 = time.perf_counter()
        stream(h1, M0 + W, T)
        h1.sync()
        torch.cuda.synchronize()
        a1 = time.perf_counter()
        configs1 = {"workload": WORKLOADS["lo"], "value": K / (a1 - a0), "unit": "scans/s", "ms_per_step": 1e3 * (a1 - a0) / K}
        h1.close()

    # ---- extra leg (never the headline): BATCHED execution — B independent sequences advanced by ONE launch chain per sweep (session index
    # in blockIdx.z, vloam_create_batch).  A single sequence is a chain of dependent, mostly latency-bound launches; the batch fills the
    # chip with B of them.  Every session drives a sequence of its OWN (session 0: the headline sequence, whose batched trajectory must
    # equal the single-sequence run to round-off; the last session's trajectory is checked against an oracle pass of its own below).
    batched = None
    batched_traj_last = None
    if extras and args.sessions > 1:
        B = args.sessions
        hb = vl.Handle(local_rank, n_sessions=B, scan_line=args.rings, with_mapping=int(with_mapping), max_points=max(n_pts, 1024), max_frames=T + 8, **cap_kw)

        def bstream(lo, hi):
            for kk in range(lo, hi):
                hb.batch_process_scan_device([seq_ptr[b] + kk * stride for b in range(B)], [n_pts] * B)

        bstream(0, M0 + W)
        hb.sync()
        torch.cuda.synchronize()
        m0 = time.perf_counter()
        bstream(M0 + W, T)
        hb.sync()
        torch.cuda.synchronize()
        m1 = time.perf_counter()
        tjs = [hb.select(b).trajectory() for b in range(B)]
        batched_traj_last = tjs[B - 1]
        distinct = all(not np.array_equal(tjs[0], t) for t in tjs[1:])
        max_diff = float(np.max(np.abs(tjs[0] - traj)))
        hb.close()
        bk = {}
        if not args.no_kernel_timer:   # per-kernel durations of the batched launches (separate replay, like the single-sequence table)
            hb = vl.Handle(local_rank, n_sessions=B, scan_line=args.rings, with_mapping=int(with_mapping), max_points=max(n_pts, 1024), max_frames=T + 8, **cap_kw)
            bstream(0, M0 + W)
            hb.sync()
            hb.profile_kernel("*", 48 * K + 64)
            bstream(M0 + W, T)
            hb.sync()
            bk = hb.profile_table()
            hb.close()
        batched = {"sessions": B, "value": B * K / (m1 - m0), "unit": "scans/s", "ms_per_batch_step": 1e3 * (m1 - m0) / K,
                   "speedup_vs_single_sequence": (B * K / (m1 - m0)) / (K / (t1 - t0)),
                   "distinct_sequences": B, "sessions_differ_from_each_other": bool(distinct),
                   "session0_max_abs_pose_diff_vs_single_sequence_run": max_diff, "finite_poses": bool(all(np.isfinite(t).all() for t in tjs)),
                   "kernel_table": bk,
                   "note": "one vloam_batch_process_scan_device per sweep for all B sessions, every session a different synthetic drive; not the headline value (BASELINE.json's metric is one sequence per GPU)"}

    # ---- extra: latency of ONE sweep (enqueue + drain, nothing in flight).  The headline value streams the sequence: the three
    # stage streams overlap consecutive sweeps, so 1 / value is a throughput period, not a latency.
    latency = None
    if extras:
        hl = new_handle()
        stream(hl, 0, M0 + W)
        hl.sync()
        L = min(32, K)
        l0 = time.perf_counter()
        for k in range(M0 + W, M0 + W + L):
            hl.process_scan_device(base_ptr + k * stride, n_pts)
            hl.sync()
        l1 = time.perf_counter()
        latency = {"ms_per_sweep": 1e3 * (l1 - l0) / L, "sweeps": L,
                   "note": "one sweep at a time (vloam_sync after each): no overlap between consecutive sweeps"}
        hl.close()

    # ---- extra: SUSTAINED streaming of the headline workload for several seconds (a long drive).  The resident sweeps are replayed
    # back and forth (0 .. T-1, T-2 .. 0, 1 .. ): driving the same road in reverse is a continuous trajectory (DISTORTION = 0: a sweep has
    # no direction of travel baked in), the local map stays at its steady-state size, and the GPU stays busy for whole seconds, which a
    # 5-second rocm-smi sample can see.  Also the long-run check of the voxel map's bookkeeping (stamps, deferred list, recentring).
    sustained = None
    if extras and args.sustain_seconds > 0:
        n_s = int(min(max(K / (t1 - t0) * args.sustain_seconds, K), 80000))
        hs = new_handle(frames=M0 + W + n_s + 8)
        stream(hs, 0, M0 + W)
        hs.sync()
        order, pos, step = [], M0 + W - 1, 1
        for _ in range(n_s):
            if pos + step < 0 or pos + step > T - 1:
                step = -step
            pos += step
            order.append(pos)
        torch.cuda.synchronize()
        s0 = time.perf_counter()
        for kk in order:
            hs.process_scan_device(base_ptr + kk * stride, n_pts)
        hs.sync()
        torch.cuda.synchronize()
        s1 = time.perf_counter()
        cs = hs.counts()
        tj = hs.trajectory()
        hs.close()
        sustained = {"value": n_s / (s1 - s0), "unit": "scans/s", "sweeps": n_s, "seconds": s1 - s0,
                     "finite_poses": bool(np.isfinite(tj).all()), "map_points_at_end": cs["M"],
                     "replay": "the %d resident sweeps back and forth, one session, mapping on" % T}

    # ---- extra: HOST input — the path the reference actually has (a host cloud per callback, scan_registration.cpp:131-152,
    # vloam_main_node.cpp:125-180): vloam_process_scan from (i) pinned and (ii) pageable host memory, a distinct buffer per sweep, next to
    # the same sweeps handed over as device pointers.  The library copies a host sweep into a device input buffer on the scan-registration stream.
    host_input = None
    if extras and not args.no_host_input:
        n_h = int(min(max(K, 400), 1200))
        order_h, pos, step = [], M0 + W - 1, 1
        for _ in range(n_h):
            if pos + step < 0 or pos + step > T - 1:
                step = -step
            pos += step
            order_h.append(pos)
        pinned = torch.from_numpy(host).pin_memory()
        runs = {}
        for how in ("device", "pinned", "pageable"):
            hh = new_handle(frames=M0 + W + n_h + 8)
            stream(hh, 0, M0 + W)
            hh.sync()
            torch.cuda.synchronize()
            q0 = time.perf_counter()
            if how == "device":
                for kk in order_h:
                    hh.process_scan_device(base_ptr + kk * stride, n_pts)
            elif how == "pinned":
                for kk in order_h:
                    hh.process_scan_host_ptr(pinned.data_ptr() + kk * stride, n_pts)
            else:
                for kk in order_h:
                    hh.process_scan(host[kk])
            hh.sync()
            torch.cuda.synchronize()
            q1 = time.perf_counter()
            runs[how] = (n_h / (q1 - q0), hh.trajectory()[-1].copy())
            hh.close()
        del pinned
        host_input = {"sweeps": n_h, "unit": "scans/s", "device_resident": runs["device"][0], "pinned": runs["pinned"][0], "pageable": runs["pageable"][0],
                      "pinned_over_device_resident": runs["pinned"][0] / runs["device"][0],
                      "same_last_pose": bool(np.array_equal(runs["device"][1], runs["pinned"][1]) and np.array_equal(runs["device"][1], runs["pageable"][1])),
                      "pageable_over_device_resident": runs["pageable"][0] / runs["device"][0],
                      "note": "vloam_process_scan, one 2 MB sweep per call from a buffer of its own; copied on the handle's copy stream into a ring of device "
                              "input buffers while the previous sweep's scan registration runs, the sweep enqueued by the next call (c_api.h); pinned = "
                              "hipHostMalloc'ed memory read by DMA, pageable = numpy memory (the runtime's staging memcpy runs on the calling thread); "
                              "tools/host_input_probe.py: the same with a few reused buffers, and the inline form (VLOAM_STAGE_INLINE=1)"}

    # ---- extra: configs[3] (synthetic analogue) — the coupled per-frame VLOAM loop, one vloam_process_frame_device per frame:
    # depth-enhanced VO solve -> VO2VeloAndBase -> SR -> LO in combined mode (detach_VO_LO = 0) -> LO -> VO prior -> mapping, no host
    # round trip; pixel matches are synthetic (the image front-end is out of scope) and come from host memory like OpenCV's would
    vo_stage = None
    if extras and args.vo_frames > 0:
        nf = n_vo
        f0 = T - nf
        hv = vl.Handle(local_rank, scan_line=args.rings, with_mapping=int(with_mapping), max_points=max(n_pts, 1024), max_frames=T + 8, detach_VO_LO=0)
        hv.vo_set_calib(*synth.kitti_like_calib())
        hv.set_extrinsics(*synth.kitti_like_extrinsics())
        ms_ = {k: matches_all[(0, k)] for k in range(f0, T)}
        stream(hv, 0, f0 - 1)                       # LiDAR-only up to the map's steady state ...
        hv.process_frame_device(base_ptr + (f0 - 1) * stride, n_pts)   # ... one frame to prime the VO depth map ...
        hv.sync()
        v0 = time.perf_counter()
        for k in range(f0, T):                      # ... then nf coupled frames
            hv.process_frame_device(base_ptr + k * stride, n_pts, ms_[k][0], ms_[k][1])
        hv.sync()
        v1 = time.perf_counter()
        r = hv.vo_result()
        traj_v = hv.trajectory()
        vo_stage = {"workload": "configs[3] analogue: coupled VO + LiDAR frame loop (vloam_process_frame_device, detach_VO_LO=0), synthetic pixel matches",
                    "value": nf / (v1 - v0), "unit": "frames/s", "ms_per_frame": 1e3 * (v1 - v0) / nf, "frames": nf, "matches": int(ms_[f0][0].shape[0]),
                    "counter32_last": r["counter32"], "counter22_last": r["counter22"],
                    "note": "the VO solve of frame k needs the LiDAR odometry of frame k-1 and feeds the one of frame k: VO and LO are one serial chain per frame (mapping still overlaps)"}
        hv.close()
        if args.sessions > 1:   # the same coupled loop for B sessions per launch chain (vloam_batch_process_frame_device), every session its own drive and matches
            Bv = args.sessions
            hvb = vl.Handle(local_rank, n_sessions=Bv, scan_line=args.rings, with_mapping=int(with_mapping), max_points=max(n_pts, 1024), max_frames=T + 8, detach_VO_LO=0)
            hvb.vo_set_calib(*synth.kitti_like_calib())
            hvb.set_extrinsics(*synth.kitti_like_extrinsics())
            for kk in range(0, f0 - 1):
                hvb.batch_process_scan_device([seq_ptr[b] + kk * stride for b in range(Bv)], [n_pts] * Bv)
            hvb.batch_process_frame_device([seq_ptr[b] + (f0 - 1) * stride for b in range(Bv)], [n_pts] * Bv, [(None, None)] * Bv)
            hvb.sync()
            w0 = time.perf_counter()
            for k in range(f0, T):
                hvb.batch_process_frame_device([seq_ptr[b] + k * stride for b in range(Bv)], [n_pts] * Bv, [matches_all[(b, k)] for b in range(Bv)])
            hvb.sync()
            w1 = time.perf_counter()
            tv = [hvb.select(b).trajectory() for b in range(Bv)]
            hvb.close()
            vo_stage["batched"] = {"sessions": Bv, "value": Bv * nf / (w1 - w0), "unit": "frames/s", "ms_per_batch_frame": 1e3 * (w1 - w0) / nf,
                                   "distinct_sequences": Bv, "session0_max_abs_pose_diff_vs_single_session": float(np.max(np.abs(tv[0] - traj_v))),
                                   "finite_poses": bool(all(np.isfinite(t).all() for t in tv))}

    # ---- extra: the same coupled loop from RAW inputs — every frame hands over the sweep and a grey camera image; corners
    # (Shi-Tomasi) and their pyramidal Lucas-Kanade flow are computed on the device and feed the VO solve directly
    # (vloam_process_frame_image_device; the reference's optical_flow_match = true configuration, visual_odometry.cpp:91-132)
    img_stage = None
    if extras and images is not None:
        ni, IH, IW = images.shape
        d_img = torch.from_numpy(images).cuda()
        hi = vl.Handle(local_rank, scan_line=args.rings, with_mapping=int(with_mapping), max_points=max(n_pts, 1024), max_frames=T + 8, detach_VO_LO=0,
                       image_width=IW, image_height=IH)
        hi.vo_set_calib(*synth.kitti_like_calib())
        hi.set_extrinsics(*synth.kitti_like_extrinsics())
        f0 = T - ni
        stream(hi, 0, f0)                           # LiDAR-only up to the map's steady state ...
        hi.process_frame_image_device(base_ptr + f0 * stride, n_pts, d_img.data_ptr(), IW, IH)   # ... the first image only primes corners / pyramid / depth map
        hi.sync()
        i0 = time.perf_counter()
        for j in range(1, ni):
            hi.process_frame_image_device(base_ptr + (f0 + j) * stride, n_pts, d_img.data_ptr() + j * IW * IH, IW, IH)
        hi.sync()
        i1 = time.perf_counter()
        r = hi.vo_result()
        ncorn = int(hi.vo_keypoints().shape[0])
        traj_i = hi.trajectory()
        hi.close()
        img_batched = None
        if args.sessions > 1:   # the same loop for B sessions per launch chain: each session's own sweep and image (the images run through the front-end one after the other on the image stream)
            Bi = n_img_seq
            d_img_all = torch.from_numpy(images_all).cuda()
            ip = [d_img_all.data_ptr() + b * ni * IW * IH for b in range(Bi)]
            hib = vl.Handle(local_rank, n_sessions=Bi, scan_line=args.rings, with_mapping=int(with_mapping), max_points=max(n_pts, 1024), max_frames=T + 8,
                            detach_VO_LO=0, image_width=IW, image_height=IH)
            hib.vo_set_calib(*synth.kitti_like_calib())
            hib.set_extrinsics(*synth.kitti_like_extrinsics())
            for kk in range(0, f0):
                hib.batch_process_scan_device([seq_ptr[b] + kk * stride for b in range(Bi)], [n_pts] * Bi)
            hib.batch_process_frame_image_device([seq_ptr[b] + f0 * stride for b in range(Bi)], [n_pts] * Bi, ip, IW, IH)
            hib.sync()
            b0 = time.perf_counter()
            for j in range(1, ni):
                hib.batch_process_frame_image_device([seq_ptr[b] + (f0 + j) * stride for b in range(Bi)], [n_pts] * Bi, [q + j * IW * IH for q in ip], IW, IH)
            hib.sync()
            b1 = time.perf_counter()
            ti = [hib.select(b).trajectory() for b in range(Bi)]
            hib.close()
            img_batched = {"sessions": Bi, "value": Bi * (ni - 1) / (b1 - b0), "unit": "frames/s", "ms_per_batch_frame": 1e3 * (b1 - b0) / (ni - 1),
                           "distinct_sequences": Bi, "session0_max_abs_pose_diff_vs_single_session": float(np.max(np.abs(ti[0] - traj_i))),
                           "finite_poses": bool(all(np.isfinite(t).all() for t in ti))}
        # the image front-end alone, images resident in HBM, and its per-kernel table
        hf = vl.Handle(local_rank, with_mapping=0, image_width=IW, image_height=IH)
        for j in range(2 * ni):
            hf.vo_process_image_device(d_img.data_ptr() + (j % ni) * IW * IH, IW, IH)
        hf.sync()
        reps = 25 * ni
        a0 = time.perf_counter()
        for j in range(reps):
            hf.vo_process_image_device(d_img.data_ptr() + (j % ni) * IW * IH, IW, IH)
        hf.sync()
        a1 = time.perf_counter()
        hf.profile_kernel("*", 16384)
        for j in range(4 * ni):
            hf.vo_process_image_device(d_img.data_ptr() + (j % ni) * IW * IH, IW, IH)
        itab = hf.profile_table()
        hf.close()
        # the same front-end in the reference's DEFAULT configuration (optical_flow_match = false: ORB descriptors + brute-force Hamming matches),
        # a seeded stand-in for OpenCV's sampling pattern
        ho = vl.Handle(local_rank, with_mapping=0, image_width=IW, image_height=IH)
        ho.vo_set_orb_pattern(synth.orb_test_pattern())
        for j in range(2 * ni):
            ho.vo_process_image_device(d_img.data_ptr() + (j % ni) * IW * IH, IW, IH)
        ho.sync()
        o0 = time.perf_counter()
        for j in range(reps):
            ho.vo_process_image_device(d_img.data_ptr() + (j % ni) * IW * IH, IW, IH)
        ho.sync()
        o1 = time.perf_counter()
        orb_matches = int(ho.vo_flow_matches()[0].shape[0])
        ho.close()
        # CPU restatement beside it (part of the cpu_baseline leg; oracle: cv::goodFeaturesToTrack + cv::calcOpticalFlowPyrLK restated, one thread)
        cpu_img_ms = None
        if not args.no_cpu_baseline:
            import orc as _orc
            c0 = time.perf_counter()
            for j in range(1, min(ni, 4)):
                cc = _orc.good_features(images[j])
                _orc.pyr_lk(images[j - 1], images[j], cc)
            cpu_img_ms = 1e3 * (time.perf_counter() - c0) / max(min(ni, 4) - 1, 1)
        img_stage = {"workload": "configs[3] analogue from raw inputs: vloam_process_frame_image_device (sweep + %d x %d grey image per frame; corners + pyramidal LK flow + "
                                 "depth-enhanced VO + LiDAR odometry + mapping, all on the device)" % (IW, IH),
                     "value": (ni - 1) / (i1 - i0), "unit": "frames/s", "ms_per_frame": 1e3 * (i1 - i0) / (ni - 1), "frames": ni - 1, "corners_last": ncorn,
                     "counter32_last": r["counter32"], "counter22_last": r["counter22"],
                     "image_front_end_alone": {"value": reps / (a1 - a0), "unit": "images/s", "us_per_image": 1e6 * (a1 - a0) / reps,
                                               "kernels_us": {k: round(1e3 * ms / n, 2) for k, (ms, n) in sorted(itab.items(), key=lambda kv: -kv[1][0])},
                                               "algorithmic_bytes_per_image": int(IW * IH * (1 + 1.33 + 4 * 1.33) + 2 * 1024 * 8),
                                               "roofline": {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBS,
                                                            "achieved": IW * IH * (1 + 1.33 + 4 * 1.33) / ((a1 - a0) / reps) / 1e9,
                                                            "frac": IW * IH * (1 + 1.33 + 4 * 1.33) / ((a1 - a0) / reps) / 1e9 / HBM_PEAK_GBS,
                                                            "bytes": "the image once, its 8-bit pyramid (x1.33) and the int16 Scharr pairs of every level (4 B x 1.33) once"},
                                               "cpu_oracle_ms_per_image": cpu_img_ms},
                     "orb_brute_force_front_end_alone": {"value": reps / (o1 - o0), "unit": "images/s", "us_per_image": 1e6 * (o1 - o0) / reps, "matches_last": orb_matches,
                                                         "what": "optical_flow_match = false (vloam_main.launch:10): Shi-Tomasi corners + ORB descriptors + BF Hamming 2-NN with the 0.8 ratio test; sampling pattern = synth.orb_test_pattern() (OpenCV's table is library data the caller hands in)"},
                     "note": "images are synthetic renders of the LiDAR scene (synth.render_image); the coupled legs run the optical-flow configuration"}
        if img_batched:
            img_stage["batched"] = img_batched

    if rank == 0:
        value = multi.aggregate_throughput(K, world, elapsed)
        assert len(trajectories) == world and all(t.shape == (T, 14) for t in trajectories)
        out = {
            "metric": "scans/sec end-to-end odometry on 64x2048 cloud", "value": value, "unit": "scans/s", "n_gpus": world, "steps": K,
            "warmup": W, "ms_per_step": 1e3 * elapsed / K, "per_rank_ms_per_step": [1e3 * s_ / K for s_ in per_rank_s],
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32 points / f64 poses+residuals", "data": "synthetic",
            "config": {"workload": WORKLOADS[args.workload], "points_per_sweep": int(n_pts), "sequences": world,
                       "map_warmup_sweeps": M0, "map_points_at_last_sweep": counts["M"],
                       "sharding": "one independent sequence per GPU, no data-path collective; all_gather of trajectories after the run",
                       "gathered_trajectories": {"ranks": len(trajectories), "frames": [int(t.shape[0]) for t in trajectories],
                                                 "last_map_position": [[float(v) for v in t[-1, 11:14]] for t in trajectories]},
                       "host_affinity_rank0": affinity,
                       "collective": None if dist is None else {"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                                                                "rccl_version": list(torch.cuda.nccl.version()) if dist.get_backend() == "nccl" else None},
                       "pipelining": "SR / LO / mapping of consecutive sweeps overlap on their own HIP streams (one sequence, one GPU)"},
            "counts_last_sweep": counts,
            "host": {"cpu": cpu_model(), "cores": cores, "synth_seconds": round(synth_s, 2), "synth_processes": procs},
        }
        if args.full:   # per-kernel table of the replay and the roofline of the kernel with the largest share of GPU time
            b_sr, b_lo, b_map = sweep_bytes(counts, with_mapping)
            tot_ms = sum(v[0] for v in ktable.values()) or 1.0
            kernels = {}
            for name, (ms, n) in sorted(ktable.items(), key=lambda kv: -kv[1][0]):
                kb = algorithmic_bytes(name, counts)
                avg_us = 1e3 * ms / n
                kernels[name] = {"launches_per_sweep": round(n / K, 2), "avg_us": round(avg_us, 2), "share_of_gpu_time": round(ms / tot_ms, 4),
                                 "algorithmic_bytes": int(kb), "achieved_GBs": round(kb / (avg_us * 1e-6) / 1e9, 2) if avg_us > 0 else 0.0}
            kernel = args.kernel or (next(iter(kernels)) if kernels else ("k_lm_solve" if with_mapping else "k_sr_ring"))
            kb = algorithmic_bytes(kernel, counts)
            k_ms, k_launches = ktable.get(kernel, (0.0, 0))
            avg_ms = k_ms / max(k_launches, 1)
            traffic, traffic_src = pmc_traffic(args.workload, kernel)
            achieved = kb / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
            # the same figures from the committed profiles of the same command, quoted only when they were measured on the kernel sources being timed
            rp_us, rp_src = rocprof_avg_us(args.workload, kernel)
            wait_pct, wait_src = sq_wait_pct(kernel)
            out["roofline"] = {"bound": "hbm", "kernel": kernel, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                               "algorithmic_bytes_per_launch": kb,
                               "algorithmic_bytes_per_unit": ALGORITHMIC_UNIT.get(kernel),
                               "avg_launch_us": 1e3 * avg_ms, "launches_timed": k_launches,
                               "avg_launch_us_source": "HIP events around every launch of the kernel on its own stream, untraced replay of the timed sweeps (the bracket adds a few us to a ~30 us kernel; rocprof_* below is the kernel's own duration)",
                               "rocprof_avg_launch_us": rp_us, "rocprof_source": rp_src,
                               "frac_rocprof": (kb / (rp_us * 1e-6) / 1e9 / HBM_PEAK_GBS) if rp_us else None,
                               # what the counters say the kernel draws from HBM: PMC bytes per launch / its duration / peak
                               "counter_frac": (traffic / ((rp_us or 1e3 * avg_ms) * 1e-6) / 1e9 / HBM_PEAK_GBS) if traffic else None,
                               "sq_wait_pct": wait_pct, "sq_wait_source": wait_src,
                               "timed_region_s": elapsed,
                               "sweep_algorithmic_bytes": {"B_SR": b_sr, "B_LO": b_lo, "B_MAP": b_map},
                               "end_to_end_frac": (b_sr + b_lo + b_map) * value / world / 1e9 / HBM_PEAK_GBS}
            out["kernels"] = kernels
            out["reference_timers"] = {name: round(sum(1e3 * ktable[k][0] for k in ks if k in ktable) / K, 2) for name, ks in REFERENCE_TIMERS.items()
                                       if any(k in ktable for k in ks)}
        if latency:
            out["latency"] = latency
        if sustained:
            out["sustained"] = sustained
        if host_input:
            out["host_input"] = host_input
        if configs1:
            out["configs1"] = configs1
        if vo_stage:
            out["configs3"] = vo_stage
        if img_stage:
            out["configs3_from_images"] = img_stage
        if batched:
            bt = batched.pop("kernel_table")
            if bt:   # roofline of the same kernel when B sessions share its launches: B x the algorithmic bytes per launch
                btot = sum(v[0] for v in bt.values()) or 1.0
                batched["kernels"] = {name: {"avg_us": round(1e3 * ms / n, 2), "share_of_gpu_time": round(ms / btot, 4),
                                             "achieved_GBs": round(batched["sessions"] * algorithmic_bytes(name, counts) / (1e3 * ms / n * 1e-6) / 1e9, 2)}
                                      for name, (ms, n) in sorted(bt.items(), key=lambda kv: -kv[1][0])}
                if kernel in bt:
                    a = batched["sessions"] * kb / (bt[kernel][0] / bt[kernel][1] * 1e-3) / 1e9
                    batched["roofline"] = {"kernel": kernel, "achieved": a, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": a / HBM_PEAK_GBS,
                                           "avg_launch_us": 1e3 * bt[kernel][0] / bt[kernel][1]}
                batched["end_to_end_frac"] = (b_sr + b_lo + b_map) * batched["value"] / 1e9 / HBM_PEAK_GBS
            out["batched"] = batched
        if world == 1 and not args.no_cpu_baseline:
            # ONE pass of the CPU oracle over the very same T sweeps (it has to start at sweep 0: the map is part of the state):
            # cpu_baseline = its rate over the sweeps the GPU's warm-up + timed region covered (same map state), and the per-frame
            # poses of the whole pass are the parity reference for EVERY frame up to the last timed sweep.
            import orc
            o = orc.Oracle(scan_line=args.rings, with_mapping=with_mapping)
            dt_max = dq_max = 0.0
            worst = 0
            stamps = [time.perf_counter()]
            st_ms = np.zeros(3)
            for k in range(T):
                o.process(host[k])
                stamps.append(time.perf_counter())
                if k >= M0:
                    st_ms += o.stage_ms()
                qw, tw, _, _ = o.lo_pose()
                qm, tm = o.map_published_pose() if with_mapping else (qw, tw)
                dt, dq = pose_err(traj[k], qw, tw, qm, tm, with_mapping)
                if dt > dt_max:
                    worst = k
                dt_max, dq_max = max(dt_max, dt), max(dq_max, dq)
            # (the pose read-outs above sit between two stamps; they are microseconds against ~50 ms per sweep)
            steady = stamps[T] - stamps[M0]
            out["cpu_baseline"] = {"value": (T - M0) / steady, "unit": "scans/s", "cores": 1, "kind": "port", "cpu": cpu_model(),
                                   "whole_pass_scans_per_s": T / (stamps[T] - stamps[0]),
                                   "stage_ms_per_sweep": {"scanRegistration": st_ms[0] / (T - M0), "laserOdometry": st_ms[1] / (T - M0), "laserMapping": st_ms[2] / (T - M0)},
                                   "sample": "sweeps %d..%d (%.1f s) of one %d-sweep pass (%.1f s) of the CPU oracle over the same synthetic sequence "
                                             "(restated reference path — NOT the original Ceres/PCL binary, which cannot be built here; single thread like the reference)"
                                             % (M0, T - 1, steady, T, stamps[T] - stamps[0])}
            if cpu_cores_leg:
                out["cpu_baseline"]["n_sequences_on_n_cores"] = cpu_cores_leg
            if batched is not None and batched_traj_last is not None:
                # the LAST session of the batch (a different drive than the headline sequence) against an oracle pass of its own
                ob = orc.Oracle(scan_line=args.rings, with_mapping=with_mapping)
                bdt = bdq = 0.0
                for k in range(T):
                    ob.process(hosts[batched["sessions"] - 1][k])
                    qw, tw, _, _ = ob.lo_pose()
                    qm, tm = ob.map_published_pose() if with_mapping else (qw, tw)
                    dt, dq = pose_err(batched_traj_last[k], qw, tw, qm, tm, with_mapping)
                    bdt, bdq = max(bdt, dt), max(bdq, dq)
                batched["parity_vs_oracle"] = {"session": batched["sessions"] - 1, "frames": T, "max_abs_dt_m": bdt, "max_abs_dq": bdq, "bar": 1e-4,
                                               "session0": "equals the headline single-sequence run (checked against the oracle below) to session0_max_abs_pose_diff_vs_single_sequence_run"}
            out["parity_vs_oracle"] = {"frames": T, "last_frame_checked": T - 1, "covers_timed_region": True, "max_abs_dt_m": dt_max,
                                       "max_abs_dq": dq_max, "worst_frame": worst, "bar": 1e-4,
                                       "poses": "laser-odometry world pose + mapping pose of every frame, HIP trajectory of the timed session vs the oracle"}
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
