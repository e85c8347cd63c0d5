#!/usr/bin/env python3
"""Run the LiDAR odometry + mapping hot path over a directory of KITTI raw sweeps (or a synthetic sequence) and write
LO0.txt / MO0.txt in the reference's results format — the part of vloam_main_node's callback
(src/vloam_main/src/vloam_main_node.cpp:134-176, 215-222) that sits either side of the HIP path, without ROS.

  python tools/run_sequence.py --velodyne /data/2011_09_26_drive_0001_sync/velodyne_points/data --out results/
  python tools/run_sequence.py --synthetic 50 --out /tmp/res        # needs an MI355X either way
  python tools/run_sequence.py --synthetic 50 --vloam --metrics /tmp/res/frames.jsonl --out /tmp/res
      --vloam:   the coupled per-frame loop (vloam_process_frame: VO solve -> LO prior -> SR -> LO -> VO prior -> mapping, combined mode)
                 on synthetic pixel matches, also writes VO0.txt
      --images:  with --vloam: the matches come from grey camera images instead (vloam_process_frame_image: Shi-Tomasi corners +
                 pyramidal Lucas-Kanade on the device, the reference's optical_flow_match = true); the synthetic sequence's images are
                 rendered from the same scene (synth.render_image).  Real data: --velodyne DIR --image-dir .../image_00/data
                 --calib-cam-to-cam calib_cam_to_cam.txt --calib-velo-to-cam calib_velo_to_cam.txt (KITTI raw layout, 8-bit grey PNGs)
  python tools/run_sequence.py --vloam --images --velodyne DRIVE/velodyne_points/data --image-dir DRIVE/image_00/data \
      --calib-cam-to-cam CALIB/calib_cam_to_cam.txt --calib-velo-to-cam CALIB/calib_velo_to_cam.txt --out results/
      --metrics: one JSON object per frame — the reference prints these through ROS_INFO / TicToc: feature counts
                 (scan_registration.cpp), correspondences and solver iterations (laser_odometry.cpp:453-465, laser_mapping.cpp:606-618),
                 per-stage milliseconds
"""
import argparse
import glob
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_pkg():
    path = os.path.join(ROOT, "vloam-cmu-16833_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location("vloam_amd", path, submodule_search_locations=[os.path.dirname(path)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["vloam_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def unwrap_boundary_points(cloud, band=4e-6):
    """Points whose azimuth lies within `band` rad (about 2 float ulp at pi) of one of scanRegistration's unwrap thresholds
    (scan_registration.cpp:236-262).  The azimuth is an f32 atan2 whose last bit differs between math libraries (the device's, glibc's),
    so these are the points whose relTime could land one revolution apart between this library and a CPU run of the reference: the count
    bounds the per-frame 'threshold flips'.  Computed from the input cloud with numpy; no device state involved."""
    xyz = np.asarray(cloud, np.float32)[:, :3]
    ok = np.isfinite(xyz).all(axis=1) & ((xyz.astype(np.float64) ** 2).sum(axis=1) >= 0.1 ** 2)
    if not ok.any():
        return 0
    x, y = xyz[ok, 0], xyz[ok, 1]
    ori = -np.arctan2(y, x).astype(np.float64)
    start = float(ori[0])
    end = float(ori[-1]) + 2 * np.pi
    if end - start > 3 * np.pi:
        end -= 2 * np.pi
    elif end - start < np.pi:
        end += 2 * np.pi
    two_pi = 2 * np.pi
    thresholds = (start - np.pi / 2, start + 1.5 * np.pi, start + np.pi, start - np.pi, end - 1.5 * np.pi - two_pi, end + np.pi / 2 - two_pi,
                  end - 1.5 * np.pi, end + np.pi / 2)
    near = np.zeros(ori.shape, bool)
    for t in thresholds:
        d = np.abs(((ori - t) + np.pi) % two_pi - np.pi)
        near |= d < band
    return int(near.sum())


def write_sweep_log(vl, hd, path):
    """One JSON line per sweep from vloam_get_sweep_log: every field of vloam_sweep_record, error_bits and flags also by name."""
    bits = [(n[len("SWEEP_"):].lower(), getattr(vl, n)) for n in ("SWEEP_EMPTY", "SWEEP_RING_TOO_LONG", "SWEEP_MAP_FULL", "SWEEP_MAP_RAW_CAPACITY",
                                                                    "SWEEP_STACK_FULL", "SWEEP_DS_TIMEOUT", "SWEEP_VO_DEGENERATE")]
    flags = [(n[len("SWEEP_FLAG_"):].lower(), getattr(vl, n)) for n in ("SWEEP_FLAG_FIRST", "SWEEP_FLAG_MAP_SKIPPED", "SWEEP_FLAG_MAP_NOT_OPTIMIZED",
                                                                        "SWEEP_FLAG_LO_LESS_CORR_0", "SWEEP_FLAG_LO_LESS_CORR_1", "SWEEP_FLAG_SOLVE_DEGRADED")]
    rows = hd.sweep_log()
    with open(path, "w") as f:
        for r in rows:
            rec = {name: (r[name].tolist() if r[name].ndim else r[name].item()) for name in rows.dtype.names if name != "reserved"}
            rec["errors"] = [n for n, b in bits if rec["error_bits"] & b]
            rec["flag_names"] = [n for n, b in flags if rec["flags"] & b]
            f.write(json.dumps(rec) + "\n")
    print("wrote %d sweep records to %s" % (rows.shape[0], path))


def read_start_pose(a):
    """--load-map DIR: (q xyzw, t) the sequence starts with in the map — --start-pose, else DIR/start_pose.txt (the saving run's last mapped
    pose: going on where it stopped), else the map's origin."""
    path = os.path.join(a.load_map, "start_pose.txt")
    if a.start_pose:
        v = [float(x) for x in a.start_pose.split()]
    elif os.path.exists(path):
        v = [float(x) for x in open(path).read().split()]
    else:
        v = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    if len(v) != 7:
        sys.exit("a start pose is seven numbers: qx qy qz qw tx ty tz")
    q = np.array(v[:4])
    return q / np.linalg.norm(q), np.array(v[4:])


def parse_relocalize(arg):
    """--relocalize "EXT_XY STEP_XY YAW_DEG STEP_DEG [TOP_K]" -> keyword arguments of Handle.map_relocalize: a grid of +-EXT_XY metres in x and y
    in steps of STEP_XY, +-YAW_DEG degrees of yaw in steps of STEP_DEG, the TOP_K (default 4) best candidates refined."""
    v = arg.split()
    if len(v) not in (4, 5):
        sys.exit("--relocalize takes \"EXT_XY STEP_XY YAW_DEG STEP_DEG [TOP_K]\"")
    ext, step, yaw, dstep = (float(x) for x in v[:4])
    if ext < 0 or yaw < 0 or yaw > 180 or (ext > 0 and step <= 0) or (yaw > 0 and dstep <= 0):
        sys.exit("--relocalize: extents are >= 0 (yaw at most 180 degrees), steps > 0")
    n_xy = int(round(2.0 * ext / step)) + 1 if ext > 0 else 1
    n_yaw = int(round(2.0 * yaw / dstep)) + 1 if yaw > 0 else 1
    return dict(n_xy=(n_xy, n_xy), n_z=1, n_yaw=n_yaw, half_extent=(ext, ext, 0.0), half_yaw=float(np.deg2rad(yaw)), top_k=int(v[4]) if len(v) == 5 else 4)


def place_centre(vl, hd, a, cloud):
    """--relocalize-global: DIR/place_db.npz loaded into the handle's place database, `cloud` matched against every row at every yaw shift; the
    centre is the best row's saved pose with its heading turned by the match's shift (c_api.h: q_query = q_row * Rz(-shift * 2 pi / S))."""
    path = os.path.join(a.load_map, "place_db.npz")
    if not os.path.exists(path):
        sys.exit("--relocalize-global needs %s: save the map with --place-db --save-map DIR" % path)
    db = np.load(path)
    geom = {k: db[k].item() for k in ("n_ring", "n_sector", "min_range", "max_range", "z_min", "z_step")}
    hd.place_enable(capacity=max(int(db["desc"].shape[0]), 1), **geom)
    hd.place_load(db["desc"], db["tags"])
    m = hd.place_query(cloud, k=1)[0]
    if m["row"] < 0:
        sys.exit("--relocalize-global: %s holds no rows" % path)
    print("place match: row %d, tag %d, shift %d, dist %d" % (m["row"], m["tag"], m["shift"], m["dist"]))
    pose = db["poses"][int(m["row"])]
    q = vl.place_yaw_pose(pose[:4], int(m["shift"]), int(geom["n_sector"]))
    return q / np.linalg.norm(q), pose[4:7].copy()


def score_json(s):
    return {"n_hit": s["n_hit"].tolist(), "n_used": s["n_used"].tolist(), "sum_d2_q24": [int(x) for x in s["sum_d2_q24"]]}


def localize_only(vl, kio, tf, hd, a, load_sweep, n, first, origin, what):
    """--resume CKPT / --load-map DIR with --localize-only: every sweep of the input against the map, each from the previous result; the first
    one from `first` (the restored sequence's last map pose / the start pose) — or, with --relocalize, relocalised on a grid of candidates
    around it (vloam_map_relocalize).  The feature clouds come from a second handle without mapping (scan registration only); the map is
    never updated.  --metrics: one JSON line per sweep (flags, factors, the localised pose); the first line of a relocalised run also carries
    the winning candidate, its coarse and fine scores and the refined pose."""
    sr = vl.Handle(a.device, with_mapping=0, **({"max_ring_points": a.max_ring_points} if a.max_ring_points else {}))
    q, t = first[0].copy(), first[1].copy()
    tf.MO2Cam0StartFrame(origin[0], origin[1], 0)   # rows are expressed in the start frame of the MAP's sequence, like MO0.txt of the saving run
    rows, solved = [], 0
    mf = open(a.metrics, "w") if a.metrics else None
    for count in range(n):
        sr.reset_frame()
        sr.scan_registration(load_sweep(count))
        corner, surf = sr.features(2), sr.features(4)
        reloc = None
        if count == 0 and a.relocalize:
            grid = parse_relocalize(a.relocalize)
            rr = hd.map_relocalize(corner, surf, q / np.linalg.norm(q), t, **grid)
            b = rr["best"]
            r = rr["refined"][b]
            reloc = {"n_candidates": rr["n_candidates"], "n_refined": rr["n_refined"], "best": b, "candidate": int(rr["candidate"][b]),
                     "candidates": rr["candidate"].tolist(), "guess": [float(x) for x in list(r["q_guess"]) + list(r["t_guess"])],
                     "coarse": score_json(rr["coarse"][b]), "fine": score_json(rr["fine"][b]),
                     "refined_pose": [float(x) for x in list(r["q_map"]) + list(r["t_map"])]}
            print("relocalised sweep 0: candidate %d of %d, start pose \"%s\"" % (reloc["candidate"], reloc["n_candidates"], " ".join("%.17g" % x for x in reloc["refined_pose"])))
        else:
            r = hd.map_localize(corner, surf, q / np.linalg.norm(q), t, pose_frame=1)
        if r["error_bits"]:
            print("sweep %d: error bits %d" % (count, r["error_bits"]), file=sys.stderr)
        solved += 1 if r["flags"] & vl.LOC_SOLVED else 0
        q, t = r["q_map"], r["t_map"]
        rows.append(tf.MO2Cam0StartFrame(q, t, count + 1))
        if mf:
            rec = {"frame": count, "flags": int(r["flags"]), "error_bits": int(r["error_bits"]), "n_factors": np.asarray(r["n_factors"]).tolist(),
                   "loc_pose": [float(x) for x in list(q) + list(t)]}
            if reloc:
                rec["relocalize"] = reloc
            mf.write(json.dumps(rec) + "\n")
    if mf:
        mf.close()
    sr.close()
    os.makedirs(a.out, exist_ok=True)
    kio.write_trajectory(os.path.join(a.out, "LOC0.txt"), rows)
    print("localised %d sweeps against %s (%d solved), wrote %s/LOC0.txt" % (n, what, solved, a.out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--velodyne", help="directory of KITTI raw velodyne .bin sweeps")
    ap.add_argument("--synthetic", type=int, default=0, help="number of synthetic 64 x --azimuth sweeps instead")
    ap.add_argument("--azimuth", type=int, default=None, help="columns of a synthetic sweep (default: 2048, hdl64e: 2083)")
    ap.add_argument("--sensor", choices=("default", "hdl64e"), default="default",
                    help="synthetic sensor model (hdl64e: two lasers share a scan line now and then: lines of more than 4096 points)")
    ap.add_argument("--max-ring-points", type=int, default=0, help="vloam_config::max_ring_points (0: the default, 4096; up to 16384)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--mapping-skip-frame", type=int, default=2)
    ap.add_argument("--vloam", action="store_true", help="coupled VO + LiDAR frames (synthetic sequences only: synthetic pixel matches)")
    ap.add_argument("--images", action="store_true", help="with --vloam: take the pixel matches from grey images (device image front-end)")
    ap.add_argument("--clahe", action="store_true", help="with --images: cv::createCLAHE(2.0) on every image first (the launch file's CLAHE parameter)")
    ap.add_argument("--image-dir", help="directory of 8-bit grey PNGs, one per sweep (KITTI raw image_00/data)")
    ap.add_argument("--calib-cam-to-cam", help="KITTI calib_cam_to_cam.txt (R_rect_00, P_rect_00)")
    ap.add_argument("--calib-velo-to-cam", help="KITTI calib_velo_to_cam.txt (R, T)")
    ap.add_argument("--metrics", help="write per-frame metrics as JSON lines to this file")
    ap.add_argument("--map-pub-number", type=int, default=0,
                    help="publish /laser_cloud_map from the mapping stream every N frames (vloam_limits::map_pub_number; the KITTI launch file: 20) "
                         "and write each publication as OUT/map_<frame>.npy (float32 [n, 4]); read through vloam_get_published_map, which waits "
                         "for the publication only, never for the pipeline")
    ap.add_argument("--sweep-log", help="write the per-sweep diagnostics log (vloam_limits_ext::sweep_log) as JSON lines to this file: one line per sweep, read "
                                        "once after the run from the rows the stage streams wrote, with no per-frame synchronisation")
    ap.add_argument("--pose-info", action="store_true",
                    help="enable the per-sweep pose information matrices (vloam_pose_info_enable, thresholds --lo-min-eig / --map-min-eig) and add "
                         "lo_min_eig, map_min_eig, lo_degenerate, map_degenerate to the per-frame metrics (null where that stage did not solve)")
    ap.add_argument("--lo-min-eig", type=float, default=0.0, help="with --pose-info: odometry degeneracy threshold on the smallest eigenvalue (0: never)")
    ap.add_argument("--map-min-eig", type=float, default=0.0, help="with --pose-info: the same for the mapping")
    ap.add_argument("--pose-cov", action="store_true",
                    help="enable the per-sweep pose covariance rows (vloam_pose_cov_enable; implies --pose-info) and add, for lo, map and vo, *_rank, "
                         "*_sigma_t and *_sigma_r to the per-frame metrics: the eigenvalues kept by the pseudo-inverse and the square root of the largest "
                         "eigenvalue of the translation / rotation block of the covariance (null where that stage has no covariance)")
    ap.add_argument("--save-checkpoint", metavar="PATH", help="write the sequence's checkpoint (vloam_checkpoint_save) to this file: after the last sweep, or with --at "
                                                              "FRAME once FRAME sweeps are done (a run resumed from it starts at sweep FRAME); the run itself goes on unchanged")
    ap.add_argument("--at", type=int, default=None, metavar="FRAME", help="with --save-checkpoint: sweeps done when the checkpoint is taken")
    ap.add_argument("--resume", metavar="PATH", help="load this checkpoint (vloam_checkpoint_load) into the fresh handle and go on with the sweep behind the saved ones: "
                                                     "the same input and the same algorithmic options as the saving run; outputs start at the restored sweep")
    ap.add_argument("--localize-only", action="store_true",
                    help="with --resume: localise EVERY sweep of the input against the restored map (vloam_map_localize, each from the previous result, "
                         "pose_frame = 1) and write LOC0.txt in the results-row format; the map is never updated, no sweep is added to the sequence")
    ap.add_argument("--save-map", metavar="DIR", help="after the last sweep write the map as DIR/corner.npy and DIR/surf.npy (vloam_get_map_kind: float32 [n, 4], map frame) "
                                                      "and the last mapped pose as DIR/start_pose.txt (qx qy qz qw tx ty tz): what --load-map takes, with any build of the library")
    ap.add_argument("--carve", metavar="\"N_LAST_SWEEPS [MIN_VOTES]\"",
                    help="after the last sweep, before --save-map: remove the map voxels that the run's last N_LAST_SWEEPS sweeps (at most 16) see through "
                         "under their mapping poses and none of them confirms (vloam_map_carve, apply; MIN_VOTES sweeps must see through, default 1) — "
                         "what a parked car or a pedestrian left in the map; the removed points are written as OUT/carved.npy")
    ap.add_argument("--merge-map", metavar="DIR", help="after the last sweep (or right after --load-map / --resume when the input has no further sweep), before --carve and "
                                                       "--save-map: fold DIR/corner.npy and DIR/surf.npy, a --save-map directory of ANOTHER run, into the live map "
                                                       "(vloam_map_merge); the result record is printed and appended to --metrics as one more JSON line {\"map_merge\": ...}")
    ap.add_argument("--merge-pose", metavar="\"qx qy qz qw tx ty tz\"", help="with --merge-map: this run's map <- the merged map's frame (default: the identity); "
                                                                             "--localize-only --relocalize of a sweep of this run against DIR finds it")
    ap.add_argument("--merge-dry-run", action="store_true", help="with --merge-map: look up only (apply = 0): the overlap is reported, the map stays as it is")
    ap.add_argument("--load-map", metavar="DIR", help="import DIR/corner.npy and DIR/surf.npy as the map of the fresh handle before the first sweep (vloam_map_import); "
                                                      "with --localize-only as --resume: every sweep is localised against the imported map, which is never updated")
    ap.add_argument("--start-pose", metavar="\"qx qy qz qw tx ty tz\"", help="with --load-map: the map<-odometry transform the sequence starts with "
                                                                           "(default: DIR/start_pose.txt if there is one, else the map's origin)")
    ap.add_argument("--relocalize", metavar="\"EXT_XY STEP_XY YAW_DEG STEP_DEG [TOP_K]\"",
                    help="with --load-map / --resume and --localize-only: the first sweep is relocalised around the start pose instead of localised from it "
                         "(vloam_map_relocalize: candidates every STEP_XY metres within +-EXT_XY in x and y and every STEP_DEG degrees within +-YAW_DEG of yaw, "
                         "the TOP_K best — default 4 — refined); the first --metrics line carries the winning candidate, its scores and the refined pose")
    ap.add_argument("--place-db", action="store_true",
                    help="keep a place database (vloam_place_enable, default geometry): every sweep's raw cloud is added, tagged with its frame index; with "
                         "--save-map DIR it is written as DIR/place_db.npz (desc, tags, the geometry, and per row the mapping pose of that frame, poses [n, 7])")
    ap.add_argument("--archive-rolled", type=int, nargs="?", const=0, default=None, metavar="CAPACITY_ROWS",
                    help="keep the map points of cubes that roll out of the 21 x 21 x 11 window (vloam_map_archive_enable; CAPACITY_ROWS rows of 32 bytes, "
                         "default 2^20) and print rows held / dropped at the end; with --save-map DIR corner.npy and surf.npy hold the archive's rows of "
                         "that kind first (in vloam_map_archive_get's order), then the window's export: the map of the whole drive in the same format.  A "
                         "voxel that was evicted, re-entered the window empty and was filled again appears twice; --load-map (vloam_map_import) merges "
                         "the points of one voxel into their centroid in input order")
    ap.add_argument("--relocalize-global", metavar="\"EXT_XY STEP_XY YAW_DEG STEP_DEG [TOP_K]\"",
                    help="with --load-map DIR --localize-only: no start pose is needed — the first sweep is matched against DIR/place_db.npz "
                         "(vloam_place_query), the best row's pose turned by the match's yaw shift becomes the start pose, and the sweep is relocalised "
                         "around it exactly as --relocalize does; one more line of output names the row, its tag, the shift and the distance")
    ap.add_argument("--first-sweep", type=int, default=0, metavar="K", help="the input starts at its sweep K (the sweeps in front of it are left out)")
    ap.add_argument("--imu-T-velo", help="16 numbers, row major (default: KITTI 2011_09_26 extrinsics, approx.)")
    ap.add_argument("--imu-T-cam0", help="16 numbers, row major")
    a = ap.parse_args()
    a.pose_info = a.pose_info or a.pose_cov
    vl = load_pkg()
    import importlib
    kio = importlib.import_module("vloam_amd.kitti_io")

    if a.velodyne:
        files = sorted(glob.glob(os.path.join(a.velodyne, "*.bin")))
        load_sweep = lambda k: kio.load_kitti_bin(files[k])
        n = len(files)
    else:
        synth = importlib.import_module("vloam_amd.synth")
        seq = synth.SynthSequence(n_rings=64, n_azimuth=a.azimuth, n_sweeps=max(a.synthetic, 2) + 1, sensor=a.sensor)
        load_sweep = seq.sweep
        n = a.synthetic
    if a.first_sweep:
        if not 0 <= a.first_sweep < n:
            sys.exit("--first-sweep K: 0 <= K < %d" % n)
        load_all, load_sweep, n = load_sweep, (lambda k: load_all(k + a.first_sweep)), n - a.first_sweep
    if n == 0:
        sys.exit("no sweeps")

    def mat(arg, default):
        return np.array([float(v) for v in arg.split()]).reshape(4, 4) if arg else default
    # static extrinsics of the KITTI raw rig (imu -> velodyne, imu -> cam0); identity base_T_imu
    imu_T_velo = mat(a.imu_T_velo, kio.make_T([0, 0, 0.0074, 0.99997], [0.81, -0.32, 0.80]))
    imu_T_cam0 = mat(a.imu_T_cam0, kio.make_T([0.5, -0.5, 0.5, -0.5], [1.08, -0.32, 0.72]))
    tf = kio.VloamTF(imu_T_velo, imu_T_cam0)

    real_images = None
    if a.vloam and a.velodyne:
        if not (a.images and a.image_dir and a.calib_cam_to_cam and a.calib_velo_to_cam):
            sys.exit("--vloam on recorded sweeps needs --images --image-dir DIR --calib-cam-to-cam FILE --calib-velo-to-cam FILE "
                     "(the pixel matches come from the images; ORB matching is not provided)")
        real_images = sorted(glob.glob(os.path.join(a.image_dir, "*.png")))
        if len(real_images) < n:
            sys.exit("%d sweeps but only %d images in %s" % (n, len(real_images), a.image_dir))
    if a.localize_only and not (a.resume or a.load_map):
        sys.exit("--localize-only needs a map: add --resume CKPT or --load-map DIR")
    if a.relocalize and not a.localize_only:
        sys.exit("--relocalize goes with --localize-only: an import fixes the start transform before any sweep arrives, so a SEQUENCE cannot start from a "
                 "relocalised pose in one run; relocalise with --localize-only, then start the sequence with --load-map DIR --start-pose and the pose it printed")
    if a.relocalize_global:
        if not (a.load_map and a.localize_only) or a.relocalize or a.start_pose:
            sys.exit("--relocalize-global goes with --load-map DIR --localize-only, and replaces --start-pose and --relocalize")
        a.relocalize = a.relocalize_global   # from the matched centre on it is --relocalize
    if a.relocalize:
        parse_relocalize(a.relocalize)
    if a.carve:
        w = a.carve.split()
        if len(w) not in (1, 2) or not all(v.isdigit() for v in w) or not 1 <= int(w[0]) <= 16 or not 1 <= int(w[-1]) <= 16:
            sys.exit("--carve \"N_LAST_SWEEPS [MIN_VOTES]\": 1 .. 16 sweeps, 1 .. 16 votes")
        if a.localize_only or a.vloam:
            sys.exit("--carve cleans the map of a LiDAR run that maps: not with --localize-only or --vloam")
        a.carve = (int(w[0]), int(w[1]) if len(w) == 2 else 1)
    if (a.merge_pose or a.merge_dry_run) and not a.merge_map:
        sys.exit("--merge-pose / --merge-dry-run belong to --merge-map")
    if a.merge_map and (a.localize_only or a.vloam):
        sys.exit("--merge-map folds a map into the map of a LiDAR run that maps: not with --localize-only or --vloam")
    if a.merge_pose:
        w = a.merge_pose.split()
        if len(w) != 7:
            sys.exit("--merge-pose \"qx qy qz qw tx ty tz\": seven numbers")
        a.merge_pose = [float(v) for v in w]
    if a.archive_rolled is not None and a.localize_only:
        sys.exit("--archive-rolled keeps what a run that MAPS rolls out of the window: not with --localize-only")
    if a.resume and a.load_map:
        sys.exit("--resume and --load-map both fill a fresh handle: choose one")
    if a.start_pose and not a.load_map:
        sys.exit("--start-pose belongs to --load-map")
    if a.vloam and (a.save_checkpoint or a.resume or a.load_map):
        sys.exit("--save-checkpoint / --resume / --load-map are for sequences driven by sweeps only: the VO's previous-frame state is not saved")
    if a.at is not None and not (a.save_checkpoint and 0 < a.at <= n):
        sys.exit("--at FRAME belongs to --save-checkpoint, 1 <= FRAME <= %d" % n)
    if a.images and not a.vloam:
        sys.exit("--images belongs to the coupled loop: add --vloam")
    img_cfg = {}
    if a.images:
        ih, iw = (kio.load_png_gray(real_images[0]).shape if real_images else (375, 1242))
        img_cfg = dict(image_width=int(iw), image_height=int(ih), CLAHE=int(a.clahe))
    loam = vl.LidarOdometryMapping(device=a.device, mapping_skip_frame=a.mapping_skip_frame, detach_VO_LO=0 if a.vloam else 1,
                                   timing=1 if (a.metrics and not a.vloam) else 0, **img_cfg,
                                   **({"max_ring_points": a.max_ring_points} if a.max_ring_points else {}),
                                   **({"map_pub_number": a.map_pub_number} if a.map_pub_number else {}),
                                   **({"sweep_log": 1} if a.sweep_log else {}))
    hd = loam.hd
    if a.pose_info:
        hd.enable_pose_info(a.lo_min_eig, a.map_min_eig)
    if a.pose_cov:
        hd.pose_cov_enable()
    if a.place_db:
        hd.place_enable(capacity=max(n, 1))
    if a.archive_rolled is not None:
        hd.map_archive_enable(capacity_rows=a.archive_rolled or None)
    if a.vloam:
        if real_images:   # PointCloudUtil::loadTransformations (point_cloud_util.cpp:5-116)
            hd.vo_set_calib(*kio.load_transformations(a.calib_cam_to_cam, a.calib_velo_to_cam))
        else:
            hd.vo_set_calib(*synth.kitti_like_calib())
        hd.set_extrinsics(tf.base_T_cam0, tf.velo_T_cam0)
    os.makedirs(a.out, exist_ok=True)
    lo_rows, mo_rows, vo_rows = [], [], []
    mf = open(a.metrics, "w") if a.metrics else None
    ms_prev = np.zeros(4)
    last_pub, n_pub = -1, 0
    start = 0
    if a.resume:
        with open(a.resume, "rb") as f:
            hd.restore(f.read())
        start = hd.frame_count()
        if a.localize_only:
            last, row0 = hd.trajectory(start - 1, 1)[0], hd.trajectory(0, 1)[0]
            localize_only(vl, kio, tf, hd, a, load_sweep, n, (last[7:11], last[11:14]), (row0[7:11], row0[11:14]), "the map of %d restored sweeps" % start)
            return
        if not 0 < start < n:
            sys.exit("the checkpoint holds %d sweeps, the input %d: nothing to resume" % (start, n))
        row0 = hd.trajectory(0, 1)[0]   # the start frame of the written trajectories is the sequence's first sweep
        tf.LO2Cam0StartFrame(row0[0:4], row0[4:7], 0)
        tf.MO2Cam0StartFrame(row0[7:11], row0[11:14], 0)
    if a.load_map:
        q0, t0 = place_centre(vl, hd, a, load_sweep(0)) if a.relocalize_global else read_start_pose(a)
        res = hd.map_import(np.load(os.path.join(a.load_map, "corner.npy")), np.load(os.path.join(a.load_map, "surf.npy")), q0, t0)
        print("imported %d corner / %d surf map points from %s (%d / %d outside the window)" % (res["n_voxels"][0], res["n_voxels"][1], a.load_map,
                                                                                              res["n_outside_window"][0], res["n_outside_window"][1]))
        if a.localize_only:
            localize_only(vl, kio, tf, hd, a, load_sweep, n, (q0, t0), (q0, t0), "the imported map")
            return
    save_at = (a.at if a.at is not None else n) if a.save_checkpoint else -1
    for count in range(start, n):
        cloud = load_sweep(count)
        if a.vloam:
            if a.images:
                hd.process_frame_image(cloud, kio.load_png_gray(real_images[count]) if real_images else synth.render_image(seq, count))
            else:
                m = synth.synth_matches(seq, count) if count > 0 else (None, None)
                hd.process_frame(cloud, m[0], m[1])
            row = hd.trajectory(count, 1)[0]
            q_lo, t_lo, q_mo, t_mo = row[0:4], row[4:7], row[7:11], row[11:14]
            v = hd.vo_trajectory(count, 1)[0]
            tf.world_VOT_base_last = kio.make_T(v[0:4], v[4:7])
            vo_rows.append(tf.VO2Cam0StartFrame(count))
        else:
            loam.reset()
            loam.scanRegistrationIO(cloud)
            loam.laserOdometryIO()
            loam.laserMappingIO()
            lo, lm = loam.laser_odometry, loam.laser_mapping
            tf.LO2CamPrior(lo.q_last_curr, lo.t_last_curr)
            q_lo, t_lo, q_mo, t_mo = lo.q_w_curr, lo.t_w_curr, lm.q_w_curr, lm.t_w_curr
        if a.place_db:
            hd.place_add(cloud, count + a.first_sweep)
        lo_rows.append(tf.LO2Cam0StartFrame(q_lo, t_lo, count))
        mo_rows.append(tf.MO2Cam0StartFrame(q_mo, t_mo, count))
        pub_points, pub_overflow = None, False
        if a.map_pub_number:
            try:
                _, _, pub_frame = hd.published_device_ptr(0)   # which sweep published last: no cloud crosses the link for an old publication
                if pub_frame != last_pub:   # a new publication (a sweep skipped by mapping_skip_frame leaves the last one current)
                    cloud_map, pub_frame = hd.published_map()
                    np.save(os.path.join(a.out, "map_%06d.npy" % pub_frame), cloud_map)
                    last_pub, n_pub, pub_points = pub_frame, n_pub + 1, int(cloud_map.shape[0])
            except vl.VloamError as e:      # a map beyond max_published_map_points is not published; the run goes on
                if e.status != vl.ERR_CAPACITY:
                    raise
                pub_overflow = True
                print("frame %d: %s" % (count, e), file=sys.stderr)
        if mf:
            c = hd.counts()
            rec = {"frame": count, "points_in": int(cloud.shape[0]), "counts": c, "unwrap_boundary_points": unwrap_boundary_points(cloud),
                   "lo_pose": [float(x) for x in list(q_lo) + list(t_lo)],
                   "map_pose": [float(x) for x in list(q_mo) + list(t_mo)]}
            if a.map_pub_number:
                rec["published_map"] = {"frame": last_pub, "points": pub_points, "overflow": pub_overflow}   # points: of a publication written by this frame, else null
            if a.pose_info:
                pi = hd.pose_info(count, 1)[0]
                fl = int(pi["flags"])
                rec["lo_min_eig"] = float(pi["lo_eig"][0]) if fl & vl.POSE_INFO_LO_VALID else None
                rec["map_min_eig"] = float(pi["map_eig"][0]) if fl & vl.POSE_INFO_MAP_VALID else None
                rec["lo_degenerate"] = bool(fl & vl.POSE_INFO_LO_DEGENERATE)
                rec["map_degenerate"] = bool(fl & vl.POSE_INFO_MAP_DEGENERATE)
            if a.pose_cov:
                pc = hd.get_pose_cov(count, 1)[0]
                # rotation block first in all three parameterisations: (delta theta, delta t) of the LiDAR stages, (angle-axis, t) of the VO
                for k, (stage, bit) in enumerate((("lo", vl.POSE_COV_LO_VALID), ("map", vl.POSE_COV_MAP_VALID), ("vo", vl.POSE_COV_VO_VALID))):
                    ok = bool(int(pc["flags"]) & bit)
                    cov = pc[stage + "_cov"].reshape(6, 6)
                    rec[stage + "_rank"] = int(pc["rank"][k]) if ok else None
                    rec[stage + "_sigma_t"] = float(np.sqrt(max(np.linalg.eigvalsh(cov[3:, 3:])[-1], 0.0))) if ok else None
                    rec[stage + "_sigma_r"] = float(np.sqrt(max(np.linalg.eigvalsh(cov[:3, :3])[-1], 0.0))) if ok else None
            if count > 0:
                for name, st, item in (("lo_round0", 1, 2), ("lo_round1", 1, 18), ("map_round0", 2, 3), ("map_round1", 2, 19)):
                    r = hd.debug_lm_record(st, item)
                    rec[name] = {"residual_blocks": r["n_factors"], "iterations": int(r["trace"].shape[0]), "evaluations": r["n_evals"],
                                 "initial_cost": r["initial_cost"], "final_cost": r["final_cost"], "termination": r["termination"]}
            if a.vloam and count > 0:
                rv = hd.vo_result()
                rec["vo"] = {"counter32": rv["counter32"], "counter22": rv["counter22"], "angles_0to1": [float(x) for x in rv["angles"]],
                             "t_0to1": [float(x) for x in rv["t"]]}
            if a.images:
                rec["image"] = {"keypoints": int(hd.vo_keypoints().shape[0]), "tracked": int(hd.vo_flow_matches()[0].shape[0])}
            if not a.vloam:
                ms, _ = hd.stage_ms()
                rec["stage_ms"] = {"scanRegistration": float(ms[0] - ms_prev[0]), "laserOdometry": float(ms[1] - ms_prev[1]),
                                   "laserMapping": float(ms[2] - ms_prev[2])}
                ms_prev = ms.copy()
            mf.write(json.dumps(rec) + "\n")
        if count + 1 == save_at:
            with open(a.save_checkpoint, "wb") as f:
                f.write(hd.checkpoint())
    if a.merge_map:   # one map out of two runs (vloam_map_merge): behind the sweeps, in front of --carve / --save-map
        mp = a.merge_pose or [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
        res = hd.map_merge(np.load(os.path.join(a.merge_map, "corner.npy")), np.load(os.path.join(a.merge_map, "surf.npy")), q=mp[:4], t=mp[4:],
                           apply=not a.merge_dry_run)
        rec = {k: [int(x) for x in v] for k, v in res.items()}
        rec.update(dir=a.merge_map, pose=mp, apply=not a.merge_dry_run)
        print("%s %s: %d / %d corner / surf points onto map points, %d / %d into %d / %d new voxels, %d / %d in raw voxels, %d / %d outside the window" % (
            "would merge" if a.merge_dry_run else "merged", a.merge_map, rec["n_hit_points"][0], rec["n_hit_points"][1], rec["n_new_points"][0], rec["n_new_points"][1],
            rec["n_new_voxels"][0], rec["n_new_voxels"][1], rec["n_skipped_raw"][0], rec["n_skipped_raw"][1], rec["n_outside_window"][0], rec["n_outside_window"][1]))
        if mf:
            mf.write(json.dumps({"map_merge": rec}) + "\n")
    if mf:
        mf.close()
    if a.sweep_log:
        write_sweep_log(vl, hd, a.sweep_log)
    kio.write_trajectory(os.path.join(a.out, "LO0.txt"), lo_rows)
    kio.write_trajectory(os.path.join(a.out, "MO0.txt"), mo_rows)
    if vo_rows:
        kio.write_trajectory(os.path.join(a.out, "VO0.txt"), vo_rows)
    print("wrote %d rows to %s/{LO0,MO0%s}.txt" % (n - start, a.out, ",VO0" if vo_rows else ""))
    if a.map_pub_number:
        print("wrote %d published maps to %s/map_<frame>.npy" % (n_pub, a.out))
    if a.carve:   # clean the map with the run's last sweeps under their mapping poses (vloam_map_carve, apply)
        n_last, votes = a.carve
        first = max(start, n - n_last)
        poses = hd.trajectory(first, n - first)[:, 7:14]
        removed, res = hd.map_carve([load_sweep(k) for k in range(first, n)], poses, apply=True, min_votes=votes)
        print("carved the map with sweeps %d .. %d (min_votes %d): %d corner / %d surf voxels removed of %d / %d examined (%d / %d confirmed)" % (
            first, n - 1, votes, res["removed"][0], res["removed"][1], res["examined"][0], res["examined"][1], res["confirmed"][0], res["confirmed"][1]))
        np.save(os.path.join(a.out, "carved.npy"), removed)
    if a.archive_rolled is not None:
        archived, info = hd.map_archive(), hd.map_archive_info()
        print("map archive: %d rows held of %d (%d corner / %d surf, %d rolls), %d dropped" % (
            info["rows"], info["capacity_rows"], int(np.count_nonzero((archived["flags"] & vl.MAP_ARCHIVE_KIND) == 0)),
            int(np.count_nonzero(archived["flags"] & vl.MAP_ARCHIVE_KIND)), info["rolls"], info["dropped"]))
    if a.save_map:
        os.makedirs(a.save_map, exist_ok=True)
        halves = [hd.get_map_kind(k) for k in (0, 1)]
        if a.archive_rolled is not None:   # the rolled-out points of each kind in front of the window's
            for k in (0, 1):
                r = archived[(archived["flags"] & vl.MAP_ARCHIVE_KIND) == k]
                halves[k] = np.concatenate([np.stack([r["x"], r["y"], r["z"], r["intensity"]], 1), halves[k]])
        np.save(os.path.join(a.save_map, "corner.npy"), halves[0])
        np.save(os.path.join(a.save_map, "surf.npy"), halves[1])
        row = hd.trajectory(n - 1, 1)[0]
        with open(os.path.join(a.save_map, "start_pose.txt"), "w") as f:
            f.write(" ".join("%.17g" % v for v in row[7:14]) + "\n")
        print("wrote %d corner / %d surf map points to %s" % (halves[0].shape[0], halves[1].shape[0], a.save_map))
        if a.place_db:
            desc, tags, _ = hd.place_get()
            o = hd.place_options
            poses = np.stack([hd.trajectory(int(t) - a.first_sweep, 1)[0][7:14] for t in tags]) if tags.shape[0] else np.zeros((0, 7))
            np.savez(os.path.join(a.save_map, "place_db.npz"), desc=desc, tags=tags, poses=poses, n_ring=o.n_ring, n_sector=o.n_sector,
                     min_range=float(np.float32(hd.cfg.minimum_range)) if o.min_range == 0 else o.min_range, max_range=o.max_range, z_min=o.z_min, z_step=o.z_step)
            print("wrote %d place rows to %s/place_db.npz" % (desc.shape[0], a.save_map))


if __name__ == "__main__":
    main()
