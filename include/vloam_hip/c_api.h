/* libvloam_hip.so — C ABI of the MI355X-native (gfx950, HIP) VLOAM per-scan odometry hot path.
 *
 * The reference (YukunXia/VLOAM-CMU-16833) has no FFI layer; the seam this ABI replaces is the C++
 * class surface its façade drives plus the Ceres cost-functor surface:
 *   vloam::ScanRegistration   src/lidar_odometry_mapping/include/lidar_odometry_mapping/scan_registration.h:71-77
 *   vloam::LaserOdometry      src/lidar_odometry_mapping/include/lidar_odometry_mapping/laser_odometry.h:70-84
 *   vloam::LaserMapping       src/lidar_odometry_mapping/include/lidar_odometry_mapping/laser_mapping.h:85-94
 *   façade call order         src/lidar_odometry_mapping/src/lidar_odometry_mapping.cpp:65-154
 *   VO residual stack         src/visual_odometry/src/visual_odometry.cpp:157-186,254-450
 * include/vloam_hip/compat.hpp presents those classes on top of this ABI; INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Conventions: plain C, opaque handle, caller-owned buffers, int status (0 = OK, < 0 = error), no
 * exceptions across the boundary.  One handle = one sequence on one HIP device (or n_sessions sequences advanced in lock
 * step, vloam_create_batch), with its own HIP streams.  A handle is not thread-safe; distinct handles are independent.  Quaternions are (x, y, z, w) — the layout of
 * the reference's para_q / parameters arrays (laser_odometry.h:126-130, laser_mapping.h:141-143).
 * Clouds are packed float4: (x, y, z, pad) on input == pcl::PointXYZ, (x, y, z, intensity) on
 * output == the payload of pcl::PointXYZI (common.h:42).
 */
#ifndef VLOAM_HIP_C_API_H
#define VLOAM_HIP_C_API_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vloam_handle vloam_handle;
typedef int vloam_status;

enum {
  VLOAM_OK = 0,
  VLOAM_ERR_INVALID = -1,     /* bad argument / unsupported scan_line (the reference ROS_BREAK()s) */
  VLOAM_ERR_HIP = -2,         /* a HIP runtime call failed; vloam_last_error() has the text */
  VLOAM_ERR_CAPACITY = -3,    /* more points / ring length / map entries than the handle was sized for (a scan line of more than
                                 vloam_config::max_ring_points points: raise it, up to 16384; more surf points after the mapping stage's
                                 VoxelGrid than vloam_limits::max_surf_stack_points: raise it, up to 131072) */
  VLOAM_ERR_EMPTY = -4,       /* no point survived NaN / minimum_range removal (reference: UB, scan_registration.cpp:166) */
  VLOAM_ERR_NO_DEVICE = -5,   /* no usable gfx950 device: there is NO CPU fallback */
  VLOAM_ERR_ORDER = -6        /* stage called out of the façade's order */
};

/* Tunables = the ROS parameters the reference reads in its init() functions:
 * LOM/launch/loam_velodyne_HDL_64_kitti.launch:3-16, MAIN/launch/vloam_main.launch:4-10. */
typedef struct vloam_config {
  int scan_line;                   /* 16 | 32 | 64                                   (64)   */
  double minimum_range;            /* removeClosedPointCloud threshold [m]           (5.0)  */
  int mapping_skip_frame;          /*                                                (1)    */
  float mapping_line_resolution;   /* corner VoxelGrid leaf [m]                      (0.4)  */
  float mapping_plane_resolution;  /* surf VoxelGrid leaf [m]                        (0.8)  */
  int detach_VO_LO;                /* 1: LO warm-starts from its own last estimate   (1)    */
  int reset_VO_to_identity;        /*                                                (0)    */
  int remove_VO_outlier;           /* pixel gate on matches                          (100)  */
  int with_mapping;                /* run laserMapping inside vloam_process_scan     (1)    */
  int max_points;                  /* capacity of one sweep                          (262144) */
  int max_frames;                  /* capacity of the on-device trajectory log       (8192) */
  int map_capacity_log2;           /* voxel-hash slots = 2^n per feature kind        (22)   */
  int debug;                       /* 1: keep parity-hook arrays (curvature, sort order, …) */
  int timing;                      /* 1: HIP-event per-stage timing (synchronises every sweep)   */
  int image_width;                 /* capacity of the image front-end (KITTI: 1242 x 375); 0 = none (0) */
  int image_height;
  int CLAHE;                       /* 1: cv::createCLAHE(2.0)->apply on every image first (vloam_main.launch:8)  (0) */
  int max_ring_points;             /* capacity of one scan line: 4096 (0 = 4096); 4097 .. 16384 add the long ring tier  (4096) */
} vloam_config;

typedef struct vloam_calib {  /* row-major f32, as PointCloudUtil holds them (point_cloud_util.h:43-46) */
  float cam_T_velo[16];
  float rect0_T_cam[16];
  float P_rect0[12];
} vloam_calib;

void vloam_default_config(vloam_config* cfg);
const char* vloam_last_error(void);
const char* vloam_version(void);

vloam_status vloam_create(const vloam_config* cfg, int device, vloam_handle** out);
vloam_status vloam_destroy(vloam_handle* h);

/* Capacities that are not in vloam_config (whose size compiled callers depend on).  The reference has no capacity on the mapping stage's
 * input: laserCloudSurfStack is whatever downSizeFilterSurf returns (laser_mapping.cpp:432-440).  A default handle takes 24576 surf points
 * there (a 64-line sweep at the KITTI leaf of 0.8 m has ~6000; at a 0.2 m leaf ~27000) and vloam_sync reports VLOAM_ERR_CAPACITY beyond; a
 * larger max_surf_stack_points adds the large stack tier: everything the mapping stage indexes by a stack point is sized by it (~2.8 KB of
 * device memory per point and session), the scan-to-map kernels run their run-time-capacity forms and the solve
 * compacts its factors in a launch of its own.  The corner stack (8192 >= the 7680 lessSharp points a sweep can have) has no such limit.
 * struct_size: sizeof(vloam_limits) as the caller compiled it (0: this header's), so that fields can be added behind the ones it knows: 8 ends
 * behind max_surf_stack_points, 20 == sizeof(vloam_limits) behind publish_registered_cloud, 24 == sizeof(vloam_limits_ext) behind sweep_log (below);
 * the fields a caller's size does not reach read as 0. */
typedef struct vloam_limits {
  int struct_size;             /* sizeof(vloam_limits) as the caller compiled it */
  int max_surf_stack_points;   /* capacity of laserCloudSurfStack: 24576 (0 = 24576); multiples of 8192 up to 131072 add the large stack tier */
  /* The clouds of LaserMapping::publish (laser_mapping.cpp:778-805), written by the mapping stream itself behind the sweep that publishes
   * them (vloam_get_published_map / _cloud / vloam_published_device_ptr below).  All three 0 (or a struct_size of 8): none, as before. */
  int map_pub_number;          /* 0: off.  >= 1: /laser_cloud_map after every MAPPED sweep with (frameCount * mapping_skip_frame) % map_pub_number == 0,
                                  frameCount = mapped sweeps so far, this one included (laser_mapping.cpp:778; the KITTI launch file sets 20).  On a
                                  sweep skipped by mapping_skip_frame the reference republishes the unchanged map; here the last publication
                                  simply stays current */
  int max_published_map_points;/* capacity of one map publication: 256 .. 16777216 (0 = 2097152); ignored when map_pub_number == 0 */
  int publish_registered_cloud;/* 0 | 1: the full-resolution cloud registered in the map frame (laser_mapping.cpp:795-805) after every sweep's mapping */
} vloam_limits;
/* The limits with the field that came after vloam_limits (which keeps its 20 bytes for the callers compiled against it): sweep_log lies right
 * behind publish_registered_cloud, at byte 20.  Hand &ext.limits to vloam_create_with_limits with limits.struct_size == sizeof(vloam_limits_ext)
 * (vloam_default_limits_ext sets it): exactly that struct_size tells the library that the field is there; with any other accepted size (0, 8, 20,
 * or a larger one: a later header's struct, of which the fields of vloam_limits are read) nothing behind vloam_limits is read and sweep_log is 0. */
typedef struct vloam_limits_ext {
  vloam_limits limits;
  int sweep_log;               /* 0 | 1: one vloam_sweep_record per sweep and session, written by the stage streams themselves (vloam_get_sweep_log below);
                                  works with with_mapping 0 or 1 */
} vloam_limits_ext;
void vloam_default_limits_ext(vloam_limits_ext* lim);
void vloam_default_limits(vloam_limits* lim);
/* vloam_create_batch with limits.  lim == NULL or the defaults: the same handle as vloam_create_batch(cfg, device, n_sessions, out).
 * VLOAM_ERR_INVALID (before any device call): max_surf_stack_points other than 0, 24576 or a multiple of 8192 in (24576, 131072], or such a
 * multiple above cfg->max_points; a struct_size that is neither 0, nor 8 (the first version of the struct: the fields behind
 * max_surf_stack_points read as 0), nor >= sizeof(vloam_limits) (only sizeof(vloam_limits_ext) itself carries sweep_log); a negative map_pub_number; a max_published_map_points outside 256 .. 16777216 (with map_pub_number >= 1); a publish_registered_cloud
 * other than 0 or 1; either product with cfg->with_mapping == 0; a sweep_log other than 0 or 1 (struct_size == sizeof(vloam_limits_ext)).
 * VLOAM_ERR_HIP: the arenas (the publication buffers are part of them) do not fit the device's memory. */
vloam_status vloam_create_with_limits(const vloam_config* cfg, const vloam_limits* lim, int device, int n_sessions, vloam_handle** out);

/* ---- Growable voxel map (opt-in, single-sequence handles).  The map is two open-addressing tables of 2^map_capacity_log2 slots; a fixed handle
 * whose table passes 60 % of its slots is finished (VLOAM_ERR_CAPACITY from every vloam_sync, for good).  With grow = 1 the handle STARTS at
 * map_capacity_log2, keeps the two tables in allocations of their own, and doubles a table between two sweeps whenever the sweeps enqueued
 * so far could fill it (a bound, not a count: INTEGRATION.md section 5), up to 2^max_capacity_log2 slots per table.  Below that ceiling no
 * table passes 60 % of its slots (tombstones included), the load a fixed handle reports as full; at the ceiling the fixed handle's behaviour returns.  Poses and map are what a fixed handle of any sufficient size
 * computes: slot positions do not matter.  A failed allocation of a larger table is reported (VLOAM_ERR_HIP) by the call that tried; the old
 * table stays in use and the handle stays usable until that table really fills.
 * struct_size: sizeof(vloam_map_options) as the caller compiled it. */
typedef struct vloam_map_options {
  int struct_size;            /* sizeof(vloam_map_options) as the caller compiled it */
  int grow;                   /* 0 | 1 */
  int max_capacity_log2;      /* ceiling per table; 0 = 28; >= cfg->map_capacity_log2 (after its clamp to 10..28), <= 28 */
} vloam_map_options;
void vloam_default_map_options(vloam_map_options* opt);
/* vloam_create_with_limits with map options.  lim: any form vloam_create_with_limits accepts, or NULL.  opt == NULL or grow == 0: the same
 * handle as vloam_create_with_limits(cfg, lim, device, n_sessions, out) in every respect.  VLOAM_ERR_INVALID (before any device call), each
 * with its own vloam_last_error(): a struct_size other than sizeof(vloam_map_options); a grow other than 0 or 1 or a max_capacity_log2 that
 * is neither 0 nor in [map_capacity_log2, 28]; grow == 1 with n_sessions > 1 or cfg->with_mapping == 0 (a batch's kernels address session
 * b's tables at the arena stride: DESIGN.md section 8). */
vloam_status vloam_create_with_options(const vloam_config* cfg, const vloam_limits* lim, const vloam_map_options* opt, int device, int n_sessions,
                                       vloam_handle** out);

/* ---- Batched execution: one handle, n_sessions independent sequences advanced in lock step.  Every kernel of the sweep chain is
 * launched once per sweep for ALL sessions (session index in blockIdx.z), so n_sessions sequences cost one launch chain — the way to
 * fill the chip with a path whose single-sequence form is a latency chain.  Each session owns an identical arena of
 * device state; integer / index / f32 point results (feature clouds, picks, down-sampled scan features, image key points) are bit-identical
 * to running the sequence alone, the f64 poses agree to round-off (~1e-13: a batch adds the partial sums of its solves over 4 / 6
 * workgroups, a single sequence over 8).  vloam_create == vloam_create_batch(…, 1, …).
 * vloam_batch_process_scan[_device]: session b gets sweep xyz_pad4[b] with n[b] points (arrays of n_sessions entries).
 * vloam_select_session: which session the getters below (trajectory, features, counts, map, parity hooks) read; 0 after creation.
 * The single-sequence entry points (vloam_scan_registration*, vloam_laser_*, vloam_process_scan*, vloam_process_frame*) return
 * VLOAM_ERR_INVALID on a handle with more than one session.
 * Co-residency bound: the Levenberg-Marquardt solves of a sweep run as cooperating workgroups (batch: 4 for the odometry, 6 for the
 * mapping; a single sequence: 8 + 8, all eight of a solve on ONE XCD — odometry on XCD 2, mapping on XCD 6 — for the first two
 * single-sequence handles alive in a process, spread over the XCDs for further ones; one compute unit's worth of registers each) that
 * exchange partial sums INSIDE one launch, so all workgroups of a solve must be
 * resident together; a session of a batch can have one odometry and one mapping solve in flight, i.e. 10 such workgroups.  vloam_create_batch
 * refuses (VLOAM_ERR_CAPACITY) when 10 * n_sessions exceeds the device's compute-unit count (256 on MI355X, so n_sessions <= 24 — the
 * library's own bound, kMaxBatch — is always accepted there); several batched handles on ONE device share that budget — keep the sum of their sessions within it.  The one-XCD
 * placement of a single sequence's solves holds at most 4 solves per XCD (32 compute units, 8 per solve).  When the workgroups of a solve
 * are NOT resident together after all (another process on the GPU, a CU-masked queue, a partitioned device), the solve does not fail: a
 * workgroup that still waits for its partners after ~0.5 s gives up, the lead workgroup runs the whole solve on its own, vloam_get_health
 * counts it, and from the next ENQUEUE on (the host polls a host-mapped word, no synchronisation needed) the handle launches one-workgroup
 * solves only (slower per solve, no co-residency needed). */
vloam_status vloam_create_batch(const vloam_config* cfg, int device, int n_sessions, vloam_handle** out);
vloam_status vloam_batch_size(vloam_handle* h, int* n_sessions);
vloam_status vloam_batch_process_scan_device(vloam_handle* h, const void* const* d_xyz_pad4, const int* n);
vloam_status vloam_batch_process_scan(vloam_handle* h, const float* const* xyz_pad4, const int* n);
vloam_status vloam_select_session(vloam_handle* h, int session);
/* one coupled VLOAM frame (vloam_process_frame_device, below) for every session: prev_uv[b] / curr_uv[b] = session b's n_match[b] pixel
 * matches in host memory; vloam_vo_set_calib / vloam_set_extrinsics apply to all sessions (one sensor rig) */
vloam_status vloam_batch_process_frame_device(vloam_handle* h, const void* const* d_xyz_pad4, const int* n, const int* const* prev_uv,
                                              const int* const* curr_uv, const int* n_match);
vloam_status vloam_batch_process_frame(vloam_handle* h, const float* const* xyz_pad4, const int* n, const int* const* prev_uv,
                                       const int* const* curr_uv, const int* n_match);   /* sweeps in host memory */

/* == LidarOdometryMapping::reset (lidar_odometry_mapping.cpp:65-71) */
vloam_status vloam_reset_frame(vloam_handle* h);

/* == ScanRegistration::input (scan_registration.cpp:131-449).  xyz_pad4: n packed float4 in HOST memory. */
vloam_status vloam_scan_registration(vloam_handle* h, const float* xyz_pad4, int n);
/* same, input already resident in this device's HBM */
vloam_status vloam_scan_registration_device(vloam_handle* h, const void* d_xyz_pad4, int n);

/* == ScanRegistration::output (scan_registration.cpp:501-512).
 * which: 0 laserCloud, 1 cornerPointsSharp, 2 cornerPointsLessSharp, 3 surfPointsFlat, 4 surfPointsLessFlat,
 *        5 laserCloudCornerLast, 6 laserCloudSurfLast (LaserOdometry::output, laser_odometry.cpp:610-629),
 *        7 laserCloudCornerStack, 8 laserCloudSurfStack (down-sampled scan features inside mapping),
 *        11 full-resolution cloud registered in the map frame (LaserMapping::publish, laser_mapping.cpp:795-799).
 * Copies min(n, cap) points to the HOST buffer xyzi4 and returns the true count in *n. Synchronises the stream. */
vloam_status vloam_get_features(vloam_handle* h, int which, float* xyzi4, int cap, int* n);

/* == the /laser_cloud_map product of LaserMapping::publish (laser_mapping.cpp:778-793): the corner cloud then the surf cloud of every
 * cube of the 21 x 21 x 11 window, cube index ascending, each cube cloud in its VoxelGrid order.  The reference publishes it every
 * map_pub_number frames.  Two ways to it: vloam_get_map, whenever the caller asks (synchronises the whole pipeline, orders the cloud on the
 * host), or vloam_limits::map_pub_number and vloam_get_published_map below (the mapping stream writes the ordered cloud behind the publishing
 * sweep).  Copies min(*n, cap) points to the HOST buffer, true count in *n. */
vloam_status vloam_get_map(vloam_handle* h, float* xyzi4, long long cap, long long* n);

/* == the clouds of LaserMapping::publish as products of the sweep pipeline (vloam_limits::map_pub_number / publish_registered_cloud).  The
 * mapping stream writes them into device buffers of the handle, in order behind the mapping of the sweep that publishes: a publication is a
 * snapshot as of that sweep, whatever has been enqueued since.  Two buffers per product and session, used alternately.
 * vloam_get_published_map / _cloud: the latest publication ENQUEUED so far.  First enqueues what the handle still owes (no wait), then waits
 *   for the event behind that publication only — not for the pipeline — and copies min(*n, cap) points to the HOST buffer (which may be NULL
 *   with cap 0); *n = the true count, *frame = the 0-based index of the publishing sweep.  Before the first publication: *n = 0, *frame = -1,
 *   VLOAM_OK.  Reads the session chosen with vloam_select_session.  The registered cloud is the one vloam_get_features(h, 11) returns for
 *   that sweep (laserCloudFullRes as handed to vloam_set_mapping_input included); on a sweep skipped by mapping_skip_frame it is registered
 *   with the last mapped pose, as there.
 * VLOAM_ERR_ORDER: the product is not enabled on this handle.  VLOAM_ERR_CAPACITY (map only): the map held more points than
 *   max_published_map_points at that sweep — nothing was written, *n is the true count (also in vloam_last_error()), no partial cloud comes
 *   back; the pipeline itself is unaffected (vloam_sync stays VLOAM_OK, vloam_get_map still works).
 * vloam_published_device_ptr: which = 0 map, 1 registered cloud.  The device address of the same publication (packed float4), its count and
 *   frame, for a consumer on the GPU; waits for the publication's event like the getters.  The address stays valid until the next call that
 *   enqueues a sweep (the product's second buffer takes the next publication, the one after that overwrites this one). */
vloam_status vloam_get_published_map(vloam_handle* h, float* xyzi4, long long cap, long long* n, int* frame);
vloam_status vloam_get_published_cloud(vloam_handle* h, float* xyzi4, int cap, int* n, int* frame);
vloam_status vloam_published_device_ptr(vloam_handle* h, int which, void** d_xyzi4, long long* n, int* frame);

/* == vloam_tf->velo_last_VOT_velo_curr, read by solveLO when detach_VO_LO == 0 (laser_odometry.cpp:223-236) */
vloam_status vloam_set_lo_prior(vloam_handle* h, const double q_xyzw[4], const double t[3]);

/* == LaserOdometry::input + solveLO + output (laser_odometry.cpp:135-146,187-536,610-629).
 * Outputs (any may be NULL): world pose q_w_curr/t_w_curr and the frame-to-frame q_last_curr/t_last_curr. */
vloam_status vloam_laser_odometry(vloam_handle* h, double q_w[4], double t_w[3], double q_lc[4], double t_lc[3]);

/* LaserOdometry::input with clouds that are NOT the ones vloam_scan_registration left on the device — the reference deep-copies whatever it is
 * handed (laser_odometry.cpp:135-146), so a caller may edit or replace the five clouds between the stages.  Call between
 * vloam_scan_registration and vloam_laser_odometry; host pointers to packed (x, y, z, intensity) floats, intensity = scan line +
 * SCAN_PERIOD * relTime as scan registration writes it (scan_registration.cpp:262-264); a NULL cloud keeps the device's.  The clouds replace
 * the sweep's own: this sweep's odometry, the next sweep's CornerLast / SurfLast (laser_odometry.cpp:506-526) and the mapping stage's input
 * all see them.  Capacity: 768 / 7 680 / 1 536 points for cornerPointsSharp / LessSharp / surfPointsFlat, max_points for the other two.
 * Enforced rule, checked on the host arrays before anything is uploaded (VLOAM_ERR_INVALID otherwise; vloam_last_error() names the cloud, the
 * point index and the rule; the handle stays as it was, so vloam_laser_odometry then runs on scan registration's own clouds):
 *   (i)   every float of all five clouds is finite;
 *   (ii)  in cornerPointsLessSharp and surfPointsLessFlat, every L = int(intensity) lies in [0, 64);
 *   (iii) in those two clouds, max_{i<j} L[i] - L[j] <= 2: no point comes after one whose line is 3 or more above its own.
 * Why (iii): the adjacent-line walks of laser_odometry.cpp:294-324,371-428 start at the closest point's index and break at the first line
 * outside r +- 2.5; the device bounds them by the first index of the cloud with a line >= r + 3 and the last with a line <= r - 3.  The two
 * agree at every index exactly under (iii).  Scan registration's clouds keep it (lines ascending up to the r / r - 1 jitter of
 * int(intensity)), and so does any filter that drops points, a shuffle inside a line, or a reorder of lines within windows of three.  The
 * rule is conservative: some orders that break (iii) still walk the same way in the reference, and they are refused too.
 * Both stage-input calls are for single-sequence handles driven stage by stage (VLOAM_ERR_INVALID on n_sessions > 1: a batch is enqueued whole). */
vloam_status vloam_set_odometry_input(vloam_handle* h, const float* laserCloud, int n_full, const float* cornerPointsSharp, int n_sharp,
                                      const float* cornerPointsLessSharp, int n_less_sharp, const float* surfPointsFlat, int n_flat,
                                      const float* surfPointsLessFlat, int n_less_flat);

/* q_w_curr / t_w_curr of the sweep in progress (after vloam_laser_odometry) or of the last finished sweep: what LaserOdometry::output hands to
 * LaserMapping::input (laser_odometry.cpp:610-616). */
vloam_status vloam_get_odometry_pose(vloam_handle* h, double q_w[4], double t_w[3]);

/* LaserMapping::input with clouds / an odometry pose that are NOT LaserOdometry::output's (laser_mapping.cpp:167-196 copies what it is handed; on a
 * sweep skipped by mapping_skip_frame only the pose).  Call between vloam_laser_odometry and vloam_laser_mapping; NULL keeps the device's.  Only
 * this sweep's mapping (and the /velodyne_cloud_registered product, vloam_get_features(11)) sees them — the odometry keeps its own
 * CornerLast / SurfLast, like the reference's separate copies.  Enforced: every float of the three clouds is finite (VLOAM_ERR_INVALID
 * otherwise, before anything is uploaded; mapping does not walk by scan line, so no line rule applies).  Stated limit: q_wodom_curr must be a unit quaternion (as any
 * Eigen::Quaterniond an odometry produces): the solver's closed-form Jacobians are those of a rotation, the reference's autodiff
 * differentiates Eigen's un-normalised q * v — with |q|^2 = 1 + 5e-6 the map poses part by 1e-9 (measured, tests/test_gpu_stage_inputs.py). */
vloam_status vloam_set_mapping_input(vloam_handle* h, const float* laserCloudCornerLast, int n_corner, const float* laserCloudSurfLast, int n_surf,
                                     const float* laserCloudFullRes, int n_full, const double q_wodom_curr[4], const double t_wodom_curr[3]);

/* == LaserMapping::input + solveMapping + the pose of publish() (laser_mapping.cpp:167-196,198-708,718-757).  Outputs the
 * map-frame pose publish() reports: q_w_curr / t_w_curr after a mapped sweep, the high-frequency pose
 * q_wmap_wodom * q_wodom_curr after a sweep skipped by mapping_skip_frame. */
vloam_status vloam_laser_mapping(vloam_handle* h, double q_map[4], double t_map[3]);

/* Whole façade for one sweep, enqueued with NO host synchronisation:
 * reset -> scanRegistrationIO -> laserOdometryIO -> laserMappingIO (MAIN/src/vloam_main_node.cpp:134,166-168).
 * d_xyz_pad4 is DEVICE memory and must stay valid until vloam_sync().  Poses go to the on-device trajectory log.
 * The odometry / mapping of a sweep may only be ENQUEUED by a later call (they trail the scan registration by one / two
 * sweeps so that no live cross-stream wait is needed); every call that returns results, vloam_sync() and the stage-wise
 * entry points first enqueue whatever is still owed, so this is invisible except through the raw device pointer below. */
vloam_status vloam_process_scan_device(vloam_handle* h, const void* d_xyz_pad4, int n);
/* same with a HOST buffer — what the reference's callback hands over (a pcl::PointCloud<pcl::PointXYZ>'s points, scan_registration.cpp:131-152).
 * The sweep is copied into one of four device input buffers on a copy stream of the handle; the call returns once the copy is enqueued, and the
 * sweep itself — like its odometry and mapping — is ENQUEUED BY THE NEXT CALL on the handle, whatever that call is (another sweep of any kind, a
 * stage-wise call, a getter, vloam_sync): by then the copy has landed, so the 2 MB cross the host link beside the previous sweep's scan
 * registration and no stream waits for another (0.96 - 0.98 x the device-resident rate; profiles/r06_host_input.txt).  The sweep counts
 * (vloam_frame_count, trajectory rows) from the moment it is handed over.  What can be refused is refused by THIS call (null / empty / oversized
 * cloud, a full trajectory log); an enqueue failure of the deferred sweep (VLOAM_ERR_HIP) is reported by the call that enqueues it.
 *   pageable memory (malloc, std::vector, a ROS message): the runtime has taken its copy of the sweep when the call returns — the buffer may
 *     be reused at once; the calling thread pays the staging memcpy (~2 MB per sweep);
 *   pinned memory (hipHostMalloc / hipHostRegister): read by DMA AFTER the call returns — leave the buffer unchanged until the next
 *     vloam_sync(); no host-side copy (bench.py: host_input).
 * vloam_batch_process_scan works the same way.  Every other entry point that takes a host sweep (vloam_scan_registration, vloam_process_frame*,
 * vloam_vo_process_point_cloud) copies it on the scan-registration stream in front of its first reader, nothing deferred (the memory rules are
 * the same); VLOAM_STAGE_INLINE=1 in the environment selects that form for the two whole-sweep calls as well. */
vloam_status vloam_process_scan(vloam_handle* h, const float* xyz_pad4, int n);
vloam_status vloam_sync(vloam_handle* h);

/* Trajectory log: per processed frame 14 doubles {q_w_curr[4], t_w_curr[3]} (laser odometry, world_LOT_base_last)
 * followed by {q_map[4], t_map[3]} (mapping, world_MOT_base_last).  first..first+count-1 -> HOST buffer. */
vloam_status vloam_get_trajectory(vloam_handle* h, int first, int count, double* poses14);
vloam_status vloam_frame_count(vloam_handle* h, int* frames);
/* device address + byte size of the trajectory log (for an RCCL gather across GPUs); rows are only complete
 * after vloam_sync() */
vloam_status vloam_trajectory_device_ptr(vloam_handle* h, void** d_ptr, long long* bytes);

/* == Per-sweep diagnostics log (vloam_limits_ext::sweep_log = 1): what the reference says about a frame while it runs -- "less correspondence!"
 * (laser_odometry.cpp:452-455), "Map corner and surf num are not enough" (laser_mapping.cpp:448,631-635), the solver summaries -- and what
 * vloam_sync can only report for "at least one sweep since the last vloam_sync", as one fixed-size record per sweep and session.  The rows live
 * beside the trajectory log in the session arena (max_frames rows of 192 bytes: 1.5 MB per session at the default 8192) and are written by
 * the stage streams themselves: scan registration writes its counts and error bits behind the sweep's scan registration, the odometry its
 * factor counts and two solves behind the sweep's odometry, the mapping the rest behind the sweep's mapping; the last of them (the odometry
 * when with_mapping == 0) stamps `frame`.  No stream waits for another and nothing synchronises.  A handle without sweep_log allocates and
 * launches nothing of this.  vloam_sync, the sticky error words and vloam_get_health are what they were, log or no log.
 * sizeof(vloam_sweep_record) == 192: 32 ints, then 8 doubles; ints without a name here are 0. */
enum {   /* vloam_sweep_record::error_bits: raised BY THIS SWEEP; the condition is the one vloam_sync words for the handle */
  VLOAM_SWEEP_EMPTY = 1,            /* no point of the sweep survived NaN / minimum_range removal (vloam_sync: VLOAM_ERR_EMPTY) */
  VLOAM_SWEEP_RING_TOO_LONG = 2,    /* a ring held more than max_ring_points points and was dropped (VLOAM_ERR_CAPACITY) */
  VLOAM_SWEEP_MAP_FULL = 4,         /* voxel hash full (map_capacity_log2; on a growable handle: at vloam_map_options::max_capacity_log2); the handle keeps this bit for good: the row is the sweep that raised it first */
  VLOAM_SWEEP_MAP_RAW_CAPACITY = 8, /* raw-point capacity of the map exceeded (more than 255 un-merged points in a voxel of a cube outside the valid
                                       block, or more than 64 raw voxels around one query); first sweep to raise it, like MAP_FULL */
  VLOAM_SWEEP_STACK_FULL = 16,      /* mapping factor table full: more surf points after VoxelGrid than max_surf_stack_points */
  VLOAM_SWEEP_DS_TIMEOUT = 32,      /* a workgroup of the scan-feature VoxelGrid gave up waiting for the bins in front of it: the sweep was not mapped */
  VLOAM_SWEEP_VO_DEGENERATE = 64    /* this frame's VO solve returned a zero rotation angle: poses are NaN from here on (visual_odometry.cpp:427-430) */
};
enum {   /* vloam_sweep_record::flags */
  VLOAM_SWEEP_FLAG_FIRST = 1,              /* first sweep of the sequence: no odometry solve (laser_odometry.cpp:196-204) */
  VLOAM_SWEEP_FLAG_MAP_SKIPPED = 2,        /* mapping skipped by mapping_skip_frame: only the high-frequency pose (laser_mapping.cpp:186-190) */
  VLOAM_SWEEP_FLAG_MAP_NOT_OPTIMIZED = 4,  /* mapped, but "Map corner and surf num are not enough": no solve (laser_mapping.cpp:448,631-635) */
  VLOAM_SWEEP_FLAG_LO_LESS_CORR_0 = 8,     /* "less correspondence!": fewer than 10 factors in odometry round 0 (laser_odometry.cpp:452-455) */
  VLOAM_SWEEP_FLAG_LO_LESS_CORR_1 = 16,    /* ... in round 1 */
  VLOAM_SWEEP_FLAG_SOLVE_DEGRADED = 32     /* a cooperative solve degraded to one workgroup (vloam_get_health) and this sweep's odometry or mapping was
                                              the first to see the handle's counter rise: the odometry and the mapping of neighbouring sweeps run side
                                              by side and share that counter, so the solve may be the neighbour's */
};
typedef struct vloam_sweep_record {
  int frame;                   /* 0-based sweep index; -1 while the row has not been completed */
  int error_bits;              /* VLOAM_SWEEP_* */
  int flags;                   /* VLOAM_SWEEP_FLAG_* */
  /* scan registration */
  int n_in;                    /* points handed in */
  int n_cloud;                 /* laserCloud->size() after NaN / minimum_range / ring removal */
  int n_sharp, n_less_sharp, n_flat, n_less_flat;
  /* laser odometry, per outer round; all 0 on the first sweep */
  int lo_corner_factors[2];    /* corner_correspondence (laser_odometry.cpp:326-341) */
  int lo_plane_factors[2];     /* plane_correspondence (laser_odometry.cpp:430-446) */
  int lo_iterations[2];        /* trust-region iterations run, accepted or not (the rows of the solver's iteration trace) */
  int lo_termination[2];       /* 0 iteration cap, 1 convergence, 2 failure */
  /* laser mapping; all 0 on a sweep skipped by mapping_skip_frame and on a handle without mapping */
  int n_corner_stack, n_surf_stack;   /* laserCloudCornerStackNum / laserCloudSurfStackNum (laser_mapping.cpp:432-440) */
  int n_map_corner, n_map_surf;       /* laserCloudCornerFromMapNum / laserCloudSurfFromMapNum: points gathered from the valid block (:404-430) */
  int map_corner_factors[2];   /* per outer round; the four solve fields are 0 when the optimisation did not run */
  int map_surf_factors[2];
  int map_iterations[2];
  int map_termination[2];
  int reserved[3];
  /* initial / final cost of the four solves (0 where a solve did not run) */
  double lo_initial_cost[2], lo_final_cost[2];
  double map_initial_cost[2], map_final_cost[2];
} vloam_sweep_record;
#if defined(__cplusplus)
static_assert(sizeof(vloam_sweep_record) == 192, "vloam_sweep_record is 32 ints and 8 doubles");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(vloam_sweep_record) == 192, "vloam_sweep_record is 32 ints and 8 doubles");
#endif
/* vloam_get_sweep_log: the rows of sweeps first .. first + count - 1 of the session chosen with vloam_select_session -> HOST buffer.  Like
 *   vloam_get_published_map it first enqueues what the handle still owes (no wait) and then waits for the work behind sweep first + count - 1
 *   only, not for sweeps enqueued after it.  VLOAM_ERR_ORDER: the handle was created without vloam_limits_ext::sweep_log.  VLOAM_ERR_INVALID: a
 *   range beyond vloam_frame_count.  A sweep whose odometry or mapping the caller left out (stage-wise driving) keeps frame == -1.
 * vloam_sweep_log_device_ptr: device address + byte size of the selected session's rows, like vloam_trajectory_device_ptr; rows are only complete
 *   after vloam_sync(). */
vloam_status vloam_get_sweep_log(vloam_handle* h, int first, int count, vloam_sweep_record* out);
vloam_status vloam_sweep_log_device_ptr(vloam_handle* h, void** d_rows, long long* bytes);

/* == Per-sweep pose information matrices and degeneracy flags (vloam_pose_info_enable): how well the scan constrained the pose.  The reference
 * leaves odomAftMapped.pose.covariance and laserOdometry.pose.covariance at zero (laser_mapping.cpp:714-757, laser_odometry.cpp:538-554).  Here,
 * for every sweep and session, one fixed-size record holds -- for the laser odometry and for the mapping -- the Gauss-Newton information matrix
 * of the LAST outer round's problem at the pose that round returned: sum of J^T J after the loss corrector (Huber 0.1) over the residual blocks
 * the solve consumed, in the 6-D tangent space (delta theta, delta t) of EigenQuaternionParameterization, unscaled; with its six eigenvalues, the
 * cost 0.5 sum rho at that pose, the residual-block counts and degeneracy flags (smallest eigenvalue below a threshold: a tunnel, an open
 * field, a ground-only view).
 * Off on every handle that does not ask.  vloam_pose_info_enable allocates max_frames rows of 832 bytes per session (6.5 MB per session at the
 * default 8192) OUTSIDE the session arenas -- arena layout and checkpoint sizes are those of a handle without it -- and from then on each LiDAR
 * stage writes its half of the row with one launch on its own stream behind its last solve; the mapping (the odometry when with_mapping == 0)
 * stamps `frame`.  No stream waits for another, nothing synchronises, no floating-point atomics: a row is bit-identical from run to run, and
 * poses and map are those of a handle without the product.
 * *_VALID is clear and that half of the record is zero -- odometry: on the first sweep (laser_odometry.cpp:196-204); mapping: on a sweep
 * skipped by mapping_skip_frame, when "Map corner and surf num are not enough" (laser_mapping.cpp:448), and on a handle without mapping.
 * Rows do NOT travel in a checkpoint: after vloam_checkpoint_load into an enabled handle the restored sweeps read frame == -1, later sweeps
 * are written normally.
 * Not in this record: the matrix of the VO solve (angle-axis problem), the eigenvectors and the inversion to a covariance.  They are the rows of
 * vloam_pose_cov_enable below (vloam_get_pose_cov), an add-on of this product that leaves these 832 bytes bit for bit what they are. */
typedef struct vloam_pose_info_options {
  int struct_size;              /* sizeof(vloam_pose_info_options) as compiled */
  int reserved;                 /* 0 */
  double lo_min_eigenvalue;     /* VLOAM_POSE_INFO_LO_DEGENERATE when the smallest eigenvalue of the odometry matrix is below this; 0 = never */
  double map_min_eigenvalue;    /* the same for the mapping matrix */
} vloam_pose_info_options;
void vloam_default_pose_info_options(vloam_pose_info_options* opt);   /* struct_size set, thresholds 0 */
enum {   /* vloam_pose_info_record::flags */
  VLOAM_POSE_INFO_LO_VALID = 1,         /* the odometry half holds this sweep's last odometry round */
  VLOAM_POSE_INFO_MAP_VALID = 2,        /* the mapping half holds this sweep's last mapping round */
  VLOAM_POSE_INFO_LO_DEGENERATE = 4,    /* LO_VALID and lo_eig[0] < lo_min_eigenvalue */
  VLOAM_POSE_INFO_MAP_DEGENERATE = 8    /* MAP_VALID and map_eig[0] < map_min_eigenvalue */
};
typedef struct vloam_pose_info_record {
  int frame;                    /* 0-based sweep index; -1 while the row has not been completed */
  int flags;                    /* VLOAM_POSE_INFO_* */
  int lo_factors[2];            /* edge, plane residual blocks of the last odometry round */
  int map_factors[2];           /* corner, surf residual blocks of the last mapping round */
  int reserved[2];
  /* per stage: the point of evaluation (q xyzw, t) = what the round returned; 0.5 sum rho there; the matrix, row-major; its eigenvalues, ascending */
  double lo_x[7], lo_cost, lo_H[36], lo_eig[6];
  double map_x[7], map_cost, map_H[36], map_eig[6];
} vloam_pose_info_record;
#if defined(__cplusplus)
static_assert(sizeof(vloam_pose_info_record) == 832, "vloam_pose_info_record is 8 ints and 100 doubles");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(vloam_pose_info_record) == 832, "vloam_pose_info_record is 8 ints and 100 doubles");
#endif
/* vloam_pose_info_enable: on a FRESH handle only (no sweep taken, stage 0; VLOAM_ERR_ORDER otherwise, also when called twice); single-sequence and
 *   batched handles, with_mapping 0 or 1.  opt may be NULL (the defaults).  The options are checked first, before the handle is looked at:
 *   VLOAM_ERR_INVALID for a struct_size other than sizeof(vloam_pose_info_options), a reserved other than 0, a negative, NaN or infinite threshold.
 * vloam_get_pose_info: the rows of sweeps first .. first + count - 1 of the session chosen with vloam_select_session -> HOST buffer.  Like
 *   vloam_get_sweep_log it first enqueues what the handle still owes (no wait) and then waits for the work behind sweep first + count - 1 only.
 *   VLOAM_ERR_ORDER: the handle never enabled the product.  VLOAM_ERR_INVALID: a range beyond vloam_frame_count.  A sweep whose odometry or
 *   mapping the caller left out (stage-wise driving) keeps frame == -1.
 * vloam_pose_info_device_ptr: device address + byte size of the selected session's rows; rows are only complete after vloam_sync(). */
vloam_status vloam_pose_info_enable(vloam_handle* h, const vloam_pose_info_options* opt);
vloam_status vloam_get_pose_info(vloam_handle* h, int first, int count, vloam_pose_info_record* out);
vloam_status vloam_pose_info_device_ptr(vloam_handle* h, void** d_rows, long long* bytes);

/* == Per-sweep pose covariance rows (vloam_pose_cov_enable): eigenvectors, covariances and the VO solve's matrix.  An add-on of the pose
 * information product for callers that feed the poses to a filter or a pose graph, or that want to know WHICH direction a degenerate sweep
 * left unobserved.  For every sweep and session one fixed-size record holds, for the laser odometry, the mapping and the VO solve:
 *   eig, V   the eigen-decomposition of the stage's information matrix H (lo_H / map_H of the pose information row; vo_H here): eig ascending,
 *            column i of V (row-major, V[r * 6 + i]) belongs to eig[i]; in every column the component of largest magnitude is positive (ties:
 *            the lowest row), so rows are bit-identical from run to run.  f64 cyclic Jacobi on one wavefront, the three disjoint rotations of
 *            a round-robin step on different lanes at once, to the stopping rule of the pose information rows' eigenvalues.
 *   rank     eigenvalues kept by the pseudo-inverse: lambda >= max(the stage's threshold, 1e-12 lambda_max) and lambda > 0; *_TRUNCATED when < 6.
 *   sigma2   2 cost / (residual rows - rank); residual rows = 3 edge + plane blocks (odometry), 3 corner + surf blocks (mapping),
 *            2 CostFunctor32 + CostFunctor22 blocks (VO).
 *   cov      sigma2 * sum over the kept eigenvalues of v v^T / lambda, row-major, in the parameters of H: (delta theta, delta t) of
 *            EigenQuaternionParameterization for the LiDAR stages, (angle-axis, t) of cam0_curr_T_cam0_last for the VO.
 * The LiDAR halves are written by ONE one-wavefront launch per stage on the stage's own stream directly behind the pose information launch of
 * the same sweep, from the H, cost and counts that launch just wrote (no second walk over the factors).  *_VALID mirrors the pose information
 * row's valid bit; a half whose bit is clear there is all zero.
 * The VO half is written by the frame entry points (vloam_process_frame*, vloam_process_frame_image*, and the batch forms) on the stream that ran
 * the VO solve, behind it: vo_x = the returned (angles_0to1, t_0to1), vo_H = sum rho' J^T J (Huber 0.1, as solveNlsAll) over the residual blocks
 * the solve consumed, at vo_x, in that problem's own 6 parameters; vo_cost = 0.5 sum rho there; vo_factors = counter32, counter22.  VO_VALID is
 * clear and the half is zero on the first frame, on sweeps driven by vloam_process_scan* or the stage-wise calls, and when the estimate is not
 * finite or its rotation angle is zero (the case in which the reference's transform is NaN, visual_odometry.cpp:427-430).  The stage-wise
 * vloam_vo_solve does NOT write rows.
 * When residual rows - rank <= 0 there is no redundancy to estimate sigma2 from: sigma2 and cov are zero and *_VALID is clear, while eig, V,
 * rank and *_TRUNCATED (and vo_x, vo_cost, vo_H, vo_factors) still describe the problem -- a frame with a handful of VO features shows here.
 * No floating-point atomics anywhere; poses, map and the 832-byte rows are those of a handle with pose information alone.  Rows do NOT travel in
 * a checkpoint (restored sweeps read frame == -1).  Not provided: propagation of the covariance along the trajectory. */
typedef struct vloam_pose_cov_options {
  int struct_size;              /* sizeof(vloam_pose_cov_options) as compiled */
  int reserved;                 /* 0 */
  double lo_min_eigenvalue;     /* eigenvalues below this are treated as unobserved in the pseudo-inverse; 0 = only lambda <= 1e-12 * lambda_max */
  double map_min_eigenvalue;
  double vo_min_eigenvalue;
} vloam_pose_cov_options;
void vloam_default_pose_cov_options(vloam_pose_cov_options* opt);   /* struct_size set, thresholds 0 */
enum {   /* vloam_pose_cov_record::flags */
  VLOAM_POSE_COV_LO_VALID = 1, VLOAM_POSE_COV_MAP_VALID = 2, VLOAM_POSE_COV_VO_VALID = 4,           /* sigma2 and cov of that stage are set */
  VLOAM_POSE_COV_LO_TRUNCATED = 8, VLOAM_POSE_COV_MAP_TRUNCATED = 16, VLOAM_POSE_COV_VO_TRUNCATED = 32   /* rank < 6 */
};
typedef struct vloam_pose_cov_record {
  int frame;                    /* 0-based sweep index; -1 while the row has not been completed */
  int flags;                    /* VLOAM_POSE_COV_* */
  int rank[3];                  /* lo, map, vo: eigenvalues kept */
  int vo_factors[2];            /* counter32, counter22 residual blocks of the VO solve */
  int reserved;
  double sigma2[3], reserved_d;
  double lo_eig[6], lo_V[36], lo_cov[36];
  double map_eig[6], map_V[36], map_cov[36];
  double vo_x[6], vo_cost, vo_reserved, vo_H[36], vo_eig[6], vo_V[36], vo_cov[36];
} vloam_pose_cov_record;
#if defined(__cplusplus)
static_assert(sizeof(vloam_pose_cov_record) == 2288, "vloam_pose_cov_record is 8 ints and 282 doubles");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(vloam_pose_cov_record) == 2288, "vloam_pose_cov_record is 8 ints and 282 doubles");
#endif
/* vloam_pose_cov_enable: only on a handle that has already enabled pose information and has taken no sweep yet (VLOAM_ERR_ORDER otherwise, also
 *   when called twice); single-sequence and batched handles.  Allocates max_frames rows of 2288 bytes per session outside the session arenas.
 *   opt may be NULL (the defaults).  The options are checked first, before the handle is looked at: VLOAM_ERR_INVALID for a struct_size other
 *   than sizeof(vloam_pose_cov_options), a reserved other than 0, a negative, NaN or infinite threshold.
 * vloam_get_pose_cov: the rows of sweeps first .. first + count - 1 of the session chosen with vloam_select_session -> HOST buffer; waiting and
 *   range rules of vloam_get_pose_info.  VLOAM_ERR_ORDER: the handle never enabled the product.  VLOAM_ERR_INVALID: a range beyond vloam_frame_count.
 * vloam_pose_cov_device_ptr: device address + byte size of the selected session's rows; rows are only complete after vloam_sync(). */
vloam_status vloam_pose_cov_enable(vloam_handle* h, const vloam_pose_cov_options* opt);
vloam_status vloam_get_pose_cov(vloam_handle* h, int first, int count, vloam_pose_cov_record* out);
vloam_status vloam_pose_cov_device_ptr(vloam_handle* h, void** d_rows, long long* bytes);

/* == VisualOdometry::processPointCloud + solveNlsAll (visual_odometry.cpp:157-186,254-450).
 * prev_uv/curr_uv: n_match integer pixel pairs (the reference truncates keypoints to int, :283-294).
 * angle_axis/t: in = initial guess (cam0_curr_LOT_cam0_prev) unless reset_VO_to_identity, out = estimate. */
vloam_status vloam_vo_set_calib(vloam_handle* h, const vloam_calib* calib);
vloam_status vloam_vo_process_point_cloud(vloam_handle* h, const float* xyz_pad4, int n);
vloam_status vloam_vo_solve(vloam_handle* h, const int* prev_uv, const int* curr_uv, int n_match, double angle_axis[3],
                            double t[3], int counters32_22[2]);

/* ---- The coupled per-frame VLOAM loop (configs[3]): MAIN/src/vloam_main_node.cpp:125-180.
 * vloam_set_extrinsics: base_T_cam0 and velo_T_cam0 as VloamTF::processStaticTransform leaves them (vloam_tf.cpp:55-56), row-major 4x4.
 * vloam_process_frame[_device]: one callback() with no host round trip — VO->reset / LOAM->reset, processPointCloud on the sweep that is
 * already in HBM (visual_odometry.cpp:157-186), solveNlsAll for every frame but the first (initial guess = cam0_curr_LOT_cam0_prev of the
 * previous frame unless reset_VO_to_identity, :258-281), VloamTF::VO2VeloAndBase (vloam_tf.cpp:59-75), scanRegistrationIO, laserOdometryIO
 * (combined mode detach_VO_LO == 0: para_q / para_t are overwritten by velo_last_VOT_velo_curr at the top of BOTH outer rounds,
 * laser_odometry.cpp:223-236; publish() refreshes cam0_curr_LOT_cam0_prev, :563-567), laserMappingIO.  prev_uv / curr_uv: n_match integer
 * pixel pairs in HOST memory, previous frame -> this frame (the image front-end is outside this library); ignored for the first frame.
 * Like the reference, a VO solve that returns a zero rotation angle makes every later pose NaN (visual_odometry.cpp:427-430 divides by
 * it); vloam_sync() then reports VLOAM_ERR_INVALID. */
vloam_status vloam_set_extrinsics(vloam_handle* h, const double base_T_cam0[16], const double velo_T_cam0[16]);
vloam_status vloam_process_frame_device(vloam_handle* h, const void* d_xyz_pad4, int n, const int* prev_uv, const int* curr_uv, int n_match);
vloam_status vloam_process_frame(vloam_handle* h, const float* xyz_pad4, int n, const int* prev_uv, const int* curr_uv, int n_match);
/* world_VOT_base_last per frame as {q xyzw, t} (7 doubles): the VO leg next to the LO / MO legs of vloam_get_trajectory */
vloam_status vloam_get_vo_trajectory(vloam_handle* h, int first, int count, double* poses7);
/* last frame: VO estimate (angles_0to1, t_0to1), counter32 / counter22, and velo_last_VOT_velo_curr derived from it (any may be NULL) */
vloam_status vloam_get_vo_result(vloam_handle* h, double angle_axis[3], double t[3], int counters32_22[2], double prior_q[4], double prior_t[3]);

/* The ORB + brute-force configuration of VisualOdometry::processImage — optical_flow_match = false, the reference's LAUNCH DEFAULT
 * (vloam_main/launch/vloam_main.launch:10; visual_odometry.cpp:106-116): ImageUtil::descKeypoints = cv::ORB::create()->compute on the Shi-Tomasi
 * corners (image_util.cpp:162-212: border filter at 31 px, 7 x 7 Gaussian blur, the 256 steered binary tests — the provided keypoints carry
 * angle -1, which OpenCV uses as -1 degree), then ImageUtil::matchDescriptors with BF / NORM_HAMMING / 2-NN + ratio 0.8 (:214-296).
 * OpenCV's sampling pattern (modules/features2d/src/orb.cpp: bit_pattern_31_, 256 tests x (x0, y0, x1, y1)) is learned DATA of the library that
 * is not in the reference tree: the caller hands it in.  pattern_256x4 != NULL switches the handle's image front-end (all sessions) to this
 * configuration, NULL back to optical flow; not in the middle of a sequence.  vloam_vo_process_image*, vloam_process_frame_image* and the
 * batched forms then work as before; vloam_vo_get_flow_matches returns the descriptor matches' pixel pairs, vloam_vo_get_flow nothing. */
vloam_status vloam_vo_set_orb_pattern(vloam_handle* h, const signed char* pattern_256x4);
/* the keypoints of the latest image that survive ORB's border filter (what DMatch indices refer to: descKeypoints edits the caller's vector)
 * and their 32-byte descriptors */
vloam_status vloam_vo_get_descriptors(vloam_handle* h, float* xy, unsigned char* desc32, int cap, int* n);

/* ---- Image front-end of the visual odometry, optical-flow configuration (vloam_main.launch: optical_flow_match = true); needs
 * cfg.image_width / image_height > 0.  Replaces, on the device:
 *   ImageUtil::detKeypoints (ShiTomasi)   src/visual_odometry/src/image_util.cpp:13-36    cv::goodFeaturesToTrack(img, 1024, 0.03, 7.5, 5)
 *   ImageUtil::calculateOpticalFlow       src/visual_odometry/src/image_util.cpp:351-372  cv::calcOpticalFlowPyrLK(15 x 15, maxLevel = 2 i.e. three pyramid levels, 10 / 0.03)
 *   VisualOdometry::processImage          src/visual_odometry/src/visual_odometry.cpp:91-132 (the NEW image's corners are tracked from the
 *                                         previous image into the new one, :121-122)
 * vloam_vo_process_image[_device]: one 8-bit grey image (row stride in bytes); every image of a sequence has the same size.  With
 *   cfg.CLAHE = 1 the image first goes through cv::createCLAHE(2.0)->apply (visual_odometry.cpp:31,97-100), on the device.
 * vloam_vo_get_keypoints: the corners of the last image, (x, y) pairs in goodFeaturesToTrack's order.
 * vloam_vo_get_flow: for the last image, per corner: where it sits in the previous image (= the corner itself), where it was tracked to
 *   in the new image, and calcOpticalFlowPyrLK's status byte (n = 0 after the first image).
 * vloam_vo_get_flow_matches: the match loop's integer pixel pairs of the tracked corners (visual_odometry.cpp:296-308), ready for
 *   vloam_vo_solve / vloam_process_frame.
 * vloam_process_frame_image[_device]: vloam_process_frame with the matches taken from the image instead of from the caller — cloud and
 *   image of one frame in, nothing comes back to the host (the image work rides on a stream of its own next to scan registration).
 * vloam_vo_match_descriptors: ImageUtil::matchDescriptors (image_util.cpp:221-296) for binary descriptors in host memory —
 *   BFMatcher(NORM_HAMMING): knnMatch k = 2 + ratio test 0.8 (select_knn != 0, the reference's SelectType::KNN) or match with crossCheck
 *   (select_knn == 0); ties resolve like cv::batchDistance (lower index).  Matches come back in query order.
 * Of the ORB + brute-force configuration (optical_flow_match = false) only the descriptor EXTRACTION is not provided: OpenCV's learned
 * ORB sampling table cannot be restated without the library — compute the descriptors with OpenCV at the corners of
 * vloam_vo_get_keypoints and match them here. */
vloam_status vloam_vo_process_image(vloam_handle* h, const unsigned char* gray, int width, int height, int stride);
vloam_status vloam_vo_process_image_device(vloam_handle* h, const void* d_gray, int width, int height, int stride);
vloam_status vloam_vo_get_keypoints(vloam_handle* h, float* xy, int cap, int* n);
vloam_status vloam_vo_get_flow(vloam_handle* h, float* prev_xy, float* curr_xy, unsigned char* status, int cap, int* n);
vloam_status vloam_vo_get_flow_matches(vloam_handle* h, int* prev_uv, int* curr_uv, int cap, int* n);
vloam_status vloam_vo_match_descriptors(vloam_handle* h, const unsigned char* desc_prev, int n_prev, const unsigned char* desc_curr, int n_curr, int bytes_per_desc,
                                        int select_knn, int* query_idx, int* train_idx, int cap, int* n_matches);
vloam_status vloam_process_frame_image_device(vloam_handle* h, const void* d_xyz_pad4, int n, const void* d_gray, int width, int height, int stride);
vloam_status vloam_process_frame_image(vloam_handle* h, const float* xyz_pad4, int n, const unsigned char* gray, int width, int height, int stride);
/* Batched coupled frames from raw inputs (handles of vloam_create_batch with an image front-end): session b gets sweep xyz_pad4[b] and the
 * grey image gray[b]; all images of a call share width / height / stride.  The sessions' images run one after the other on the image
 * stream (each session has the image buffers of its own arena); everything behind them is the batched frame chain.  The getters
 * vloam_vo_get_keypoints / _flow / _flow_matches read the session chosen with vloam_select_session. */
vloam_status vloam_batch_process_frame_image_device(vloam_handle* h, const void* const* d_xyz_pad4, const int* n, const void* const* d_gray, int width, int height,
                                                    int stride);
vloam_status vloam_batch_process_frame_image(vloam_handle* h, const float* const* xyz_pad4, const int* n, const unsigned char* const* gray, int width, int height,
                                             int stride);

/* Parity hooks (tests only; need cfg.debug = 1 for the per-point arrays).  Copies up to cap elements of
 * the named array into buf (element type given per item) and returns the element count in *n.
 *   stage 0 (scan registration): item 0 curvature f32[N2], 1 sort order i32[N2], 2 picked i32[N2],
 *       3 label i32[N2], 4 scanStartInd i32[64], 5 scanEndInd i32[64], 6 sharp idx i32, 7 lessSharp idx i32,
 *       8 flat idx i32, 9 scalars f32{startOri,endOri,halfPassedAt,n_after_s1,N2}
 *   stage 1 (laser odometry, item = outer*16 + k): k=0 corner corr i32[n][3] (i,a,b; -1 = none),
 *       1 plane corr i32[n][4], 2 LM record f64 (see vloam_device.h LMRecord), 3 per-factor residuals f64
 *   stage 2 (laser mapping, same k layout; corr rows are f64 geometry: corner a,b[6] / plane n,d[4] / flag)
 *   stage 3 (VO): 0 buckets, 1 per-match rows, 2 LM record */
vloam_status vloam_debug_get(vloam_handle* h, int stage, int item, void* buf, long long cap_bytes, long long* n_bytes);

/* Test hook: the shared device primitives on caller-supplied arguments (dev_probe.hip; tests/test_gpu_dev_probe.py compares the results with
 * the host build of the same headers bit for bit).  `in` and `out` are HOST pointers to n elements in the layout of the probe; out_bytes
 * must be exactly n * (the probe's output element size).  The call needs no handle: it allocates, copies, launches one trivially parallel
 * kernel on a stream of its own, synchronises and frees.  An unknown `which`, n < 0, a null pointer with n > 0 or a wrong out_bytes returns
 * VLOAM_ERR_INVALID before anything is allocated or launched; n == 0 returns VLOAM_OK the same way.
 *   which                      in (per element)                 out (per element)        calls
 *   VLOAM_PROBE_ATANF          f32 x                            f32                      fd_atanf(x)
 *   VLOAM_PROBE_ATAN2F         f32 y, x                         f32                      fd_atan2f(y, x)
 *   VLOAM_PROBE_ELEV           f32 x, y, z                      f32                      fd_atanf(z / sqrtf(x * x + y * y))
 *   VLOAM_PROBE_TF_ROUNDTRIP   f64 q[4] (xyzw, any norm)        f64 m[9], q[4]           tf_set_rotation, tf_get_rotation of the result
 *   VLOAM_PROBE_TF_GETROT      f64 m[9] (any matrix)            f64 q[4]                 tf_get_rotation
 *   VLOAM_PROBE_TF_CHAIN       f64 a.m[9], a.o[3], b.m, b.o     f64 m[9], o[3]           tf_mul(a, tf_inverse(b))
 *   VLOAM_PROBE_ASSOC          f32 p[4]; f64 q[4], t[3] (72 B)  f32 [4]                  associate_to_map(p, q, t)
 *   VLOAM_PROBE_QUAT           f64 a[4], b[4], v[3]             f64 r[4], o[3]           dquat_mul(a, b), dquat_rot(a, v)
 *   VLOAM_PROBE_SORT(P2, T)    u64 [P2]: one problem            u64 [P2], ascending      block_bitonic_sort_u64(a, P2, tid, T), one workgroup of
 *                                                                                        T lanes per problem; only the (P2, T) pairs the
 *                                                                                        library's own kernels use (the table in dev_probe.hip) */
enum {
  VLOAM_PROBE_ATANF = 1, VLOAM_PROBE_ATAN2F = 2, VLOAM_PROBE_ELEV = 3, VLOAM_PROBE_TF_ROUNDTRIP = 4, VLOAM_PROBE_TF_GETROT = 5,
  VLOAM_PROBE_TF_CHAIN = 6, VLOAM_PROBE_ASSOC = 7, VLOAM_PROBE_QUAT = 8
};
#define VLOAM_PROBE_SORT(P2, T) (0x40000000 | ((T) << 16) | ((P2) >> 4))   /* P2 <= 16384, a multiple of 256; T 256 or 512 */
vloam_status vloam_debug_probe(int device, int which, const void* in, long long n, void* out, long long out_bytes);

/* Per-kernel HIP-event timer for bench.py's roofline line: brackets every launch of the kernel whose __global__
 * symbol is `name` (e.g. "k_lo_assoc") with an event pair on the handle's own stream.  "" disables.
 * vloam_profile_read returns the summed milliseconds and launch count since the last read. */
vloam_status vloam_profile_kernel(vloam_handle* h, const char* name, int max_launches);
vloam_status vloam_profile_read(vloam_handle* h, double* total_ms, int* launches);
/* name "*" brackets every launch of every kernel; vloam_profile_read_table then returns the per-kernel sums, ms[k] / launches[k]
 * for kernel id k < n_kernels (ids 0..vloam_profile_kernel_count()-1, symbol names through vloam_profile_kernel_name).  This is
 * also where the reference's per-substage timers map to ("sort q time" / "seperate points" -> k_sr_ring,
 * "data association" -> k_lo_assoc / k_map_assoc + k_map_fit, "solver time" -> k_lm_compact + k_lm_solve,
 * "build tree" -> k_lo_grid_*, "filter time" -> k_map_ds_*, "add points" -> k_map_insert + k_map_finalize). */
vloam_status vloam_profile_read_table(vloam_handle* h, int n_kernels, double* ms, int* launches);
int vloam_profile_kernel_count(void);
const char* vloam_profile_kernel_name(int k);

/* Health counters (synchronises): out8[0] cooperative Levenberg-Marquardt solves that found their partner workgroups missing and finished on ONE
 * workgroup instead (same factors, same trust-region loop; the pose agrees with the cooperative form to round-off, the solve is ~0.5 s late
 * because the workgroup first waited for its partners), summed over the sessions; out8[1] 1 once the handle has reacted to that by launching
 * one-workgroup solves only (vloam_sync does, see the co-residency note at vloam_create_batch); out8[2] voxel-table rebuilds; on a growable handle
 * (vloam_map_options::grow) out8[3] growth steps enqueued so far (both tables) and out8[4], out8[5] the current log2 of the corner and the surf
 * table, 0 on any other handle; out8[6..7] 0. */
vloam_status vloam_get_health(vloam_handle* h, long long out8[8]);

/* Checkpoint and restore: a sequence saved into host memory and resumed in another handle (another process, another GPU, other capacities).
 * vloam_checkpoint_size / _save first enqueue whatever the handle still owes (a deferred host sweep, trailing odometry and mapping) and
 *   synchronise.  _size: the exact size of a checkpoint taken now.  _save: writes it into buf; *bytes is always the true size; cap smaller than
 *   that: VLOAM_ERR_CAPACITY, nothing written.  Neither changes the handle: the next sweeps produce byte-identical results.
 * vloam_checkpoint_load: on a FRESH single-sequence handle (vloam_frame_count == 0, stage 0; VLOAM_ERR_ORDER otherwise).  Afterwards the handle
 *   is the saved sequence at the saved sweep: vloam_frame_count, vloam_get_trajectory(0 .. frames - 1), vloam_get_map, vloam_get_features(5 .. 8)
 *   and vloam_get_odometry_pose return what the saving handle returned, and every later sweep produces what the uninterrupted handle would have.
 *   The capacities may differ from the saver's (map_capacity_log2, fixed or growable, max_frames, max_points, max_ring_points,
 *   max_surf_stack_points, the publication options, sweep_log); the algorithmic parameters must be equal: scan_line, minimum_range,
 *   mapping_skip_frame, mapping_line_resolution, mapping_plane_resolution, detach_VO_LO, with_mapping (VLOAM_ERR_INVALID, vloam_last_error() names
 *   the field) — and both handles or neither must have the large stack tier (max_surf_stack_points > 24576: the arrival stamps of raw points
 *   have another width there; VLOAM_ERR_INVALID).  VLOAM_ERR_CAPACITY, naming what is too small: more frames than max_frames, clouds larger
 *   than max_points / the stack capacity, or — on a fixed handle — more live records or block keys than 60 % of a table's slots; a growable
 *   handle first takes a table size under which its own growth bound holds, up to its ceiling.  The buffer is validated in full (magic, format
 *   version, struct sizes, checksum, every section offset, length and record count) before any device call: VLOAM_ERR_INVALID; nothing outside
 *   [buf, buf + bytes) is read.  On every refusal the handle stays fresh and usable.
 * A checkpoint is for the SAME BUILD of the library (it stores device structs verbatim).  Its size does not depend on map_capacity_log2: the map
 * travels as its live records, 32 bytes each.
 * Not supported, each refused with its own message: handles with n_sessions > 1 (VLOAM_ERR_INVALID); a sequence that used a VO, frame or image
 * entry point — the VO's previous-frame state is not saved (VLOAM_ERR_ORDER from size / save); a handle in the middle of a stage-wise sweep
 * (VLOAM_ERR_ORDER); a handle whose vloam_sync reports a sticky error (size / save return that error).
 * What does not travel: the publication buffers (after load it is "before the first publication": *n = 0, *frame = -1; the map_pub_number
 * schedule continues from the restored mapped-sweep count); the health counters (out8[0..3] start at 0); vloam_get_features(0 .. 4, 11) of the
 * last sweep; sweep-log rows 0 .. frames - 1 travel when both handles keep a log, otherwise the rows of restored sweeps read frame == -1;
 * the place database (vloam_place_enable: a restored handle is not enabled and holds no rows — carry them with vloam_place_get / _load). */
vloam_status vloam_checkpoint_size(vloam_handle* h, long long* bytes);
vloam_status vloam_checkpoint_save(vloam_handle* h, void* buf, long long cap, long long* bytes);
vloam_status vloam_checkpoint_load(vloam_handle* h, const void* buf, long long bytes);

/* Map queries: the k nearest map points of caller-supplied points, answered on the device from the map's own occupancy-block index.  Opt-in by
 * calling: a handle that never queries allocates and launches nothing of this, and no kernel of a sweep changes.
 *   Query points are packed float4 (w ignored) in the MAP frame — the frame of vloam_get_map and of the registered cloud, so
 *   vloam_published_device_ptr(h, 1, ...) can be fed straight in.  The searched set is exactly what vloam_get_map returns at that moment for the
 *   session chosen with vloam_select_session (kind 0: its corner clouds, 1: its surf clouds, 2: both).  Per query q: count[q] in 0 .. k;
 *   neighbour j < count[q] at xyzi4[q*k + j] with squared distance d2[q*k + j], ascending; entries j >= count[q] are zero.
 *   d2 = (dx*dx + dy*dy) + dz*dz in f32, every product and sum rounded on its own (no FMA); a neighbour qualifies when d2 <= max_radius*max_radius
 *   (f32 product); equal d2 resolve to the point that comes first in vloam_get_map.  A query with a non-finite coordinate, or far outside the
 *   map, returns count 0 and no error.
 * Ordering: both calls first enqueue what the handle still owes (a deferred host sweep, trailing odometry and mapping); the query runs on the
 *   mapping stream behind the last mapping (and any growth step of a growable handle).  vloam_map_query works with temporary allocations,
 *   waits for the mapping stream only, and then returns a sticky map error of the handle (the one vloam_sync reports) instead of VLOAM_OK.
 *   vloam_map_query_device enqueues and returns: all five addresses are device memory, results are complete after vloam_sync, and the buffers must
 *   stay valid until then.
 * Refusals, options first and before the handle is looked at (VLOAM_ERR_INVALID, each with its own vloam_last_error()): struct_size, kind
 *   outside 0 .. 2, k outside 1 .. 8, reserved != 0, a radius that is <= 0 or not finite, a null buffer with n > 0, n < 0.  Then against the
 *   handle: a radius above 16 leaves of the finest kind queried (mapping_line_resolution for 0 and 2, mapping_plane_resolution for 1:
 *   VLOAM_ERR_INVALID naming the bound in metres); with_mapping == 0 (VLOAM_ERR_ORDER).  n == 0: VLOAM_OK, nothing launched.
 * Not offered: queries in the sensor frame; points outside the 21 x 21 x 11 cube window (they are not part of the map). */
typedef struct vloam_map_query_options {
  int struct_size;     /* sizeof as compiled */
  int kind;            /* 0 corner map, 1 surf map, 2 both (nearest over the union) */
  int k;               /* 1 .. 8 neighbours per query */
  int reserved;        /* 0 */
  float max_radius;    /* metres, > 0, finite; <= 16 leaves of the finest kind queried */
} vloam_map_query_options;
void vloam_default_map_query_options(vloam_map_query_options* o);   /* kind 2, k 5, radius 1.0 */
vloam_status vloam_map_query(vloam_handle* h, const vloam_map_query_options* o, const float* xyz_pad4, int n, float* xyzi4, float* d2, int* count);
vloam_status vloam_map_query_device(vloam_handle* h, const vloam_map_query_options* o, const void* d_xyz_pad4, int n, void* d_xyzi4, void* d_d2,
                                    void* d_count);
/* The corner (kind 0) or surf (kind 1) half of vloam_get_map, same order within the half; same calling convention. */
vloam_status vloam_get_map_kind(vloam_handle* h, int kind, float* xyzi4, long long cap, long long* n);

/* Localisation: a dry run of LaserMapping::input + solveMapping (laser_mapping.cpp:167-196, 198-636) against the map as it is.  It stops in
 * front of the map update (laser_mapping.cpp:637 onwards) and returns the pose the mapping would have reported; nothing the sequence can see
 * changes: no odometry row is consumed, the cube window does not roll, no voxel is inserted, q_wmap_wodom stays, no trajectory / sweep-log /
 * pose-information row is written, and the handle's sticky error words are not touched.  Opt-in by calling: the scratch state (its own
 * MapState, counters, stacks, factor tables, candidate cache) is allocated by the first call, outside the session arena, and freed by
 * vloam_destroy; a handle that never localises allocates and launches nothing of this, and no kernel of a sweep changes.
 *   Clouds: what vloam_set_mapping_input takes as laserCloudCornerLast / laserCloudSurfLast — packed (x, y, z, intensity) in the sensor frame,
 *   at most 7680 corner points and max_points surf points, every float finite (the host form checks; the device form trusts its caller).
 *   (q, t): pose_frame 0 — an odometry-frame pose q_wodom_curr / t_wodom_curr; the guess is formed with the handle's current q_wmap_wodom /
 *   t_wmap_wodom exactly as LaserMapping::input does (laser_mapping.cpp:182-195).  pose_frame 1 — the guess itself, in the map frame.
 *   corner == NULL && surf == NULL: the sweep in progress, between vloam_laser_odometry and vloam_laser_mapping of a stage-wise sweep — the
 *   stacks the real mapping will consume (clouds handed to vloam_set_mapping_input included), read-only; with q == NULL && t == NULL also that
 *   sweep's odometry pose (pose_frame is then ignored: it is an odometry pose).  The record's q_map / t_map are then bit for bit what the
 *   vloam_laser_mapping that follows returns.
 * Ordering: both calls first enqueue what the handle still owes; the chain runs on the mapping stream behind the last mapping (and any growth
 *   step of a growable handle).  vloam_map_localize waits for that stream only, copies the record out, and then returns a sticky map error of
 *   the handle (the one vloam_sync reports) instead of VLOAM_OK.  vloam_map_localize_device enqueues and returns: d_corner, d_surf and d_result
 *   (sizeof(vloam_localize_result) bytes) are device memory, the record is complete after vloam_sync, the buffers must stay valid until then.
 * Refusals, options first and before the handle is looked at (VLOAM_ERR_INVALID, each with its own vloam_last_error()): struct_size,
 *   pose_frame outside 0 .. 1, reserved != 0, only one of the two clouds null, a null pose with non-null clouds (or only one of q, t null), a
 *   negative count, more than 7680 corner or 16777216 surf points, a null result, a non-finite float or pose component, a quaternion whose
 *   norm is off 1 by more than 1e-6.  Then the handle: with_mapping == 0 (VLOAM_ERR_ORDER); n_sessions > 1 (VLOAM_ERR_INVALID); a handle of
 *   the large stack tier (VLOAM_ERR_INVALID, "not offered"); more surf points than max_points (VLOAM_ERR_CAPACITY); null clouds outside the
 *   odometry-to-mapping window of a stage-wise, mapped sweep (VLOAM_ERR_ORDER).
 * Not offered: batched handles, the large stack tier, raw sweeps as input (run vloam_scan_registration on a second handle with
 *   with_mapping == 0 and take vloam_get_features(h, 2) / (h, 4)), information matrices of a localisation.  Several hypotheses per launch:
 *   vloam_map_score_poses scores them, vloam_map_relocalize refines the best few with this chain (below). */
enum {
  VLOAM_LOC_SOLVED = 1,          /* both outer rounds ran their solve */
  VLOAM_LOC_NOT_OPTIMIZED = 2,   /* "Map corner and surf num are not enough" (laser_mapping.cpp:448,631-635): q_map / t_map == q_guess / t_guess */
  VLOAM_LOC_WOULD_ROLL = 4,      /* a mapping at this pose would have shifted the cube window */
  VLOAM_LOC_DEGRADED = 8         /* a cooperative solve of this call fell back to one workgroup */
};
typedef struct vloam_localize_options {
  int struct_size;     /* sizeof as compiled */
  int pose_frame;      /* 0: (q, t) is an odometry-frame pose; 1: (q, t) is the guess itself, in the map frame */
  int reserved[2];     /* 0 */
} vloam_localize_options;
typedef struct vloam_localize_result {   /* 216 bytes: 18 ints (the last one padding), then 18 doubles */
  int flags;                       /* VLOAM_LOC_* */
  int error_bits;                  /* VLOAM_SWEEP_* bits this call raised on its own scratch (STACK_FULL, DS_TIMEOUT, MAP_FULL, MAP_RAW_CAPACITY) */
  int center_cube[3];              /* laserCloudCen{Width,Height,Depth} indices of the pose's cube in the (would-be shifted) window */
  int n_stack[2], n_map[2];        /* scan features after VoxelGrid; map points in the valid 5x5x3 block (laser_mapping.cpp:404-430) */
  int n_factors[2][2];             /* [round][corner, surf] */
  int iterations[2], termination[2];
  int pad;
  double q_guess[4], t_guess[3];   /* the pose the solve started from */
  double q_map[4], t_map[3];       /* what vloam_laser_mapping would have returned */
  double initial_cost[2], final_cost[2];
} vloam_localize_result;
void vloam_default_localize_options(vloam_localize_options* o);   /* pose_frame 0 */
vloam_status vloam_map_localize(vloam_handle* h, const vloam_localize_options* o, const float* corner_xyzi4, int n_corner, const float* surf_xyzi4,
                                int n_surf, const double q[4], const double t[3], vloam_localize_result* out);
vloam_status vloam_map_localize_device(vloam_handle* h, const vloam_localize_options* o, const void* d_corner, int n_corner, const void* d_surf,
                                       int n_surf, const double q[4], const double t[3], void* d_result);

/* Pose scores: M candidate poses of one sweep's feature clouds scored against the map in one launch, and on top of them a coarse-to-fine
 * relocalisation — for a caller who knows only roughly where the sensor is.  Opt-in by calling: a handle that never scores allocates and
 * launches nothing of this, and no kernel of a sweep changes.
 *   Clouds: what vloam_map_localize takes — packed (x, y, z, intensity) in the SENSOR frame, at most 7680 corner and 16777216 surf points.
 *   Poses: q4t3[m] = (q xyzw, t) in the MAP frame, f64.  Per kind (0 corner, 1 surf) a radius and a point stride s >= 1: points 0, s, 2s, ...
 *   Per pose m, kind and used point i: p = q_m * point_i + t_m as pointAssociateToMap computes it (Eigen q * v in f64, + t, each component
 *   rounded to f32); the searched set is vloam_get_map_kind(h, kind) at that moment (corner points against the corner map, surf points
 *   against the surf map); d2 = (dx*dx + dy*dy) + dz*dz in f32, every product and sum rounded on its own, as vloam_map_query defines it; dmin
 *   the smallest d2 over the set; the point is a HIT when dmin <= radius*radius (f32 product).  A p with a non-finite component, or one beyond
 *   +-1e6, is no hit and no error.  Record m: n_hit[kind], n_used[kind] (points of the kind that were scored, the same for every pose) and
 *   sum_d2_q24[kind], the sum over the hits of (unsigned long long)(dmin * 16777216.0f) — an exact scaling and a truncation.  Hits and sums
 *   are integers and accumulate as integers: a record is a function of the inputs alone, bit for bit from run to run.
 *   Ranking, wherever a best pose is chosen: more hits (both kinds added) first, then the smaller sum (both kinds added), then the smaller index.
 * Ordering: as vloam_map_query — both calls first enqueue what the handle still owes and run on the mapping stream behind the last mapping
 *   (and any growth step).  vloam_map_score_poses works with temporary allocations, waits for that stream only and then returns a sticky map
 *   error of the handle instead of VLOAM_OK; vloam_map_score_poses_device enqueues and returns: the four addresses are device memory (d_out: M
 *   records), complete after vloam_sync, valid until then.
 * Refusals, before the handle is looked at (VLOAM_ERR_INVALID, each with its own vloam_last_error()): null options or struct_size,
 *   reserved != 0, a stride < 1, a radius that is <= 0 or not finite, a negative count, M < 0 or M > 65536, more than 7680 corner or 16777216
 *   surf points, a null buffer with a positive count; host form only: a non-finite float in a cloud, a non-finite pose component, a quaternion
 *   whose norm is off 1 by more than 1e-6 (the device form trusts its caller).  Then the handle: a radius above 16 leaves of its kind
 *   (VLOAM_ERR_INVALID naming the bound in metres); with_mapping == 0 (VLOAM_ERR_ORDER); n_sessions > 1 (VLOAM_ERR_INVALID).  M == 0:
 *   VLOAM_OK, nothing launched; both clouds empty: records of zeros.
 * vloam_map_relocalize: candidates on a grid around (q_center, t_center) — index m = ix + n_xy[0]*(iy + n_xy[1]*(iz + n_z*iyaw)); the offset
 *   along an axis with n steps and half extent e is -e + 2*e*i/(n-1) (0 when n == 1); t = t_center + (dx, dy, dz) along the map's axes,
 *   q = q_yaw * q_center with q_yaw = (0, 0, sin(a/2), cos(a/2)), all f64 on the host; 1 <= n_candidates <= 65536.  The call scores every
 *   candidate (coarse), takes the top_k by the ranking (candidate[j], coarse[j]), runs vloam_map_localize with pose_frame 1 from each
 *   (refined[j] is what that call returns for that guess), scores the refined poses once more (fine[j]) and sets best to the first of the
 *   ranking of fine[].  Synchronous, host clouds only; every refusal of vloam_map_localize and of vloam_map_score_poses applies (a handle of
 *   the large stack tier can score but not relocalise).  Nothing the sequence can see changes, as with vloam_map_localize.
 * Not offered: batched handles, scores in the odometry frame, roll and pitch in the grid, scores weighted by fit quality, a search with no
 *   centre (vloam_place_query below supplies one), starting a live sequence from the result in one call (vloam_map_import with the refined pose does that on a fresh handle). */
typedef struct vloam_score_options {
  int struct_size;     /* sizeof as compiled */
  int stride[2];       /* [corner, surf] every stride-th point is scored, >= 1 */
  int reserved;        /* 0 */
  float radius[2];     /* [corner, surf] metres, > 0, finite; <= 16 leaves of the kind */
} vloam_score_options;
typedef struct vloam_pose_score {   /* 32 bytes */
  int n_hit[2];                       /* [corner, surf] */
  int n_used[2];                      /* points scored per kind */
  unsigned long long sum_d2_q24[2];   /* sum over the hits of (unsigned long long)(dmin * 2^24) */
} vloam_pose_score;
void vloam_default_score_options(vloam_score_options* o);   /* stride 1, 1; radius 1.0, 1.0 */
vloam_status vloam_map_score_poses(vloam_handle* h, const vloam_score_options* o, const float* corner_xyzi4, int n_corner, const float* surf_xyzi4,
                                   int n_surf, const double* q4t3, int M, vloam_pose_score* out);
vloam_status vloam_map_score_poses_device(vloam_handle* h, const vloam_score_options* o, const void* d_corner, int n_corner, const void* d_surf,
                                          int n_surf, const void* d_q4t3, int M, void* d_out);
typedef struct vloam_relocalize_options {   /* 88 bytes */
  int struct_size;          /* sizeof as compiled */
  int n_xy[2], n_z, n_yaw;  /* steps per axis, >= 1; their product is 1 .. 65536 */
  int top_k;                /* 1 .. 8 candidates refined */
  int reserved[2];          /* 0 */
  double half_extent[3];    /* metres, >= 0: the grid spans t_center -+ half_extent */
  double half_yaw;          /* radians, 0 .. pi */
  vloam_score_options score;
} vloam_relocalize_options;
typedef struct vloam_relocalize_result {   /* 2288 bytes */
  int n_candidates, n_refined, best /* index into the arrays below */, pad;
  int candidate[8];                    /* grid index of the j-th best candidate */
  vloam_pose_score coarse[8];          /* its score */
  vloam_localize_result refined[8];    /* vloam_map_localize from it (q_guess / t_guess: the candidate) */
  vloam_pose_score fine[8];            /* the score of refined[j].q_map / t_map */
} vloam_relocalize_result;
void vloam_default_relocalize_options(vloam_relocalize_options* o);   /* 9 x 9 x 1 x 9 steps over +-2 m, +-10 degrees; top_k 4; default score options */
vloam_status vloam_map_relocalize(vloam_handle* h, const vloam_relocalize_options* o, const float* corner_xyzi4, int n_corner, const float* surf_xyzi4,
                                  int n_surf, const double q_center[4], const double t_center[3], vloam_relocalize_result* out);

/* Place recognition: a rotation-tolerant descriptor of one sweep, a database of such descriptors kept on the device, and a match of one
 * descriptor against every row at every yaw shift in one launch — the centre vloam_map_relocalize asks for when the caller has none, and
 * loop detection's "have I been here before, and at which sweep?".  Opt-in: a handle that never calls vloam_place_enable allocates and
 * launches nothing of this, and no kernel of a sweep changes; nothing here reads or writes what a sequence owns (works with
 * with_mapping == 0 as well).  Everything is enqueued on the handle's scan-registration stream; no stream is created.
 *   Descriptor (geometry: vloam_place_options).  Input: a sweep as vloam_process_scan_device takes it — packed float4 in the SENSOR frame, w
 *   ignored, n <= 16777216.  A point is used when x, y, z are finite and min_range^2 <= r2 < max_range^2, r2 = x*x + y*y in f32 with every
 *   operation rounded on its own, the two squares f32 products.  Ring: the number of i in 1 .. R-1 with r2 >= edge2[i], edge2[i] the f32
 *   square of (float)((float)i * w), w = max_range / (float)R (a host table: no square root on the device).  Sector:
 *   min(S-1, (int)floorf((atan2f(y, x) + PI_F) * k)), atan2f glibc's, PI_F = 0x40490fdb, k = (float)S / (2 * PI_F) in f32.  Height:
 *   q = min(254, max(0, (int)floorf((z - z_min) / z_step))) + 1, an f32 divide: 1 .. 255, 0 an empty cell.  A cell holds the largest q of
 *   its points (integer maxima: order-free).  Packed: sector-major bytes desc[sector][ring], the rings of a sector padded with zero bytes
 *   to W = ceil(R/4) little-endian words, S*W words per descriptor.  info2: n_used (points that passed the filters; -1 for a row that came
 *   through vloam_place_load) and n_occupied (non-zero cells).
 *   Distance: dist(Q, D, s) = sum over sector j and ring i of |Q[(j + s) mod S][i] - D[j][i]|; best(Q, D) the smallest over s = 0 .. S-1,
 *   ties to the smallest s.  Rows rank by dist ascending, then row index ascending; rows with index >= count - exclude_last are skipped.
 *   All integers: records are bit for bit a function of the inputs, from run to run.
 *   Yaw convention: when the query's content is the row's content turned by +m sectors in the sensor frame (a point at azimuth a in the
 *   row's sweep lies at a + m*2pi/S in the query's), the match has shift == m, and the query sensor's heading is the row's turned by
 *   -shift*2pi/S about z: q_query ~= q_row * Rz(-shift*2pi/S), Rz(a) = (0, 0, sin(a/2), cos(a/2)).
 * vloam_place_enable: once per handle (a second call: VLOAM_ERR_ORDER); allocates capacity rows (S*W*4 + 20 bytes each) and the scratch,
 *   freed by vloam_destroy.  vloam_place_describe: the descriptor of a cloud, the database untouched (info2 may be null).
 *   vloam_place_add: describe and append; tag is the caller's (e.g. the sweep's frame index); *row_out (may be null) the row's index, known
 *   when the call returns; a full database: VLOAM_ERR_CAPACITY, unchanged.  vloam_place_get: rows first .. first + count - 1 copied out
 *   (tags, info2 may be null).  vloam_place_load: appends rows made elsewhere — how a database travels; pad bytes must be zero
 *   (VLOAM_ERR_INVALID), more rows than fit: VLOAM_ERR_CAPACITY, unchanged.  vloam_place_query*: the k best rows as vloam_place_match
 *   records, unused places row == -1 and the rest zero; an empty or fully excluded database: VLOAM_OK, every row == -1.
 *   Host forms wait for that one stream only.  Device forms (_device: the cloud, and for describe / query the outputs, are device
 *   addresses) enqueue and return; results are complete after vloam_sync and the buffers must stay valid until then.
 * The database is NOT part of a checkpoint (vloam_checkpoint_save): carry it with vloam_place_get / vloam_place_load.
 * Refusals, options first and before the handle is looked at (VLOAM_ERR_INVALID, each with its own vloam_last_error()): null options or
 *   struct_size, reserved != 0, n_ring outside 1 .. 32, n_sector outside 1 .. 120, capacity outside 1 .. 1048576, a max_range or z_step
 *   that is not finite and positive, a z_min that is not finite, a min_range that is negative or not finite, min_range >= max_range; k
 *   outside 1 .. 8, exclude_last < 0; a negative count, n > 16777216, a null buffer with a positive count, a null result.  Then the
 *   handle: null (VLOAM_ERR_INVALID); n_sessions > 1 (VLOAM_ERR_INVALID, "not offered"); any call but vloam_place_enable on a handle that
 *   was not enabled (VLOAM_ERR_ORDER).
 * Not offered: batched handles; automatic appends from inside the sweep pipeline; cosine or learned distances; roll or pitch tolerance; a
 *   pose graph or any correction of the trajectory. */
typedef struct vloam_place_options {   /* 36 bytes */
  int struct_size;     /* sizeof as compiled */
  int n_ring;          /* R, 1 .. 32; default 20 */
  int n_sector;        /* S, 1 .. 120; default 60 */
  int capacity;        /* database rows, 1 .. 1048576; default 16384 */
  float min_range;     /* metres; 0: the handle's minimum_range */
  float max_range;     /* metres; default 80 */
  float z_min;         /* metres; default -3 */
  float z_step;        /* metres; default 0.05 */
  int reserved;        /* 0 */
} vloam_place_options;
typedef struct vloam_place_query_options {
  int struct_size;     /* sizeof as compiled */
  int k;               /* 1 .. 8 matches */
  int exclude_last;    /* >= 0: the youngest rows are skipped */
  int reserved;        /* 0 */
} vloam_place_query_options;
typedef struct vloam_place_match {   /* 32 bytes */
  int row, tag, shift, dist;
  int n_occupied_query, n_occupied_row;
  int pad[2];
} vloam_place_match;
void vloam_default_place_options(vloam_place_options* o);               /* 20 rings, 60 sectors, 16384 rows, 0 / 80 m, -3 m, 0.05 m */
void vloam_default_place_query_options(vloam_place_query_options* o);   /* k 1, exclude_last 0 */
vloam_status vloam_place_enable(vloam_handle* h, const vloam_place_options* o);
vloam_status vloam_place_describe(vloam_handle* h, const float* xyzi4, int n, unsigned int* desc_words, int* info2);
vloam_status vloam_place_describe_device(vloam_handle* h, const void* d_xyzi4, int n, void* d_desc_words, void* d_info2);
vloam_status vloam_place_add(vloam_handle* h, const float* xyzi4, int n, int tag, int* row_out);
vloam_status vloam_place_add_device(vloam_handle* h, const void* d_xyzi4, int n, int tag, int* row_out);
vloam_status vloam_place_count(vloam_handle* h, int* count);
vloam_status vloam_place_get(vloam_handle* h, int first, int count, unsigned int* desc_words, int* tags, int* info2);
vloam_status vloam_place_load(vloam_handle* h, const unsigned int* desc_words, const int* tags, int count);
vloam_status vloam_place_query(vloam_handle* h, const vloam_place_query_options* o, const float* xyzi4, int n, vloam_place_match* matches);
vloam_status vloam_place_query_device(vloam_handle* h, const vloam_place_query_options* o, const void* d_xyzi4, int n, void* d_matches);
vloam_status vloam_place_query_descriptor(vloam_handle* h, const vloam_place_query_options* o, const unsigned int* desc_words, vloam_place_match* matches);
/* Measurement hook (tools/place_probe.py): the match of vloam_place_query_descriptor launched `repeats` (1 .. 1024) times back to back, each
 * bracketed by HIP events on the stream; ms[r] the device milliseconds of repeat r (match + top-k launches, no copies).  Synchronous. */
vloam_status vloam_place_time_query(vloam_handle* h, const vloam_place_query_options* o, const unsigned int* desc_words, int repeats, float* ms);

/* Map import: a FRESH handle is given two point clouds in the map frame — the corner map and the surf map, packed (x, y, z, intensity), e.g. what
 * vloam_get_map_kind(h, 0 / 1) of any build of the library returned — and the map<-odometry transform the sequence starts with.  Afterwards it
 * behaves like a handle that built that map itself: vloam_map_query, vloam_map_localize, the publications, checkpoints and ordinary sweeps work.
 * Opt-in by calling: a handle that never imports allocates and launches nothing of this, and no kernel of a sweep changes.
 *   1. The 21 x 21 x 11 cube window is placed for a sensor at t_wmap_wodom by the six shift loops of LaserMapping::solveMapping
 *      (laser_mapping.cpp:207-402); every cube is still empty, so only laserCloudCen{Width,Height,Depth} and the centre cube change.
 *   2. q_wmap_wodom / t_wmap_wodom are set, and the mapping's pose to that transform composed with the identity odometry pose
 *      (laser_mapping.cpp:182-195).  The sweep count, vloam_frame_count and the trajectory stay at zero: the first sweep is sweep 0, its
 *      odometry pose the identity, its mapping guess the imported transform.
 *   3. Every point whose four floats are finite gets the cube and the voxel the mapping's own insert would give that map-frame point at its
 *      kind's leaf (mapping_line_resolution / mapping_plane_resolution; laser_mapping.cpp:643-659).  A point whose cube lies outside the placed
 *      window (or outside the voxel key's range) is dropped and counted in n_outside_window.
 *   4. All points of a kind that share a voxel become ONE map point: their f32 sum in INPUT order, every component divided by (float)n — per
 *      cube, what the reference holds after appending the points and running that cube's VoxelGrid filter once (laser_mapping.cpp:689-702).
 *      Every cube is filtered, inside the valid 5 x 5 x 3 block or not: an import leaves no un-merged points.  A cloud with one point per voxel
 *      (a vloam_get_map_kind export whose points do not sit on a voxel face) comes back from vloam_get_map_kind bit for bit, in order.
 *   5. The per-cube point counts, the occupancy blocks and the table counters are what a handle holds that inserted those points itself.
 *   The result is a function of the two arrays and the options alone, bit for bit from run to run (no floating-point atomics).
 * Both forms run on the mapping stream with temporary allocations only, wait for that stream, and free them before they return.  The device form
 *   takes device addresses (clouds and a vloam_map_import_result) and drops non-finite points, counted in n_nonfinite, where the host form refuses them.
 * Refusals, options first and before the handle is looked at (VLOAM_ERR_INVALID, each with its own vloam_last_error()): null options,
 *   struct_size, reserved != 0, a non-finite component of q or t, a quaternion whose norm is off 1 by more than 1e-6, a negative count, more
 *   than 16777216 points of a kind, a null cloud with a positive count, a null result, host form only: a non-finite float in a cloud.  Then the
 *   handle: with_mapping == 0 (VLOAM_ERR_ORDER); n_sessions > 1 (VLOAM_ERR_INVALID); not fresh — vloam_frame_count != 0, a sweep handed over, a
 *   stage-wise sweep in progress, a checkpoint loaded or an earlier import (VLOAM_ERR_ORDER).  On every such refusal the handle stays fresh and
 *   usable.  Both clouds empty: VLOAM_OK, only the window and the start pose are set.
 * Capacity: a growable handle (vloam_map_options::grow) first steps its empty tables to the size its growth bound asks for with the point count
 *   of each kind as the bound on records, as vloam_checkpoint_load does.  A fixed handle cannot be refused up front — how many DISTINCT voxels
 *   the clouds hold is known only after keying: when they exceed 60 % of a table's slots (or a probe chain reaches its bound) the call returns
 *   VLOAM_ERR_CAPACITY naming the table, the handle carries the sticky map-full error a sweep would have raised (vloam_sync reports it) and is
 *   finished, as after such a sweep.
 * Not offered: batched handles; importing into a handle that has taken sweeps (vloam_map_merge below folds clouds into a live map); un-merged raw points (an export that
 *   holds several points of one voxel comes back as their centroid); normals, covariances or any per-point attribute beyond intensity. */
typedef struct vloam_map_import_options {
  int struct_size;            /* sizeof as compiled */
  int reserved[3];            /* 0 */
  double q_wmap_wodom[4];     /* (x, y, z, w), unit within 1e-6; default identity */
  double t_wmap_wodom[3];     /* default 0: where the odometry frame's origin (the first sweep) lies in the map */
} vloam_map_import_options;
typedef struct vloam_map_import_result {   /* 88 bytes: 8 long long, then 6 ints */
  long long n_in[2], n_voxels[2];      /* [corner, surf]: points given, map points (voxel records) created */
  long long n_outside_window[2];       /* dropped: cube outside the placed 21 x 21 x 11 window (or outside the key range) */
  long long n_nonfinite[2];            /* dropped by the device form; the host form refuses instead */
  int max_per_voxel[2];                /* most points merged into one map point */
  int center_cube[3];                  /* laserCloudCen{Width,Height,Depth} after placing the window: cube (i, j, k) of the window holds the
                                          points of [50 (i - center_cube[0]) - 25, ... + 50) m in x, likewise y and z */
  int pad;
} vloam_map_import_result;
void vloam_default_map_import_options(vloam_map_import_options* o);   /* identity, zero */
vloam_status vloam_map_import(vloam_handle* h, const vloam_map_import_options* o, const float* corner_xyzi4, long long n_corner,
                              const float* surf_xyzi4, long long n_surf, vloam_map_import_result* out);
vloam_status vloam_map_import_device(vloam_handle* h, const vloam_map_import_options* o, const void* d_corner, long long n_corner,
                                     const void* d_surf, long long n_surf, void* d_result);

/* Map merge: two point clouds of ANOTHER map — its corner map and its surf map, packed (x, y, z, intensity), e.g. the files of a --save-map
 * directory or vloam_get_map_kind(h2, 0 / 1) of another handle — are folded into the voxel map of a handle that is live (or fresh), given the
 * transform between the two maps (vloam_place_query and vloam_map_relocalize find it: where today's drive sits in yesterday's map).  One map out
 * of two sessions.  Opt-in by calling: a handle that never merges allocates and launches nothing of this, and no kernel of a sweep changes.
 *   1. Transform.  Every point whose four floats are finite goes into this map's frame in f64 from its f32 components: q_map_src is normalised
 *      and R formed from it on the host, as vloam_map_carve forms its poses; each output component is ((R_r0*x + R_r1*y) + R_r2*z) + t_r, every
 *      operation rounded on its own, then rounded to f32.  Intensity is unchanged.  With q = (0, 0, 0, 1) and t = 0 the point is taken as it
 *      is: an exported map goes in bit for bit.
 *   2. Keying.  The transformed point gets the cube and the voxel the mapping's own insert would give it at its kind's leaf, against the
 *      handle's CURRENT window offsets (step 3 of vloam_map_import).  A point whose cube lies outside the window (or outside the voxel key's
 *      range) is dropped and counted in n_outside_window.  The window does not move, the pose does not change, and no trajectory row, sweep
 *      count or odometry state is touched.  (A handle that never placed its window — no sweep mapped, nothing imported or restored — gets the
 *      default window and the identity pose, as from vloam_map_import at the identity, and from then on counts as one that imported.)
 *   3. Fold, per voxel and kind: what the reference holds after appending the points to the cube's cloud and re-filtering that cube
 *      (laser_mapping.cpp:654-659, 689-702).  A voxel without a live record: the f32 sum of its new points in INPUT order, every component
 *      divided by (float)n, one map point (vloam_map_import's rule; a purged record of the same key is reused).  A voxel that holds a merged
 *      map point: that centroid, plus the new points in input order, divided by (float)(1 + n), one map point; the cube's point count is
 *      unchanged.  A voxel that holds un-merged raw points (its cube was outside the valid 5 x 5 x 3 block when they arrived): untouched, its new
 *      points are dropped and counted in n_skipped_raw, as vloam_map_carve skips such voxels.  New voxels get their occupancy block, their
 *      cube's point count and the table counters that a handle has which inserted them itself.
 *      The result is a function of the tables' state, the two arrays and the options alone, bit for bit from run to run (no floating-point atomics).
 *   4. Dry run (apply == 0): lookups only.  n_in, n_new_points, n_hit_points, n_skipped_raw, n_outside_window and n_nonfinite are those of
 *      the applied call; nothing the sequence owns is written.  n_new_points bounds the records the applied call creates.
 *   5. Order.  Both forms first do what vloam_sync does (a host sweep that vloam_process_scan deferred is flushed and mapped first; a sticky
 *      error is reported as there), run on the mapping stream with temporary allocations only, wait for that stream and free them before they
 *      return.  The device form takes device addresses (clouds and a vloam_map_merge_result) and drops non-finite points, counted in
 *      n_nonfinite, where the host form refuses them.
 * Refusals, options first and before the handle is looked at (VLOAM_ERR_INVALID, each with its own vloam_last_error()): null options,
 *   struct_size, apply outside 0 .. 1, reserved != 0, a non-finite component of q or t, a quaternion whose norm is off 1 by more than 1e-6, a
 *   negative count, more than 16777216 points of a kind, a null cloud with a positive count, a null result, host form only: a non-finite float in
 *   a cloud.  Then the handle: null (VLOAM_ERR_INVALID); with_mapping == 0 (VLOAM_ERR_ORDER); n_sessions > 1 (VLOAM_ERR_INVALID); a stage-wise
 *   sweep in progress (VLOAM_ERR_ORDER).  After any refusal the handle is unchanged and usable.
 * Capacity: a growable handle (vloam_map_options::grow) first steps its tables to the size its growth bound asks for with live records + n_in
 *   of each kind as the bound on records (apply only), as vloam_map_import does on empty tables.  A fixed handle cannot be refused up front —
 *   how many NEW voxels the clouds bring is known only after the lookups (n_new_points of a dry run bounds them): when the live records
 *   exceed 60 % of a table's slots (or a probe chain reaches its bound) the call returns VLOAM_ERR_CAPACITY naming the table, the handle
 *   carries the sticky map-full error a sweep would have raised (vloam_sync reports it) and is finished, as after such a sweep.
 * Not offered: batched handles; collapsing raw voxels; merging place databases or trajectories; estimating the transform (vloam_map_relocalize
 *   does). */
typedef struct vloam_map_merge_options {   /* 72 bytes: 4 ints, then 7 doubles */
  int struct_size;            /* sizeof as compiled */
  int apply;                  /* 1 merge (default), 0 dry run */
  int reserved[2];            /* 0 */
  double q_map_src[4];        /* (x, y, z, w), unit within 1e-6; default identity: this map <- the clouds' frame */
  double t_map_src[3];        /* default 0 */
} vloam_map_merge_options;
typedef struct vloam_map_merge_result {    /* 120 bytes: 14 long long, then 2 ints; [corner, surf] */
  long long n_in[2];               /* points given */
  long long n_new_points[2];       /* points whose voxel had no live record */
  long long n_hit_points[2];       /* points whose voxel held a merged map point (overlap = n_hit_points / n_in) */
  long long n_skipped_raw[2];      /* points whose voxel holds un-merged raw points: dropped */
  long long n_outside_window[2];   /* dropped: cube outside the 21 x 21 x 11 window (or outside the key range) */
  long long n_nonfinite[2];        /* dropped by the device form; the host form refuses instead */
  long long n_new_voxels[2];       /* apply only, 0 in a dry run: map points (voxel records) created */
  int max_per_voxel[2];            /* apply only: most points of the call folded into one map point */
} vloam_map_merge_result;
void vloam_default_map_merge_options(vloam_map_merge_options* o);   /* apply, identity, zero */
vloam_status vloam_map_merge(vloam_handle* h, const vloam_map_merge_options* o, const float* corner_xyzi4, long long n_corner,
                             const float* surf_xyzi4, long long n_surf, vloam_map_merge_result* out);
vloam_status vloam_map_merge_device(vloam_handle* h, const vloam_map_merge_options* o, const void* d_corner, long long n_corner,
                                    const void* d_surf, long long n_surf, void* d_result);

/* Timing of the last vloam_sync()ed scans: HIP-event milliseconds accumulated per stage
 * {scanRegistration, laserOdometry, laserMapping, vo} and number of scans covered. */
vloam_status vloam_get_stage_ms(vloam_handle* h, double ms4[4], int* scans);
/* Measured per-run counts that DESIGN.md's algorithmic-byte formulas need:
 * {N_in, N2, n_sharp, n_lessSharp, n_flat, n_lessFlat, C, S, F_o_corner, F_o_plane, E_o, n_c, n_s, K_m, E_m, M} of the last scan. */
vloam_status vloam_get_counts(vloam_handle* h, long long counts16[16]);

/* Map clean-up: voxels that later sweeps see THROUGH are removed from the map — what a parked car, a pedestrian or a bus leaves behind.  A
 * visibility test in the sensor's range image (one image per sweep), not a ray walk: conservative at grazing incidence, and integers from the
 * projection on.  Opt-in by calling: a handle that never carves allocates and launches nothing of this, and no kernel of a sweep changes.
 *   Projection of a point (x, y, z), all f32, every operation rounded on its own, atanf / atan2f glibc's (csrc/fdlibm_f32.h): h2 = x*x + y*y;
 *   r = sqrtf(h2 + z*z); the point projects when x, y, z are finite, min_range <= r <= max_range and 0 <= rf < rows with
 *   rf = (atanf(z / sqrtf(h2)) - e0) * ((float)rows / (e1 - e0)), e0 / e1 = elev_min_deg / elev_max_deg * 0.017453292f;
 *   row = (int)floorf(rf); col = (int)floorf((atan2f(y, x) + PI_F) * ((float)cols / (2.0f * PI_F))), PI_F = 0x40490fdb, col == cols wraps to 0;
 *   quantised range q = (unsigned)floorf(r / range_res).
 *   1. Range images: per sweep rows x cols words, empty = 0xffffffff; every point of the sweep that projects leaves min(q) in its pixel.
 *   2. Candidates: the live voxel records of the selected kinds (kind_mask: 1 corner map | 2 surf map) whose cube lies inside the 21 x 21 x 11
 *      window, at the point vloam_get_map_kind returns for them.  Voxels that hold un-merged raw points (cubes outside the valid 5 x 5 x 3
 *      block) are never removed: counted in skipped_raw.  Per sweep s the candidate goes into the sensor frame, p_s = R^T (p - t) with
 *      q normalised and R from it in f64 on the host, d = (double)p - t, each component (R0c*d0 + R1c*d1) + R2c*d2 in f64, rounded to f32 —
 *      and is projected as above (no projection: the sweep does not vote).  c the image's pixel there, m the minimum over the 3 x 3 pixels around
 *      it (columns wrap, rows clamp), qm the candidate's quantised range, margin_q = (unsigned)floorf(margin / range_res):
 *      the sweep SEES THROUGH the candidate when c is a return and qm + margin_q < m; it CONFIRMS it when c is a return and |qm - c| <= margin_q.
 *      A candidate is removed when at least min_votes sweeps see through it and none confirms it.
 *   3. apply == 1 (single-sequence handles): the removed records are dropped, the per-cube counts follow, and the table's same-size
 *      reclamation (the rebuild of a fixed handle, the same-size rehash of a growable one) is enqueued before the call returns: table and
 *      occupancy blocks keep no trace of them.  apply == 0 writes nothing the sequence owns.
 *   The removed points come as packed (x, y, z, intensity) in unspecified order; counters and the removed SET are a function of the inputs alone.
 * Poses: poses7[s] = (qx, qy, qz, qw, tx, ty, tz), map <- sensor of sweep s; NULL (n_sweeps == 1 only): the handle's last mapped pose.
 * Both forms first synchronise the handle (as vloam_get_map_kind), run on the mapping stream and wait for their result: opt, n, poses7 and res
 *   are host memory in both; vloam_map_carve takes host sweeps and a host list, vloam_map_carve_device a HOST array of n_sweeps device
 *   addresses (packed float4 each) and a device list of cap points.  The scratch is one allocation made by the first call, kept until vloam_destroy.
 * More removals than cap: VLOAM_ERR_CAPACITY, res filled (n_removed_out the capacity needed), the list's content undefined, nothing applied.
 * Refusals, options first and before the handle is looked at (VLOAM_ERR_INVALID, each with its own vloam_last_error()): null options or
 *   struct_size; kind_mask outside 1 .. 3; rows < 1, cols < 4 or rows * cols > 1048576; elevations that are not finite, outside -90 .. 90 or
 *   less than 0.001 degrees apart; ranges that are not finite, min_range <= 0 or >= max_range; range_res not finite and positive or below
 *   max_range / 2^30; margin negative, not finite or above 2^30 range_res; min_votes outside 1 .. 16; apply outside 0 .. 1; n_sweeps outside
 *   1 .. 16; null arrays; a count outside 0 .. 262144; a null sweep with a positive count; null poses with n_sweeps > 1; a non-finite pose
 *   component; a quaternion whose norm is off 1 by more than 1e-6; cap < 0 or a null list with cap > 0; a null result.  Then the handle: null
 *   (VLOAM_ERR_INVALID); with_mapping == 0 (VLOAM_ERR_ORDER); apply on a handle with n_sessions > 1 (VLOAM_ERR_INVALID; a dry run works on
 *   the selected session).
 * Not offered: ray walking through free space, votes kept across calls, removal of un-merged raw points, re-insertion of what a sweep
 *   confirms, per-point labels of the sweeps (which returns were dynamic). */
typedef struct vloam_carve_options {   /* 48 bytes */
  int struct_size;                     /* sizeof as compiled */
  int kind_mask;                       /* 1 corner map | 2 surf map; default 3 */
  int rows, cols;                      /* range image; default 64 x 1024 */
  float elev_min_deg, elev_max_deg;    /* its vertical field of view; default -25, +3 */
  float min_range, max_range;          /* metres; default 2, 80 */
  float range_res;                     /* metres per range step; default 0.05 */
  float margin;                        /* metres; default 0.5 */
  int min_votes;                       /* sweeps that must see through; default 1 */
  int apply;                           /* 0 dry run (default), 1 remove */
} vloam_carve_options;
typedef struct vloam_carve_result {    /* 104 bytes; [corner map, surf map] */
  long long examined[2];               /* candidates */
  long long in_view[2];                /* ... that project into at least one sweep's image */
  long long seen_through[2];           /* ... that at least one sweep sees through */
  long long confirmed[2];              /* ... that at least one sweep confirms */
  long long removed[2];
  long long skipped_raw[2];            /* voxels of un-merged raw points: never candidates */
  long long n_removed_out;             /* points the list holds (VLOAM_ERR_CAPACITY: would have to hold) */
} vloam_carve_result;
void vloam_default_carve_options(vloam_carve_options* o);
vloam_status vloam_map_carve(vloam_handle* h, const vloam_carve_options* o, const float* const* xyz_pad4, const int* n, const double* poses7,
                             int n_sweeps, float* removed_xyzi4, long long cap, vloam_carve_result* res);
vloam_status vloam_map_carve_device(vloam_handle* h, const vloam_carve_options* o, const void* const* d_xyz_pad4, const int* n, const double* poses7,
                                    int n_sweeps, void* d_removed_xyzi4, long long cap, vloam_carve_result* res);

/* Map archive: keep the points of cubes that roll out of the window.  The map is a window of 21 x 21 x 11 cubes of 50 m around the sensor; when
 * it rolls, the points of the cubes that leave it are dropped for good (as the reference clears the slab that wraps).  On a handle that enabled
 * the archive, every such point is first copied into a list on the device, so that the map of a whole drive can be saved.  Opt-in and read-only
 * against the map: a handle that never enables it allocates and launches nothing of this, no kernel of a sweep changes, and an enabled handle
 * computes byte for byte what it computed without (one more launch per mapped sweep on the mapping stream, which returns at once when the
 * window did not roll).
 *   A row is a live record of a cube outside the window the sweep has just placed, at the point vloam_get_map_kind would have returned for it
 *   before that sweep; a voxel of un-merged raw points contributes those points.  Rows land in the device buffer in unspecified order within a
 *   sweep; (sweep, kind, cube_k, cube_j, cube_i, tail, order) is unique per row, vloam_map_archive_get sorts by it, and within one cube and kind
 *   that is the order vloam_get_map_kind had.  A voxel that was evicted, re-entered the window empty and was filled and evicted again has two
 *   rows (vloam_map_import merges the points of one voxel into their centroid in input order).
 * vloam_map_archive_enable: synchronises the handle and allocates capacity_rows rows and the counters (an allocation of its own, kept until
 *   vloam_destroy); rows are collected from the next mapped sweep on.  Refusals (VLOAM_ERR_INVALID, each with its own vloam_last_error()): null
 *   options or a wrong struct_size; capacity_rows < 1 or > 2^26; a null handle; n_sessions > 1; with_mapping == 0; a second enable.
 * vloam_map_archive_info: synchronises; out4 = rows held, rows dropped since the last clear, capacity_rows, rolls seen since the enable.
 * vloam_map_archive_get: synchronises, copies the rows held into rows (host memory, cap rows) sorted by the key above; *n is always the number
 *   held; cap smaller than that: VLOAM_ERR_CAPACITY, nothing copied and nothing cleared.  clear == 1: rows held and rows dropped start over at 0.
 * vloam_map_archive_device_ptr: the unsorted device buffer and the address of its counters (n_rows[0] rows held, n_rows[1] rows dropped); the
 *   content is complete after vloam_sync().
 * Before the enable the last three return VLOAM_ERR_INVALID.  A full archive never fails the sequence: rows beyond the capacity are not written
 *   and counted as dropped.
 * The archive is no part of a checkpoint: vloam_checkpoint_size / _save / _load behave exactly as without it, and a restored handle is not
 *   enabled and holds no rows.  On a growable handle the launch follows growth steps and same-size reclamations (it takes the tables as they are
 *   when the sweep is enqueued).  vloam_map_import, vloam_map_merge and vloam_map_localize never roll the window, so they never archive.
 * Not offered: putting archived cubes back when the window returns (vloam_map_merge with the identity takes the rows), batched handles,
 *   spilling to the host during a run. */
typedef struct vloam_map_archive_options {
  int struct_size;                     /* sizeof as compiled */
  long long capacity_rows;             /* 1 .. 2^26; default 2^20 (32 MiB) */
} vloam_map_archive_options;
typedef struct vloam_map_archive_row {   /* 32 bytes */
  float x, y, z, intensity;            /* the point vloam_get_map_kind would have returned */
  unsigned int order;                  /* voxel (lz, ly, lx), 9 bits each, of a merged voxel; the arrival stamp of an un-merged point */
  short cube_i, cube_j, cube_k;        /* absolute cube (0, 0, 0: the cube the sequence started in), independent of where the window is */
  unsigned short flags;                /* bit 0: kind (0 corner, 1 surf); bit 1: tail (an un-merged arrival, behind the cube's voxel-ordered part) */
  int sweep;                           /* 0-based index of the sweep whose roll evicted the point */
} vloam_map_archive_row;
void vloam_default_map_archive_options(vloam_map_archive_options* o);   /* 2^20 rows */
vloam_status vloam_map_archive_enable(vloam_handle* h, const vloam_map_archive_options* o);
vloam_status vloam_map_archive_info(vloam_handle* h, long long out4[4]);
vloam_status vloam_map_archive_get(vloam_handle* h, vloam_map_archive_row* rows, long long cap, long long* n, int clear);
vloam_status vloam_map_archive_device_ptr(vloam_handle* h, void** d_rows, int** d_n_rows);

#ifdef __cplusplus
}
#endif
#endif
