// Host-only: the handle behind the C ABI and what the translation units of the host side share (c_api.cpp: creation and destruction;
// capi_sweep.cpp: the sweep pipeline; capi_frame.cpp: coupled frames, images, VO; capi_results.cpp: getters and debug hooks; capi_rows.cpp: the
// per-sweep row products; capi_ckpt.cpp: checkpoints; capi_query.cpp: map queries; capi_localize.cpp: localisation; capi_import.cpp: map import; capi_merge.cpp: map merge; capi_score.cpp: pose scores and relocalisation; capi_place.cpp: place recognition; capi_carve.cpp: map clean-up; capi_archive.cpp: map archive).  No .hip file includes this.  Helpers that cross files live in namespace vloam (mangled,
// out of the C symbol list); a helper of one file is static there.
#pragma once
#include "../../include/vloam_hip/c_api.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <float.h>
#include <limits.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "ckpt_format.h"
#include "lm_solve.h"
#include "lo_kernels.h"
#include "map_kernels.h"
#include "place.h"
#include "pose_cov.h"
#include "pose_info.h"
#include "sr_kernels.h"
#include "stage_input_check.h"
#include "stream_plan.h"
#include "sweep_log.h"
#include "vloam_device.h"
#include "vo_kernels.h"
#include "img_kernels.h"

using namespace vloam;

namespace vloam {
// defined in c_api.cpp, read once when the library is loaded
extern const bool g_host_prof;     // VLOAM_HOST_PROF
extern const int g_stage_inline;   // VLOAM_STAGE_INLINE; 1: vloam_process_scan / vloam_batch_process_scan stage inline too (no deferred ring)
void set_err(const char* fmt, ...);   // the text vloam_last_error returns to this thread
}  // namespace vloam

#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);     \
      return VLOAM_ERR_HIP;                                                                   \
    }                                                                                         \
  } while (0)

// a helper's refusal or failure is the caller's
#define TRY(expr)                              \
  do {                                         \
    const vloam_status try_s_ = (expr);        \
    if (try_s_ != VLOAM_OK) return try_s_;     \
  } while (0)

// The events behind the row writes of a per-sweep row product (sweep log, pose information): the event behind each stage's row write, a ring of
// kSlots sweeps per stage; a slot that a later sweep has taken over belongs to a sweep whose writes
// the host has long seen finished (enqueue_sr waits for the odometry of sweep k - kSets + 1 and the mapping of sweep k - kSets before it
// enqueues sweep k, and every stream is in order), so the reader only ever waits for an event that still carries its sweep's number
struct RowEvents {
  static constexpr int kMaxStages = 3, kSlots = 2 * kBufferSets;
  int stages = 0;
  hipEvent_t ev[kMaxStages][kSlots] = {};
  int frame[kMaxStages][kSlots];   // the sweep each slot was last bound to (create: -1)
  hipError_t create(int n_stages) {
    stages = n_stages;
    for (int s = 0; s < kMaxStages; s++) for (int k = 0; k < kSlots; k++) frame[s][k] = -1;
    hipError_t e = hipSuccess;
    for (int s = 0; s < stages; s++)
      for (int k = 0; k < kSlots && e == hipSuccess; k++) e = hipEventCreateWithFlags(&ev[s][k], hipEventDisableTiming | hipEventBlockingSync);
    return e;
  }
  void destroy() {
    for (int s = 0; s < kMaxStages; s++) for (hipEvent_t e : ev[s]) if (e) (void)hipEventDestroy(e);
  }
  // the event a stage's row write of sweep `sweep` is bound to
  hipEvent_t bind(int stage, int sweep) {
    const int slot = sweep % kSlots;
    frame[stage][slot] = sweep;
    return ev[stage][slot];
  }
  // rows complete in sweep order on every stream: wait for the writers of row `last`, nothing younger
  hipError_t wait_row(int last) const {
    const int slot = last % kSlots;
    hipError_t e = hipSuccess;
    for (int s = 0; s < stages && e == hipSuccess; s++)
      if (frame[s][slot] == last) e = hipEventSynchronize(ev[s][slot]);
    return e;
  }
};

struct vloam_handle {
  vloam_config cfg;
  int device = 0;
  // Three in-order streams, one per stage of the façade: scan registration of sweep k + 1 overlaps laser odometry of sweep k
  // and laser mapping of sweep k - 1 (each stage only needs the previous stage's result of the SAME sweep plus its own state
  // of the previous sweep).  Cross-stage edges are HIP events; SR output lives in kSets rotating buffer sets so that a stage
  // running ahead never overwrites what a slower stage still reads.
  hipStream_t stream = nullptr;   // scan registration (+ NN grid build); also creation / VO work
  hipStream_t s_lo = nullptr;     // laser odometry
  hipStream_t s_map = nullptr;    // laser mapping
  hipStream_t s_img = nullptr;    // image front-end of the coupled frame loop (needs the image only: next to the scan-registration stream)
  hipStream_t s_ds = nullptr;     // VoxelGrid of the scan features for mapping (needs the sweep's feature clouds only: off the SR stream's chain)
  int prio[vloam_plan::kStreams] = {};   // the HIP priority each stream is created with (= its hardware-queue pool: stream_plan.h)
  static constexpr int kSets = kBufferSets;   // 3 suffice for correctness; the rest is run-ahead for the host (vloam_device.h)
  hipEvent_t ev_sr[kSets] = {}, ev_lo[kSets] = {}, ev_map[kSets] = {}, ev_stack[kSets] = {};  // "stage finished for the sweep in set c"
  static_assert(kSets == MapContext::kSets, "the stack sets rotate with the SR buffer sets");
  // Device memory: B session arenas of identical layout, `se.ss` bytes apart, in ONE allocation; every device pointer below is
  // session 0's (kernels add blockIdx.z * se.ss, host-side getters add sel * se.ss)
  char* arena = nullptr;
  size_t arena_bytes = 0;
  Sess se;
  int sel = 0;          // session the getters read (vloam_select_session)
  double* sync_pool = nullptr;
  bool counted_single = false; // this handle is in g_single_handles
  int* ring_watch = nullptr;   // host-mapped [2][kMaxBatch]: a ring of that session came near the small ring tier's capacity / near kMaxRingLen (k_sr_ring)
  int* coop_flag = nullptr;    // host-mapped [1]: a cooperative solve of this handle degraded to one workgroup (k_lm_solve) — polled before every enqueue
  long long fallback_solves = 0;   // cooperative solves that degraded to one workgroup, as of the last vloam_sync
  int frame = 0;        // sweeps accepted (scan registration enqueued)
  int lo_done = 0;      // sweeps whose laser odometry has been enqueued (vloam_process_scan defers it, see drain_deferred)
  int map_done = 0;     // sweeps whose laser mapping has been enqueued
  int stage = 0;        // façade order inside a sweep: 0 idle, 1 after SR, 2 after LO
  int nblk_max = 0;
  // scan registration
  // Host sweeps.  vloam_process_scan / vloam_batch_process_scan (the asynchronous whole-sweep calls): a copy stream + a ring of kInRing device
  // input buffers, and the sweep itself is ENQUEUED BY THE NEXT CALL (like its odometry and mapping: drain_deferred) — by then its copy has
  // landed, so nothing on the device ever waits for the host link and no stream waits for another: the copy of sweep k + 1 runs beside the scan
  // registration of sweep k.  ev_in_copied: the copy into the slot has landed (checked by the HOST); in_reader: the event behind the slot's last
  // reader (the sweep's own "scan registration finished" event; checked by the HOST before the slot is copied into again, three calls later).
  // Every other host-pointer entry point (stage-wise calls, frames) stages INLINE: hipMemcpyAsync on the scan-registration stream into a
  // buffer of its own (slot kInRing), the stream's order being the dependency.
  static constexpr int kInRing = 4;
  float4* d_in = nullptr;         // [kInRing + 1][max_points]
  hipStream_t s_copy = nullptr;   // host-sweep copies: vloam_create (plan.copy_first) or the first deferred host sweep
  hipEvent_t ev_in_copied[kInRing] = {};
  hipEvent_t in_reader[kInRing] = {};
  int in_next = 0;                // next ring slot
  struct { bool valid = false; BatchIn bi; int slot = -1; } pend;   // the host sweep whose copy is in flight: enqueued by the next call / any drain
  SRBuffers sr[kSets];  // rotating sets: S, cloud and the feature clouds are per set, the scratch arrays are shared (SR stream only)
  // clouds / odometry pose the caller handed to LaserMapping::input instead of the odometry's own (vloam_set_mapping_input): the mapping of
  // that one sweep reads them from here, the odometry keeps its CornerLast / SurfLast (the reference's stages hold separate copies)
  SRBuffers sub{};             // S, cloud, less_sharp, less_flat only
  double* sub_row = nullptr;   // [14] trajectory row of the substituted sweep: odometry pose in, map pose out
  int sub_cloud_frame = -1, sub_pose_frame = -1;
  // laser odometry
  LOState* lo = nullptr;
  FactorTable lo_F{};
  int* lo_corr[2] = {nullptr, nullptr};
  int* lo_queue = nullptr;     // [kMaxLoFactors] queries k_lo_assoc_fast left to the wave-per-query pass
  int* lo_queue_n = nullptr;   // [2] entries of the queue, by launch parity
  int lo_launches = 0;
  long long* lo_cyc[2] = {nullptr, nullptr};  // debug: per-slot shader-clock cycles of k_lo_assoc (NN, walks, emit, exact radius)
  LMRecord* lo_rec = nullptr;  // [2]
  double* lo_resid[2] = {nullptr, nullptr};
  double* traj = nullptr;      // [max_frames][14]
  double* vo_traj = nullptr;   // [max_frames][7] world_VOT_base_last per frame (coupled frame loop)
  // per-sweep diagnostics log (vloam_limits_ext::sweep_log; everything below stays null / unused on a handle without it).  log_ring: the event
  // behind each stage's row write (scan registration, odometry, mapping)
  bool sweep_log = false;
  vloam_sweep_record* log_rows = nullptr;   // [max_frames]
  SweepLogScratch* log_scratch = nullptr;
  RowEvents log_ring;
  // per-sweep pose information matrices (vloam_pose_info_enable; null / unused on a handle without it).  Rows and scratch are allocations of their
  // own, outside the arena.  pi_ring: the event behind each LiDAR stage's row write (odometry, mapping)
  bool pose_info = false;
  PoseInfo pi;
  RowEvents pi_ring;
  // ... and its add-on, the pose covariance rows (vloam_pose_cov_enable; null / unused without it).  No ring of its own: once enabled, the launch
  // behind each stage's pose information launch is the one pi_ring's event is bound to (the last writer of both products on that stream)
  bool pose_cov = false;
  PoseCov pc;
  hipEvent_t ev_vo[kSets] = {};     // depth map + matches of the frame in set c are in HBM
  bool vo_frame[kSets] = {};        // the sweep in set c came through vloam_process_frame (its odometry is preceded by the VO solve)
  bool have_extrinsics = false;
  bool map_imported = false;        // vloam_map_import* has filled the map: no second import, no checkpoint load
  bool vo_used = false;             // a VO, frame or image entry point was called: the sequence cannot be checkpointed (the VO's previous-frame state is not saved)
  ImgContext img;
  std::vector<unsigned char> img_pack;   // host scratch: a padded image packed to width-stride rows
  hipEvent_t ev_img[kSets] = {};    // the image-derived matches of the frame in set c are in HBM
  bool img_frame[kSets] = {};
  LoGrid grid[kSets];          // per set: NN grid over that sweep's lessSharp / lessFlat
  // mapping + vo
  MapContext map;
  VOContext vo;
  // timing
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // cfg.timing: begin / end of SR, LO, mapping
  double stage_ms[4] = {0, 0, 0, 0};
  int timed_scans = 0;
  int last_n_in = 0;
  ProfHook prof;
  // VLOAM_HOST_PROF=1: host seconds spent inside the enqueue helpers (printed by vloam_destroy): throttle waits | SR (+ grids, scan-feature VoxelGrid) | LO | mapping
  double host_s[4] = {0, 0, 0, 0};
  long long host_calls = 0;
  std::vector<hipEvent_t> prof_events;
  std::vector<int> prof_kids;
  // place recognition (vloam_place_enable; null / unused on a handle without it): descriptors, the database and the match scratch, allocations of
  // their own; all of its work goes to `stream`.  Last, so that no other member's place in the handle depends on it
  PlaceContext place;
};

#define SINGLE_SESSION_ONLY(h) do { if ((h)->se.B != 1) { set_err("this entry point drives one sequence: the handle has %d sessions (use the vloam_batch_* calls)", (h)->se.B); return VLOAM_ERR_INVALID; } } while (0)

// session-relative pointer for the host-side getters
template <class T>
static inline T* SEL(const vloam_handle* h, T* p) { return p ? (T*)((char*)p + (size_t)h->sel * h->se.ss) : p; }

static inline int set_of(int frame) { return frame % vloam_handle::kSets; }
// the sweep the getters show: the one in progress, or (between sweeps: finish_frame has counted it) the last finished one
static inline int shown_frame(const vloam_handle* h) { return (h->stage == 0 && h->frame > 0) ? h->frame - 1 : h->frame; }
// sweeps handed over (the last host sweep may still be in flight: deferred ring; every drain enqueues it)
static inline int handed_over(const vloam_handle* h) { return h->frame + (h->pend.valid ? 1 : 0); }
// right after creation: no sweep taken, none pending, not inside a stage-wise sweep
static inline bool is_fresh(const vloam_handle* h) { return h->frame == 0 && !h->pend.valid && h->stage == 0; }
// from now on this handle launches one-workgroup solves (capi_sweep.cpp: poll_coop_flag; vloam_sync)
static inline void set_no_coop(vloam_handle* h) { h->se.no_coop = 1; h->map.se.no_coop = 1; h->vo.se.no_coop = 1; }

// ------------------------------------------------------------------ helpers that cross files (all defined in capi_sweep.cpp, but the first: capi_results.cpp)
namespace vloam {
vloam_status sticky_map_status(const vloam_handle* h, int merr);         // the sticky map / solver bits of a handle's error word as vloam_sync reports them
vloam_status sync_all(vloam_handle* h);                                  // drain, then synchronise every stream of the handle
vloam_status drain_deferred(vloam_handle* h, int lag_lo, int lag_map);   // enqueue the odometry / mapping still owed (0, 0: all of it, the pending host sweep first)
vloam_status check_host_sweeps(const vloam_handle* h, const float* const* xyz_pad4, const int* n);   // admission of host sweeps, before anything is copied
BatchIn batch_in(const vloam_handle* h, const void* const* ptrs, const int* n);
vloam_status stage_inline(vloam_handle* h, int b, const float* xyz_pad4, int n, const void** d_out);
vloam_status enqueue_sr(vloam_handle* h, const BatchIn& bi);
vloam_status begin_sweep(vloam_handle* h);
vloam_status end_sweep(vloam_handle* h);
}  // namespace vloam
