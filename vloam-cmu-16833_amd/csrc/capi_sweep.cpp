// The sweep pipeline of libvloam_hip.so: admission of sweeps, the three stage enqueues and their deferral, the host-sweep ring, the stage-wise
// entry points and the whole-sweep calls.  Every enqueue of a sweep's kernels is in this file.
#include "handle.h"

static inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The admission rule of substituted clouds (stage_input_check.h), applied to the HOST arrays before anything is synchronised or uploaded: a
// refused call leaves the handle as it was.  Null clouds (keep the device's) are not checked.
static_assert(vloam_stage_check::kStageLines == kMaxRings, "the walk-stop tables hold kMaxRings lines");
static vloam_status check_stage_clouds(const char* call, int count, const char* const* names, const float* const* src, const int* n, const bool* walked) {
  for (int k = 0; k < count; k++) {
    if (!src[k]) continue;
    const vloam_stage_check::Fault f = vloam_stage_check::check_cloud(src[k], n[k], walked[k]);
    if (f.rule == vloam_stage_check::kOk) continue;
    if (f.rule == vloam_stage_check::kLineOrder)
      set_err("%s: %s, point %d: intensity %.9g, line %d after line %d: %s", call, names[k], f.point, (double)f.value, (int)f.value, f.max_line,
              vloam_stage_check::rule_text(f.rule));
    else
      set_err("%s: %s, point %d: intensity %.9g: %s", call, names[k], f.point, (double)f.value, vloam_stage_check::rule_text(f.rule));
    return VLOAM_ERR_INVALID;
  }
  return VLOAM_OK;
}

// ------------------------------------------------------------------ stage enqueue helpers
static vloam_status flush_pending(vloam_handle* h);
vloam_status vloam::sync_all(vloam_handle* h) {
  TRY(drain_deferred(h, 0, 0));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipStreamSynchronize(h->s_lo));
  if (h->s_ds) HIPCHK(hipStreamSynchronize(h->s_ds));
  if (h->s_map) HIPCHK(hipStreamSynchronize(h->s_map));
  if (h->s_img) HIPCHK(hipStreamSynchronize(h->s_img));
  return VLOAM_OK;
}

// ------------------------------------------------------------------ admission: what every entry point asks of its sweeps and images
// One sweep per session (a single-sequence call passes the addresses of its two arguments).  Host sweeps are admitted by their entry point,
// before anything is copied; device sweeps by enqueue_sr, which the deferred ring reaches a call later.  A null host sweep is a null
// argument like any other (no message); a null device sweep says which session.
static vloam_status check_sweeps(const vloam_handle* h, const void* const* ptrs, const int* n, bool device) {
  for (int b = 0; b < h->se.B; b++) {
    if (!ptrs[b]) { if (device) set_err("null sweep pointer for session %d", b); return VLOAM_ERR_INVALID; }
    if (n[b] > h->cfg.max_points) { set_err("cloud of %d points exceeds max_points=%d", n[b], h->cfg.max_points); return VLOAM_ERR_CAPACITY; }
    if (n[b] <= 0) { set_err("empty cloud"); return VLOAM_ERR_EMPTY; }
  }
  return VLOAM_OK;
}
vloam_status vloam::check_host_sweeps(const vloam_handle* h, const float* const* xyz_pad4, const int* n) {
  return check_sweeps(h, (const void* const*)xyz_pad4, n, false);
}

// the sweeps of one call, one per session, as the kernels take them
BatchIn vloam::batch_in(const vloam_handle* h, const void* const* ptrs, const int* n) {
  BatchIn bi;
  memset(&bi, 0, sizeof(bi));
  for (int b = 0; b < h->se.B; b++) { bi.in[b] = (const float4*)ptrs[b]; bi.n[b] = n[b]; }
  return bi;
}

// the mapping stage's VoxelGrid of the scan features of sweep `frame`, if it is a mapped sweep: it only needs the sweep's feature clouds, so
// it runs on a stream of its own, off the mapping stream
static vloam_status enqueue_scan_feature_grid(vloam_handle* h, const SRBuffers& bufs, int frame, int cur) {
  if (!h->cfg.with_mapping || ((frame + 1) % h->cfg.mapping_skip_frame) != 0) return VLOAM_OK;
  HIPCHK(hipStreamWaitEvent(h->s_ds, h->ev_sr[cur], 0));   // the feature clouds (ev_sr is bound to k_sr_compact); a live wait: on a queue of its own, or SR's (budget 1, or several handles alive at a small budget: stream_plan.h)
  if (map_stack_enqueue(&h->map, h->s_ds, bufs, cur, &h->prof, h->ev_stack[cur]) != VLOAM_OK) { set_err("map_stack_enqueue failed"); return VLOAM_ERR_HIP; }
  return VLOAM_OK;
}

vloam_status vloam::enqueue_sr(vloam_handle* h, const BatchIn& bi) {
  TRY(check_sweeps(h, (const void* const*)bi.in, bi.n, true));
  int n = 0;
  for (int b = 0; b < h->se.B; b++) n = bi.n[b] > n ? bi.n[b] : n;
  if (h->frame >= h->cfg.max_frames) { set_err("trajectory log full (max_frames=%d)", h->cfg.max_frames); return VLOAM_ERR_CAPACITY; }
  const int k = h->frame, cur = set_of(k);
  // Set `cur` still holds sweep k - 3: read by odometry of sweeps k - 3 (current) and k - 2 (previous), mapping of sweep k - 3.
  // The HOST waits for those before enqueueing (it may run at most two sweeps ahead of the odometry, three ahead of the
  // mapping): a cross-stream barrier packet in front of every sweep costs ~12 us on the stream that bounds the throughput,
  // a host-side check of an event that has almost always fired costs nothing on the device.
  constexpr int kS = vloam_handle::kSets;  // set `cur` holds sweep k - kS: odometry of sweeps k - kS and k - kS + 1, mapping of k - kS
  const double tw0 = g_host_prof ? now_s() : 0.0;
  if (k >= kS - 1) HIPCHK(hipEventSynchronize(h->ev_lo[set_of(k - (kS - 1))]));
  if (k >= kS && h->cfg.with_mapping) HIPCHK(hipEventSynchronize(h->ev_map[set_of(k - kS)]));
  if (g_host_prof) h->host_s[0] += now_s() - tw0;
  if (h->cfg.timing) HIPCHK(hipEventRecord(h->ev[0], h->stream));
  // the full grid of the big ring tier only while long rings are around (watch word of an earlier sweep: plain read of host-mapped memory);
  // whatever the host knows or does not know, ONE catch-all workgroup of the big tier follows the small tier on every sweep, so any ring of up
  // to kMaxRingLen points is processed (sr_launch); the same for the long tier and rings of up to max_ring_points on handles that have it
  bool big_tier = false, long_tier = false;
  for (int b = 0; b < h->se.B; b++) big_tier = big_tier || __atomic_load_n(&h->ring_watch[b], __ATOMIC_RELAXED) != 0;
  if (h->cfg.max_ring_points > kMaxRingLen)
    for (int b = 0; b < h->se.B; b++) long_tier = long_tier || __atomic_load_n(&h->ring_watch[kMaxBatch + b], __ATOMIC_RELAXED) != 0;
  HIPCHK(sr_launch(h->stream, h->sr[cur], bi, h->se, h->cfg.scan_line, (float)h->cfg.minimum_range, h->cfg.debug, &h->prof,
                   h->ev_sr[cur], h->ring_watch, big_tier, long_tier));  // the odometry of THIS sweep needs the feature clouds only (its NN grids were built with the previous sweep)
  // == kdtreeCornerLast / kdtreeSurfLast->setInputCloud (laser_odometry.cpp:525-526): index this sweep's clouds for the next one
  // (the next sweep's ev_sr is recorded behind this on the same stream, so its odometry sees the finished grids)
  lo_grid_build_launch(h->stream, h->se, h->sr[cur].less_sharp, h->sr[cur].less_flat, h->sr[cur].S, h->grid[cur], &h->prof);
  if (h->sweep_log) sweep_log_sr_launch(h->stream, h->se, h->log_rows, k, h->sr[cur].S, bi, &h->prof, h->log_ring.bind(0, k));
  HIPCHK(hipGetLastError());
  if (h->cfg.timing) HIPCHK(hipEventRecord(h->ev[1], h->stream));
  TRY(enqueue_scan_feature_grid(h, h->sr[cur], k, cur));
  h->last_n_in = n;
  h->stage = 1;
  h->vo_frame[cur] = false;
  h->img_frame[cur] = false;
  return VLOAM_OK;
}

// A cooperative solve that found its partners missing finished on one workgroup and said so in a host-mapped word: from the next enqueue on
// this handle launches one-workgroup solves (no host synchronisation needed: a host that streams thousands of sweeps between two vloam_sync
// calls pays the ~0.2 s wait once, not per solve).
static inline void poll_coop_flag(vloam_handle* h) {
  if (!h->se.no_coop && h->coop_flag && __atomic_load_n(h->coop_flag, __ATOMIC_RELAXED)) set_no_coop(h);
}

static vloam_status enqueue_lo(vloam_handle* h, int frame) {
  poll_coop_flag(h);
  const int cur = set_of(frame), prev = set_of(frame + vloam_handle::kSets - 1);
  HIPCHK(hipStreamWaitEvent(h->s_lo, h->ev_sr[cur], 0));
  if (h->cfg.timing) HIPCHK(hipEventRecord(h->ev[2], h->s_lo));
  const bool coupled = h->vo_frame[cur];  // MAIN/src/vloam_main_node.cpp:125-180: this frame's VO runs in front of its laser odometry
  const bool use_prior = !h->cfg.detach_VO_LO;
  if (coupled) {
    HIPCHK(hipStreamWaitEvent(h->s_lo, h->ev_vo[cur], 0));
    if (h->img_frame[cur]) HIPCHK(hipStreamWaitEvent(h->s_lo, h->ev_img[cur], 0));
    if (frame > 0) {  // Section 4: if (count > 0) VO->solveNlsAll()
      vloam_status s = vo_solve_enqueue(&h->vo, h->cfg, h->s_lo, frame, h->lo, &h->prof);
      if (s != VLOAM_OK) { set_err("vo_solve_enqueue failed"); return s; }
      // the VO half of the covariance row: the solve's own factor storage at the estimate it just left in vo.x
      if (h->pose_cov) pose_cov_vo_launch(h->s_lo, h->se, h->pc, frame, h->vo.F, h->vo.x);
    }
    // vloam_tf->VO2VeloAndBase(VO->cam0_curr_T_cam0_last) + (combined mode) the first outer round's para_q / para_t overwrite
    lo_set_prior_launch(h->s_lo, h->se, h->lo, use_prior && frame > 0, h->vo.x, frame > 0, h->vo_traj + (size_t)frame * 7, &h->map.frame->error);
  }
  if (frame > 0) {  // first sweep only initialises (laser_odometry.cpp:196-204)
    for (int outer = 0; outer < 2; outer++) {  // laser_odometry.cpp:211
      if (use_prior && !(coupled && outer == 0)) lo_set_prior_launch(h->s_lo, h->se, h->lo);  // laser_odometry.cpp:223-236, both rounds (quirk A.8-4)
      FactorTable F = h->lo_F;
      F.resid = h->lo_resid[outer];
      lo_assoc_launch(h->s_lo, h->se, h->sr[cur].sharp, h->sr[cur].flat, h->sr[cur].S, h->sr[prev].less_sharp, h->sr[prev].less_flat,
                      h->sr[prev].S, h->grid[prev], h->lo, F, h->lo_corr[outer], h->lo_cyc[outer], h->lo_queue, h->lo_queue_n, h->lo_launches++, &h->prof);
      // the second solve also integrates the pose and writes the trajectory row (laser_odometry.cpp:530-531)
      lm_launch(h->s_lo, h->se, F, kMaxSharp, h->lo->para_q, h->lo_rec + outer, 4, 0.1, true, nullptr, &h->prof, outer == 1 ? h->lo : nullptr,
                outer == 1 ? h->traj + (size_t)frame * 14 : nullptr, outer == 1 ? h->ev_lo[cur] : nullptr);
    }
  } else {
    lo_finish_launch(h->s_lo, h->se, h->lo, h->traj + (size_t)frame * 14, false, &h->prof);
    HIPCHK(hipEventRecord(h->ev_lo[cur], h->s_lo));
  }
  if (h->sweep_log)
    sweep_log_lo_launch(h->s_lo, h->se, h->log_rows, frame, h->log_scratch, h->lo, h->lo_corr[0], h->lo_corr[1], h->lo_rec, &h->map.frame->fallback_solves,
                        !h->cfg.with_mapping, &h->prof, h->log_ring.bind(1, frame));
  // the information matrix of the second round's problem at the pose it returned: the table still holds that round's factors
  if (h->pose_info) {
    hipEvent_t done = h->pi_ring.bind(0, frame);
    pose_info_launch(h->s_lo, h->se, h->pi, 0, frame, h->lo_F, h->lo_rec + 1, frame > 0, nullptr, !h->cfg.with_mapping, &h->prof, h->pose_cov ? nullptr : done);
    if (h->pose_cov) pose_cov_launch(h->s_lo, h->se, h->pc, h->pi.rows, 0, frame, !h->cfg.with_mapping, done);   // from the row that launch just wrote
  }
  HIPCHK(hipGetLastError());
  if (h->cfg.timing) HIPCHK(hipEventRecord(h->ev[3], h->s_lo));
  return VLOAM_OK;
}

static vloam_status enqueue_map(vloam_handle* h, int frame) {
  poll_coop_flag(h);
  const int cur = set_of(frame);
  HIPCHK(hipStreamWaitEvent(h->s_map, h->ev_lo[cur], 0));
  HIPCHK(hipStreamWaitEvent(h->s_map, h->ev_stack[cur], 0));
  if (h->cfg.timing) HIPCHK(hipEventRecord(h->ev[4], h->s_map));
  // LaserOdometry::output: skip_frame = (frameCount % mapping_skip_frame != 0), frameCount already incremented (laser_odometry.cpp:535,618)
  const bool skip = ((frame + 1) % h->cfg.mapping_skip_frame) != 0;
  const bool sub_pose = h->sub_pose_frame == frame;   // LaserMapping::input was handed another odometry pose (vloam_set_mapping_input)
  // the registered cloud (vloam_limits::publish_registered_cloud) still reads the sweep's buffer set behind the mapping: such a sweep releases the
  // set behind k_map_register.  The published map reads the voxel tables only, so it leaves the event where it is.
  const bool publishes = map_publishes(&h->map, skip), reads_set = h->map.pub.cloud_on != 0;
  if (h->sweep_log) sweep_log_map_begin_launch(h->s_map, h->se, h->log_scratch, h->map.frame, h->map.stack_info[cur], skip, &h->prof);
  if (h->map.archive) h->map.archive->frame = frame;
  vloam_status s = map_enqueue(&h->map, h->cfg, h->s_map, h->sr[cur], h->lo, sub_pose ? h->sub_row : h->traj + (size_t)frame * 14, skip, cur, &h->prof,
                               reads_set ? nullptr : h->ev_map[cur]);
  if (s != VLOAM_OK && h->map.grow && h->map.grow->failed_log2) {   // a growth step's allocation: the old table stays in use, the sweep's mapping is enqueued by a later call
    set_err("could not allocate a voxel table of 2^%d slots (hipMalloc); the corner / surf tables stay at 2^%d / 2^%d", h->map.grow->failed_log2, h->map.grow->lg[0], h->map.grow->lg[1]);
    h->map.grow->failed_log2 = 0;
    return VLOAM_ERR_HIP;
  }
  if (s != VLOAM_OK) { set_err("map_enqueue failed: %s", hipGetErrorString(hipGetLastError())); return VLOAM_ERR_HIP; }
  if (h->sweep_log) {
    sweep_log_map_launch(h->s_map, h->se, h->log_rows, frame, h->log_scratch, h->map.state, h->map.frame, h->map.rec, skip, &h->prof, h->log_ring.bind(2, frame));
    HIPCHK(hipGetLastError());
  }
  // behind k_map_finalize: the second round's table is not rewritten before the next sweep's fit, and MapState::do_optimize is still this sweep's
  if (h->pose_info) {
    hipEvent_t done = h->pi_ring.bind(1, frame);
    pose_info_launch(h->s_map, h->se, h->pi, 1, frame, h->map.F[1], h->map.rec + 1, !skip, &h->map.state->do_optimize, true, &h->prof, h->pose_cov ? nullptr : done);
    if (h->pose_cov) pose_cov_launch(h->s_map, h->se, h->pc, h->pi.rows, 1, frame, true, done);
    HIPCHK(hipGetLastError());
  }
  if (sub_pose) HIPCHK(hipMemcpyAsync(h->traj + (size_t)frame * 14 + 7, h->sub_row + 7, 7 * sizeof(double), hipMemcpyDeviceToDevice, h->s_map));   // the map half of the log
  if (publishes) {
    const bool sub_cloud = h->sub_cloud_frame == frame;   // laserCloudFullRes as handed to LaserMapping::input (what vloam_get_features(h, 11) shows)
    s = map_publish_enqueue(&h->map, h->s_map, sub_cloud ? h->sub.cloud : h->sr[cur].cloud, sub_cloud ? h->sub.S : h->sr[cur].S, frame, skip, &h->prof,
                            reads_set ? h->ev_map[cur] : nullptr);
    if (s != VLOAM_OK) { set_err("map_publish_enqueue failed: %s", hipGetErrorString(hipGetLastError())); return VLOAM_ERR_HIP; }
  }
  if (h->cfg.timing) HIPCHK(hipEventRecord(h->ev[5], h->s_map));
  return VLOAM_OK;
}

// vloam_process_scan leaves the odometry of its sweep (and the mapping of the sweep before) to the NEXT call: by then the
// producing stage has normally finished, hipStreamWaitEvent on a completed event inserts nothing, and the ~11 us cross-stream
// barrier packet disappears from the stream that bounds the throughput.  Everything that reads results drains first (sync_all).
vloam_status vloam::drain_deferred(vloam_handle* h, int lag_lo, int lag_map) {
  if (lag_lo == 0 && lag_map == 0) TRY(flush_pending(h));   // a full drain: the host sweep still in flight first
  while (h->lo_done < h->frame - lag_lo) {
    const double t0 = g_host_prof ? now_s() : 0.0;
    vloam_status s = enqueue_lo(h, h->lo_done);
    if (g_host_prof) h->host_s[2] += now_s() - t0;
    if (s != VLOAM_OK) return s;
    h->lo_done++;
  }
  if (!h->cfg.with_mapping) { h->map_done = h->lo_done; return VLOAM_OK; }
  const int lim = h->frame - lag_map < h->lo_done ? h->frame - lag_map : h->lo_done;
  while (h->map_done < lim) {
    const double t0 = g_host_prof ? now_s() : 0.0;
    vloam_status s = enqueue_map(h, h->map_done);
    if (g_host_prof) h->host_s[3] += now_s() - t0;
    if (s != VLOAM_OK) return s;
    h->map_done++;
  }
  return VLOAM_OK;
}

static vloam_status finish_frame(vloam_handle* h) {
  if (h->cfg.timing) {  // per-stage times need the sweep drained: timing mode gives up the overlap between sweeps
    TRY(sync_all(h));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, h->ev[0], h->ev[1])); h->stage_ms[0] += ms;
    HIPCHK(hipEventElapsedTime(&ms, h->ev[2], h->ev[3])); h->stage_ms[1] += ms;
    if (h->cfg.with_mapping) { HIPCHK(hipEventElapsedTime(&ms, h->ev[4], h->ev[5])); h->stage_ms[2] += ms; }
    h->timed_scans++;
  }
  h->frame++;
  h->stage = 0;
  if (h->lo_done < h->frame) h->lo_done = h->frame;    // stage-wise callers may leave stages out: nothing is owed for this sweep
  if (h->map_done < h->frame) h->map_done = h->frame;
  return VLOAM_OK;
}

// ------------------------------------------------------------------ host sweeps in
// Two forms (vloam_handle: "Host sweeps").
//   INLINE: hipMemcpyAsync on the scan-registration stream itself into the inline buffer, no events — the stream's order IS the dependency.
//     Every host-pointer entry point except the two below; with VLOAM_STAGE_INLINE=1 those two as well.  The 2 MB cross the link IN FRONT of the
//     sweep's scan registration (24 GB/s inside hipMemcpyAsync: ~87 us on a stream with ~30 us to spare per period): 0.88 - 0.92 x the
//     device-resident rate.
//   DEFERRED RING (vloam_process_scan, vloam_batch_process_scan): copy on a stream of its own into ring slot k % kInRing, the sweep enqueued
//     by the NEXT call once the HOST has seen the copy's event — no stream ever waits for another one, the copy of sweep k + 1 runs beside
//     the scan registration of sweep k: 0.95 - 0.98 x (tools/host_input_probe.py).  Rounds 4 - 5 had a ring WITHOUT the deferral (two live
//     cross-stream waits per sweep): 2 200 - 4 400 scans/s depending on what else the process had created (profiles/r05_host_input.txt); a copy
//     KERNEL reading the pinned buffer (49 GB/s) slows every kernel beside it by ~45 us (profiles/r06_host_input.txt).  Both are gone.
// Pageable source memory: hipMemcpyAsync has taken its copy when it returns (the caller may reuse the buffer at once).  Pinned source
// memory (hipHostMalloc / hipHostRegister) is read by DMA later: it must stay unchanged until the next vloam_sync() (c_api.h).

// The inline form, session b of a call.  Whatever host sweep is still pending goes first, once per call: it is older than this call's sweep.
vloam_status vloam::stage_inline(vloam_handle* h, int b, const float* xyz_pad4, int n, const void** d_out) {
  if (b == 0) TRY(flush_pending(h));
  float4* dst = (float4*)((char*)(h->d_in + (size_t)vloam_handle::kInRing * (size_t)h->cfg.max_points) + (size_t)b * h->se.ss);
  HIPCHK(hipMemcpyAsync(dst, xyz_pad4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
  *d_out = dst;
  return VLOAM_OK;
}
static vloam_status process_scan_batch(vloam_handle* h, const BatchIn& bi);
// the host sweep whose copy is in flight: enqueue it (every drain, every new sweep of whatever kind, vloam_sync)
static vloam_status flush_pending(vloam_handle* h) {
  if (!h->pend.valid) return VLOAM_OK;
  h->pend.valid = false;
  const int slot = h->pend.slot;
  HIPCHK(hipEventSynchronize(h->ev_in_copied[slot]));   // host side; the copy was enqueued a whole call ago
  const vloam_status st = process_scan_batch(h, h->pend.bi);
  // the slot's last reader is this sweep's scan registration (its event belongs to the sweep until the buffer set comes round again: kInRing < kSets)
  h->in_reader[slot] = st == VLOAM_OK ? h->ev_sr[set_of(h->frame - 1)] : nullptr;
  if (st != VLOAM_OK) HIPCHK(hipStreamSynchronize(h->stream));   // a refused sweep: whatever was enqueued before the refusal may still read the slot
  return st;
}
static vloam_status host_scan_deferred(vloam_handle* h, const float* const* xyz_pad4, const int* n) {
  if (handed_over(h) >= h->cfg.max_frames) { set_err("trajectory log full (max_frames=%d)", h->cfg.max_frames); return VLOAM_ERR_CAPACITY; }
  if (!h->s_copy) HIPCHK(hipStreamCreateWithPriority(&h->s_copy, hipStreamNonBlocking, h->prio[vloam_plan::kCopy]));   // (plan.copy_first: created by vloam_create)
  if (!h->ev_in_copied[0]) for (int k = 0; k < vloam_handle::kInRing; k++) HIPCHK(hipEventCreateWithFlags(&h->ev_in_copied[k], hipEventDisableTiming));
  const int slot = h->in_next % vloam_handle::kInRing;
  h->in_next++;
  // host side.  The slot's reader was enqueued kInRing - 1 calls ago; it can still be running while the host sprints ahead at the start of a
  // burst (measured: without this wait the last pose of a 300-sweep run changes from run to run)
  if (h->in_reader[slot]) HIPCHK(hipEventSynchronize(h->in_reader[slot]));
  const void* d[kMaxBatch];
  for (int b = 0; b < h->se.B; b++) {
    float4* dst = (float4*)((char*)(h->d_in + (size_t)slot * (size_t)h->cfg.max_points) + (size_t)b * h->se.ss);
    HIPCHK(hipMemcpyAsync(dst, xyz_pad4[b], (size_t)n[b] * sizeof(float4), hipMemcpyHostToDevice, h->s_copy));
    d[b] = dst;
  }
  HIPCHK(hipEventRecord(h->ev_in_copied[slot], h->s_copy));
  const vloam_status st = flush_pending(h);   // the sweep before this one
  h->pend.bi = batch_in(h, d, n); h->pend.slot = slot; h->pend.valid = true;
  return st;
}
static_assert(vloam_handle::kInRing < vloam_handle::kSets, "a slot's reader event (per buffer set) must not be re-recorded before the slot is reused");

extern "C" {

// ------------------------------------------------------------------ stage-wise API (façade order)
vloam_status vloam_scan_registration_device(vloam_handle* h, const void* d_xyz_pad4, int n) {
  if (!h || !d_xyz_pad4) return VLOAM_ERR_INVALID;
  SINGLE_SESSION_ONLY(h);
  HIPCHK(hipSetDevice(h->device));
  if (h->stage == 2) TRY(finish_frame(h));  // previous sweep ended after LO (no mapping call)
  TRY(drain_deferred(h, 0, 0));               // stages owed by earlier vloam_process_scan calls
  return enqueue_sr(h, batch_in(h, &d_xyz_pad4, &n));
}

vloam_status vloam_scan_registration(vloam_handle* h, const float* xyz_pad4, int n) {
  if (!h || !xyz_pad4) return VLOAM_ERR_INVALID;
  SINGLE_SESSION_ONLY(h);
  TRY(check_host_sweeps(h, &xyz_pad4, &n));
  HIPCHK(hipSetDevice(h->device));
  const void* d = nullptr;
  TRY(stage_inline(h, 0, xyz_pad4, n, &d));
  return vloam_scan_registration_device(h, d, n);
}

static vloam_status read_sr_error(vloam_handle* h, int cur) {
  int err = 0;
  TRY(sync_all(h));
  HIPCHK(hipMemcpy(&err, &SEL(h, h->sr[cur].S)->error, sizeof(int), hipMemcpyDeviceToHost));
  if (err & kErrEmpty) { set_err("no point survived NaN / minimum_range removal"); return VLOAM_ERR_EMPTY; }
  if (err & kErrRingTooLong) { set_err("a ring holds more than %d points", h->cfg.max_ring_points); return VLOAM_ERR_CAPACITY; }
  return VLOAM_OK;
}

vloam_status vloam_set_lo_prior(vloam_handle* h, const double q[4], const double t[3]) {
  if (!h || !q || !t) return VLOAM_ERR_INVALID;
  SINGLE_SESSION_ONLY(h);
  HIPCHK(hipSetDevice(h->device));
  TRY(drain_deferred(h, 0, 0));  // the prior belongs to the NEXT sweep's odometry
  double buf[7] = {q[0], q[1], q[2], q[3], t[0], t[1], t[2]};
  HIPCHK(hipMemcpyAsync(h->lo->prior_q, buf, sizeof(buf), hipMemcpyHostToDevice, h->s_lo));
  HIPCHK(hipStreamSynchronize(h->s_lo));
  return VLOAM_OK;
}

// LaserOdometry::input with clouds that are NOT what scan registration left on the device (the reference deep-copies whatever it is handed,
// laser_odometry.cpp:141-145).  Between vloam_scan_registration and vloam_laser_odometry; a null cloud keeps the device's.  The clouds go
// into the sweep's buffer set, and what scan registration had derived from them is rebuilt: counts, the NN grids over the two less-clouds
// (the NEXT sweep's CornerLast / SurfLast, laser_odometry.cpp:506-526) and the mapping stage's VoxelGrid of them.
vloam_status vloam_set_odometry_input(vloam_handle* h, const float* laserCloud, int n_full, const float* cornerPointsSharp, int n_sharp,
                                      const float* cornerPointsLessSharp, int n_less_sharp, const float* surfPointsFlat, int n_flat,
                                      const float* surfPointsLessFlat, int n_less_flat) {
  if (!h) return VLOAM_ERR_INVALID;
  SINGLE_SESSION_ONLY(h);
  HIPCHK(hipSetDevice(h->device));
  if (h->stage != 1) { set_err("vloam_set_odometry_input belongs between scan registration and laser odometry"); return VLOAM_ERR_ORDER; }
  const float* src[5] = {laserCloud, cornerPointsSharp, cornerPointsLessSharp, surfPointsFlat, surfPointsLessFlat};
  int n[5] = {n_full, n_sharp, n_less_sharp, n_flat, n_less_flat};
  const int cap[5] = {h->cfg.max_points, kMaxSharp, kMaxLessSharp, kMaxFlat, h->cfg.max_points};
  for (int k = 0; k < 5; k++) {
    if (!src[k]) { n[k] = -1; continue; }
    if (n[k] < 0) { set_err("negative cloud size"); return VLOAM_ERR_INVALID; }
    if (n[k] > cap[k]) { set_err("substituted cloud %d holds %d points, the buffer takes %d", k, n[k], cap[k]); return VLOAM_ERR_CAPACITY; }
  }
  {   // the two less-clouds are the next sweep's CornerLast / SurfLast, walked by scan line (stage_input_check.h)
    static const char* const names[5] = {"laserCloud (cloud 0)", "cornerPointsSharp (cloud 1)", "cornerPointsLessSharp (cloud 2)", "surfPointsFlat (cloud 3)",
                                         "surfPointsLessFlat (cloud 4)"};
    static const bool walked[5] = {false, false, true, false, true};
    TRY(check_stage_clouds("vloam_set_odometry_input", 5, names, src, n, walked));
  }
  TRY(sync_all(h));
  const int cur = set_of(h->frame);
  const SRBuffers& b = h->sr[cur];
  float4* dst[5] = {b.cloud, b.sharp, b.less_sharp, b.flat, b.less_flat};
  for (int k = 0; k < 5; k++) if (src[k] && n[k] > 0) HIPCHK(hipMemcpy(dst[k], src[k], (size_t)n[k] * sizeof(float4), hipMemcpyHostToDevice));
  sr_adopt_launch(h->stream, b, n[0], n[1], n[2], n[3], n[4]);
  if (src[2] || src[4]) {
    lo_grid_build_launch(h->stream, h->se, b.less_sharp, b.less_flat, b.S, h->grid[cur], &h->prof);
    HIPCHK(hipEventRecord(h->ev_sr[cur], h->stream));
    TRY(enqueue_scan_feature_grid(h, b, h->frame, cur));
  } else HIPCHK(hipEventRecord(h->ev_sr[cur], h->stream));
  HIPCHK(hipGetLastError());
  return VLOAM_OK;
}

// LaserMapping::input with clouds / an odometry pose that are NOT LaserOdometry::output's (laser_mapping.cpp:167-196 copies what it is handed;
// on a skipped sweep only the pose, :172-181).  Between vloam_laser_odometry and vloam_laser_mapping; null = keep the device's.  Only this
// sweep's mapping sees them: the odometry's CornerLast / SurfLast stay what they were.
vloam_status vloam_set_mapping_input(vloam_handle* h, const float* laserCloudCornerLast, int n_corner, const float* laserCloudSurfLast, int n_surf,
                                     const float* laserCloudFullRes, int n_full, const double q_wodom_curr[4], const double t_wodom_curr[3]) {
  if (!h) return VLOAM_ERR_INVALID;
  SINGLE_SESSION_ONLY(h);
  HIPCHK(hipSetDevice(h->device));
  if (h->stage != 2 || !h->cfg.with_mapping) { set_err("vloam_set_mapping_input belongs between laser odometry and laser mapping of a handle with mapping"); return VLOAM_ERR_ORDER; }
  if ((laserCloudCornerLast && (n_corner < 0 || n_corner > kMaxLessSharp)) || (laserCloudSurfLast && (n_surf < 0 || n_surf > h->cfg.max_points)) ||
      (laserCloudFullRes && (n_full < 0 || n_full > h->cfg.max_points))) { set_err("substituted cloud does not fit its buffer"); return VLOAM_ERR_CAPACITY; }
  if ((q_wodom_curr == nullptr) != (t_wodom_curr == nullptr)) { set_err("the odometry pose is q AND t"); return VLOAM_ERR_INVALID; }
  {   // mapping does not walk by line: finiteness only (stage_input_check.h)
    static const char* const names[3] = {"laserCloudCornerLast (cloud 0)", "laserCloudSurfLast (cloud 1)", "laserCloudFullRes (cloud 2)"};
    static const bool walked[3] = {false, false, false};
    const float* src[3] = {laserCloudCornerLast, laserCloudSurfLast, laserCloudFullRes};
    const int n[3] = {n_corner, n_surf, n_full};
    TRY(check_stage_clouds("vloam_set_mapping_input", 3, names, src, n, walked));
  }
  TRY(sync_all(h));
  const int frame = h->frame, cur = set_of(frame);
  const bool skip = ((frame + 1) % h->cfg.mapping_skip_frame) != 0;
  if (q_wodom_curr) {
    double row[14];
    HIPCHK(hipMemcpy(row, h->traj + (size_t)frame * 14, sizeof(row), hipMemcpyDeviceToHost));
    memcpy(row, q_wodom_curr, 4 * sizeof(double)); memcpy(row + 4, t_wodom_curr, 3 * sizeof(double));
    HIPCHK(hipMemcpy(h->sub_row, row, sizeof(row), hipMemcpyHostToDevice));
    h->sub_pose_frame = frame;
  }
  if (!skip && (laserCloudCornerLast || laserCloudSurfLast || laserCloudFullRes)) {
    const SRBuffers& b = h->sr[cur];
    FrameScalars S;
    HIPCHK(hipMemcpy(&S, b.S, sizeof(S), hipMemcpyDeviceToHost));
    struct { const float* src; int n; float4* own; int n_own; float4* dst; } c[3] = {
      {laserCloudCornerLast, n_corner, b.less_sharp, S.n_less_sharp, h->sub.less_sharp}, {laserCloudSurfLast, n_surf, b.less_flat, S.n_less_flat, h->sub.less_flat},
      {laserCloudFullRes, n_full, b.cloud, S.N2, h->sub.cloud}};
    int n[3];
    for (int k = 0; k < 3; k++) {
      n[k] = c[k].src ? c[k].n : c[k].n_own;
      if (n[k] > 0) HIPCHK(hipMemcpy(c[k].dst, c[k].src ? (const void*)c[k].src : (const void*)c[k].own, (size_t)n[k] * sizeof(float4),
                                     c[k].src ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice));
    }
    HIPCHK(hipMemcpy(h->sub.S, &S, sizeof(S), hipMemcpyHostToDevice));
    sr_adopt_launch(h->stream, h->sub, n[2], -1, n[0], -1, n[1]);
    HIPCHK(hipStreamSynchronize(h->stream));
    h->sub_cloud_frame = frame;
    if (laserCloudCornerLast || laserCloudSurfLast)
      if (map_stack_enqueue(&h->map, h->s_ds, h->sub, cur, &h->prof, h->ev_stack[cur]) != VLOAM_OK) { set_err("map_stack_enqueue failed"); return VLOAM_ERR_HIP; }
  }
  HIPCHK(hipGetLastError());
  return VLOAM_OK;
}

vloam_status vloam_laser_odometry(vloam_handle* h, double q_w[4], double t_w[3], double q_lc[4], double t_lc[3]) {
  if (!h) return VLOAM_ERR_INVALID;
  HIPCHK(hipSetDevice(h->device));
  if (h->stage != 1) { set_err("laser odometry called before scan registration"); return VLOAM_ERR_ORDER; }
  vloam_status s = enqueue_lo(h, h->frame);
  if (s != VLOAM_OK) return s;
  h->lo_done = h->frame + 1;
  h->stage = 2;
  s = read_sr_error(h, set_of(h->frame));
  if (s != VLOAM_OK) return s;
  LOState lo;
  HIPCHK(hipMemcpy(&lo, SEL(h, h->lo), sizeof(lo), hipMemcpyDeviceToHost));
  if (q_w) memcpy(q_w, lo.q_w_curr, sizeof(double) * 4);
  if (t_w) memcpy(t_w, lo.t_w_curr, sizeof(double) * 3);
  if (q_lc) memcpy(q_lc, lo.para_q, sizeof(double) * 4);
  if (t_lc) memcpy(t_lc, lo.para_t, sizeof(double) * 3);
  if (!h->cfg.with_mapping) return finish_frame(h);
  return VLOAM_OK;
}

vloam_status vloam_laser_mapping(vloam_handle* h, double q_map[4], double t_map[3]) {
  if (!h) return VLOAM_ERR_INVALID;
  HIPCHK(hipSetDevice(h->device));
  if (h->stage != 2) { set_err("laser mapping called before laser odometry"); return VLOAM_ERR_ORDER; }
  vloam_status s = enqueue_map(h, h->frame);
  if (s != VLOAM_OK) return s;
  h->map_done = h->frame + 1;
  s = sync_all(h);
  if (s != VLOAM_OK) return s;
  // what LaserMapping::publish reports (laser_mapping.cpp:718-757): q_w_curr / t_w_curr after a mapped sweep, the
  // high-frequency pose q_wmap_wodom * q_wodom_curr after a skipped one — the map half of this sweep's trajectory row
  double row[14];
  HIPCHK(hipMemcpy(row, SEL(h, h->traj) + (size_t)h->frame * 14, sizeof(row), hipMemcpyDeviceToHost));
  if (q_map) memcpy(q_map, row + 7, sizeof(double) * 4);
  if (t_map) memcpy(t_map, row + 11, sizeof(double) * 3);
  return finish_frame(h);
}

}  // extern "C"

// ------------------------------------------------------------------ whole façade, asynchronous
// sweeps by which the odometry / mapping enqueue trails the scan registration enqueue (see drain_deferred); the buffer-reuse
// waits of enqueue_sr (odometry of sweep k - 3, mapping of sweep k - 4) stay behind what is enqueued here
static constexpr int kLagLO = 1, kLagMap = 2;
static_assert(kLagLO <= vloam_handle::kSets - 2 && kLagMap <= vloam_handle::kSets - 1, "deferred stages must be enqueued before enqueue_sr waits for them");
// what opens and closes a whole sweep, of either kind (process_scan_batch, process_frame_common)
vloam_status vloam::begin_sweep(vloam_handle* h) {
  HIPCHK(hipSetDevice(h->device));
  TRY(flush_pending(h));   // a host sweep of vloam_process_scan still in flight: the older one first
  if (h->stage == 2) TRY(finish_frame(h));
  return VLOAM_OK;
}
vloam_status vloam::end_sweep(vloam_handle* h) {
  if (h->cfg.timing) {  // per-stage times: nothing deferred, the sweep is drained in finish_frame
    TRY(enqueue_lo(h, h->frame));
    if (h->cfg.with_mapping) TRY(enqueue_map(h, h->frame));
    return finish_frame(h);
  }
  h->frame++;
  h->stage = 0;
  return drain_deferred(h, kLagLO, kLagMap);
}

static vloam_status process_scan_batch(vloam_handle* h, const BatchIn& bi) {
  TRY(begin_sweep(h));
  const double ts0 = g_host_prof ? now_s() : 0.0;
  const vloam_status s = enqueue_sr(h, bi);
  if (g_host_prof) { h->host_s[1] += now_s() - ts0; h->host_calls++; }
  if (s != VLOAM_OK) return s;
  return end_sweep(h);
}

extern "C" {

vloam_status vloam_process_scan_device(vloam_handle* h, const void* d_xyz_pad4, int n) {
  if (!h || !d_xyz_pad4) return VLOAM_ERR_INVALID;
  SINGLE_SESSION_ONLY(h);
  return process_scan_batch(h, batch_in(h, &d_xyz_pad4, &n));
}

// Batched execution: one call advances ALL sessions of the handle by one sweep (session b gets d_xyz_pad4[b], n[b] points); every kernel
// of the sweep chain is launched ONCE with the session index in blockIdx.z.  The sessions are independent sequences that share nothing
// but the launch chain; results per session through vloam_select_session + the getters.
vloam_status vloam_batch_process_scan_device(vloam_handle* h, const void* const* d_xyz_pad4, const int* n) {
  if (!h || !d_xyz_pad4 || !n) return VLOAM_ERR_INVALID;
  return process_scan_batch(h, batch_in(h, d_xyz_pad4, n));
}

vloam_status vloam_batch_process_scan(vloam_handle* h, const float* const* xyz_pad4, const int* n) {
  if (!h || !xyz_pad4 || !n) return VLOAM_ERR_INVALID;
  TRY(check_host_sweeps(h, xyz_pad4, n));
  HIPCHK(hipSetDevice(h->device));
  if (!g_stage_inline && !h->cfg.timing) return host_scan_deferred(h, xyz_pad4, n);
  const void* d[kMaxBatch];
  for (int b = 0; b < h->se.B; b++) TRY(stage_inline(h, b, xyz_pad4[b], n[b], &d[b]));
  return vloam_batch_process_scan_device(h, d, n);
}

vloam_status vloam_process_scan(vloam_handle* h, const float* xyz_pad4, int n) {
  if (!h || !xyz_pad4) return VLOAM_ERR_INVALID;
  SINGLE_SESSION_ONLY(h);
  return vloam_batch_process_scan(h, &xyz_pad4, &n);
}

}  // extern "C"
