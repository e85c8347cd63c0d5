// What a caller reads back from libvloam_hip.so: vloam_sync and its sticky errors, features, map and published clouds, trajectory, counts,
// health, stage times, the parity hooks (vloam_debug_get) and the per-kernel timer.
#include "handle.h"

// the handle's sticky map / solver error bits as the status and text vloam_sync reports them with (also vloam_map_query)
vloam_status vloam::sticky_map_status(const vloam_handle* h, int merr) {
  if ((merr & kErrMapFull) && h->map.grow) {
    set_err("voxel hash full at the growable map's ceiling (max_capacity_log2=%d; corner table 2^%d, surf table 2^%d slots)", h->map.grow->max_log2, h->map.grow->lg[0], h->map.grow->lg[1]);
    return VLOAM_ERR_CAPACITY;
  }
  if (merr & kErrMapFull) { set_err("voxel hash full (map_capacity_log2=%d)", h->cfg.map_capacity_log2); return VLOAM_ERR_CAPACITY; }
  if (merr & kErrStackFull) {
    set_err("mapping factor table full: more than %d surf points after VoxelGrid; raise vloam_limits::max_surf_stack_points", h->map.surf_cap);
    return VLOAM_ERR_CAPACITY;
  }
  if (merr & kErrMapDeferred) { set_err("raw-point capacity of the map exceeded (more than 255 un-merged points in a voxel of a cube outside the valid block, or more than 64 raw voxels around one query)"); return VLOAM_ERR_CAPACITY; }
  if (merr & kErrSolverSync) { set_err("a workgroup of the scan-feature VoxelGrid gave up waiting for the bins in front of it"); return VLOAM_ERR_HIP; }
  if (merr & kErrVoDegenerate) { set_err("a VO solve returned a zero rotation angle: poses are NaN from that frame on, as in the reference (visual_odometry.cpp:427-430)"); return VLOAM_ERR_INVALID; }
  return VLOAM_OK;
}

extern "C" {

vloam_status vloam_get_features(vloam_handle* h, int which, float* xyzi4, int cap, int* n) {
  if (!h || !n) return VLOAM_ERR_INVALID;
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));   // (first: a host sweep still in flight is enqueued by this and counts)
  const int f = shown_frame(h);
  const int cur = set_of(f);
  SRBuffers bsel = h->sr[cur];
  if (which == 11 && h->sub_cloud_frame == f) { bsel.cloud = h->sub.cloud; bsel.S = h->sub.S; }   // laserCloudFullRes as handed to LaserMapping::input
  bsel.rebase((size_t)h->sel * h->se.ss);
  FrameScalars S;
  HIPCHK(hipMemcpy(&S, bsel.S, sizeof(S), hipMemcpyDeviceToHost));
  const float4* src = nullptr;
  int cnt = 0;
  switch (which) {
    case 0: src = bsel.cloud; cnt = S.N2; break;
    case 1: src = bsel.sharp; cnt = S.n_sharp; break;
    case 2: case 5: src = bsel.less_sharp; cnt = S.n_less_sharp; break;
    case 3: src = bsel.flat; cnt = S.n_flat; break;
    case 4: case 6: src = bsel.less_flat; cnt = S.n_less_flat; break;
    default: return map_get_cloud(&h->map, h->stream, which, bsel, xyzi4, cap, n);
  }
  *n = cnt;
  const int m = cnt < cap ? cnt : cap;
  if (xyzi4 && m > 0) HIPCHK(hipMemcpy(xyzi4, src, (size_t)m * sizeof(float4), hipMemcpyDeviceToHost));
  return VLOAM_OK;
}

// == the /laser_cloud_map product of LaserMapping::publish (laser_mapping.cpp:778-793)
vloam_status vloam_get_map(vloam_handle* h, float* xyzi4, long long cap, long long* n) {
  if (!h || !n) return VLOAM_ERR_INVALID;
  if (!h->cfg.with_mapping) { *n = 0; return VLOAM_OK; }
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  return map_export(&h->map, h->s_map, xyzi4, cap, n);
}

// == the same cloud, and the registered full-resolution cloud, as the mapping stream published them (vloam_limits)
static vloam_status published_get(vloam_handle* h, int which, float* xyzi4, long long cap, long long* n, int* frame, void** d_ptr) {
  const MapPub& P = h->map.pub;
  if (which == 0 ? P.pub_number == 0 : !P.cloud_on) {
    set_err(which == 0 ? "the handle was created without vloam_limits::map_pub_number: no map is published (vloam_get_map exports it on request)"
                       : "the handle was created without vloam_limits::publish_registered_cloud (vloam_get_features(h, 11) registers the cloud on request)");
    return VLOAM_ERR_ORDER;
  }
  HIPCHK(hipSetDevice(h->device));
  TRY(drain_deferred(h, 0, 0));   // enqueue only: the publication of every sweep handed over so far is then on the mapping stream
  const vloam_status s = map_published_get(&h->map, which, xyzi4, cap, n, frame, d_ptr);
  if (s == VLOAM_ERR_CAPACITY) set_err("the map published after sweep %d holds %lld points, more than max_published_map_points = %lld", *frame, *n, P.cap);
  else if (s != VLOAM_OK) set_err("reading the published cloud failed: %s", hipGetErrorString(hipGetLastError()));
  return s;
}

vloam_status vloam_get_published_map(vloam_handle* h, float* xyzi4, long long cap, long long* n, int* frame) {
  if (!h || !n || !frame || cap < 0) return VLOAM_ERR_INVALID;
  return published_get(h, 0, xyzi4, cap, n, frame, nullptr);
}

vloam_status vloam_get_published_cloud(vloam_handle* h, float* xyzi4, int cap, int* n, int* frame) {
  if (!h || !n || !frame || cap < 0) return VLOAM_ERR_INVALID;
  long long nn = 0;
  const vloam_status s = published_get(h, 1, xyzi4, cap, &nn, frame, nullptr);
  *n = (int)nn;
  return s;
}

vloam_status vloam_published_device_ptr(vloam_handle* h, int which, void** d_xyzi4, long long* n, int* frame) {
  if (!h || !d_xyzi4 || !n || !frame || (which != 0 && which != 1)) return VLOAM_ERR_INVALID;
  return published_get(h, which, nullptr, 0, n, frame, d_xyzi4);
}

// The laser-odometry pose of the sweep in progress (after vloam_laser_odometry) or of the last finished sweep: q_w_curr / t_w_curr as
// LaserOdometry::output hands them on (laser_odometry.cpp:610-616).
vloam_status vloam_get_odometry_pose(vloam_handle* h, double q_w[4], double t_w[3]) {
  if (!h) return VLOAM_ERR_INVALID;
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  const int f = shown_frame(h);
  double row[7] = {0, 0, 0, 1, 0, 0, 0};
  if (f < h->cfg.max_frames && (h->stage == 2 || h->frame > 0)) HIPCHK(hipMemcpy(row, SEL(h, h->traj) + (size_t)f * 14, sizeof(row), hipMemcpyDeviceToHost));
  if (q_w) memcpy(q_w, row, sizeof(double) * 4);
  if (t_w) memcpy(t_w, row + 4, sizeof(double) * 3);
  return VLOAM_OK;
}

vloam_status vloam_sync(vloam_handle* h) {
  if (!h) return VLOAM_ERR_INVALID;
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  map_grow_release(&h->map);   // nothing of the handle is in flight: tables a finished growth step left behind are freed here
  if (h->frame > 0 || h->map_imported) {   // (an import can fill a fixed table before the first sweep)
    // surface sticky device-side errors: scan-registration bits of ANY sweep since the last vloam_sync (k_sr_compact folds every
    // sweep's word into the handle's sticky word; reported once, then cleared), map / solver bits for good
    int merr = 0;
    long long fb = 0;
    vloam_status s = map_error(&h->map, &merr, kErrEmpty | kErrRingTooLong, &fb);
    if (s != VLOAM_OK) return s;
    if (fb > h->fallback_solves) {
      // a cooperative solve found its partner workgroups missing and finished on one workgroup (lm_solve.hip): same answer, ~0.5 s late.
      // Whatever kept them apart (a CU-masked or partitioned device, another process' solves holding the compute units) is likely to last:
      // this handle launches one-workgroup solves from now on.
      set_no_coop(h);
    }
    h->fallback_solves = fb;
    if (merr & kErrEmpty) { set_err("no point survived NaN / minimum_range removal in at least one sweep since the last vloam_sync"); return VLOAM_ERR_EMPTY; }
    if (merr & kErrRingTooLong) { set_err("a ring held more than %d points (dropped) in at least one sweep since the last vloam_sync", h->cfg.max_ring_points); return VLOAM_ERR_CAPACITY; }
    TRY(sticky_map_status(h, merr));
  }
  if (h->img.max_w != 0 && h->img.count >= 0) {
    // the image front-end's own sticky word: a corner / match set cut by one of its capacities differs from goodFeaturesToTrack's and was
    // fed into the VO solve of the coupled loop — say so here too, not only in the vloam_vo_get_* getters
    for (int b = 0; b < h->se.B; b++) {
      int ierr = 0;
      HIPCHK(hipMemcpy(&ierr, (const char*)h->img.error + (size_t)b * h->se.ss, sizeof(int), hipMemcpyDeviceToHost));
      if (ierr) { set_err("image front-end capacity exceeded in session %d (bits %d: 1 candidates > %d, 2 neighbours > %d, 4 corners > %d)", b, ierr, kImgCandCap, kImgNbrCap, kImgAccCap); return VLOAM_ERR_CAPACITY; }
    }
  }
  return VLOAM_OK;
}

vloam_status vloam_get_trajectory(vloam_handle* h, int first, int count, double* poses14) {
  if (!h || !poses14 || first < 0 || count < 0 || first + count > handed_over(h)) return VLOAM_ERR_INVALID;   // (a host sweep in flight is enqueued by the sync below)
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  if (count) HIPCHK(hipMemcpy(poses14, SEL(h, h->traj) + (size_t)first * 14, sizeof(double) * 14 * (size_t)count, hipMemcpyDeviceToHost));
  return VLOAM_OK;
}
vloam_status vloam_frame_count(vloam_handle* h, int* frames) {
  if (!h || !frames) return VLOAM_ERR_INVALID;
  *frames = handed_over(h);   // sweeps handed over (the last host sweep may still be in flight: deferred ring)
  return VLOAM_OK;
}
vloam_status vloam_trajectory_device_ptr(vloam_handle* h, void** d_ptr, long long* bytes) {
  if (!h || !d_ptr || !bytes) return VLOAM_ERR_INVALID;
  *d_ptr = SEL(h, h->traj);
  *bytes = (long long)h->cfg.max_frames * 14 * (long long)sizeof(double);
  return VLOAM_OK;
}

// ------------------------------------------------------------------ parity hooks
// copy_dev (vloam_device.h) + what HIPCHK adds to a failure: the text of vloam_last_error
static vloam_status copy_out(const void* d_src, size_t bytes, void* buf, long long cap, long long* n) {
  const vloam_status s = copy_dev(d_src, bytes, buf, cap, n);
  if (s != VLOAM_OK) set_err("hipMemcpy(buf, d_src, m, hipMemcpyDeviceToHost) failed: %s (%s:%d)", hipGetErrorString(hipPeekAtLastError()), __FILE__, __LINE__);
  return s;
}

vloam_status vloam_debug_get(vloam_handle* h, int stage, int item, void* buf, long long cap, long long* n) {
  if (!h) return VLOAM_ERR_INVALID;
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  const int f = shown_frame(h);
  const int cur = set_of(f);
  if (stage == 0) {
    SRBuffers b = h->sr[cur];
    b.rebase((size_t)h->sel * h->se.ss);
    FrameScalars S;
    HIPCHK(hipMemcpy(&S, b.S, sizeof(S), hipMemcpyDeviceToHost));
    switch (item) {
      case 0: return copy_out(b.dbg_curv, sizeof(float) * S.N2, buf, cap, n);
      case 1: return copy_out(b.dbg_sort, sizeof(int) * S.N2, buf, cap, n);
      case 2: return copy_out(b.dbg_picked, sizeof(int) * S.N2, buf, cap, n);
      case 3: return copy_out(b.dbg_label, sizeof(int) * S.N2, buf, cap, n);
      case 11: return copy_out(b.dbg_cyc, sizeof(long long) * kMaxRings * 8, buf, cap, n);
      case 4: return copy_out(&b.S->scanStartInd[0], sizeof(int) * kMaxRings, buf, cap, n);
      case 5: return copy_out(&b.S->scanEndInd[0], sizeof(int) * kMaxRings, buf, cap, n);
      case 6: return copy_out(b.dbg_feat_idx, sizeof(int) * S.n_sharp, buf, cap, n);
      case 7: return copy_out(b.dbg_feat_idx + kMaxLessSharp, sizeof(int) * S.n_less_sharp, buf, cap, n);
      case 8: return copy_out(b.dbg_feat_idx + 2 * kMaxLessSharp, sizeof(int) * S.n_flat, buf, cap, n);
      case 9: {
        float sc[5] = {S.startOri, S.endOri, (float)S.istar, (float)S.n_after_s1, (float)S.N2};
        if (n) *n = sizeof(sc);
        if (buf) memcpy(buf, sc, (size_t)cap < sizeof(sc) ? (size_t)cap : sizeof(sc));
        return VLOAM_OK;
      }
      case 10: return copy_out(b.S, sizeof(FrameScalars), buf, cap, n);
    }
    return VLOAM_ERR_INVALID;
  }
  if (stage == 1) {
    const int outer = item / 16, k = item % 16;
    if (outer < 0 || outer > 1) return VLOAM_ERR_INVALID;
    switch (k) {
      case 0: return copy_out(SEL(h, h->lo_corr[outer]), sizeof(int) * 4 * kMaxSharp, buf, cap, n);
      case 1: return copy_out(SEL(h, h->lo_corr[outer]) + 4 * kMaxSharp, sizeof(int) * 4 * kMaxFlat, buf, cap, n);
      case 2: return copy_out(SEL(h, h->lo_rec) + outer, sizeof(LMRecord), buf, cap, n);
      case 3: return copy_out(SEL(h, h->lo_resid[outer]), sizeof(double) * 3 * kMaxLoFactors, buf, cap, n);
      case 6: return copy_out(SEL(h, h->lo_queue), sizeof(int) * kMaxLoFactors, buf, cap, n);   // the queue itself: slot | reason << 16 (1 block over capacity, 2 closest point beyond 1 m, 3 dense 5 m neighbourhood)
      case 5: return copy_out(SEL(h, h->lo_queue_n), sizeof(int) * 2, buf, cap, n);   // queries k_lo_assoc_fast left to the wave-per-query pass (last launch pair of a batch)
      case 4: if (!h->lo_cyc[outer]) return VLOAM_ERR_INVALID;
              return copy_out(SEL(h, h->lo_cyc[outer]), sizeof(long long) * 4 * kMaxLoFactors, buf, cap, n);
    }
    return VLOAM_ERR_INVALID;
  }
  if (stage == 2 && item == 70) {  // test hook: rebuild both voxel tables now (the production trigger is k_map_finalize's host-mapped flag)
    if (n) *n = 0;
    return h->cfg.with_mapping ? map_force_rebuild(&h->map, h->s_map) : VLOAM_OK;
  }
  if (stage == 2 && item == 74) {  // test hook: one growth step of both tables of a growable handle now (the production trigger is map_enqueue's bound)
    if (n) *n = 0;
    return map_force_grow(&h->map, h->s_map);
  }
  if (stage == 2) return map_debug_get(&h->map, item, buf, cap, n);
  if (stage == 3) return vo_debug_get(&h->vo, item, buf, cap, n);
  if (stage == 4) return img_debug_get(&h->img, item, buf, cap, n);
  return VLOAM_ERR_INVALID;
}

// Per-kernel HIP-event timer: every launch of the named kernel (its __global__ symbol, e.g. "k_lo_assoc") is
// bracketed by an event pair on the handle's stream; max_launches bounds the event pool.  name == "" disables.
vloam_status vloam_profile_kernel(vloam_handle* h, const char* name, int max_launches) {
  if (!h || !name) return VLOAM_ERR_INVALID;
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  int id = kKNone;
  for (int k = 1; k < kKCount; k++) if (strcmp(name, kKernelNames[k]) == 0) id = k;
  if (strcmp(name, "*") == 0) id = kKAll;  // every launch of every kernel (vloam_profile_read_table)
  if (id == kKNone && name[0] != 0) { set_err("unknown kernel %s", name); return VLOAM_ERR_INVALID; }
  while ((int)h->prof_events.size() < 2 * max_launches) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    h->prof_events.push_back(e);
  }
  h->prof_kids.assign((size_t)max_launches + 1, 0);
  h->prof.id = id;
  h->prof.kid_of = h->prof_kids.data();
  h->prof.ev = h->prof_events.data();
  h->prof.cap = max_launches;
  h->prof.used = 0;
  return VLOAM_OK;
}
vloam_status vloam_profile_read(vloam_handle* h, double* total_ms, int* launches) {
  if (!h || !total_ms || !launches) return VLOAM_ERR_INVALID;
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  double tot = 0;
  for (int k = 0; k < h->prof.used; k++) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, h->prof.ev[2 * k], h->prof.ev[2 * k + 1]));
    tot += ms;
  }
  *total_ms = tot;
  *launches = h->prof.used;
  h->prof.used = 0;
  return VLOAM_OK;
}

// Per-kernel totals of the recorded launches (all-kernel mode "*", or the one selected kernel): ms[k], launches[k] for kernel id k
// < n_kernels; names through vloam_profile_kernel_name.  Resets the recorder like vloam_profile_read.
vloam_status vloam_profile_read_table(vloam_handle* h, int n_kernels, double* ms, int* launches) {
  if (!h || !ms || !launches || n_kernels < 0) return VLOAM_ERR_INVALID;
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  for (int k = 0; k < n_kernels; k++) { ms[k] = 0; launches[k] = 0; }
  for (int k = 0; k < h->prof.used; k++) {
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, h->prof.ev[2 * k], h->prof.ev[2 * k + 1]));
    const int kid = h->prof.kid_of[k];
    if (kid >= 0 && kid < n_kernels) { ms[kid] += t; launches[kid]++; }
  }
  h->prof.used = 0;
  return VLOAM_OK;
}
int vloam_profile_kernel_count(void) { return kKCount; }
const char* vloam_profile_kernel_name(int k) { return (k >= 0 && k < kKCount) ? kKernelNames[k] : ""; }

// {cooperative solves that degraded to one workgroup (all sessions), 1 if the handle has switched to one-workgroup solves, voxel-table
// rebuilds, growable handles: growth steps, log2 of the corner table, log2 of the surf table, 0 ...}
vloam_status vloam_get_health(vloam_handle* h, long long out8[8]) {
  if (!h || !out8) return VLOAM_ERR_INVALID;
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  for (int k = 0; k < 8; k++) out8[k] = 0;
  int merr = 0;
  long long fb = 0;
  if (h->frame > 0) TRY(map_error(&h->map, &merr, 0, &fb));
  out8[0] = fb; out8[1] = h->se.no_coop; out8[2] = h->map.rebuilds;
  if (h->map.grow) { out8[3] = h->map.grow->steps; out8[4] = h->map.grow->lg[0]; out8[5] = h->map.grow->lg[1]; }
  return VLOAM_OK;
}

vloam_status vloam_get_stage_ms(vloam_handle* h, double ms4[4], int* scans) {
  if (!h || !ms4) return VLOAM_ERR_INVALID;
  for (int k = 0; k < 4; k++) ms4[k] = h->stage_ms[k];
  if (scans) *scans = h->timed_scans;
  return VLOAM_OK;
}

vloam_status vloam_get_counts(vloam_handle* h, long long c[16]) {
  if (!h || !c) return VLOAM_ERR_INVALID;
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  memset(c, 0, sizeof(long long) * 16);
  if (h->frame == 0) return VLOAM_OK;
  const int f = shown_frame(h);
  const int cur = set_of(f), prev = set_of(f + vloam_handle::kSets - 1);
  FrameScalars S, Sp;
  HIPCHK(hipMemcpy(&S, SEL(h, h->sr[cur].S), sizeof(S), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&Sp, SEL(h, h->sr[prev].S), sizeof(Sp), hipMemcpyDeviceToHost));
  LMRecord rec[2];
  HIPCHK(hipMemcpy(rec, SEL(h, h->lo_rec), sizeof(rec), hipMemcpyDeviceToHost));
  c[0] = h->last_n_in; c[1] = S.N2; c[2] = S.n_sharp; c[3] = S.n_less_sharp; c[4] = S.n_flat; c[5] = S.n_less_flat;
  c[6] = Sp.n_less_sharp; c[7] = Sp.n_less_flat;
  if (f > 0) {
    // factor counts of the 2nd outer round; evaluations summed over both rounds
    int corr[4 * kMaxLoFactors];
    HIPCHK(hipMemcpy(corr, SEL(h, h->lo_corr[1]), sizeof(corr), hipMemcpyDeviceToHost));
    for (int k = 0; k < kMaxLoFactors; k++) if (corr[4 * k] >= 0) c[k < kMaxSharp ? 8 : 9]++;
    c[10] = (long long)(rec[0].n_evals + rec[1].n_evals);
  }
  return map_counts(&h->map, c);
}

}  // extern "C"
