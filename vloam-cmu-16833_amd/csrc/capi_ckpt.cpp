// Checkpoint size / save / load of libvloam_hip.so.
#include "handle.h"

extern "C" {

// ------------------------------------------------------------------ checkpoint and restore (c_api.h; format: ckpt_format.h; map: map_ckpt.hip)
// What a sweep reads that an earlier sweep wrote: LOState; the previous sweep's cornerPointsLessSharp / surfPointsLessFlat with its FrameScalars
// (the NN grids over them are rebuilt by load); MapState, cube_cnt, the two voxel tables (live records; slots, blocks, pend[], tombstones and
// the deferred lists are rebuilt), the trajectory rows (the mapping reads the odometry half of its sweep's row) and the host-side counters:
// sweeps taken (= the buffer-set rotation and the skip-frame phase), mapped sweeps, ds_gen, the odometry's launch parity.  The arrival-stamp
// sweep number is MapState::sweep_no.  Scratch — everything a stage rewrites before it reads it — is not stored.
static vloam_ckpt::CkptExpect ckpt_expect() {
  vloam_ckpt::CkptExpect ex;
  memset(&ex, 0, sizeof(ex));
  ex.struct_size[vloam_ckpt::kSzLoState] = (int)sizeof(LOState); ex.struct_size[vloam_ckpt::kSzMapState] = (int)sizeof(MapState);
  ex.struct_size[vloam_ckpt::kSzVoxelRec] = (int)sizeof(VoxelRec); ex.struct_size[vloam_ckpt::kSzFrameScalars] = (int)sizeof(FrameScalars);
  ex.struct_size[vloam_ckpt::kSzSweepRecord] = (int)sizeof(vloam_sweep_record); ex.struct_size[vloam_ckpt::kSzCubeInts] = 2 * kCubeNum;
  return ex;
}
// bench hook (tools): VLOAM_CKPT_TIMES=1 prints the map kernels' times of every save / load to stderr
static const bool g_ckpt_times = getenv("VLOAM_CKPT_TIMES") != nullptr;

// the refusals of size / save, the drain, and the header of a checkpoint taken now
static vloam_status ckpt_describe(vloam_handle* h, const char* call, vloam_ckpt::CkptHeader* hd) {
  using namespace vloam_ckpt;
  if (h->se.B != 1) { set_err("%s: a checkpoint holds one sequence: the handle has n_sessions = %d", call, h->se.B); return VLOAM_ERR_INVALID; }
  if (h->vo_used) { set_err("%s: the sequence used a VO, frame or image entry point: the VO's previous-frame state is not saved", call); return VLOAM_ERR_ORDER; }
  if (h->stage != 0) { set_err("%s: the handle is in the middle of a stage-wise sweep (stage %d): finish the sweep first", call, h->stage); return VLOAM_ERR_ORDER; }
  TRY(vloam_sync(h));   // drains (a deferred host sweep, trailing odometry and mapping), synchronises, and reports a sticky error as it would
  memset(hd, 0, sizeof(*hd));
  memcpy(hd->magic, kMagic, sizeof(kMagic));
  hd->version = kVersion; hd->header_bytes = (int)sizeof(CkptHeader);
  const CkptExpect ex = ckpt_expect();
  memcpy(hd->struct_size, ex.struct_size, sizeof(ex.struct_size));
  hd->scan_line = h->cfg.scan_line; hd->mapping_skip_frame = h->cfg.mapping_skip_frame; hd->detach_VO_LO = h->cfg.detach_VO_LO ? 1 : 0;
  hd->with_mapping = h->cfg.with_mapping ? 1 : 0; hd->stack_tier = h->map.tier() ? 1 : 0;
  hd->mapping_line_resolution = h->cfg.mapping_line_resolution; hd->mapping_plane_resolution = h->cfg.mapping_plane_resolution;
  hd->minimum_range = h->cfg.minimum_range;
  hd->frames = h->frame; hd->mapped = h->map.pub.mapped; hd->ds_gen = h->map.ds_gen; hd->lo_launches = h->lo_launches;
  if (h->frame > 0) {
    FrameScalars S;
    HIPCHK(hipMemcpy(&S, h->sr[(h->frame - 1) % vloam_handle::kSets].S, sizeof(S), hipMemcpyDeviceToHost));
    hd->n_less[0] = std::max(0, std::min(S.n_less_sharp, kMaxLessSharp)); hd->n_less[1] = std::max(0, std::min(S.n_less_flat, h->cfg.max_points));
  }
  if (h->cfg.with_mapping) {
    MapState ms;
    MapFrame fr;
    HIPCHK(hipMemcpy(&ms, h->map.state, sizeof(ms), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&fr, h->map.frame, sizeof(fr), hipMemcpyDeviceToHost));
    hd->n_stack[0] = std::max(0, std::min(ms.n_corner_stack, kStackCapCorner)); hd->n_stack[1] = std::max(0, std::min(ms.n_surf_stack, h->map.surf_cap));
    for (int k = 0; k < 2; k++) {
      int stats[4];
      HIPCHK(hipMemcpy(stats, h->map.tab[k].stats, sizeof(stats), hipMemcpyDeviceToHost));
      hd->n_blk[k] = stats[2];
      hd->n_deferred[k] = fr.n_deferred[k] + fr.n_newraw[k];
    }
  }
  hd->n_sections = kSecCount;
  return VLOAM_OK;
}
static void ckpt_finish_header(vloam_handle* h, vloam_ckpt::CkptHeader* hd) {
  using namespace vloam_ckpt;
  const long long have = hd->frames > 0 ? 1 : 0, m = hd->with_mapping ? 1 : 0;
  const long long cnt[kSecCount] = {1, m, m * 2 * kCubeNum, hd->n_rec[0] + hd->n_rec[1], have, hd->n_less[0], hd->n_less[1], hd->n_stack[0], hd->n_stack[1],
                                    hd->frames, h->sweep_log ? hd->frames : 0};
  for (int s = 0; s < kSecCount; s++) hd->sec[s].count = cnt[s];
  for (int k = 0; k < 2; k++) hd->n_deferred[k] = (int)std::min<long long>(hd->n_deferred[k], hd->n_rec[k]);
  layout(hd);
  hd->checksum = header_checksum(*hd);
}

vloam_status vloam_checkpoint_size(vloam_handle* h, long long* bytes) {
  if (!h || !bytes) { set_err("vloam_checkpoint_size: null argument"); return VLOAM_ERR_INVALID; }
  HIPCHK(hipSetDevice(h->device));
  vloam_ckpt::CkptHeader hd;
  TRY(ckpt_describe(h, "vloam_checkpoint_size", &hd));
  if (h->cfg.with_mapping && map_ckpt_pack(&h->map, h->s_map, hd.n_rec, nullptr, nullptr) != VLOAM_OK) { set_err("vloam_checkpoint_size: counting the map's records failed: %s", hipGetErrorString(hipGetLastError())); return VLOAM_ERR_HIP; }
  ckpt_finish_header(h, &hd);
  *bytes = hd.total_bytes;
  return VLOAM_OK;
}

vloam_status vloam_checkpoint_save(vloam_handle* h, void* buf, long long cap, long long* bytes) {
  using namespace vloam_ckpt;
  if (!h || !bytes || (!buf && cap > 0)) { set_err("vloam_checkpoint_save: null argument"); return VLOAM_ERR_INVALID; }
  HIPCHK(hipSetDevice(h->device));
  CkptHeader hd;
  TRY(ckpt_describe(h, "vloam_checkpoint_save", &hd));
  VoxelRec* d_recs = nullptr;
  float ms[2] = {0.f, 0.f};
  if (h->cfg.with_mapping && map_ckpt_pack(&h->map, h->s_map, hd.n_rec, nullptr, nullptr) != VLOAM_OK) { set_err("vloam_checkpoint_save: counting the map's records failed: %s", hipGetErrorString(hipGetLastError())); return VLOAM_ERR_HIP; }
  ckpt_finish_header(h, &hd);
  *bytes = hd.total_bytes;
  if (cap < hd.total_bytes) { set_err("vloam_checkpoint_save: the checkpoint takes %lld bytes, the buffer holds %lld", hd.total_bytes, cap); return VLOAM_ERR_CAPACITY; }
  if (h->cfg.with_mapping) {
    long long n2[2];
    if (map_ckpt_pack(&h->map, h->s_map, n2, &d_recs, ms) != VLOAM_OK) { set_err("vloam_checkpoint_save: packing the map failed: %s", hipGetErrorString(hipGetLastError())); return VLOAM_ERR_HIP; }
    if (n2[0] != hd.n_rec[0] || n2[1] != hd.n_rec[1]) { (void)hipFree(d_recs); set_err("vloam_checkpoint_save: the map changed while it was saved (internal)"); return VLOAM_ERR_HIP; }
    if (g_ckpt_times) fprintf(stderr, "[vloam ckpt] pack: count+scan %.1f us, scatter %.1f us, %lld records, tables 2^%d / 2^%d slots\n", 1e3 * ms[0], 1e3 * ms[1], n2[0] + n2[1],
                              __builtin_ctz(h->map.tab[0].mask + 1), __builtin_ctz(h->map.tab[1].mask + 1));
  }
  char* out = (char*)buf;
  memset(out, 0, (size_t)hd.total_bytes);   // (the padding between sections)
  memcpy(out, &hd, sizeof(hd));
  const int last = h->frame > 0 ? (h->frame - 1) % vloam_handle::kSets : 0;
  const void* src[kSecCount] = {h->lo, h->map.state, h->map.cube_cnt, d_recs, h->sr[last].S, h->sr[last].less_sharp, h->sr[last].less_flat,
                                h->map.stack[0], h->map.stack[1], h->traj, h->log_rows};
  vloam_status rc = VLOAM_OK;
  for (int s = 0; s < kSecCount && rc == VLOAM_OK; s++)
    if (hd.sec[s].bytes > 0 && hipMemcpy(out + hd.sec[s].offset, src[s], (size_t)hd.sec[s].bytes, hipMemcpyDeviceToHost) != hipSuccess) {
      set_err("vloam_checkpoint_save: reading section %d failed: %s", s, hipGetErrorString(hipGetLastError())); rc = VLOAM_ERR_HIP;
    }
  if (d_recs) (void)hipFree(d_recs);
  return rc;
}

vloam_status vloam_checkpoint_load(vloam_handle* h, const void* buf, long long bytes) {
  using namespace vloam_ckpt;
  // the format first: before any device call, before anything of the handle is looked at
  CkptHeader hd;
  char why[256];
  if (!ckpt_parse(buf, bytes, ckpt_expect(), &hd, why, sizeof(why))) { set_err("vloam_checkpoint_load: %s", why); return VLOAM_ERR_INVALID; }
  if (!h) { set_err("vloam_checkpoint_load: null handle"); return VLOAM_ERR_INVALID; }
  if (h->se.B != 1) { set_err("vloam_checkpoint_load: a checkpoint holds one sequence: the handle has n_sessions = %d", h->se.B); return VLOAM_ERR_INVALID; }
  if (h->map_imported) { set_err("vloam_checkpoint_load: the handle has imported a map (vloam_map_import): load works on a handle right after its creation"); return VLOAM_ERR_ORDER; }
  if (!is_fresh(h) || h->vo_used) {
    set_err("vloam_checkpoint_load: the handle is not fresh (%d sweeps taken, stage %d): load works on a handle right after its creation", handed_over(h), h->stage);
    return VLOAM_ERR_ORDER;
  }
  // the algorithmic parameters
#define CKPT_SAME(field, fmt, mine)                                                                                                              \
  if (hd.field != (mine)) { set_err("vloam_checkpoint_load: " #field " differs: the checkpoint was taken with " fmt ", the handle has " fmt, hd.field, (mine)); return VLOAM_ERR_INVALID; }
  CKPT_SAME(scan_line, "%d", h->cfg.scan_line);
  CKPT_SAME(minimum_range, "%.17g", h->cfg.minimum_range);
  CKPT_SAME(mapping_skip_frame, "%d", h->cfg.mapping_skip_frame);
  CKPT_SAME(mapping_line_resolution, "%.9g", (double)h->cfg.mapping_line_resolution);
  CKPT_SAME(mapping_plane_resolution, "%.9g", (double)h->cfg.mapping_plane_resolution);
  CKPT_SAME(detach_VO_LO, "%d", h->cfg.detach_VO_LO ? 1 : 0);
  CKPT_SAME(with_mapping, "%d", h->cfg.with_mapping ? 1 : 0);
#undef CKPT_SAME
  if (hd.with_mapping && hd.stack_tier != (h->map.tier() ? 1 : 0)) {
    set_err("vloam_checkpoint_load: max_surf_stack_points: the checkpoint was taken %s the large stack tier, the handle is %s it (the arrival stamps of raw points have another width there)",
            hd.stack_tier ? "with" : "without", h->map.tier() ? "with" : "without");
    return VLOAM_ERR_INVALID;
  }
  // capacities
  if (hd.frames > h->cfg.max_frames) { set_err("vloam_checkpoint_load: the checkpoint holds %d sweeps, more than max_frames = %d", hd.frames, h->cfg.max_frames); return VLOAM_ERR_CAPACITY; }
  if (hd.n_less[0] > kMaxLessSharp || hd.n_less[1] > h->cfg.max_points) {
    set_err("vloam_checkpoint_load: the last sweep's clouds hold %d / %d points, more than %d / max_points = %d", hd.n_less[0], hd.n_less[1], kMaxLessSharp, h->cfg.max_points); return VLOAM_ERR_CAPACITY;
  }
  int lg[2] = {0, 0};
  if (hd.with_mapping) {
    const int scap[2] = {kStackCapCorner, h->map.surf_cap};
    for (int k = 0; k < 2; k++) {
      if (hd.n_stack[k] > scap[k] || hd.n_deferred[k] > scap[k]) {
        set_err("vloam_checkpoint_load: %s stack: %d points / %d raw voxels, more than the capacity %d (vloam_limits::max_surf_stack_points)", k ? "surf" : "corner", hd.n_stack[k], hd.n_deferred[k], scap[k]);
        return VLOAM_ERR_CAPACITY;
      }
      if (h->map.grow) lg[k] = map_grow_restore_log2(&h->map, k, hd.n_rec[k], hd.n_blk[k]);
      const long long slots = h->map.grow ? (long long)1 << lg[k] : (long long)h->map.tab[k].mask + 1;
      if (hd.n_rec[k] * 10 > slots * 6 || hd.n_blk[k] * 10 > slots / 2 * 6) {
        if (h->map.grow) set_err("vloam_checkpoint_load: the %s table holds %lld live records and %lld block keys, more than 60 %% of 2^%d slots: the growable map's ceiling (max_capacity_log2=%d) is too small",
                                 k ? "surf" : "corner", hd.n_rec[k], hd.n_blk[k], lg[k], h->map.grow->max_log2);
        else set_err("vloam_checkpoint_load: the %s table holds %lld live records and %lld block keys, more than 60 %% of the 2^%d slots (2^%d block slots) of map_capacity_log2",
                     k ? "surf" : "corner", hd.n_rec[k], hd.n_blk[k], __builtin_ctzll((unsigned long long)slots), __builtin_ctzll((unsigned long long)slots) - 1);
        return VLOAM_ERR_CAPACITY;
      }
    }
  }
  // ---- from here on the handle changes
  HIPCHK(hipSetDevice(h->device));
  const char* in = (const char*)buf;
  auto up = [&](void* dst, int s) { return hd.sec[s].bytes == 0 || hipMemcpy(dst, in + hd.sec[s].offset, (size_t)hd.sec[s].bytes, hipMemcpyHostToDevice) == hipSuccess; };
  const int last = hd.frames > 0 ? (hd.frames - 1) % vloam_handle::kSets : 0;
  bool ok = up(h->lo, kSecLoState) && up(h->sr[last].S, kSecScalars) && up(h->sr[last].less_sharp, kSecLessSharp) && up(h->sr[last].less_flat, kSecLessFlat) && up(h->traj, kSecTraj);
  if (ok && h->sweep_log && hd.sec[kSecLog].count == hd.frames) ok = up(h->log_rows, kSecLog);
  if (ok && hd.with_mapping) {
    h->map.stack[0] = h->map.stack_sets[last][0]; h->map.stack[1] = h->map.stack_sets[last][1];
    ok = up(h->map.state, kSecMapState) && up(h->map.cube_cnt, kSecCubeCnt) && up(h->map.stack[0], kSecStack0) && up(h->map.stack[1], kSecStack1);
    if (ok && h->map.grow && map_grow_restore(&h->map, h->s_map, lg, hd.n_rec, hd.n_blk, hd.mapped) != VLOAM_OK) {
      set_err("vloam_checkpoint_load: could not allocate voxel tables of 2^%d / 2^%d slots (hipMalloc)", lg[0], lg[1]); h->map.grow->failed_log2 = 0; return VLOAM_ERR_HIP;
    }
    float ms = 0.f;
    if (ok && map_ckpt_unpack(&h->map, h->s_map, in + hd.sec[kSecMap].offset, hd.n_rec, g_ckpt_times ? &ms : nullptr) != VLOAM_OK) ok = false;
    if (ok && g_ckpt_times) fprintf(stderr, "[vloam ckpt] unpack: %.1f us, %lld records, tables 2^%d / 2^%d slots\n", 1e3 * ms, hd.n_rec[0] + hd.n_rec[1],
                                    __builtin_ctz(h->map.tab[0].mask + 1), __builtin_ctz(h->map.tab[1].mask + 1));
  }
  if (!ok) { set_err("vloam_checkpoint_load: restoring the device state failed: %s", hipGetErrorString(hipGetLastError())); return VLOAM_ERR_HIP; }
  if (hd.frames > 0) {   // == kdtreeCornerLast / kdtreeSurfLast->setInputCloud over the restored clouds, as enqueue_sr builds them behind a sweep
    lo_grid_build_launch(h->stream, h->se, h->sr[last].less_sharp, h->sr[last].less_flat, h->sr[last].S, h->grid[last], nullptr);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->s_map) HIPCHK(hipStreamSynchronize(h->s_map));
  h->frame = h->lo_done = h->map_done = hd.frames;
  h->stage = 0;
  h->lo_launches = hd.lo_launches;
  h->map.pub.mapped = hd.mapped;
  h->map.ds_gen = hd.ds_gen;
  return VLOAM_OK;
}

}  // extern "C"
