// Host side of libvloam_hip.so: the C ABI declared in include/vloam_hip/c_api.h.
// One handle = one HIP device, B sequences advanced in lock step (B = 1 unless vloam_create_batch), one in-order stream per façade stage
// (scan registration, odometry, mapping) plus one for the mapping stage's scan-feature VoxelGrid;
// every per-frame count stays in HBM, so a sweep is a fixed chain of kernel launches with no host synchronisation until
// the caller asks for results (the only host waits are the back-pressure on buffer sets that are still being read).
// There is NO CPU fallback: without a usable HIP device vloam_create fails.
#include "handle.h"

static thread_local std::string g_err;
const bool vloam::g_host_prof = getenv("VLOAM_HOST_PROF") != nullptr;
namespace vloam { int g_vl_plain_events = getenv("VLOAM_PLAIN_EVENTS") ? atoi(getenv("VLOAM_PLAIN_EVENTS")) : 0; }
const int vloam::g_stage_inline = getenv("VLOAM_STAGE_INLINE") ? atoi(getenv("VLOAM_STAGE_INLINE")) : 0;
void vloam::set_err(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

#define TAKE(p, n) do { if (!A.take(&(p), (size_t)(n))) { set_err("session arena too small (internal)"); return VLOAM_ERR_HIP; } } while (0)

static vloam_status take_factor_table(Arena& A, FactorTable* F, int cap) {
  F->cap = cap;
  TAKE(F->type, cap);
  TAKE(F->p, 3 * (size_t)cap);
  TAKE(F->A, 3 * (size_t)cap);
  TAKE(F->B, 3 * (size_t)cap);
  TAKE(F->resid, 3 * (size_t)cap);
  TAKE(F->ctype, cap);
  TAKE(F->cslot, cap);
  TAKE(F->cpack, 11 * (size_t)cap);
  TAKE(F->dg, 8 * (size_t)cap);
  TAKE(F->rowcnt, (size_t)cap / 64 + 1);
  F->rowmask = nullptr;  // the odometry / VO tables use the per-row counters
  F->gsync = nullptr;  // placed by lm_sync_calibrate once everything is allocated
  F->err = nullptr;    // set once the mapping context (owner of the sticky error word) exists
  F->fallbacks = nullptr; F->host_degraded = nullptr; F->gen = 0; F->spin_limit = 1 << 18;
  return VLOAM_OK;
}

constexpr int kSyncCand = 48;          // candidate cache lines for the sync words of the cooperative solves
constexpr size_t kSyncStride = 8448;   // 8 KB + 256 B: walks page and sub-page address bits; >= one slot
static_assert(kSyncStride >= kLmSyncDoubles * sizeof(double), "slots must not overlap");

// Carve one session's device state out of its arena.  Runs twice: dry (A.base == nullptr) to measure, then for real.
static vloam_status handle_layout(vloam_handle* h, Arena& A) {
  const vloam_config* cfg = &h->cfg;
  const int P = cfg->max_points;
  h->nblk_max = (P + kLabelBlock - 1) / kLabelBlock;
  TAKE(h->d_in, (size_t)(vloam_handle::kInRing + 1) * (size_t)P);   // the ring of the deferred host sweeps + the inline staging buffer
  SRBuffers& a = h->sr[0];
  TAKE(a.sid, (size_t)P);
  TAKE(a.ori, (size_t)P);
  TAKE(a.blockhist, (size_t)h->nblk_max * kMaxRings);
  TAKE(a.blockoff, (size_t)h->nblk_max * kMaxRings);
  TAKE(a.sharp_idx, kMaxSharp);
  TAKE(a.less_sharp_idx, kMaxLessSharp);
  TAKE(a.flat_idx, kMaxFlat);
  TAKE(a.ring_ds, (size_t)kMaxRings * kMaxRingLen);
  TAKE(a.dbg_curv, (size_t)P);
  TAKE(a.dbg_sort, (size_t)P);
  TAKE(a.dbg_picked, (size_t)P);
  TAKE(a.dbg_label, (size_t)P);
  TAKE(a.dbg_cyc, (size_t)kMaxRings * 8);
  TAKE(a.dbg_feat_idx, 3 * kMaxLessSharp);
  if (cfg->max_ring_points > kMaxRingLen) {   // the long ring tier's working arrays (k_sr_ring_long); nothing on a default handle
    a.long_cap = cfg->max_ring_points;
    a.long_kcap = 1;
    while (a.long_kcap < a.long_cap) a.long_kcap <<= 1;
    TAKE(a.long_keys, (size_t)kMaxRings * a.long_kcap);
    TAKE(a.long_iscr, (size_t)kMaxRings * a.long_kcap);
    TAKE(a.long_bytes, (size_t)kMaxRings * 4 * a.long_cap);
    TAKE(a.long_ds, (size_t)kMaxRings * a.long_cap);
  }
  for (int k = 1; k < vloam_handle::kSets; k++) h->sr[k] = a;
  for (int k = 0; k < vloam_handle::kSets; k++) {
    TAKE(h->sr[k].S, 1);
    TAKE(h->sr[k].cloud, (size_t)P);
    TAKE(h->sr[k].sharp, kMaxSharp);
    TAKE(h->sr[k].flat, kMaxFlat);
    TAKE(h->sr[k].less_sharp, kMaxLessSharp);
    TAKE(h->sr[k].less_flat, (size_t)P);
  }
  for (int k = 0; k < vloam_handle::kSets; k++) {
    TAKE(h->grid[k].occ, 4 * kMaxRings);
    TAKE(h->grid[k].stops, 4 * kStopLen);
    for (int g = 0; g < 4; g++) {
      h->grid[k].mask[g] = kGridBuckets[g] - 1;
      TAKE(h->grid[k].cnt[g], kGridBuckets[g]);
      TAKE(h->grid[k].start[g], kGridBuckets[g] + 2);
      TAKE(h->grid[k].pts[g], (g & 1) ? (size_t)P : (size_t)kMaxLessSharp);
    }
  }
  TAKE(h->sub.S, 1);
  TAKE(h->sub.cloud, (size_t)P);
  TAKE(h->sub.less_sharp, kMaxLessSharp);
  TAKE(h->sub.less_flat, (size_t)P);
  TAKE(h->sub_row, 14);
  TAKE(h->lo, 1);
  TRY(take_factor_table(A, &h->lo_F, kMaxLoFactors));
  for (int k = 0; k < 2; k++) { TAKE(h->lo_corr[k], kMaxLoFactors * 4); TAKE(h->lo_resid[k], 3 * kMaxLoFactors); if (h->cfg.debug) TAKE(h->lo_cyc[k], 4 * kMaxLoFactors); }
  TAKE(h->lo_rec, 2);
  TAKE(h->lo_queue, kMaxLoFactors);
  TAKE(h->lo_queue_n, 2);
  TAKE(h->traj, (size_t)cfg->max_frames * 14);
  TAKE(h->vo_traj, (size_t)cfg->max_frames * 7);
  if (h->sweep_log) { TAKE(h->log_rows, (size_t)cfg->max_frames); TAKE(h->log_scratch, 1); }
  if (map_layout(&h->map, h->cfg, A) != VLOAM_OK) { set_err("map_layout failed"); return VLOAM_ERR_HIP; }
  TAKE(h->sync_pool, kSyncCand * kSyncStride / sizeof(double));
  if (vo_layout(&h->vo, h->cfg, A) != VLOAM_OK) { set_err("vo_layout failed"); return VLOAM_ERR_HIP; }
  if (img_layout(&h->img, h->cfg, A) != VLOAM_OK) { set_err("img_layout failed"); return VLOAM_ERR_HIP; }
  h->lo_F.err = &h->map.frame->error;
  h->lo_F.fallbacks = &h->map.frame->fallback_solves;
  for (int k = 0; k < vloam_handle::kSets; k++) h->sr[k].sticky_err = &h->map.frame->error;
  return VLOAM_OK;
}

static std::atomic<int> g_single_handles{0};   // single-sequence handles alive in this process (Sess::crowd)

// ------------------------------------------------------------------ vloam_create, in three parts
// 1. What a configuration must satisfy, checked before any HIP call (so without a device too).  *out: what to build with, every field
// resolved (defaults for 0, fields the caller's struct_size does not reach read as 0).
constexpr int kLimitsSizeV1 = 8;   // sizeof(vloam_limits) when it ended behind max_surf_stack_points
static_assert(sizeof(vloam_limits) == 20 && sizeof(vloam_limits_ext) == 24 && offsetof(vloam_limits_ext, sweep_log) == sizeof(vloam_limits),
              "vloam_limits keeps its size; sweep_log lies right behind it");
constexpr int kMapLog2Min = 10, kMapLog2Max = 28;   // map_layout's clamp of map_capacity_log2 (map_kernels.hip)
struct CreateSpec {
  vloam_limits lim = {};
  int sweep_log = 0;
  int grow_max_log2 = 0;   // > 0: a growable map with this ceiling
};
static vloam_status validate_create(const vloam_config* cfg, const vloam_limits* lim, const vloam_map_options* opt, int n_sessions, CreateSpec* out) {
  *out = CreateSpec();
  vloam_limits* lim_out = &out->lim;
  lim_out->struct_size = (int)sizeof(vloam_limits);
  lim_out->max_surf_stack_points = kStackCapSurf;
  if (lim) {
    const int S = lim->max_surf_stack_points;
    const bool size_ok = lim->struct_size == 0 || lim->struct_size == kLimitsSizeV1 || lim->struct_size >= (int)sizeof(vloam_limits);
    const bool value_ok = S == 0 || S == kStackCapSurf || (S > kStackCapSurf && S <= kStackCapSurfMax && S % kStackCapSurfStep == 0);
    if (!size_ok || !value_ok || (S > kStackCapSurf && S > cfg->max_points)) {   // (the default holds whatever max_points is, as it always has)
      set_err("vloam_limits: max_surf_stack_points must be 0 or %d (default), or a multiple of %d up to %d, and at most max_points; struct_size 0, 8 or >= %d",
              kStackCapSurf, kStackCapSurfStep, kStackCapSurfMax, (int)sizeof(vloam_limits));
      return VLOAM_ERR_INVALID;
    }
    if (S != 0) lim_out->max_surf_stack_points = S;
    if (lim->struct_size != kLimitsSizeV1) {   // the published clouds (a first-version caller has no such fields: whatever lies behind its struct is not read)
      const int N = lim->map_pub_number, C = lim->max_published_map_points, R = lim->publish_registered_cloud;
      if (N < 0) { set_err("vloam_limits: map_pub_number must be 0 (off) or 1 .. %d", INT_MAX); return VLOAM_ERR_INVALID; }
      if (N > 0 && C != 0 && (C < kPubMapCapMin || C > kPubMapCapMax)) {
        set_err("vloam_limits: max_published_map_points must be 0 (= %lld) or %lld .. %lld", kPubMapCapDefault, kPubMapCapMin, kPubMapCapMax); return VLOAM_ERR_INVALID;
      }
      if (R != 0 && R != 1) { set_err("vloam_limits: publish_registered_cloud must be 0 or 1"); return VLOAM_ERR_INVALID; }
      if ((N > 0 || R) && !cfg->with_mapping) {
        set_err("vloam_limits: map_pub_number (0 or 1 .. %d) and publish_registered_cloud (0 or 1) must be 0 on a handle with with_mapping == 0: the mapping stage publishes", INT_MAX);
        return VLOAM_ERR_INVALID;
      }
      lim_out->map_pub_number = N;
      lim_out->max_published_map_points = N > 0 ? (C != 0 ? C : (int)kPubMapCapDefault) : 0;
      lim_out->publish_registered_cloud = R;
    }
    // exactly vloam_limits_ext's size: the caller's struct IS one.  Any other accepted size says nothing about what lies behind vloam_limits
    // (0 = sizeof(vloam_limits); a larger size is a later header's struct, of which the fields of vloam_limits are read): nothing there is read
    if (lim->struct_size == (int)sizeof(vloam_limits_ext)) {
      const int L = reinterpret_cast<const vloam_limits_ext*>(lim)->sweep_log;
      if (L != 0 && L != 1) { set_err("vloam_limits_ext: sweep_log must be 0 or 1"); return VLOAM_ERR_INVALID; }
      out->sweep_log = L;
    }
  }
  if (n_sessions < 1 || n_sessions > kMaxBatch) { set_err("n_sessions must be 1..%d", kMaxBatch); return VLOAM_ERR_INVALID; }
  if (cfg->scan_line != 16 && cfg->scan_line != 32 && cfg->scan_line != 64) {
    set_err("only support velodyne with 16, 32 or 64 scan line!");  // scan_registration.cpp:54-58
    return VLOAM_ERR_INVALID;
  }
  if (cfg->max_points < 64 || cfg->max_points > (1 << 24) || cfg->max_frames < 1 || cfg->mapping_skip_frame < 1) {  // 24-bit point tags
    set_err("bad capacity"); return VLOAM_ERR_INVALID;
  }
  if (cfg->max_ring_points != 0 && (cfg->max_ring_points < kMaxRingLen || cfg->max_ring_points > kMaxRingLenLong)) {
    set_err("max_ring_points must be 0 or %d (default) .. %d", kMaxRingLen, kMaxRingLenLong); return VLOAM_ERR_INVALID;
  }
  // laser_mapping.cpp:95-101 takes any leaf; the reference's launch files use 0.2 / 0.4 (VLP-16, HDL-32) and 0.4 / 0.8 (KITTI).  Here the
  // position of a voxel in the gathered map cloud (the 5-NN tie rank) is a 32-bit mixed-radix number: 75 cubes x radix^3 voxels.
  for (const float leaf : {cfg->mapping_line_resolution, cfg->mapping_plane_resolution}) {
    const double nv = leaf > 0.f ? (double)vox_radix(1.0f / leaf) : 1e9;
    if (!(leaf > 0.f) || 75.0 * nv * nv * nv >= 4294967295.0) { set_err("mapping resolutions below 0.132 m are not supported"); return VLOAM_ERR_INVALID; }
  }
  if (cfg->image_width < 0 || cfg->image_height < 0 || (long long)cfg->image_width * cfg->image_height > (1ll << 24) ||
      ((cfg->image_width > 0) != (cfg->image_height > 0)) || (cfg->image_width > 0 && (cfg->image_width < 2 * kImgWin || cfg->image_height < 2 * kImgWin))) {
    set_err("image_width x image_height must be 0 x 0 (no image front-end) or between %d x %d and 2^24 pixels", 2 * kImgWin, 2 * kImgWin); return VLOAM_ERR_INVALID;
  }
  if (opt) {
    const int lg0 = std::min(std::max(cfg->map_capacity_log2, kMapLog2Min), kMapLog2Max);
    if (opt->struct_size != (int)sizeof(vloam_map_options)) { set_err("vloam_map_options: struct_size must be %d", (int)sizeof(vloam_map_options)); return VLOAM_ERR_INVALID; }
    if ((opt->grow != 0 && opt->grow != 1) || (opt->max_capacity_log2 != 0 && (opt->max_capacity_log2 < lg0 || opt->max_capacity_log2 > kMapLog2Max))) {
      set_err("vloam_map_options: grow must be 0 or 1 and max_capacity_log2 0 (= %d) or map_capacity_log2 (%d) .. %d", kMapLog2Max, lg0, kMapLog2Max); return VLOAM_ERR_INVALID;
    }
    if (opt->grow == 1 && (n_sessions > 1 || !cfg->with_mapping)) {
      set_err("vloam_map_options: grow = 1 needs a single-sequence handle (n_sessions == 1) with with_mapping == 1"); return VLOAM_ERR_INVALID;
    }
    if (opt->grow == 1) out->grow_max_log2 = opt->max_capacity_log2 ? opt->max_capacity_log2 : kMapLog2Max;
  }
  return VLOAM_OK;
}

// 2. The handle's streams, each with the HIP priority of its pool in the plan.
static vloam_status create_streams(vloam_handle* h, const vloam_plan::Plan& plan, const vloam_config* cfg) {
  using namespace vloam_plan;
  int lo_p = 0, hi_p = 0;
  if (hipDeviceGetStreamPriorityRange(&lo_p, &hi_p) != hipSuccess) { lo_p = hi_p = 0; }   // lo_p = numerically greatest = lowest priority
  const int pool_prio[kPools] = {0, hi_p, lo_p};
  for (int w = 0; w < kStreams; w++) h->prio[w] = pool_prio[plan.pool[w]];
  auto mk = [&](hipStream_t* s, int which) { return hipStreamCreateWithPriority(s, hipStreamNonBlocking, h->prio[which]) == hipSuccess; };
  // the runtime gives a stream its hardware queue when the stream is created, so the order matters (stream_plan.h).  plan.copy_first: the
  // copy stream of the deferred host-sweep ring comes FIRST and is used once before any other stream of the handle has work — measured
  // (tools/host_input_probe.py, extring / extring_late; profiles/r06_host_input.txt) a copy stream that gets its hardware queue after the
  // compute streams runs host-fed sequences at 3 900 - 4 600 scans/s, one that got it before them at 5 650
  if (plan.copy_first && !g_stage_inline && !cfg->timing) {
    if (!mk(&h->s_copy, kCopy)) { set_err("hipStreamCreate failed"); return VLOAM_ERR_HIP; }
    static int warm_src = 0;
    int* warm_dst = nullptr;
    if (hipMalloc(&warm_dst, sizeof(int)) == hipSuccess) {
      (void)hipMemcpyAsync(warm_dst, &warm_src, sizeof(int), hipMemcpyHostToDevice, h->s_copy);
      (void)hipStreamSynchronize(h->s_copy);
      (void)hipFree(warm_dst);
    }
  }
  bool ok = mk(&h->stream, kSR) && mk(&h->s_lo, kLO);
  if (ok && cfg->with_mapping) ok = mk(&h->s_map, kMap) && mk(&h->s_ds, kDS);   // no mapping: no further hardware queues
  if (ok && cfg->image_width > 0) ok = mk(&h->s_img, kImg);
  if (!ok) { set_err("hipStreamCreate failed"); return VLOAM_ERR_HIP; }
  return VLOAM_OK;
}

// 3. One allocation for all sessions, session 0 laid out and initialised, the others copied from it.  n_cus: the device's compute units,
// from the one property query of vloam_create (a failed query fails the creation; there is no second query left to fall back from).
static vloam_status init_sessions(vloam_handle* h, int n_sessions, int n_cus) {
  // measure one session, then one allocation for all sessions (zeroed), then lay session 0 out for real
  Arena dry;
  TRY(handle_layout(h, dry));
  // 2 MB granules + a skew: with arenas exactly 2 MB-aligned every session's hot words (bucket counters, cursors, table heads) share
  // their low address bits, i.e. ALL sessions of a batch hit the same memory channels at the same time (k_lo_grid_count's atomics:
  // 2 150 cycles of vector-memory latency alone, 8 160 at B = 16, profiles/r05_batch_pmc.txt); the skew walks the sessions over the channels
  static const size_t skew = getenv("VLOAM_ARENA_SKEW") ? (size_t)atol(getenv("VLOAM_ARENA_SKEW")) & ~(size_t)255 : 0;
  const size_t ss = ((dry.off + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1)) + (n_sessions > 1 ? skew : 0);
  h->se.B = n_sessions;
  h->se.ss = ss;
  // The cooperative solves of a single sequence are placed on ONE XCD each (lm_solve.hip: lm_coop_block): 8 + 8 compute units of XCDs 2 and
  // 6.  Several single-sequence handles in one process would crowd those two XCDs (and their solves wait for each other's compute
  // units): only the first two alive get the placement, the others launch spread over the XCDs like before round 4.  Same arithmetic.
  if (n_sessions == 1) { h->se.crowd = g_single_handles.fetch_add(1); h->counted_single = true; }
  // ... and only on the device the placement was measured on: 256 compute units dealt round-robin to 8 XCDs (SPX mode).  Anything else
  // (a CPX / NPS partition, a CU-masked context, another part) keeps the plain spread launch; and whatever the placement, a solve
  // whose workgroups do not end up resident together degrades to one workgroup instead of failing (lm_solve.hip).
  if (n_cus != 256) h->se.crowd = 1 << 20;
  h->arena_bytes = ss * (size_t)n_sessions;
  if (hipMalloc((void**)&h->arena, h->arena_bytes) != hipSuccess) {
    set_err("hipMalloc of %zu MB for %d session(s) failed", h->arena_bytes >> 20, n_sessions); h->arena = nullptr; return VLOAM_ERR_HIP;
  }
  HIPCHK(hipMemsetAsync(h->arena, 0, h->arena_bytes, h->stream));
  Arena A;
  A.base = h->arena; A.cap = ss; A.dry = false;
  TRY(handle_layout(h, A));
  h->map.se = h->se;
  h->vo.se = h->se;
  // ---- initial state of session 0
  for (int k = 0; k < vloam_handle::kSets; k++) {
    int arm[4 * kMaxRings];
    for (int q = 0; q < 4 * kMaxRings; q++) arm[q] = ((q / kMaxRings) & 1) ? -1 : INT_MAX;
    HIPCHK(hipMemcpyAsync(h->grid[k].occ, arm, sizeof(arm), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  LOState init;
  memset(&init, 0, sizeof(init));
  init.para_q[3] = 1.0; init.q_w_curr[3] = 1.0; init.prior_q[3] = 1.0;  // laser_odometry.cpp:80-90
  tf_identity(&init.tf.base_T_cam0); tf_identity(&init.tf.velo_T_cam0); tf_identity(&init.tf.cam0_curr_T_cam0_last);  // visual_odometry.cpp:73-74
  tf_identity(&init.tf.cam0_curr_LOT_cam0_prev); tf_identity(&init.tf.world_VOT_base_last);                            // vloam_tf.cpp:10-11
  HIPCHK(hipMemcpyAsync(h->lo, &init, sizeof(init), hipMemcpyHostToDevice, h->stream));
  if (hipHostMalloc((void**)&h->ring_watch, sizeof(int) * 2 * kMaxBatch, hipHostMallocMapped) != hipSuccess) { h->ring_watch = nullptr; set_err("hipHostMalloc failed"); return VLOAM_ERR_HIP; }
  for (int b = 0; b < 2 * kMaxBatch; b++) h->ring_watch[b] = 0;
  if (hipHostMalloc((void**)&h->coop_flag, sizeof(int), hipHostMallocMapped) != hipSuccess) { h->coop_flag = nullptr; set_err("hipHostMalloc failed"); return VLOAM_ERR_HIP; }
  *h->coop_flag = 0;
  h->lo_F.host_degraded = h->coop_flag; h->map.F[0].host_degraded = h->coop_flag; h->map.F[1].host_degraded = h->coop_flag;
  {
    // patience of the workgroups of a cooperative solve (polls before one gives up on its partners, ~0.2 s by default): read ONCE per handle,
    // here — not on the enqueue path, where a getenv per launch would also race a host thread's setenv.  Tests force the degraded path
    // with VLOAM_LM_SPIN_LIMIT=1; anything below 1 (a typo, an empty string) would degrade every solve for good and means "default".
    const char* e = getenv("VLOAM_LM_SPIN_LIMIT");
    const int v = e ? atoi(e) : 0;
    const int limit = v >= 1 ? v : (1 << 18);
    h->lo_F.spin_limit = limit; h->map.F[0].spin_limit = limit; h->map.F[1].spin_limit = limit; h->vo.F.spin_limit = limit;
  }
  if (map_init(&h->map, h->stream) != VLOAM_OK) { set_err("map_init failed: %s", hipGetErrorString(hipGetLastError())); return VLOAM_ERR_HIP; }
  {
    // sync words of the three cooperative solves (odometry, mapping outer rounds): the fastest of 48 candidate lines, probed
    // on session 0 (the other sessions' arenas start on 2 MB boundaries: same low address bits)
    int order[kSyncCand];
    if (lm_sync_calibrate(h->stream, h->sync_pool, kSyncCand - 1, kSyncStride, order) != 0) { set_err("lm_sync_calibrate failed"); return VLOAM_ERR_HIP; }
    auto slot = [&](int r) { return reinterpret_cast<double*>(reinterpret_cast<char*>(h->sync_pool) + kSyncStride * (size_t)order[r]); };
    h->lo_F.gsync = slot(0);
    h->map.F[0].gsync = slot(1);
    h->map.F[1].gsync = slot(2);
  }
  for (int k = 0; k < 6; k++) HIPCHK(hipEventCreate(&h->ev[k]));
  for (int k = 0; k < vloam_handle::kSets; k++) {
    HIPCHK(hipEventCreateWithFlags(&h->ev_sr[k], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_lo[k], hipEventDisableTiming | hipEventBlockingSync));   // the host throttle sleeps on these
    HIPCHK(hipEventCreateWithFlags(&h->ev_map[k], hipEventDisableTiming | hipEventBlockingSync));
    HIPCHK(hipEventCreateWithFlags(&h->ev_stack[k], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_vo[k], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_img[k], hipEventDisableTiming));
  }
  if (h->sweep_log) {
    HIPCHK(sweep_log_init(h->stream, h->log_rows, h->cfg.max_frames));
    HIPCHK(h->log_ring.create(3));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  // ---- the other sessions start as byte-for-byte copies of session 0
  for (int b = 1; b < n_sessions; b++)
    HIPCHK(hipMemcpyAsync(h->arena + (size_t)b * ss, h->arena, dry.off, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VLOAM_OK;
}

extern "C" {

void vloam_default_config(vloam_config* c) {
  memset(c, 0, sizeof(*c));
  c->scan_line = 64;
  c->minimum_range = 5.0;
  c->mapping_skip_frame = 1;
  c->mapping_line_resolution = 0.4f;
  c->mapping_plane_resolution = 0.8f;
  c->detach_VO_LO = 1;
  c->reset_VO_to_identity = 0;
  c->remove_VO_outlier = 100;
  c->with_mapping = 1;
  c->max_points = 262144;
  c->max_frames = 8192;
  c->map_capacity_log2 = 22;
  c->debug = 0;
  c->timing = 0;
  c->image_width = 0;
  c->image_height = 0;
  c->CLAHE = 0;
  c->max_ring_points = kMaxRingLen;
}

const char* vloam_last_error(void) { return g_err.c_str(); }
const char* vloam_version(void) { return "vloam_hip 0.1 (gfx950)"; }

void vloam_default_limits(vloam_limits* lim) {
  lim->struct_size = (int)sizeof(vloam_limits);
  lim->max_surf_stack_points = kStackCapSurf;
  lim->map_pub_number = 0;
  lim->max_published_map_points = (int)kPubMapCapDefault;
  lim->publish_registered_cloud = 0;
}

void vloam_default_limits_ext(vloam_limits_ext* lim) {
  vloam_default_limits(&lim->limits);
  lim->limits.struct_size = (int)sizeof(vloam_limits_ext);
  lim->sweep_log = 0;
}

vloam_status vloam_create_batch(const vloam_config* cfg, int device, int n_sessions, vloam_handle** out) {
  return vloam_create_with_limits(cfg, nullptr, device, n_sessions, out);
}

void vloam_default_map_options(vloam_map_options* opt) {
  opt->struct_size = (int)sizeof(vloam_map_options);
  opt->grow = 0;
  opt->max_capacity_log2 = kMapLog2Max;
}

vloam_status vloam_create_with_limits(const vloam_config* cfg, const vloam_limits* lim, int device, int n_sessions, vloam_handle** out) {
  return vloam_create_with_options(cfg, lim, nullptr, device, n_sessions, out);
}

vloam_status vloam_create_with_options(const vloam_config* cfg, const vloam_limits* lim, const vloam_map_options* opt, int device, int n_sessions,
                                       vloam_handle** out) {
  if (!cfg || !out) { set_err("null argument"); return VLOAM_ERR_INVALID; }
  CreateSpec spec;
  TRY(validate_create(cfg, lim, opt, n_sessions, &spec));
  // A handle drives two to six HIP streams that must run side by side (scan registration | odometry [| mapping | scan-feature VoxelGrid]
  // [| images] [| host-sweep copies]).  GPU_MAX_HW_QUEUES (read by the runtime when it initialises: it belongs to the HOST's environment, and a
  // library must not setenv() behind a multi-threaded host) caps each of the runtime's three priority pools of hardware queues; the handle
  // picks its streams' priorities from it (stream_plan.h).  Said once per process when the plan is the pooled one.
  const int queue_budget = vloam_plan::budget_from_env(getenv("GPU_MAX_HW_QUEUES"));
  const vloam_plan::Plan plan = vloam_plan::make_plan(queue_budget, cfg->with_mapping != 0, cfg->image_width > 0);
  {
    static std::atomic<bool> warned{false};   // (handles may be created from several threads)
    if (plan.pooled && !warned.exchange(true)) {
      fprintf(stderr, "libvloam_hip: GPU_MAX_HW_QUEUES is %d: the stage streams of a handle take hardware queues from the runtime's three priority "
                      "pools (scan registration low, odometry normal, mapping high), so that no two of them share one; export GPU_MAX_HW_QUEUES=16 "
                      "to keep them all at normal priority\n", queue_budget);
    }
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_err("no HIP device visible: libvloam_hip has no CPU fallback");
    return VLOAM_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) { set_err("device %d out of range (%d visible)", device, ndev); return VLOAM_ERR_NO_DEVICE; }
  HIPCHK(hipSetDevice(device));
  // co-residency of the cooperative solves (c_api.h): 4 + 6 workgroups per session may have to be resident at once
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (10 * n_sessions > prop.multiProcessorCount) {
    set_err("%d sessions need %d co-resident solver workgroups, the device has %d compute units", n_sessions, 10 * n_sessions, prop.multiProcessorCount);
    return VLOAM_ERR_CAPACITY;
  }
  vloam_handle* h = new vloam_handle;
  h->cfg = *cfg;
  if (h->cfg.max_ring_points == 0) h->cfg.max_ring_points = kMaxRingLen;   // zero-initialised configs: the default
  h->map.surf_cap = spec.lim.max_surf_stack_points;   // before the layout: the mapping stage's arrays are sized by it (map_layout)
  h->map.pub.pub_number = spec.lim.map_pub_number;    // ... and so are the publication buffers
  h->map.pub.skip_n = cfg->mapping_skip_frame;
  h->map.pub.cap = spec.lim.max_published_map_points;
  h->map.pub.cloud_on = spec.lim.publish_registered_cloud;
  if (spec.grow_max_log2 > 0) {   // before the layout: the tables then stay out of the arena (map_layout)
    MapGrow* G = new MapGrow;
    G->max_log2 = spec.grow_max_log2;
    // What one mapped sweep can add to a table at most.  Stack points: no more than the sweep's lessSharp cloud (kMaxLessSharp; a caller's
    // own clouds, vloam_set_mapping_input, included) / the surf stack's capacity, and than the sweep has points.  Records: TWO per stack point
    // — a point of a cube outside the valid block costs its voxel's record and a raw-point record of its own (k_map_finalize).  Block keys: one.
    const long long pts[2] = {std::min<long long>(kMaxLessSharp, cfg->max_points), std::min<long long>(spec.lim.max_surf_stack_points, cfg->max_points)};
    for (int k = 0; k < 2; k++) { G->inc_rec[k] = 2 * pts[k]; G->inc_blk[k] = pts[k]; }
    for (int k = 0; k < 2; k++) { h->map.tab[k].rec = nullptr; h->map.tab[k].pend = nullptr; h->map.tab[k].blk = nullptr; }   // (map_destroy frees them, whatever creation reached)
    h->map.grow = G;
  }
  h->sweep_log = spec.sweep_log != 0;
  h->device = device;
  *out = nullptr;
  vloam_status st = create_streams(h, plan, cfg);
  if (st == VLOAM_OK && sr_init() != hipSuccess) { set_err("sr_init failed (no gfx950 code object for this device?)"); st = VLOAM_ERR_HIP; }
  if (st == VLOAM_OK && cfg->image_width > 0 && img_init() != hipSuccess) { set_err("img_init failed"); st = VLOAM_ERR_HIP; }
  if (st == VLOAM_OK) st = init_sessions(h, n_sessions, prop.multiProcessorCount);
  if (st != VLOAM_OK) { vloam_destroy(h); return st; }
  *out = h;
  return VLOAM_OK;
}

vloam_status vloam_create(const vloam_config* cfg, int device, vloam_handle** out) { return vloam_create_batch(cfg, device, 1, out); }

vloam_status vloam_batch_size(vloam_handle* h, int* n_sessions) {
  if (!h || !n_sessions) return VLOAM_ERR_INVALID;
  *n_sessions = h->se.B;
  return VLOAM_OK;
}

// which session the getters (trajectory, features, counts, map, parity hooks) read; 0 after creation
vloam_status vloam_select_session(vloam_handle* h, int session) {
  if (!h || session < 0 || session >= h->se.B) return VLOAM_ERR_INVALID;
  h->sel = session;
  h->map.sel = session;
  return VLOAM_OK;
}

vloam_status vloam_destroy(vloam_handle* h) {
  if (!h) return VLOAM_OK;
  if (h->counted_single) g_single_handles.fetch_sub(1);
  if (g_host_prof && h->host_calls > 0)
    fprintf(stderr, "[vloam host prof] %lld sweeps: per sweep %.1f us in the buffer-set throttle, %.1f us enqueueing SR (incl. throttle), %.1f us LO, %.1f us mapping\n",
            h->host_calls, 1e6 * h->host_s[0] / h->host_calls, 1e6 * h->host_s[1] / h->host_calls, 1e6 * h->host_s[2] / h->host_calls, 1e6 * h->host_s[3] / h->host_calls);
  (void)hipSetDevice(h->device);
  for (hipStream_t st : {h->s_copy, h->stream, h->s_lo, h->s_map, h->s_ds, h->s_img}) if (st) (void)hipStreamSynchronize(st);
  if (h->arena) (void)hipFree(h->arena);
  if (h->pi.rows) (void)hipFree(h->pi.rows);
  if (h->pi.scratch) (void)hipFree(h->pi.scratch);
  h->pi_ring.destroy();
  if (h->pc.rows) (void)hipFree(h->pc.rows);
  if (h->pc.scratch) (void)hipFree(h->pc.scratch);
  for (void* p : {(void*)h->place.db, (void*)h->place.tags, (void*)h->place.info, (void*)h->place.best, (void*)h->place.cells, (void*)h->place.qdesc,
                  (void*)h->place.qinfo, (void*)h->place.qmatch, (void*)h->place.cloud}) if (p) (void)hipFree(p);
  for (int k = 0; k < vloam_handle::kInRing; k++) if (h->ev_in_copied[k]) (void)hipEventDestroy(h->ev_in_copied[k]);
  for (int k = 0; k < 6; k++) if (h->ev[k]) (void)hipEventDestroy(h->ev[k]);
  for (int k = 0; k < vloam_handle::kSets; k++)
    for (hipEvent_t e : {h->ev_sr[k], h->ev_lo[k], h->ev_map[k], h->ev_stack[k], h->ev_vo[k], h->ev_img[k]}) if (e) (void)hipEventDestroy(e);
  h->log_ring.destroy();
  for (hipEvent_t e : h->prof_events) (void)hipEventDestroy(e);
  for (hipStream_t st : {h->s_copy, h->stream, h->s_lo, h->s_map, h->s_ds, h->s_img}) if (st) (void)hipStreamDestroy(st);
  map_destroy(&h->map);
  if (h->ring_watch) (void)hipHostFree(h->ring_watch);
  if (h->coop_flag) (void)hipHostFree(h->coop_flag);
  delete h;
  return VLOAM_OK;
}

vloam_status vloam_reset_frame(vloam_handle* h) {
  if (!h) return VLOAM_ERR_INVALID;
  h->stage = 0;  // scan_registration.reset() clears the per-frame clouds; laser_mapping.reset() zeroes the valid-cube counters
  return VLOAM_OK;
}

}  // extern "C"
