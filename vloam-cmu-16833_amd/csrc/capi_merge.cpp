// Map merge of libvloam_hip.so: vloam_map_merge / vloam_map_merge_device — two point clouds of another map and the transform between the maps
// into the voxel tables of a live handle (kernels and chain: map_merge.hip).
#include "handle.h"

static_assert(sizeof(vloam_map_merge_options) == 72 && offsetof(vloam_map_merge_options, apply) == 4 && offsetof(vloam_map_merge_options, q_map_src) == 16 &&
              offsetof(vloam_map_merge_options, t_map_src) == 48, "vloam_map_merge_options: 4 ints, then 7 doubles");
static_assert(sizeof(vloam_map_merge_result) == 120 && offsetof(vloam_map_merge_result, n_new_voxels) == 96 && offsetof(vloam_map_merge_result, max_per_voxel) == 112,
              "vloam_map_merge_result: 14 long long, then 2 ints");

constexpr long long kMergeMaxPoints = 16777216;   // per kind, as an import: point indices and segment offsets are ints

// the refusals that need no handle, in the order c_api.h lists them; host_clouds: the clouds are host arrays (their floats are checked)
static vloam_status merge_check_options(const char* call, const vloam_map_merge_options* o, const void* corner, long long n_corner, const void* surf, long long n_surf,
                                        const void* out, bool host_clouds) {
  if (!o) { set_err("%s: null options", call); return VLOAM_ERR_INVALID; }
  if (o->struct_size != (int)sizeof(vloam_map_merge_options)) { set_err("%s: vloam_map_merge_options: struct_size must be %d", call, (int)sizeof(vloam_map_merge_options)); return VLOAM_ERR_INVALID; }
  if (o->apply < 0 || o->apply > 1) { set_err("%s: apply must be 0 (dry run) or 1, not %d", call, o->apply); return VLOAM_ERR_INVALID; }
  if (o->reserved[0] != 0 || o->reserved[1] != 0) { set_err("%s: reserved must be 0", call); return VLOAM_ERR_INVALID; }
  for (int k = 0; k < 7; k++)
    if (!std::isfinite(k < 4 ? o->q_map_src[k] : o->t_map_src[k - 4])) {
      set_err("%s: transform component %s[%d] is not finite", call, k < 4 ? "q_map_src" : "t_map_src", k < 4 ? k : k - 4); return VLOAM_ERR_INVALID;
    }
  const double* q = o->q_map_src;
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (fabs(nrm - 1.0) > 1e-6) { set_err("%s: the norm of q_map_src is %.9g: it must be within 1e-6 of 1", call, nrm); return VLOAM_ERR_INVALID; }
  if (n_corner < 0 || n_surf < 0) { set_err("%s: negative cloud size (%lld corner, %lld surf points)", call, n_corner, n_surf); return VLOAM_ERR_INVALID; }
  if (n_corner > kMergeMaxPoints || n_surf > kMergeMaxPoints) {
    set_err("%s: %lld corner / %lld surf points: a merge takes at most %lld points of a kind", call, n_corner, n_surf, kMergeMaxPoints); return VLOAM_ERR_INVALID;
  }
  if ((n_corner > 0 && !corner) || (n_surf > 0 && !surf)) { set_err("%s: null %s cloud with a positive point count", call, (n_corner > 0 && !corner) ? "corner" : "surf"); return VLOAM_ERR_INVALID; }
  if (!out) { set_err("%s: null result", call); return VLOAM_ERR_INVALID; }
  if (host_clouds) {
    const float* src[2] = {(const float*)corner, (const float*)surf};
    const long long n[2] = {n_corner, n_surf};
    for (int k = 0; k < 2; k++)
      for (long long e = 0; e < 4 * n[k]; e++)
        if (!std::isfinite(src[k][e])) { set_err("%s: %s cloud, point %lld: component %d is not finite", call, k ? "surf" : "corner", e / 4, (int)(e % 4)); return VLOAM_ERR_INVALID; }
  }
  return VLOAM_OK;
}

// this map <- the clouds' frame from (q xyzw, t): q normalised, then the rotation matrix, all f64 in the order of capi_carve.cpp's carve_pose
// (tests/carve_model.py::pose_matrix states the same)
static MergeXf merge_xf(const vloam_map_merge_options* o) {
  const double* p = o->q_map_src;
  const double nrm = sqrt(((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]) + p[3] * p[3]);
  const double x = p[0] / nrm, y = p[1] / nrm, z = p[2] / nrm, w = p[3] / nrm;
  MergeXf X;
  X.R[0] = 1.0 - 2.0 * (y * y + z * z); X.R[1] = 2.0 * (x * y - z * w); X.R[2] = 2.0 * (x * z + y * w);
  X.R[3] = 2.0 * (x * y + z * w); X.R[4] = 1.0 - 2.0 * (x * x + z * z); X.R[5] = 2.0 * (y * z - x * w);
  X.R[6] = 2.0 * (x * z - y * w); X.R[7] = 2.0 * (y * z + x * w); X.R[8] = 1.0 - 2.0 * (x * x + y * y);
  for (int k = 0; k < 3; k++) X.t[k] = o->t_map_src[k];
  X.identity = (p[0] == 0.0 && p[1] == 0.0 && p[2] == 0.0 && p[3] == 1.0 && X.t[0] == 0.0 && X.t[1] == 0.0 && X.t[2] == 0.0) ? 1 : 0;
  return X;
}

// ... and the ones that do; then the chain.  result: host or device memory, as the clouds
static vloam_status merge_run(const char* call, vloam_handle* h, const vloam_map_merge_options* o, const void* corner, long long n_corner, const void* surf, long long n_surf,
                              void* result, bool host_form) {
  if (!h) { set_err("%s: null handle", call); return VLOAM_ERR_INVALID; }
  if (!h->cfg.with_mapping) { set_err("%s: the handle was created with with_mapping == 0: it keeps no map", call); return VLOAM_ERR_ORDER; }
  if (h->se.B != 1) { set_err("%s: a merge works on one sequence's map: the handle has n_sessions = %d", call, h->se.B); return VLOAM_ERR_INVALID; }
  if (h->stage != 0) { set_err("%s: the handle is in the middle of a stage-wise sweep (stage %d): finish the sweep first", call, h->stage); return VLOAM_ERR_ORDER; }
  TRY(vloam_sync(h));   // drains (a deferred host sweep, trailing odometry and mapping), synchronises, and reports a sticky error as it would
  const bool apply = o->apply != 0;
  const int n[2] = {(int)n_corner, (int)n_surf};
  // one condition for "the window was never placed": the chain then starts the handle at the identity, and the handle counts as imported
  MapState ms0;
  HIPCHK(hipMemcpy(&ms0, h->map.state, sizeof(ms0), hipMemcpyDeviceToHost));
  const bool place_start = apply && map_window_never_placed(ms0);
  if (apply && h->map.grow) {   // the tables step to the size the growth bound asks for, every point a new record and a new block key at most
    MapGrow& G = *h->map.grow;
    int lg[2];
    const int lg0[2] = {G.lg[0], G.lg[1]};
    const long long step_at0[2] = {G.step_at[0], G.step_at[1]};
    long long live[2], blk[2], keys[2];
    for (int k = 0; k < 2; k++) {
      int stats[4];
      HIPCHK(hipMemcpy(stats, h->map.tab[k].stats, sizeof(stats), hipMemcpyDeviceToHost));
      const long long n_in = k ? n_surf : n_corner;
      live[k] = (long long)(stats[0] - stats[1]) + n_in;
      blk[k] = (long long)stats[2] + n_in;
      keys[k] = (long long)stats[0] + n_in;
      lg[k] = map_grow_restore_log2(&h->map, k, live[k], blk[k]);
    }
    if (map_grow_restore(&h->map, h->s_map, lg, live, blk, h->map.pub.mapped) != VLOAM_OK) {
      set_err("%s: could not allocate voxel tables of 2^%d / 2^%d slots (hipMalloc)", call, lg[0], lg[1]); G.failed_log2 = 0; return VLOAM_ERR_HIP;
    }
    // a table that did not step keeps its tombstones: it was not rehashed (step_at stays), and its slots-in-use bound counts them
    for (int k = 0; k < 2; k++)
      if (lg[k] == lg0[k]) {
        G.step_at[k] = step_at0[k];
        G.progress[3 * k + 2] = ((unsigned long long)(unsigned)h->map.pub.mapped << 32) | (unsigned long long)(unsigned)keys[k];
      }
  }
  const void* const cloud[2] = {corner, surf};
  vloam_map_merge_result r;
  if (map_merge_run(&h->map, h->s_map, merge_xf(o), cloud, n, host_form, apply, place_start, &r) != VLOAM_OK) {
    set_err("%s: the merge chain failed: %s", call, hipGetErrorString(hipGetLastError())); return VLOAM_ERR_HIP;
  }
  if (place_start) h->map_imported = true;   // the handle started at the identity like an import: no import, no checkpoint load, and vloam_sync reads the map's error word
  if (host_form) memcpy(result, &r, sizeof(r));
  else HIPCHK(hipMemcpy(result, &r, sizeof(r), hipMemcpyHostToDevice));
  if (!apply) return VLOAM_OK;
  // the sticky error word: the chain raises the map-full error a sweep would have raised
  int merr = 0;
  HIPCHK(hipMemcpy(&merr, &h->map.frame->error, sizeof(int), hipMemcpyDeviceToHost));
  if (merr & kErrMapFull) {
    for (int k = 0; k < 2; k++) {
      int stats[4];
      HIPCHK(hipMemcpy(stats, h->map.tab[k].stats, sizeof(stats), hipMemcpyDeviceToHost));
      const long long slots = (long long)h->map.tab[k].mask + 1, live = (long long)stats[0] - stats[1];
      if (live * 10 > slots * 6) {
        set_err("%s: the %s table holds %lld live records after %lld new voxels, more than 60 %% of its 2^%d slots (%s): the handle is finished", call, k ? "surf" : "corner", live,
                r.n_new_voxels[k], __builtin_ctzll((unsigned long long)slots), h->map.grow ? "the growable map's ceiling" : "map_capacity_log2");
        return VLOAM_ERR_CAPACITY;
      }
    }
    set_err("%s: a voxel table ran out of slots within its probe bound, or the occupancy-block table passed 60 %% (corner table 2^%d, surf table 2^%d slots): the handle is finished", call,
            __builtin_ctzll((unsigned long long)h->map.tab[0].mask + 1), __builtin_ctzll((unsigned long long)h->map.tab[1].mask + 1));
    return VLOAM_ERR_CAPACITY;
  }
  return VLOAM_OK;
}

extern "C" {

void vloam_default_map_merge_options(vloam_map_merge_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->struct_size = (int)sizeof(*o);
  o->apply = 1;
  o->q_map_src[3] = 1.0;
}

vloam_status vloam_map_merge(vloam_handle* h, const vloam_map_merge_options* o, const float* corner_xyzi4, long long n_corner, const float* surf_xyzi4, long long n_surf,
                             vloam_map_merge_result* out) {
  static const char* const call = "vloam_map_merge";
  TRY(merge_check_options(call, o, corner_xyzi4, n_corner, surf_xyzi4, n_surf, out, true));
  return merge_run(call, h, o, corner_xyzi4, n_corner, surf_xyzi4, n_surf, out, true);
}

vloam_status vloam_map_merge_device(vloam_handle* h, const vloam_map_merge_options* o, const void* d_corner, long long n_corner, const void* d_surf, long long n_surf,
                                    void* d_result) {
  static const char* const call = "vloam_map_merge_device";
  TRY(merge_check_options(call, o, d_corner, n_corner, d_surf, n_surf, d_result, false));
  return merge_run(call, h, o, d_corner, n_corner, d_surf, n_surf, d_result, false);
}

}  // extern "C"
