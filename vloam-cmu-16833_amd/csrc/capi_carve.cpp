// Map clean-up of libvloam_hip.so: vloam_map_carve / vloam_map_carve_device — voxels that later sweeps see through leave the map (kernels and
// chain: map_carve.hip).
#include "handle.h"

static_assert(sizeof(vloam_carve_options) == 48 && offsetof(vloam_carve_options, elev_min_deg) == 16 && offsetof(vloam_carve_options, min_votes) == 40,
              "vloam_carve_options: 4 ints, 6 floats, 2 ints");
static_assert(sizeof(vloam_carve_result) == 104 && offsetof(vloam_carve_result, n_removed_out) == 96, "vloam_carve_result: 13 long long");

// the refusals that need no handle, in the order c_api.h lists them
static vloam_status carve_check(const char* call, const vloam_carve_options* o, const void* const* clouds, const int* n, const double* poses7, int n_sweeps,
                                const void* removed, long long cap, const void* res) {
  if (!o) { set_err("%s: null options", call); return VLOAM_ERR_INVALID; }
  if (o->struct_size != (int)sizeof(vloam_carve_options)) { set_err("%s: vloam_carve_options: struct_size must be %d", call, (int)sizeof(vloam_carve_options)); return VLOAM_ERR_INVALID; }
  if (o->kind_mask < 1 || o->kind_mask > 3) { set_err("%s: kind_mask must be 1 (corner map), 2 (surf map) or 3 (both), not %d", call, o->kind_mask); return VLOAM_ERR_INVALID; }
  if (o->rows < 1 || o->cols < 4 || (long long)o->rows * o->cols > kCarveMaxPixels) {
    set_err("%s: a range image of %d rows x %d columns: at least 1 x 4, at most %d pixels (rows * cols > 2^20 is refused)", call, o->rows, o->cols, kCarveMaxPixels); return VLOAM_ERR_INVALID;
  }
  if (!std::isfinite(o->elev_min_deg) || !std::isfinite(o->elev_max_deg) || o->elev_min_deg < -90.f || o->elev_max_deg > 90.f || !(o->elev_max_deg - o->elev_min_deg >= 0.001f)) {
    set_err("%s: elevations %.9g .. %.9g degrees: finite, within -90 .. 90 and at least 0.001 apart", call, (double)o->elev_min_deg, (double)o->elev_max_deg); return VLOAM_ERR_INVALID;
  }
  if (!std::isfinite(o->min_range) || !std::isfinite(o->max_range) || !(o->min_range > 0.f) || !(o->min_range < o->max_range)) {
    set_err("%s: ranges %.9g .. %.9g m: finite, 0 < min_range < max_range", call, (double)o->min_range, (double)o->max_range); return VLOAM_ERR_INVALID;
  }
  if (!std::isfinite(o->range_res) || !(o->range_res > 0.f) || !((double)o->max_range / (double)o->range_res < 1073741824.0)) {
    set_err("%s: range_res %.9g m: finite, positive and at least max_range / 2^30", call, (double)o->range_res); return VLOAM_ERR_INVALID;
  }
  if (!std::isfinite(o->margin) || o->margin < 0.f || !((double)o->margin / (double)o->range_res < 1073741824.0)) {
    set_err("%s: margin %.9g m: finite, not negative and below 2^30 range_res", call, (double)o->margin); return VLOAM_ERR_INVALID;
  }
  if (o->min_votes < 1 || o->min_votes > kCarveMaxSweeps) { set_err("%s: min_votes must be 1 .. %d, not %d", call, kCarveMaxSweeps, o->min_votes); return VLOAM_ERR_INVALID; }
  if (o->apply < 0 || o->apply > 1) { set_err("%s: apply must be 0 (dry run) or 1, not %d", call, o->apply); return VLOAM_ERR_INVALID; }
  if (n_sweeps < 1 || n_sweeps > kCarveMaxSweeps) { set_err("%s: n_sweeps must be 1 .. %d, not %d", call, kCarveMaxSweeps, n_sweeps); return VLOAM_ERR_INVALID; }
  if (!clouds || !n) { set_err("%s: null array of sweeps or of counts", call); return VLOAM_ERR_INVALID; }
  for (int s = 0; s < n_sweeps; s++) {
    if (n[s] < 0 || n[s] > kCarveMaxPoints) { set_err("%s: sweep %d has %d points: 0 .. %d", call, s, n[s], kCarveMaxPoints); return VLOAM_ERR_INVALID; }
    if (n[s] > 0 && !clouds[s]) { set_err("%s: null sweep pointer %d with a positive point count", call, s); return VLOAM_ERR_INVALID; }
  }
  if (!poses7 && n_sweeps != 1) { set_err("%s: null poses mean the handle's last mapped pose: with n_sweeps == 1 only, not %d", call, n_sweeps); return VLOAM_ERR_INVALID; }
  if (poses7)
    for (int s = 0; s < n_sweeps; s++) {
      const double* p = poses7 + 7 * s;
      for (int k = 0; k < 7; k++)
        if (!std::isfinite(p[k])) { set_err("%s: pose %d, component %d is not finite", call, s, k); return VLOAM_ERR_INVALID; }
      const double nrm = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3]);
      if (fabs(nrm - 1.0) > 1e-6) { set_err("%s: pose %d: the quaternion's norm is %.9g: it must be within 1e-6 of 1", call, s, nrm); return VLOAM_ERR_INVALID; }
    }
  if (cap < 0 || (cap > 0 && !removed)) { set_err("%s: a list of %lld points at a %s address", call, cap, removed ? "non-null" : "null"); return VLOAM_ERR_INVALID; }
  if (!res) { set_err("%s: null result", call); return VLOAM_ERR_INVALID; }
  return VLOAM_OK;
}

// the projection's constants in f32, as c_api.h states them
static CarveGeom carve_geom(const vloam_carve_options* o, int n_sweeps) {
  const float deg = 0.017453292f, pi = 3.14159274f;   // f32(pi / 180), PI_F = 0x40490fdb
  CarveGeom G;
  G.rows = o->rows; G.cols = o->cols; G.n_sweeps = n_sweeps; G.min_votes = o->min_votes;
  G.min_range = o->min_range; G.max_range = o->max_range; G.range_res = o->range_res;
  G.elev_min = o->elev_min_deg * deg;
  const float elev_max = o->elev_max_deg * deg;
  G.row_scale = (float)o->rows / (elev_max - G.elev_min);
  G.col_scale = (float)o->cols / (2.0f * pi);
  G.margin_q = (unsigned)floorf(o->margin / o->range_res);
  return G;
}

// map <- sensor from (q xyzw, t): q normalised, then the rotation matrix, all f64 in this order (tests/carve_model.py states the same)
static CarvePose carve_pose(const double* p) {
  const double nrm = sqrt(((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]) + p[3] * p[3]);
  const double x = p[0] / nrm, y = p[1] / nrm, z = p[2] / nrm, w = p[3] / nrm;
  CarvePose P;
  P.R[0] = 1.0 - 2.0 * (y * y + z * z); P.R[1] = 2.0 * (x * y - z * w); P.R[2] = 2.0 * (x * z + y * w);
  P.R[3] = 2.0 * (x * y + z * w); P.R[4] = 1.0 - 2.0 * (x * x + z * z); P.R[5] = 2.0 * (y * z - x * w);
  P.R[6] = 2.0 * (x * z - y * w); P.R[7] = 2.0 * (y * z + x * w); P.R[8] = 1.0 - 2.0 * (x * x + y * y);
  P.t[0] = p[4]; P.t[1] = p[5]; P.t[2] = p[6];
  return P;
}

static vloam_status carve_run(const char* call, vloam_handle* h, const vloam_carve_options* o, const void* const* clouds, const int* n, const double* poses7,
                              int n_sweeps, void* removed, long long cap, vloam_carve_result* res, bool host_io) {
  TRY(carve_check(call, o, clouds, n, poses7, n_sweeps, removed, cap, res));
  if (!h) { set_err("%s: null handle", call); return VLOAM_ERR_INVALID; }
  if (!h->cfg.with_mapping) { set_err("%s: the handle was created with with_mapping == 0: it keeps no map", call); return VLOAM_ERR_ORDER; }
  if (o->apply && h->se.B != 1) { set_err("%s: apply removes voxels of one sequence: the handle has %d sessions (a dry run works on the selected one)", call, h->se.B); return VLOAM_ERR_INVALID; }
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  CarvePose poses[kCarveMaxSweeps];
  if (poses7) for (int s = 0; s < n_sweeps; s++) poses[s] = carve_pose(poses7 + 7 * s);
  else {   // the mapping's own pose of the last mapped sweep (MapState::parameters: q_w_curr, t_w_curr)
    double last[7];
    HIPCHK(hipMemcpy(last, SEL(h, h->map.state)->parameters, sizeof(last), hipMemcpyDeviceToHost));
    poses[0] = carve_pose(last);
  }
  CarveCounters c;
  memset(&c, 0, sizeof(c));
  if (map_carve_run(&h->map, h->sel, h->s_map, carve_geom(o, n_sweeps), o->kind_mask, clouds, n, poses, host_io, removed, cap, o->apply != 0, &c) != VLOAM_OK) {
    set_err("%s: the chain failed: %s", call, hipGetErrorString(hipGetLastError())); return VLOAM_ERR_HIP;
  }
  for (int k = 0; k < 2; k++) {
    res->examined[k] = (long long)c.cnt[k][0]; res->in_view[k] = (long long)c.cnt[k][1]; res->seen_through[k] = (long long)c.cnt[k][2];
    res->confirmed[k] = (long long)c.cnt[k][3]; res->removed[k] = (long long)c.cnt[k][4]; res->skipped_raw[k] = (long long)c.cnt[k][5];
  }
  res->n_removed_out = (long long)c.n_removed;
  if (res->n_removed_out > cap) {
    set_err("%s: %lld voxels would be removed, the list holds %lld: nothing was %s", call, res->n_removed_out, cap, o->apply ? "applied" : "listed"); return VLOAM_ERR_CAPACITY;
  }
  int merr = 0;
  HIPCHK(hipMemcpy(&merr, &SEL(h, h->map.frame)->error, sizeof(int), hipMemcpyDeviceToHost));
  return sticky_map_status(h, merr);
}

extern "C" {

void vloam_default_carve_options(vloam_carve_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->struct_size = (int)sizeof(*o);
  o->kind_mask = 3;
  o->rows = 64; o->cols = 1024;
  o->elev_min_deg = -25.f; o->elev_max_deg = 3.f;
  o->min_range = 2.f; o->max_range = 80.f;
  o->range_res = 0.05f; o->margin = 0.5f;
  o->min_votes = 1; o->apply = 0;
}

vloam_status vloam_map_carve(vloam_handle* h, const vloam_carve_options* o, const float* const* xyz_pad4, const int* n, const double* poses7, int n_sweeps,
                             float* removed_xyzi4, long long cap, vloam_carve_result* res) {
  return carve_run("vloam_map_carve", h, o, (const void* const*)xyz_pad4, n, poses7, n_sweeps, removed_xyzi4, cap, res, true);
}

vloam_status vloam_map_carve_device(vloam_handle* h, const vloam_carve_options* o, const void* const* d_xyz_pad4, const int* n, const double* poses7,
                                    int n_sweeps, void* d_removed_xyzi4, long long cap, vloam_carve_result* res) {
  return carve_run("vloam_map_carve_device", h, o, d_xyz_pad4, n, poses7, n_sweeps, d_removed_xyzi4, cap, res, false);
}

}  // extern "C"
