// Map import of libvloam_hip.so: vloam_map_import / vloam_map_import_device — two map-frame point clouds and a start transform into the voxel
// tables of a fresh handle (kernels and chain: map_import.hip).
#include "handle.h"

static_assert(sizeof(vloam_map_import_options) == 72 && offsetof(vloam_map_import_options, q_wmap_wodom) == 16 && offsetof(vloam_map_import_options, t_wmap_wodom) == 48,
              "vloam_map_import_options: 4 ints, then 7 doubles");
static_assert(sizeof(vloam_map_import_result) == 88 && offsetof(vloam_map_import_result, max_per_voxel) == 64 && offsetof(vloam_map_import_result, center_cube) == 72,
              "vloam_map_import_result: 8 long long, then 6 ints");

constexpr long long kImportMaxPoints = 16777216;   // per kind: point indices and segment offsets are ints, and the table's ceiling is 2^28 slots

// the refusals that need no handle, in the order c_api.h lists them; host_clouds: the clouds are host arrays (their floats are checked)
static vloam_status import_check_options(const char* call, const vloam_map_import_options* o, const void* corner, long long n_corner, const void* surf, long long n_surf,
                                         const void* out, bool host_clouds) {
  if (!o) { set_err("%s: null options", call); return VLOAM_ERR_INVALID; }
  if (o->struct_size != (int)sizeof(vloam_map_import_options)) { set_err("%s: vloam_map_import_options: struct_size must be %d", call, (int)sizeof(vloam_map_import_options)); return VLOAM_ERR_INVALID; }
  if (o->reserved[0] != 0 || o->reserved[1] != 0 || o->reserved[2] != 0) { set_err("%s: reserved must be 0", call); return VLOAM_ERR_INVALID; }
  for (int k = 0; k < 7; k++)
    if (!std::isfinite(k < 4 ? o->q_wmap_wodom[k] : o->t_wmap_wodom[k - 4])) {
      set_err("%s: start transform component %s[%d] is not finite", call, k < 4 ? "q_wmap_wodom" : "t_wmap_wodom", k < 4 ? k : k - 4); return VLOAM_ERR_INVALID;
    }
  const double* q = o->q_wmap_wodom;
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (fabs(nrm - 1.0) > 1e-6) { set_err("%s: the norm of q_wmap_wodom is %.9g: it must be within 1e-6 of 1", call, nrm); return VLOAM_ERR_INVALID; }
  if (n_corner < 0 || n_surf < 0) { set_err("%s: negative cloud size (%lld corner, %lld surf points)", call, n_corner, n_surf); return VLOAM_ERR_INVALID; }
  if (n_corner > kImportMaxPoints || n_surf > kImportMaxPoints) {
    set_err("%s: %lld corner / %lld surf points: an import takes at most %lld points of a kind", call, n_corner, n_surf, kImportMaxPoints); return VLOAM_ERR_INVALID;
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

// ... and the ones that do; then the chain.  result: host or device memory, as the clouds
static vloam_status import_run(const char* call, vloam_handle* h, const vloam_map_import_options* o, const void* corner, long long n_corner, const void* surf, long long n_surf,
                               void* result, bool host_form) {
  if (!h) { set_err("%s: null handle", call); return VLOAM_ERR_INVALID; }
  if (!h->cfg.with_mapping) { set_err("%s: the handle was created with with_mapping == 0: it keeps no map", call); return VLOAM_ERR_ORDER; }
  if (h->se.B != 1) { set_err("%s: an import starts one sequence: the handle has n_sessions = %d", call, h->se.B); return VLOAM_ERR_INVALID; }
  if (!is_fresh(h) || h->vo_used || h->map_imported) {
    if (h->map_imported) set_err("%s: the handle has already imported a map: an import works on a handle right after its creation", call);
    else set_err("%s: the handle is not fresh (%d sweeps taken, stage %d): an import works on a handle right after its creation", call, handed_over(h), h->stage);
    return VLOAM_ERR_ORDER;
  }
  HIPCHK(hipSetDevice(h->device));
  const int n[2] = {(int)n_corner, (int)n_surf};
  if (h->map.grow) {   // the empty tables step to the size the growth bound asks for, every point a record and a block key at most
    int lg[2];
    const long long bound[2] = {n_corner, n_surf};
    for (int k = 0; k < 2; k++) lg[k] = map_grow_restore_log2(&h->map, k, bound[k], bound[k]);
    if (map_grow_restore(&h->map, h->s_map, lg, bound, bound, 0) != VLOAM_OK) {
      set_err("%s: could not allocate voxel tables of 2^%d / 2^%d slots (hipMalloc)", call, lg[0], lg[1]); h->map.grow->failed_log2 = 0; return VLOAM_ERR_HIP;
    }
  }
  double pose[7];
  memcpy(pose, o->q_wmap_wodom, 4 * sizeof(double));
  memcpy(pose + 4, o->t_wmap_wodom, 3 * sizeof(double));
  const void* const cloud[2] = {corner, surf};
  vloam_map_import_result r;
  if (map_import_run(&h->map, h->s_map, pose, cloud, n, host_form, &r) != VLOAM_OK) {
    set_err("%s: the import chain failed: %s", call, hipGetErrorString(hipGetLastError())); return VLOAM_ERR_HIP;
  }
  h->map_imported = true;
  if (host_form) memcpy(result, &r, sizeof(r));
  else HIPCHK(hipMemcpy(result, &r, sizeof(r), hipMemcpyHostToDevice));
  // the sticky error word: the chain raises the map-full error a sweep would have raised
  int merr = 0;
  HIPCHK(hipMemcpy(&merr, &h->map.frame->error, sizeof(int), hipMemcpyDeviceToHost));
  if (merr & kErrMapFull) {
    for (int k = 0; k < 2; k++) {
      const long long slots = (long long)h->map.tab[k].mask + 1;
      if (r.n_voxels[k] * 10 > slots * 6) {
        set_err("%s: the %s cloud holds %lld distinct voxels, more than 60 %% of the %s table's 2^%d slots (%s): the handle is finished", call, k ? "surf" : "corner", r.n_voxels[k],
                k ? "surf" : "corner", __builtin_ctzll((unsigned long long)slots), h->map.grow ? "the growable map's ceiling" : "map_capacity_log2");
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

void vloam_default_map_import_options(vloam_map_import_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->struct_size = (int)sizeof(*o);
  o->q_wmap_wodom[3] = 1.0;
}

vloam_status vloam_map_import(vloam_handle* h, const vloam_map_import_options* o, const float* corner_xyzi4, long long n_corner, const float* surf_xyzi4, long long n_surf,
                              vloam_map_import_result* out) {
  static const char* const call = "vloam_map_import";
  TRY(import_check_options(call, o, corner_xyzi4, n_corner, surf_xyzi4, n_surf, out, true));
  return import_run(call, h, o, corner_xyzi4, n_corner, surf_xyzi4, n_surf, out, true);
}

vloam_status vloam_map_import_device(vloam_handle* h, const vloam_map_import_options* o, const void* d_corner, long long n_corner, const void* d_surf, long long n_surf,
                                     void* d_result) {
  static const char* const call = "vloam_map_import_device";
  TRY(import_check_options(call, o, d_corner, n_corner, d_surf, n_surf, d_result, false));
  return import_run(call, h, o, d_corner, n_corner, d_surf, n_surf, d_result, false);
}

}  // extern "C"
