// Localisation of libvloam_hip.so: vloam_map_localize / vloam_map_localize_device — a dry run of the mapping stage against the map as it is
// (kernels: map_localize.hip; the chain: map_localize_enqueue, map_kernels.hip).
#include "handle.h"

static_assert(sizeof(vloam_localize_options) == 16 && sizeof(vloam_localize_result) == 216 && offsetof(vloam_localize_result, q_guess) == 72 &&
              offsetof(vloam_localize_result, final_cost) == 200, "vloam_localize_result: 18 ints, then 18 doubles");

// the refusals that need no handle, in the order c_api.h lists them; host_clouds: the clouds are host arrays (their floats are checked)
static vloam_status localize_check_options(const char* call, const vloam_localize_options* o, const void* corner, int n_corner, const void* surf, int n_surf,
                                           const double* q, const double* t, const void* out, bool host_clouds) {
  if (!o) { set_err("%s: null options", call); return VLOAM_ERR_INVALID; }
  if (o->struct_size != (int)sizeof(vloam_localize_options)) { set_err("%s: vloam_localize_options: struct_size must be %d", call, (int)sizeof(vloam_localize_options)); return VLOAM_ERR_INVALID; }
  if (o->pose_frame < 0 || o->pose_frame > 1) { set_err("%s: pose_frame must be 0 (odometry-frame pose) or 1 (the guess itself, map frame), not %d", call, o->pose_frame); return VLOAM_ERR_INVALID; }
  if (o->reserved[0] != 0 || o->reserved[1] != 0) { set_err("%s: reserved must be 0", call); return VLOAM_ERR_INVALID; }
  if ((corner == nullptr) != (surf == nullptr)) { set_err("%s: the clouds are corner AND surf, or both null (the sweep in progress)", call); return VLOAM_ERR_INVALID; }
  if ((q == nullptr) != (t == nullptr)) { set_err("%s: the pose is q AND t", call); return VLOAM_ERR_INVALID; }
  if (corner && !q) { set_err("%s: a null pose goes with null clouds only (the sweep in progress and its odometry pose)", call); return VLOAM_ERR_INVALID; }
  if (corner && (n_corner < 0 || n_surf < 0)) { set_err("%s: negative cloud size (%d corner, %d surf points)", call, n_corner, n_surf); return VLOAM_ERR_INVALID; }
  if (corner && (n_corner > kMaxLessSharp || n_surf > (1 << 24))) {
    set_err("%s: %d corner / %d surf points: the corner cloud takes %d points, the surf cloud max_points (at most %d)", call, n_corner, n_surf, kMaxLessSharp, 1 << 24);
    return VLOAM_ERR_INVALID;
  }
  if (!out) { set_err("%s: null result", call); return VLOAM_ERR_INVALID; }
  if (host_clouds && corner) {
    const float* src[2] = {(const float*)corner, (const float*)surf};
    const int n[2] = {n_corner, n_surf};
    for (int k = 0; k < 2; k++)
      for (long long e = 0; e < 4ll * n[k]; e++)
        if (!std::isfinite(src[k][e])) { set_err("%s: %s cloud, point %lld: component %d is not finite", call, k ? "surf" : "corner", e / 4, (int)(e % 4)); return VLOAM_ERR_INVALID; }
  }
  if (q) {
    for (int k = 0; k < 7; k++)
      if (!std::isfinite(k < 4 ? q[k] : t[k - 4])) { set_err("%s: pose component %s[%d] is not finite", call, k < 4 ? "q" : "t", k < 4 ? k : k - 4); return VLOAM_ERR_INVALID; }
    const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (fabs(nrm - 1.0) > 1e-6) { set_err("%s: the quaternion's norm is %.9g: it must be within 1e-6 of 1", call, nrm); return VLOAM_ERR_INVALID; }
  }
  return VLOAM_OK;
}

// ... and the ones that do; then what the handle still owes is enqueued and the scratch exists
static vloam_status localize_admit(const char* call, vloam_handle* h, bool current_sweep, int n_corner, int n_surf) {
  if (!h) { set_err("%s: null handle", call); return VLOAM_ERR_INVALID; }
  if (!h->cfg.with_mapping) { set_err("%s: the handle was created with with_mapping == 0: it keeps no map", call); return VLOAM_ERR_ORDER; }
  if (h->se.B != 1) { set_err("%s: localisation drives one sequence: the handle has %d sessions", call, h->se.B); return VLOAM_ERR_INVALID; }
  if (h->map.tier()) { set_err("%s: not offered on a handle of the large stack tier (max_surf_stack_points = %d)", call, h->map.surf_cap); return VLOAM_ERR_INVALID; }
  if (!current_sweep && (n_surf > h->cfg.max_points || n_corner > h->cfg.max_points)) {
    set_err("%s: cloud of %d points exceeds max_points=%d", call, std::max(n_surf, n_corner), h->cfg.max_points); return VLOAM_ERR_CAPACITY;
  }
  if (current_sweep && (h->stage != 2 || ((h->frame + 1) % h->cfg.mapping_skip_frame) != 0)) {
    set_err("%s: null clouds mean the sweep in progress: between vloam_laser_odometry and vloam_laser_mapping of a stage-wise, mapped sweep", call);
    return VLOAM_ERR_ORDER;
  }
  HIPCHK(hipSetDevice(h->device));
  TRY(drain_deferred(h, 0, 0));
  if (map_localize_alloc(&h->map, h->s_map) != VLOAM_OK) { set_err("%s: the scratch allocation failed: %s", call, hipGetErrorString(hipGetLastError())); return VLOAM_ERR_HIP; }
  return VLOAM_OK;
}

// the chain, on the mapping stream; d_corner / d_surf: device clouds or both null
static vloam_status localize_enqueue(const char* call, vloam_handle* h, const vloam_localize_options* o, const float4* d_corner, int n_corner, const float4* d_surf,
                                     int n_surf, const double* q, const double* t, vloam_localize_result* d_result) {
  const int frame = h->frame, cur = set_of(frame);
  const double* row = nullptr;
  if (!d_corner) {   // the stacks of the sweep in progress (and, with a null pose, its odometry row): what enqueue_map would wait for
    HIPCHK(hipStreamWaitEvent(h->s_map, h->ev_lo[cur], 0));
    HIPCHK(hipStreamWaitEvent(h->s_map, h->ev_stack[cur], 0));
    if (!q) row = h->sub_pose_frame == frame ? h->sub_row : h->traj + (size_t)frame * 14;
  }
  double pose[7] = {0, 0, 0, 1, 0, 0, 0};
  if (q) { memcpy(pose, q, 4 * sizeof(double)); memcpy(pose + 4, t, 3 * sizeof(double)); }
  if (map_localize_enqueue(&h->map, h->s_map, d_corner, n_corner, d_surf, n_surf, cur, row, pose, q ? o->pose_frame : 0, d_result) != VLOAM_OK) {
    set_err("%s: the launch failed: %s", call, hipGetErrorString(hipGetLastError())); return VLOAM_ERR_HIP;
  }
  return VLOAM_OK;
}

extern "C" {

void vloam_default_localize_options(vloam_localize_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->struct_size = (int)sizeof(*o);
}

vloam_status vloam_map_localize_device(vloam_handle* h, const vloam_localize_options* o, const void* d_corner, int n_corner, const void* d_surf, int n_surf,
                                       const double q[4], const double t[3], void* d_result) {
  static const char* const call = "vloam_map_localize_device";
  TRY(localize_check_options(call, o, d_corner, n_corner, d_surf, n_surf, q, t, d_result, false));
  TRY(localize_admit(call, h, d_corner == nullptr, n_corner, n_surf));
  return localize_enqueue(call, h, o, (const float4*)d_corner, n_corner, (const float4*)d_surf, n_surf, q, t, (vloam_localize_result*)d_result);
}

vloam_status vloam_map_localize(vloam_handle* h, const vloam_localize_options* o, const float* corner_xyzi4, int n_corner, const float* surf_xyzi4, int n_surf,
                                const double q[4], const double t[3], vloam_localize_result* out) {
  static const char* const call = "vloam_map_localize";
  TRY(localize_check_options(call, o, corner_xyzi4, n_corner, surf_xyzi4, n_surf, q, t, out, true));
  TRY(localize_admit(call, h, corner_xyzi4 == nullptr, n_corner, n_surf));
  MapLocalize* L = h->map.loc;
  if (corner_xyzi4) {   // uploaded on the mapping stream: behind the previous call's chain, which may still read the buffers
    if (n_corner > 0) HIPCHK(hipMemcpyAsync(L->in[0], corner_xyzi4, (size_t)n_corner * sizeof(float4), hipMemcpyHostToDevice, h->s_map));
    if (n_surf > 0) HIPCHK(hipMemcpyAsync(L->in[1], surf_xyzi4, (size_t)n_surf * sizeof(float4), hipMemcpyHostToDevice, h->s_map));
  }
  TRY(localize_enqueue(call, h, o, corner_xyzi4 ? L->in[0] : nullptr, n_corner, corner_xyzi4 ? L->in[1] : nullptr, n_surf, q, t, L->result));
  HIPCHK(hipMemcpyAsync(out, L->result, sizeof(*out), hipMemcpyDeviceToHost, h->s_map));
  HIPCHK(hipStreamSynchronize(h->s_map));
  // the handle's sticky error word, as vloam_map_query: every mapping enqueued so far has run (this call wrote none of it)
  int merr = 0;
  HIPCHK(hipMemcpy(&merr, &h->map.frame->error, sizeof(int), hipMemcpyDeviceToHost));
  return sticky_map_status(h, merr);
}

}  // extern "C"
