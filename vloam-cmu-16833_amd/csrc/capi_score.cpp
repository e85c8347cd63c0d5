// Pose scores of libvloam_hip.so: vloam_map_score_poses / vloam_map_score_poses_device (M candidate poses of a sweep's feature clouds against the
// map in one launch; kernel: map_score.hip) and vloam_map_relocalize (a grid of candidates scored, the best few refined by vloam_map_localize).
#include "handle.h"

static_assert(sizeof(vloam_score_options) == 24 && sizeof(vloam_pose_score) == 32 && offsetof(vloam_pose_score, sum_d2_q24) == 16, "vloam_pose_score: 4 ints, 2 u64");
static_assert(sizeof(vloam_relocalize_options) == 88 && offsetof(vloam_relocalize_options, half_extent) == 32 && offsetof(vloam_relocalize_options, score) == 64,
              "vloam_relocalize_options: 8 ints, 4 doubles, the score options");
static_assert(sizeof(vloam_relocalize_result) == 2288 && offsetof(vloam_relocalize_result, coarse) == 48 && offsetof(vloam_relocalize_result, refined) == 304 &&
              offsetof(vloam_relocalize_result, fine) == 2032, "vloam_relocalize_result: 12 ints, 8 scores, 8 localisations, 8 scores");

static constexpr int kScoreMaxPoses = 65536;

// the refusals that need no handle, in the order c_api.h lists them; host: clouds and poses are host arrays (their values are checked)
static vloam_status score_check_options(const char* call, const vloam_score_options* o, const void* corner, int n_corner, const void* surf, int n_surf,
                                        const double* q4t3, int M, const void* out, bool host) {
  if (!o) { set_err("%s: null options", call); return VLOAM_ERR_INVALID; }
  if (o->struct_size != (int)sizeof(vloam_score_options)) { set_err("%s: vloam_score_options: struct_size must be %d", call, (int)sizeof(vloam_score_options)); return VLOAM_ERR_INVALID; }
  if (o->reserved != 0) { set_err("%s: reserved must be 0", call); return VLOAM_ERR_INVALID; }
  for (int k = 0; k < 2; k++)
    if (o->stride[k] < 1) { set_err("%s: stride[%d] must be at least 1, not %d", call, k, o->stride[k]); return VLOAM_ERR_INVALID; }
  for (int k = 0; k < 2; k++)
    if (!(o->radius[k] > 0.f) || !(o->radius[k] <= FLT_MAX)) { set_err("%s: radius[%d] must be positive and finite", call, k); return VLOAM_ERR_INVALID; }
  if (n_corner < 0 || n_surf < 0) { set_err("%s: negative cloud size (%d corner, %d surf points)", call, n_corner, n_surf); return VLOAM_ERR_INVALID; }
  if (M < 0 || M > kScoreMaxPoses) { set_err("%s: M must be 0 .. %d poses, not %d", call, kScoreMaxPoses, M); return VLOAM_ERR_INVALID; }
  if (n_corner > kMaxLessSharp || n_surf > (1 << 24)) {
    set_err("%s: %d corner / %d surf points: at most %d corner and %d surf points", call, n_corner, n_surf, kMaxLessSharp, 1 << 24);
    return VLOAM_ERR_INVALID;
  }
  if ((n_corner > 0 && !corner) || (n_surf > 0 && !surf) || (M > 0 && (!q4t3 || !out))) {
    set_err("%s: null buffer with a positive count (%d corner, %d surf points, %d poses)", call, n_corner, n_surf, M); return VLOAM_ERR_INVALID;
  }
  if (!host) return VLOAM_OK;
  const float* src[2] = {(const float*)corner, (const float*)surf};
  const int n[2] = {n_corner, n_surf};
  for (int k = 0; k < 2; k++)
    for (long long e = 0; e < 4ll * n[k]; e++)
      if (!std::isfinite(src[k][e])) { set_err("%s: %s cloud, point %lld: component %d is not finite", call, k ? "surf" : "corner", e / 4, (int)(e % 4)); return VLOAM_ERR_INVALID; }
  for (int m = 0; m < M; m++) {
    const double* p = q4t3 + (size_t)m * 7;
    for (int k = 0; k < 7; k++)
      if (!std::isfinite(p[k])) { set_err("%s: pose %d: component %s[%d] is not finite", call, m, k < 4 ? "q" : "t", k < 4 ? k : k - 4); return VLOAM_ERR_INVALID; }
    const double nrm = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3]);
    if (fabs(nrm - 1.0) > 1e-6) { set_err("%s: pose %d: the quaternion's norm is %.9g: it must be within 1e-6 of 1", call, m, nrm); return VLOAM_ERR_INVALID; }
  }
  return VLOAM_OK;
}

// ... and the ones that do; then what the handle still owes is enqueued, so that the mapping stream's order puts the score behind it
static vloam_status score_admit(const char* call, vloam_handle* h, const vloam_score_options* o) {
  if (!h) { set_err("%s: null handle", call); return VLOAM_ERR_INVALID; }
  for (int k = 0; k < 2; k++) {
    const float leaf = k ? h->cfg.mapping_plane_resolution : h->cfg.mapping_line_resolution;
    const float bound = 16.0f * leaf;
    if (o->radius[k] > bound) {
      set_err("%s: radius[%d] %.9g m is above 16 leaves of the %s map: at most %.9g m", call, k, (double)o->radius[k], k ? "surf" : "corner", (double)bound);
      return VLOAM_ERR_INVALID;
    }
  }
  if (!h->cfg.with_mapping) { set_err("%s: the handle was created with with_mapping == 0: it keeps no map", call); return VLOAM_ERR_ORDER; }
  if (h->se.B != 1) { set_err("%s: pose scores drive one sequence: the handle has %d sessions", call, h->se.B); return VLOAM_ERR_INVALID; }
  HIPCHK(hipSetDevice(h->device));
  return drain_deferred(h, 0, 0);
}

// the host form behind its checks: temporary allocations, the mapping stream only
static vloam_status score_host(const char* call, vloam_handle* h, const vloam_score_options* o, const float* corner, int n_corner, const float* surf, int n_surf,
                               const double* q4t3, int M, vloam_pose_score* out) {
  if (M == 0) return VLOAM_OK;
  // one temporary allocation: poses | records | corner cloud | surf cloud
  const size_t off_out = (size_t)M * 7 * sizeof(double), off_c = off_out + (size_t)M * sizeof(vloam_pose_score), off_s = off_c + (size_t)n_corner * sizeof(float4),
               total = off_s + (size_t)n_surf * sizeof(float4);
  char* d = nullptr;
  if (hipMalloc((void**)&d, total) != hipSuccess) { set_err("%s: hipMalloc of %zu bytes failed", call, total); return VLOAM_ERR_HIP; }
  bool ok = hipMemcpyAsync(d, q4t3, off_out, hipMemcpyHostToDevice, h->s_map) == hipSuccess;
  if (n_corner > 0) ok = ok && hipMemcpyAsync(d + off_c, corner, (size_t)n_corner * sizeof(float4), hipMemcpyHostToDevice, h->s_map) == hipSuccess;
  if (n_surf > 0) ok = ok && hipMemcpyAsync(d + off_s, surf, (size_t)n_surf * sizeof(float4), hipMemcpyHostToDevice, h->s_map) == hipSuccess;
  ok = ok && map_score_enqueue(&h->map, h->s_map, d + off_c, n_corner, d + off_s, n_surf, o->stride, o->radius, (const double*)d, M, d + off_out) == VLOAM_OK &&
       hipMemcpyAsync(out, d + off_out, (size_t)M * sizeof(vloam_pose_score), hipMemcpyDeviceToHost, h->s_map) == hipSuccess;
  ok = hipStreamSynchronize(h->s_map) == hipSuccess && ok;
  // the sticky error word: every mapping enqueued so far has run, and so has the score (whose own lookups report a probe chain at its bound)
  int merr = 0;
  ok = ok && hipMemcpy(&merr, &h->map.frame->error, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
  if (!ok) set_err("%s: %s", call, hipGetErrorString(hipGetLastError()));
  (void)hipFree(d);
  if (!ok) return VLOAM_ERR_HIP;
  return sticky_map_status(h, merr);
}

// the ranking of c_api.h: more hits, then the smaller sum, then the smaller index
static bool score_before(const vloam_pose_score& a, int ia, const vloam_pose_score& b, int ib) {
  const long long ha = (long long)a.n_hit[0] + a.n_hit[1], hb = (long long)b.n_hit[0] + b.n_hit[1];
  if (ha != hb) return ha > hb;
  const unsigned long long sa = a.sum_d2_q24[0] + a.sum_d2_q24[1], sb = b.sum_d2_q24[0] + b.sum_d2_q24[1];
  if (sa != sb) return sa < sb;
  return ia < ib;
}

extern "C" {

void vloam_default_score_options(vloam_score_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->struct_size = (int)sizeof(*o);
  o->stride[0] = o->stride[1] = 1;
  o->radius[0] = o->radius[1] = 1.0f;
}

vloam_status vloam_map_score_poses_device(vloam_handle* h, const vloam_score_options* o, const void* d_corner, int n_corner, const void* d_surf, int n_surf,
                                          const void* d_q4t3, int M, void* d_out) {
  static const char* const call = "vloam_map_score_poses_device";
  TRY(score_check_options(call, o, d_corner, n_corner, d_surf, n_surf, (const double*)d_q4t3, M, d_out, false));
  TRY(score_admit(call, h, o));
  if (M == 0) return VLOAM_OK;
  if (map_score_enqueue(&h->map, h->s_map, d_corner, n_corner, d_surf, n_surf, o->stride, o->radius, (const double*)d_q4t3, M, d_out) != VLOAM_OK) {
    set_err("%s: the launch failed: %s", call, hipGetErrorString(hipGetLastError())); return VLOAM_ERR_HIP;
  }
  return VLOAM_OK;
}

vloam_status vloam_map_score_poses(vloam_handle* h, const vloam_score_options* o, const float* corner_xyzi4, int n_corner, const float* surf_xyzi4, int n_surf,
                                   const double* q4t3, int M, vloam_pose_score* out) {
  static const char* const call = "vloam_map_score_poses";
  TRY(score_check_options(call, o, corner_xyzi4, n_corner, surf_xyzi4, n_surf, q4t3, M, out, true));
  TRY(score_admit(call, h, o));
  return score_host(call, h, o, corner_xyzi4, n_corner, surf_xyzi4, n_surf, q4t3, M, out);
}

void vloam_default_relocalize_options(vloam_relocalize_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->struct_size = (int)sizeof(*o);
  o->n_xy[0] = o->n_xy[1] = 9; o->n_z = 1; o->n_yaw = 9;
  o->top_k = 4;
  o->half_extent[0] = o->half_extent[1] = 2.0; o->half_extent[2] = 0.0;
  o->half_yaw = 10.0 * 3.14159265358979323846 / 180.0;
  vloam_default_score_options(&o->score);
}

vloam_status vloam_map_relocalize(vloam_handle* h, const vloam_relocalize_options* o, const float* corner_xyzi4, int n_corner, const float* surf_xyzi4, int n_surf,
                                  const double q_center[4], const double t_center[3], vloam_relocalize_result* out) {
  static const char* const call = "vloam_map_relocalize";
  if (!o) { set_err("%s: null options", call); return VLOAM_ERR_INVALID; }
  if (o->struct_size != (int)sizeof(vloam_relocalize_options)) { set_err("%s: vloam_relocalize_options: struct_size must be %d", call, (int)sizeof(vloam_relocalize_options)); return VLOAM_ERR_INVALID; }
  if (o->reserved[0] != 0 || o->reserved[1] != 0) { set_err("%s: reserved must be 0", call); return VLOAM_ERR_INVALID; }
  const int steps[4] = {o->n_xy[0], o->n_xy[1], o->n_z, o->n_yaw};
  long long prod = 1;
  for (int k = 0; k < 4; k++) {
    if (steps[k] < 1 || steps[k] > kScoreMaxPoses) { set_err("%s: every step count is 1 .. %d (n_xy %d, %d; n_z %d; n_yaw %d)", call, kScoreMaxPoses, steps[0], steps[1], steps[2], steps[3]); return VLOAM_ERR_INVALID; }
    prod *= steps[k];
    if (prod > kScoreMaxPoses) { set_err("%s: the grid has more than %d candidates (n_xy %d, %d; n_z %d; n_yaw %d)", call, kScoreMaxPoses, steps[0], steps[1], steps[2], steps[3]); return VLOAM_ERR_INVALID; }
  }
  if (o->top_k < 1 || o->top_k > 8) { set_err("%s: top_k must be 1 .. 8 candidates, not %d", call, o->top_k); return VLOAM_ERR_INVALID; }
  for (int k = 0; k < 3; k++)
    if (!(o->half_extent[k] >= 0.0) || !(o->half_extent[k] <= DBL_MAX)) { set_err("%s: half_extent[%d] must be finite and not negative", call, k); return VLOAM_ERR_INVALID; }
  if (!(o->half_yaw >= 0.0) || !(o->half_yaw <= 3.14159265358979323846)) { set_err("%s: half_yaw must be 0 .. pi radians", call); return VLOAM_ERR_INVALID; }
  if (!corner_xyzi4 || !surf_xyzi4) { set_err("%s: the clouds are corner AND surf (the sweep in progress cannot be relocalised)", call); return VLOAM_ERR_INVALID; }
  if (!q_center || !t_center) { set_err("%s: the centre is q AND t", call); return VLOAM_ERR_INVALID; }
  if (!out) { set_err("%s: null result", call); return VLOAM_ERR_INVALID; }
  const int M = (int)prod;
  double centre[7];
  memcpy(centre, q_center, 4 * sizeof(double)); memcpy(centre + 4, t_center, 3 * sizeof(double));
  vloam_pose_score dummy;
  TRY(score_check_options(call, &o->score, corner_xyzi4, n_corner, surf_xyzi4, n_surf, centre, 1, &dummy, true));
  // the handle: the score's refusals, then the ones vloam_map_localize would make only after the candidates had been scored
  TRY(score_admit(call, h, &o->score));
  if (h->map.tier()) { set_err("%s: not offered on a handle of the large stack tier (max_surf_stack_points = %d)", call, h->map.surf_cap); return VLOAM_ERR_INVALID; }
  if (n_surf > h->cfg.max_points || n_corner > h->cfg.max_points) {
    set_err("%s: cloud of %d points exceeds max_points=%d", call, std::max(n_surf, n_corner), h->cfg.max_points); return VLOAM_ERR_CAPACITY;
  }
  // candidates, f64 on the host
  std::vector<double> poses((size_t)M * 7);
  const double ext[4] = {o->half_extent[0], o->half_extent[1], o->half_extent[2], o->half_yaw};
  auto offset = [&](int axis, int i) { return steps[axis] == 1 ? 0.0 : -ext[axis] + 2.0 * ext[axis] * (double)i / (double)(steps[axis] - 1); };
  for (int m = 0; m < M; m++) {
    const int ix = m % steps[0], iy = (m / steps[0]) % steps[1], iz = (m / (steps[0] * steps[1])) % steps[2], iyaw = m / (steps[0] * steps[1] * steps[2]);
    const double a = offset(3, iyaw), sz = sin(a / 2.0), cw = cos(a / 2.0);
    double* p = &poses[(size_t)m * 7];
    // (0, 0, sz, cw) * q_center
    p[0] = cw * centre[0] - sz * centre[1];
    p[1] = cw * centre[1] + sz * centre[0];
    p[2] = cw * centre[2] + sz * centre[3];
    p[3] = cw * centre[3] - sz * centre[2];
    p[4] = centre[4] + offset(0, ix); p[5] = centre[5] + offset(1, iy); p[6] = centre[6] + offset(2, iz);
  }
  std::vector<vloam_pose_score> coarse((size_t)M);
  TRY(score_host(call, h, &o->score, corner_xyzi4, n_corner, surf_xyzi4, n_surf, poses.data(), M, coarse.data()));
  std::vector<int> order((size_t)M);
  for (int m = 0; m < M; m++) order[m] = m;
  const int K = std::min(o->top_k, M);
  std::partial_sort(order.begin(), order.begin() + K, order.end(), [&](int a, int b) { return score_before(coarse[a], a, coarse[b], b); });
  memset(out, 0, sizeof(*out));
  out->n_candidates = M;
  vloam_localize_options lo;
  vloam_default_localize_options(&lo);
  lo.pose_frame = 1;
  double fine_poses[8 * 7];
  for (int j = 0; j < K; j++) {
    const int m = order[j];
    out->candidate[j] = m;
    out->coarse[j] = coarse[m];
    TRY(vloam_map_localize(h, &lo, corner_xyzi4, n_corner, surf_xyzi4, n_surf, &poses[(size_t)m * 7], &poses[(size_t)m * 7 + 4], &out->refined[j]));
    out->n_refined = j + 1;
    memcpy(fine_poses + 7 * j, out->refined[j].q_map, 4 * sizeof(double)); memcpy(fine_poses + 7 * j + 4, out->refined[j].t_map, 3 * sizeof(double));
  }
  TRY(score_host(call, h, &o->score, corner_xyzi4, n_corner, surf_xyzi4, n_surf, fine_poses, K, out->fine));
  int best = 0;
  for (int j = 1; j < K; j++)
    if (score_before(out->fine[j], j, out->fine[best], best)) best = j;
  out->best = best;
  return VLOAM_OK;
}

}  // extern "C"
