// Map queries of libvloam_hip.so: vloam_map_query / vloam_map_query_device (k nearest map points of caller-supplied points; kernel:
// map_query.hip) and vloam_get_map_kind (one half of vloam_get_map).
#include "handle.h"

// the refusals that need no handle, in the order c_api.h lists them
static vloam_status query_check_options(const char* call, const vloam_map_query_options* o, const void* q, int n, const void* xyzi4, const void* d2, const void* count) {
  if (!o) { set_err("%s: null options", call); return VLOAM_ERR_INVALID; }
  if (o->struct_size != (int)sizeof(vloam_map_query_options)) { set_err("%s: vloam_map_query_options: struct_size must be %d", call, (int)sizeof(vloam_map_query_options)); return VLOAM_ERR_INVALID; }
  if (o->kind < 0 || o->kind > 2) { set_err("%s: kind must be 0 (corner map), 1 (surf map) or 2 (both), not %d", call, o->kind); return VLOAM_ERR_INVALID; }
  if (o->k < 1 || o->k > 8) { set_err("%s: k must be 1 .. 8 neighbours, not %d", call, o->k); return VLOAM_ERR_INVALID; }
  if (o->reserved != 0) { set_err("%s: reserved must be 0", call); return VLOAM_ERR_INVALID; }
  if (!(o->max_radius > 0.f) || !(o->max_radius <= FLT_MAX)) { set_err("%s: max_radius must be positive and finite", call); return VLOAM_ERR_INVALID; }
  if (n > 0 && (!q || !xyzi4 || !d2 || !count)) { set_err("%s: null buffer with n = %d", call, n); return VLOAM_ERR_INVALID; }
  if (n < 0) { set_err("%s: negative n (%d)", call, n); return VLOAM_ERR_INVALID; }
  return VLOAM_OK;
}

// ... and the ones that do; then what the handle still owes is enqueued, so that the mapping stream's order puts the query behind it
static vloam_status query_admit(const char* call, vloam_handle* h, const vloam_map_query_options* o) {
  if (!h) { set_err("%s: null handle", call); return VLOAM_ERR_INVALID; }
  const float leaf = o->kind == 1 ? h->cfg.mapping_plane_resolution : (o->kind == 0 ? h->cfg.mapping_line_resolution : std::min(h->cfg.mapping_line_resolution, h->cfg.mapping_plane_resolution));
  const float bound = 16.0f * leaf;
  if (o->max_radius > bound) { set_err("%s: max_radius %.9g m is above 16 leaves of the finest kind queried: at most %.9g m", call, (double)o->max_radius, (double)bound); return VLOAM_ERR_INVALID; }
  if (!h->cfg.with_mapping) { set_err("%s: the handle was created with with_mapping == 0: it keeps no map", call); return VLOAM_ERR_ORDER; }
  HIPCHK(hipSetDevice(h->device));
  return drain_deferred(h, 0, 0);
}

extern "C" {

void vloam_default_map_query_options(vloam_map_query_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->struct_size = (int)sizeof(*o);
  o->kind = 2; o->k = 5; o->max_radius = 1.0f;
}

vloam_status vloam_map_query_device(vloam_handle* h, const vloam_map_query_options* o, const void* d_xyz_pad4, int n, void* d_xyzi4, void* d_d2, void* d_count) {
  TRY(query_check_options("vloam_map_query_device", o, d_xyz_pad4, n, d_xyzi4, d_d2, d_count));
  TRY(query_admit("vloam_map_query_device", h, o));
  if (n == 0) return VLOAM_OK;
  if (map_query_enqueue(&h->map, h->s_map, o->kind, o->k, o->max_radius, d_xyz_pad4, n, d_xyzi4, d_d2, d_count) != VLOAM_OK) {
    set_err("vloam_map_query_device: the launch failed: %s", hipGetErrorString(hipGetLastError())); return VLOAM_ERR_HIP;
  }
  return VLOAM_OK;
}

vloam_status vloam_map_query(vloam_handle* h, const vloam_map_query_options* o, const float* xyz_pad4, int n, float* xyzi4, float* d2, int* count) {
  TRY(query_check_options("vloam_map_query", o, xyz_pad4, n, xyzi4, d2, count));
  TRY(query_admit("vloam_map_query", h, o));
  if (n == 0) return VLOAM_OK;
  // one temporary allocation: queries | points | distances | counts
  const size_t nk = (size_t)n * (size_t)o->k;
  const size_t off_out = (size_t)n * sizeof(float4), off_d2 = off_out + nk * sizeof(float4), off_cnt = off_d2 + nk * sizeof(float), total = off_cnt + (size_t)n * sizeof(int);
  char* d = nullptr;
  if (hipMalloc((void**)&d, total) != hipSuccess) { set_err("vloam_map_query: hipMalloc of %zu bytes failed", total); return VLOAM_ERR_HIP; }
  bool ok = hipMemcpyAsync(d, xyz_pad4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->s_map) == hipSuccess &&
            map_query_enqueue(&h->map, h->s_map, o->kind, o->k, o->max_radius, d, n, d + off_out, d + off_d2, d + off_cnt) == VLOAM_OK &&
            hipMemcpyAsync(xyzi4, d + off_out, nk * sizeof(float4), hipMemcpyDeviceToHost, h->s_map) == hipSuccess &&
            hipMemcpyAsync(d2, d + off_d2, nk * sizeof(float), hipMemcpyDeviceToHost, h->s_map) == hipSuccess &&
            hipMemcpyAsync(count, d + off_cnt, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->s_map) == hipSuccess;
  ok = hipStreamSynchronize(h->s_map) == hipSuccess && ok;
  // the sticky error words: every mapping enqueued so far has run, and so has the query (whose own lookups report a probe chain at its bound)
  int merr = 0;
  for (int b = 0; ok && b < h->se.B; b++) {
    int e = 0;
    ok = hipMemcpy(&e, (const char*)&h->map.frame->error + (size_t)b * h->se.ss, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
    merr |= e;
  }
  if (!ok) set_err("vloam_map_query: %s", hipGetErrorString(hipGetLastError()));
  (void)hipFree(d);
  if (!ok) return VLOAM_ERR_HIP;
  return sticky_map_status(h, merr);
}

vloam_status vloam_get_map_kind(vloam_handle* h, int kind, float* xyzi4, long long cap, long long* n) {
  if (kind != 0 && kind != 1) { set_err("vloam_get_map_kind: kind must be 0 (corner clouds) or 1 (surf clouds), not %d", kind); return VLOAM_ERR_INVALID; }
  if (!h || !n) return VLOAM_ERR_INVALID;
  if (!h->cfg.with_mapping) { *n = 0; return VLOAM_OK; }
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  return map_export_kind(&h->map, h->s_map, kind, xyzi4, cap, n);
}

}  // extern "C"
