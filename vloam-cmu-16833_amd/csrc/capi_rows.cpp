// The per-sweep row products of libvloam_hip.so: one row per sweep, written by the stage streams themselves behind events of a RowEvents ring
// (handle.h), read without synchronising the pipeline.  Three products: the sweep log (rows in the arena), pose information (rows of its own) and its add-on, the pose covariance rows.
#include "handle.h"

// Rows first .. first + count - 1 of a product, row 0 of the selected session at `row0`: enqueue what is still owed, wait for the writers of the
// last row asked for, copy.
static vloam_status read_rows(vloam_handle* h, const char* call, const RowEvents& ring, const void* row0, size_t row_bytes, int first, int count, void* out) {
  if (!out || first < 0 || count < 0 || first + count > handed_over(h)) {   // (a host sweep in flight is enqueued by the drain below)
    set_err("%s: sweeps %d .. %d are not all handed over (vloam_frame_count)", call, first, first + count - 1); return VLOAM_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(h->device));
  TRY(drain_deferred(h, 0, 0));   // enqueue only: every stage of every sweep handed over so far is then on its stream
  if (count == 0) return VLOAM_OK;
  HIPCHK(ring.wait_row(first + count - 1));
  HIPCHK(hipMemcpy(out, (const char*)row0 + (size_t)first * row_bytes, row_bytes * (size_t)count, hipMemcpyDeviceToHost));
  return VLOAM_OK;
}

extern "C" {

// ------------------------------------------------------------------ per-sweep diagnostics log (vloam_limits_ext::sweep_log)
static vloam_status require_sweep_log(const vloam_handle* h) {
  if (!h->sweep_log) { set_err("the handle was created without vloam_limits_ext::sweep_log: no per-sweep log is kept"); return VLOAM_ERR_ORDER; }
  return VLOAM_OK;
}
// row 0 of the selected session
static vloam_sweep_record* sweep_log_rows(const vloam_handle* h) { return SEL(h, h->log_rows); }
vloam_status vloam_get_sweep_log(vloam_handle* h, int first, int count, vloam_sweep_record* out) {
  if (!h) return VLOAM_ERR_INVALID;
  TRY(require_sweep_log(h));
  return read_rows(h, "vloam_get_sweep_log", h->log_ring, sweep_log_rows(h), sizeof(vloam_sweep_record), first, count, out);
}
vloam_status vloam_sweep_log_device_ptr(vloam_handle* h, void** d_rows, long long* bytes) {
  if (!h || !d_rows || !bytes) return VLOAM_ERR_INVALID;
  TRY(require_sweep_log(h));
  *d_rows = sweep_log_rows(h);
  *bytes = (long long)h->cfg.max_frames * (long long)sizeof(vloam_sweep_record);
  return VLOAM_OK;
}

// ------------------------------------------------------------------ per-sweep pose information matrices (vloam_pose_info_enable)
void vloam_default_pose_info_options(vloam_pose_info_options* opt) {
  if (!opt) return;
  opt->struct_size = (int)sizeof(vloam_pose_info_options);
  opt->reserved = 0;
  opt->lo_min_eigenvalue = 0.0;
  opt->map_min_eigenvalue = 0.0;
}
vloam_status vloam_pose_info_enable(vloam_handle* h, const vloam_pose_info_options* opt) {
  vloam_pose_info_options o;
  vloam_default_pose_info_options(&o);
  if (opt) {   // the options first: before any device call, before anything of the handle is looked at
    if (opt->struct_size != (int)sizeof(vloam_pose_info_options)) { set_err("vloam_pose_info_options: struct_size must be %d", (int)sizeof(vloam_pose_info_options)); return VLOAM_ERR_INVALID; }
    if (opt->reserved != 0) { set_err("vloam_pose_info_options: reserved must be 0"); return VLOAM_ERR_INVALID; }
    for (const double v : {opt->lo_min_eigenvalue, opt->map_min_eigenvalue})
      if (!(v >= 0.0) || !(v <= DBL_MAX)) { set_err("vloam_pose_info_options: lo_min_eigenvalue / map_min_eigenvalue must be finite and >= 0 (0 = never degenerate)"); return VLOAM_ERR_INVALID; }
    o = *opt;
  }
  if (!h) { set_err("vloam_pose_info_enable: null handle"); return VLOAM_ERR_INVALID; }
  if (h->pose_info || !is_fresh(h)) {
    set_err("vloam_pose_info_enable: the handle is not fresh (%d sweeps taken, stage %d%s): the product is enabled right after creation, once", handed_over(h),
            h->stage, h->pose_info ? ", already enabled" : "");
    return VLOAM_ERR_ORDER;
  }
  HIPCHK(hipSetDevice(h->device));
  const size_t row_bytes = sizeof(vloam_pose_info_record) * (size_t)h->cfg.max_frames * (size_t)h->se.B;
  PoseInfo P;
  P.max_frames = h->cfg.max_frames;
  P.min_eig[0] = o.lo_min_eigenvalue; P.min_eig[1] = o.map_min_eigenvalue;
  if (hipMalloc((void**)&P.rows, row_bytes) != hipSuccess) { set_err("vloam_pose_info_enable: hipMalloc of %zu MB failed", row_bytes >> 20); return VLOAM_ERR_HIP; }
  if (hipMalloc((void**)&P.scratch, sizeof(PoseInfoScratch) * 2 * (size_t)h->se.B) != hipSuccess) {
    (void)hipFree(P.rows); set_err("vloam_pose_info_enable: hipMalloc failed"); return VLOAM_ERR_HIP;
  }
  h->pi = P;   // (vloam_destroy frees them, whatever the rest reaches)
  HIPCHK(h->pi_ring.create(2));
  HIPCHK(pose_info_init(h->stream, h->pi, h->se.B));
  HIPCHK(hipStreamSynchronize(h->stream));   // the stage streams do not wait for this one
  h->pose_info = true;
  return VLOAM_OK;
}
static vloam_status require_pose_info(const vloam_handle* h) {
  if (!h->pose_info) { set_err("the handle never enabled the pose information product (vloam_pose_info_enable)"); return VLOAM_ERR_ORDER; }
  return VLOAM_OK;
}
// row 0 of the selected session
static vloam_pose_info_record* pose_info_rows(const vloam_handle* h) { return h->pi.rows + (size_t)h->sel * (size_t)h->cfg.max_frames; }
vloam_status vloam_get_pose_info(vloam_handle* h, int first, int count, vloam_pose_info_record* out) {
  if (!h) return VLOAM_ERR_INVALID;
  TRY(require_pose_info(h));
  return read_rows(h, "vloam_get_pose_info", h->pi_ring, pose_info_rows(h), sizeof(vloam_pose_info_record), first, count, out);
}
vloam_status vloam_pose_info_device_ptr(vloam_handle* h, void** d_rows, long long* bytes) {
  if (!h || !d_rows || !bytes) return VLOAM_ERR_INVALID;
  TRY(require_pose_info(h));
  *d_rows = pose_info_rows(h);
  *bytes = (long long)h->cfg.max_frames * (long long)sizeof(vloam_pose_info_record);
  return VLOAM_OK;
}

// ------------------------------------------------------------------ per-sweep pose covariance rows (vloam_pose_cov_enable), an add-on of the above
void vloam_default_pose_cov_options(vloam_pose_cov_options* opt) {
  if (!opt) return;
  opt->struct_size = (int)sizeof(vloam_pose_cov_options);
  opt->reserved = 0;
  opt->lo_min_eigenvalue = 0.0;
  opt->map_min_eigenvalue = 0.0;
  opt->vo_min_eigenvalue = 0.0;
}
vloam_status vloam_pose_cov_enable(vloam_handle* h, const vloam_pose_cov_options* opt) {
  vloam_pose_cov_options o;
  vloam_default_pose_cov_options(&o);
  if (opt) {   // the options first: before any device call, before anything of the handle is looked at
    if (opt->struct_size != (int)sizeof(vloam_pose_cov_options)) { set_err("vloam_pose_cov_options: struct_size must be %d", (int)sizeof(vloam_pose_cov_options)); return VLOAM_ERR_INVALID; }
    if (opt->reserved != 0) { set_err("vloam_pose_cov_options: reserved must be 0"); return VLOAM_ERR_INVALID; }
    for (const double v : {opt->lo_min_eigenvalue, opt->map_min_eigenvalue, opt->vo_min_eigenvalue})
      if (!(v >= 0.0) || !(v <= DBL_MAX)) { set_err("vloam_pose_cov_options: lo_min_eigenvalue / map_min_eigenvalue / vo_min_eigenvalue must be finite and >= 0"); return VLOAM_ERR_INVALID; }
    o = *opt;
  }
  if (!h) { set_err("vloam_pose_cov_enable: null handle"); return VLOAM_ERR_INVALID; }
  if (!h->pose_info) { set_err("vloam_pose_cov_enable: the rows are computed from the pose information rows: call vloam_pose_info_enable first"); return VLOAM_ERR_ORDER; }
  if (h->pose_cov || !is_fresh(h)) {
    set_err("vloam_pose_cov_enable: the handle is not fresh (%d sweeps taken, stage %d%s): the product is enabled right after vloam_pose_info_enable, once",
            handed_over(h), h->stage, h->pose_cov ? ", already enabled" : "");
    return VLOAM_ERR_ORDER;
  }
  HIPCHK(hipSetDevice(h->device));
  const size_t row_bytes = sizeof(vloam_pose_cov_record) * (size_t)h->cfg.max_frames * (size_t)h->se.B;
  PoseCov P;
  P.max_frames = h->cfg.max_frames;
  P.min_eig[0] = o.lo_min_eigenvalue; P.min_eig[1] = o.map_min_eigenvalue; P.min_eig[2] = o.vo_min_eigenvalue;
  if (hipMalloc((void**)&P.rows, row_bytes) != hipSuccess) { set_err("vloam_pose_cov_enable: hipMalloc of %zu MB failed", row_bytes >> 20); return VLOAM_ERR_HIP; }
  if (hipMalloc((void**)&P.scratch, sizeof(PoseCovScratch) * (size_t)h->se.B) != hipSuccess) {
    (void)hipFree(P.rows); set_err("vloam_pose_cov_enable: hipMalloc failed"); return VLOAM_ERR_HIP;
  }
  h->pc = P;   // (vloam_destroy frees them, whatever the rest reaches)
  HIPCHK(pose_cov_init(h->stream, h->pc, h->se.B));
  HIPCHK(hipStreamSynchronize(h->stream));   // the stage streams do not wait for this one
  h->pose_cov = true;
  return VLOAM_OK;
}
static vloam_status require_pose_cov(const vloam_handle* h) {
  if (!h->pose_cov) { set_err("the handle never enabled the pose covariance product (vloam_pose_cov_enable)"); return VLOAM_ERR_ORDER; }
  return VLOAM_OK;
}
// row 0 of the selected session
static vloam_pose_cov_record* pose_cov_rows(const vloam_handle* h) { return h->pc.rows + (size_t)h->sel * (size_t)h->cfg.max_frames; }
vloam_status vloam_get_pose_cov(vloam_handle* h, int first, int count, vloam_pose_cov_record* out) {
  if (!h) return VLOAM_ERR_INVALID;
  TRY(require_pose_cov(h));
  return read_rows(h, "vloam_get_pose_cov", h->pi_ring, pose_cov_rows(h), sizeof(vloam_pose_cov_record), first, count, out);   // (one ring for both products: handle.h)
}
vloam_status vloam_pose_cov_device_ptr(vloam_handle* h, void** d_rows, long long* bytes) {
  if (!h || !d_rows || !bytes) return VLOAM_ERR_INVALID;
  TRY(require_pose_cov(h));
  *d_rows = pose_cov_rows(h);
  *bytes = (long long)h->cfg.max_frames * (long long)sizeof(vloam_pose_cov_record);
  return VLOAM_OK;
}

}  // extern "C"
