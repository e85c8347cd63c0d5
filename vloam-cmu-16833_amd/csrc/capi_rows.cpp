// The per-sweep row products of libvloam_hip.so: one row per sweep, written by the stage streams themselves behind events of a RowEvents ring
// (handle.h), read without synchronising the pipeline.  Three products: the sweep log (rows in the arena), pose information (rows of its own) and its add-on, the pose covariance rows.
#include "handle.h"

// What a product is to the entry points below.  All three: Rec, its record; on, the handle's flag that the product is kept; row0, row 0 of the
// selected session; ring, where its writers' events are; missing, what a call says on a handle without the product.  The two that are enabled
// after creation also: Opt / defaults, the options; Dev / dev, the handle's device memory of the product; min_eig, the options' thresholds in
// the order of Dev::min_eig, and eig_rule, what they must be; after, what the enable call must follow directly; needs, why the handle cannot
// take the product at all (null: it can); scratch_bytes and init (pose_info.h, pose_cov.h).
struct SweepLogRows {
  typedef vloam_sweep_record Rec;
  static bool& on(vloam_handle* h) { return h->sweep_log; }
  static Rec* row0(const vloam_handle* h) { return SEL(h, h->log_rows); }
  static const RowEvents& ring(const vloam_handle* h) { return h->log_ring; }
  static constexpr const char* missing = "the handle was created without vloam_limits_ext::sweep_log: no per-sweep log is kept";
};
struct PoseInfoRows {
  typedef vloam_pose_info_record Rec;
  typedef vloam_pose_info_options Opt;
  typedef PoseInfo Dev;
  static bool& on(vloam_handle* h) { return h->pose_info; }
  static Rec* row0(const vloam_handle* h) { return h->pi.rows + (size_t)h->sel * (size_t)h->cfg.max_frames; }
  static const RowEvents& ring(const vloam_handle* h) { return h->pi_ring; }
  static constexpr const char* missing = "the handle never enabled the pose information product (vloam_pose_info_enable)";
  static constexpr const char* name = "pose_info";
  static constexpr void (*defaults)(Opt*) = vloam_default_pose_info_options;
  static constexpr double Opt::*min_eig[] = {&Opt::lo_min_eigenvalue, &Opt::map_min_eigenvalue};
  static constexpr const char* eig_rule = "lo_min_eigenvalue / map_min_eigenvalue must be finite and >= 0 (0 = never degenerate)";
  static constexpr const char* after = "creation";
  static const char* needs(const vloam_handle*) { return nullptr; }
  static Dev& dev(vloam_handle* h) { return h->pi; }
  static constexpr size_t (*scratch_bytes)(int) = vloam::pose_info_scratch_bytes;
  static hipError_t init(vloam_handle* h) {
    const hipError_t e = h->pi_ring.create(2);
    return e != hipSuccess ? e : pose_info_init(h->stream, h->pi, h->se.B);
  }
};
struct PoseCovRows {
  typedef vloam_pose_cov_record Rec;
  typedef vloam_pose_cov_options Opt;
  typedef PoseCov Dev;
  static bool& on(vloam_handle* h) { return h->pose_cov; }
  static Rec* row0(const vloam_handle* h) { return h->pc.rows + (size_t)h->sel * (size_t)h->cfg.max_frames; }
  static const RowEvents& ring(const vloam_handle* h) { return h->pi_ring; }   // (one ring for both products: handle.h)
  static constexpr const char* missing = "the handle never enabled the pose covariance product (vloam_pose_cov_enable)";
  static constexpr const char* name = "pose_cov";
  static constexpr void (*defaults)(Opt*) = vloam_default_pose_cov_options;
  static constexpr double Opt::*min_eig[] = {&Opt::lo_min_eigenvalue, &Opt::map_min_eigenvalue, &Opt::vo_min_eigenvalue};
  static constexpr const char* eig_rule = "lo_min_eigenvalue / map_min_eigenvalue / vo_min_eigenvalue must be finite and >= 0";
  static constexpr const char* after = "vloam_pose_info_enable";
  static const char* needs(const vloam_handle* h) {
    return h->pose_info ? nullptr : "the rows are computed from the pose information rows: call vloam_pose_info_enable first";
  }
  static Dev& dev(vloam_handle* h) { return h->pc; }
  static constexpr size_t (*scratch_bytes)(int) = vloam::pose_cov_scratch_bytes;
  static hipError_t init(vloam_handle* h) { return pose_cov_init(h->stream, h->pc, h->se.B); }
};

template <class R>
static vloam_status require_rows(vloam_handle* h) {
  if (!R::on(h)) { set_err("%s", R::missing); return VLOAM_ERR_ORDER; }
  return VLOAM_OK;
}
// Rows first .. first + count - 1 of the selected session: enqueue what is still owed, wait for the writers of the last row asked for, copy.
template <class R>
static vloam_status get_rows(vloam_handle* h, const char* call, int first, int count, typename R::Rec* out) {
  if (!h) return VLOAM_ERR_INVALID;
  TRY(require_rows<R>(h));
  if (!out || first < 0 || count < 0 || first + count > handed_over(h)) {   // (a host sweep in flight is enqueued by the drain below)
    set_err("%s: sweeps %d .. %d are not all handed over (vloam_frame_count)", call, first, first + count - 1); return VLOAM_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(h->device));
  TRY(drain_deferred(h, 0, 0));   // enqueue only: every stage of every sweep handed over so far is then on its stream
  if (count == 0) return VLOAM_OK;
  HIPCHK(R::ring(h).wait_row(first + count - 1));
  HIPCHK(hipMemcpy(out, R::row0(h) + first, sizeof(typename R::Rec) * (size_t)count, hipMemcpyDeviceToHost));
  return VLOAM_OK;
}
template <class R>
static vloam_status rows_device_ptr(vloam_handle* h, void** d_rows, long long* bytes) {
  if (!h || !d_rows || !bytes) return VLOAM_ERR_INVALID;
  TRY(require_rows<R>(h));
  *d_rows = R::row0(h);
  *bytes = (long long)h->cfg.max_frames * (long long)sizeof(typename R::Rec);
  return VLOAM_OK;
}
template <class R>
static vloam_status enable_rows(vloam_handle* h, const typename R::Opt* opt) {
  typename R::Opt o;
  R::defaults(&o);
  if (opt) {   // the options first: before any device call, before anything of the handle is looked at
    if (opt->struct_size != (int)sizeof(o)) { set_err("vloam_%s_options: struct_size must be %d", R::name, (int)sizeof(o)); return VLOAM_ERR_INVALID; }
    if (opt->reserved != 0) { set_err("vloam_%s_options: reserved must be 0", R::name); return VLOAM_ERR_INVALID; }
    for (const auto m : R::min_eig)
      if (!(opt->*m >= 0.0) || !(opt->*m <= DBL_MAX)) { set_err("vloam_%s_options: %s", R::name, R::eig_rule); return VLOAM_ERR_INVALID; }
    o = *opt;
  }
  if (!h) { set_err("vloam_%s_enable: null handle", R::name); return VLOAM_ERR_INVALID; }
  if (R::needs(h)) { set_err("vloam_%s_enable: %s", R::name, R::needs(h)); return VLOAM_ERR_ORDER; }
  if (R::on(h) || !is_fresh(h)) {
    set_err("vloam_%s_enable: the handle is not fresh (%d sweeps taken, stage %d%s): the product is enabled right after %s, once", R::name, handed_over(h),
            h->stage, R::on(h) ? ", already enabled" : "", R::after);
    return VLOAM_ERR_ORDER;
  }
  HIPCHK(hipSetDevice(h->device));
  const size_t row_bytes = sizeof(typename R::Rec) * (size_t)h->cfg.max_frames * (size_t)h->se.B;
  typename R::Dev P;
  P.max_frames = h->cfg.max_frames;
  int k = 0;
  for (const auto m : R::min_eig) P.min_eig[k++] = o.*m;
  if (hipMalloc((void**)&P.rows, row_bytes) != hipSuccess) { set_err("vloam_%s_enable: hipMalloc of %zu MB failed", R::name, row_bytes >> 20); return VLOAM_ERR_HIP; }
  if (hipMalloc((void**)&P.scratch, R::scratch_bytes(h->se.B)) != hipSuccess) {
    (void)hipFree(P.rows); set_err("vloam_%s_enable: hipMalloc failed", R::name); return VLOAM_ERR_HIP;
  }
  R::dev(h) = P;   // (vloam_destroy frees them, whatever the rest reaches)
  HIPCHK(R::init(h));
  HIPCHK(hipStreamSynchronize(h->stream));   // the stage streams do not wait for this one
  R::on(h) = true;
  return VLOAM_OK;
}

extern "C" {

// ------------------------------------------------------------------ per-sweep diagnostics log (vloam_limits_ext::sweep_log)
vloam_status vloam_get_sweep_log(vloam_handle* h, int first, int count, vloam_sweep_record* out) { return get_rows<SweepLogRows>(h, "vloam_get_sweep_log", first, count, out); }
vloam_status vloam_sweep_log_device_ptr(vloam_handle* h, void** d_rows, long long* bytes) { return rows_device_ptr<SweepLogRows>(h, d_rows, bytes); }

// ------------------------------------------------------------------ per-sweep pose information matrices (vloam_pose_info_enable)
void vloam_default_pose_info_options(vloam_pose_info_options* opt) {
  if (!opt) return;
  opt->struct_size = (int)sizeof(vloam_pose_info_options);
  opt->reserved = 0;
  opt->lo_min_eigenvalue = 0.0;
  opt->map_min_eigenvalue = 0.0;
}
vloam_status vloam_pose_info_enable(vloam_handle* h, const vloam_pose_info_options* opt) { return enable_rows<PoseInfoRows>(h, opt); }
vloam_status vloam_get_pose_info(vloam_handle* h, int first, int count, vloam_pose_info_record* out) { return get_rows<PoseInfoRows>(h, "vloam_get_pose_info", first, count, out); }
vloam_status vloam_pose_info_device_ptr(vloam_handle* h, void** d_rows, long long* bytes) { return rows_device_ptr<PoseInfoRows>(h, d_rows, bytes); }

// ------------------------------------------------------------------ per-sweep pose covariance rows (vloam_pose_cov_enable), an add-on of the above
void vloam_default_pose_cov_options(vloam_pose_cov_options* opt) {
  if (!opt) return;
  opt->struct_size = (int)sizeof(vloam_pose_cov_options);
  opt->reserved = 0;
  opt->lo_min_eigenvalue = 0.0;
  opt->map_min_eigenvalue = 0.0;
  opt->vo_min_eigenvalue = 0.0;
}
vloam_status vloam_pose_cov_enable(vloam_handle* h, const vloam_pose_cov_options* opt) { return enable_rows<PoseCovRows>(h, opt); }
vloam_status vloam_get_pose_cov(vloam_handle* h, int first, int count, vloam_pose_cov_record* out) { return get_rows<PoseCovRows>(h, "vloam_get_pose_cov", first, count, out); }
vloam_status vloam_pose_cov_device_ptr(vloam_handle* h, void** d_rows, long long* bytes) { return rows_device_ptr<PoseCovRows>(h, d_rows, bytes); }

}  // extern "C"
