// Coupled VLOAM frames, the image front-end with its getters, and the stand-alone VO calls of libvloam_hip.so.
#include "handle.h"

static vloam_status require_image_front_end(const vloam_handle* h) {
  if (h->img.max_w == 0) { set_err("the handle was created without an image front-end (cfg.image_width / image_height)"); return VLOAM_ERR_ORDER; }
  return VLOAM_OK;
}
// a host image, before it is uploaded
static vloam_status check_host_image(const vloam_handle* h, int width, int height, int stride) {
  TRY(require_image_front_end(h));
  if (width <= 0 || height <= 0 || stride < width || width > h->img.max_w || height > h->img.max_h) {
    set_err("bad image size (%d x %d; the handle was created for at most %d x %d)", width, height, h->img.max_w, h->img.max_h);
    return VLOAM_ERR_INVALID;
  }
  return VLOAM_OK;
}
// what img_check / img_process refused (img_kernels.h)
static void set_image_size_err(const vloam_handle* h, int width, int height, int stride) {
  set_err("image front-end: bad image size (%d x %d, stride %d; capacity %d x %d, one size per sequence)", width, height, stride, h->img.max_w, h->img.max_h);
}

extern "C" {

// ------------------------------------------------------------------ coupled VLOAM frame (configs[3])
// == vloam_tf->processStaticTransform()'s products base_T_cam0 / velo_T_cam0 (vloam_tf.cpp:55-56), row-major 4x4
vloam_status vloam_set_extrinsics(vloam_handle* h, const double base_T_cam0[16], const double velo_T_cam0[16]) {
  if (!h || !base_T_cam0 || !velo_T_cam0) return VLOAM_ERR_INVALID;
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  for (int b = 0; b < h->se.B; b++) {   // one sensor rig for all sessions of a batched handle
    LOState* lo = (LOState*)((char*)h->lo + (size_t)b * h->se.ss);
    VloamTfState tf;
    HIPCHK(hipMemcpy(&tf, &lo->tf, sizeof(tf), hipMemcpyDeviceToHost));
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) { tf.base_T_cam0.m[r * 3 + c] = base_T_cam0[r * 4 + c]; tf.velo_T_cam0.m[r * 3 + c] = velo_T_cam0[r * 4 + c]; }
      tf.base_T_cam0.o[r] = base_T_cam0[r * 4 + 3]; tf.velo_T_cam0.o[r] = velo_T_cam0[r * 4 + 3];
    }
    tf.coupled = 1;
    HIPCHK(hipMemcpy(&lo->tf, &tf, sizeof(tf), hipMemcpyHostToDevice));
  }
  h->have_extrinsics = true;
  return VLOAM_OK;
}

// One callback() of MAIN/src/vloam_main_node.cpp:125-180 without a host round trip: VO->reset / LOAM->reset, processPointCloud (depth map
// from the SAME device-resident sweep scan registration reads), solveNlsAll for count > 0 (initial guess = the previous frame's
// cam0_curr_LOT_cam0_prev, on the device), VO2VeloAndBase (-> velo_last_VOT_velo_curr, read by solveLO when detach_VO_LO == 0),
// scanRegistrationIO, laserOdometryIO (publish() refreshes cam0_curr_LOT_cam0_prev), laserMappingIO.
// prev_uv / curr_uv: n_match integer pixel pairs in HOST memory (previous frame -> this frame; ignored for the first frame).
// Host image -> the device staging buffer, on the image stream.  hipMemcpyAsync from pageable memory has taken its copy of the source when
// it returns; hipMemcpy2DAsync has NOT (measured: tools/microbench/pageable_async_copy.py) — so a padded image is packed on the host
// first, and the caller may reuse its buffer as soon as the call is back either way.
static vloam_status upload_image(vloam_handle* h, const unsigned char* gray, int width, int height, int stride, int session = 0) {
  const unsigned char* src = gray;
  if (stride != width) {
    h->img_pack.resize((size_t)width * height);
    for (int y = 0; y < height; y++) memcpy(h->img_pack.data() + (size_t)y * width, gray + (size_t)y * stride, (size_t)width);
    src = h->img_pack.data();
  }
  HIPCHK(hipMemcpyAsync(h->img.staging + (size_t)session * h->se.ss, src, (size_t)width * height, hipMemcpyHostToDevice, h->s_img));
  return VLOAM_OK;
}

// One coupled frame of every session.  n_match == null: an image frame (d_gray: one device image per session), whose matches come from the
// image front-end; otherwise n_match[b] pixel pairs prev_uv[b] -> curr_uv[b] in host memory.
static vloam_status process_frame_common(vloam_handle* h, const void* const* d_xyz_pad4, const int* n, const int* const* prev_uv, const int* const* curr_uv,
                                         const int* n_match, const void* const* d_gray, int width, int height, int stride) {
  if (!h->vo.have_calib || !h->have_extrinsics) { set_err("vloam_process_frame needs vloam_vo_set_calib and vloam_set_extrinsics first"); return VLOAM_ERR_ORDER; }
  h->vo_used = true;
  const int* const no_uv[kMaxBatch] = {};
  const int no_match[kMaxBatch] = {};
  if (!n_match) { prev_uv = curr_uv = no_uv; n_match = no_match; }
  for (int b = 0; b < h->se.B; b++) {
    if (n_match[b] < 0 || (n_match[b] > 0 && (!prev_uv[b] || !curr_uv[b]))) { set_err("bad match arrays for session %d", b); return VLOAM_ERR_INVALID; }
    if (n_match[b] > kVoMaxMatches) { set_err("%d matches exceed the capacity of %d", n_match[b], kVoMaxMatches); return VLOAM_ERR_CAPACITY; }
  }
  if (d_gray) {   // before anything of this frame is enqueued
    for (int b = 0; b < h->se.B; b++) if (!d_gray[b]) { set_err("null image pointer for session %d", b); return VLOAM_ERR_INVALID; }
    TRY(require_image_front_end(h));
    if (img_check(&h->img, width, height, stride) != VLOAM_OK) { set_image_size_err(h, width, height, stride); return VLOAM_ERR_INVALID; }
  }
  TRY(begin_sweep(h));
  const BatchIn bi = batch_in(h, d_xyz_pad4, n);
  vloam_status s = enqueue_sr(h, bi);
  if (s != VLOAM_OK) return s;
  const int k = h->frame, cur = set_of(k);
  // depth map + matches ride on the scan-registration stream (they only need the sweep); the solve itself belongs to the odometry stream
  s = vo_depth_enqueue(&h->vo, h->stream, bi, k, prev_uv, curr_uv, d_gray ? no_match : n_match, &h->prof);
  if (s != VLOAM_OK) { set_err("vo_depth_enqueue failed"); return s; }
  HIPCHK(hipEventRecord(h->ev_vo[cur], h->stream));
  h->vo_frame[cur] = true;
  if (d_gray) {
    // processImage on its own stream: corners + flow straight into this frame's match arrays (one entry per corner slot, untracked
    // slots marked), consumed by the VO solve in front of this frame's laser odometry
    // (a batched handle runs its sessions' images one after the other on that stream: each session has the image buffers of its own arena)
    const int vset = k % VOContext::kSets;
    ImgContext after = h->img;
    for (int b = 0; b < h->se.B; b++) {
      const size_t so = (size_t)b * h->se.ss;
      ImgContext cb = h->img.rebased(so);
      s = img_process(&cb, h->s_img, (const unsigned char*)d_gray[b], width, height, stride, (int*)((char*)h->vo.d_prev_set[vset] + so), (int*)((char*)h->vo.d_curr_set[vset] + so), &h->prof);
      if (s != VLOAM_OK) { set_image_size_err(h, width, height, stride); return s; }
      h->vo.n_match_set[vset].n[b] = k > 0 ? kImgMaxCorners : 0;
      after = cb;
    }
    h->img.adopt_host_state(after);
    HIPCHK(hipEventRecord(h->ev_img[cur], h->s_img));
    h->img_frame[cur] = true;
  }
  return end_sweep(h);
}

vloam_status vloam_process_frame_device(vloam_handle* h, const void* d_xyz_pad4, int n, const int* prev_uv, const int* curr_uv, int n_match) {
  if (!h || !d_xyz_pad4 || n_match < 0 || (n_match > 0 && (!prev_uv || !curr_uv))) return VLOAM_ERR_INVALID;
  SINGLE_SESSION_ONLY(h);
  return process_frame_common(h, &d_xyz_pad4, &n, &prev_uv, &curr_uv, &n_match, nullptr, 0, 0, 0);
}

// Batched coupled frames: one call advances ALL sessions of the handle by one VLOAM frame (session b: sweep d_xyz_pad4[b] with n[b] points,
// n_match[b] pixel matches prev_uv[b] -> curr_uv[b] in HOST memory); every kernel of the frame chain — depth map, match + VO solve,
// VO2VeloAndBase, scan registration, odometry in combined mode, mapping — is launched once with the session index in blockIdx.z.
vloam_status vloam_batch_process_frame_device(vloam_handle* h, const void* const* d_xyz_pad4, const int* n, const int* const* prev_uv,
                                              const int* const* curr_uv, const int* n_match) {
  if (!h || !d_xyz_pad4 || !n || !prev_uv || !curr_uv || !n_match) return VLOAM_ERR_INVALID;
  return process_frame_common(h, d_xyz_pad4, n, prev_uv, curr_uv, n_match, nullptr, 0, 0, 0);
}

vloam_status vloam_batch_process_frame(vloam_handle* h, const float* const* xyz_pad4, const int* n, const int* const* prev_uv,
                                       const int* const* curr_uv, const int* n_match) {
  if (!h || !xyz_pad4 || !n || !prev_uv || !curr_uv || !n_match) return VLOAM_ERR_INVALID;
  TRY(check_host_sweeps(h, xyz_pad4, n));
  HIPCHK(hipSetDevice(h->device));
  const void* d[kMaxBatch];
  for (int b = 0; b < h->se.B; b++) TRY(stage_inline(h, b, xyz_pad4[b], n[b], &d[b]));
  return vloam_batch_process_frame_device(h, d, n, prev_uv, curr_uv, n_match);
}

vloam_status vloam_process_frame(vloam_handle* h, const float* xyz_pad4, int n, const int* prev_uv, const int* curr_uv, int n_match) {
  if (!h || !xyz_pad4 || n_match < 0 || (n_match > 0 && (!prev_uv || !curr_uv))) return VLOAM_ERR_INVALID;
  SINGLE_SESSION_ONLY(h);
  return vloam_batch_process_frame(h, &xyz_pad4, &n, &prev_uv, &curr_uv, &n_match);
}

vloam_status vloam_process_frame_image_device(vloam_handle* h, const void* d_xyz_pad4, int n, const void* d_gray, int width, int height, int stride) {
  if (!h || !d_xyz_pad4 || !d_gray) return VLOAM_ERR_INVALID;
  SINGLE_SESSION_ONLY(h);
  return process_frame_common(h, &d_xyz_pad4, &n, nullptr, nullptr, nullptr, &d_gray, width, height, stride);
}

// Batched coupled frames from raw inputs: session b gets sweep d_xyz_pad4[b] and the 8-bit grey image d_gray[b] (all images of one size).
vloam_status vloam_batch_process_frame_image_device(vloam_handle* h, const void* const* d_xyz_pad4, const int* n, const void* const* d_gray, int width, int height,
                                                    int stride) {
  if (!h || !d_xyz_pad4 || !n || !d_gray) return VLOAM_ERR_INVALID;
  return process_frame_common(h, d_xyz_pad4, n, nullptr, nullptr, nullptr, d_gray, width, height, stride);
}

vloam_status vloam_batch_process_frame_image(vloam_handle* h, const float* const* xyz_pad4, const int* n, const unsigned char* const* gray, int width, int height,
                                             int stride) {
  if (!h || !xyz_pad4 || !n || !gray) return VLOAM_ERR_INVALID;
  for (int b = 0; b < h->se.B; b++) if (!gray[b]) return VLOAM_ERR_INVALID;
  TRY(check_host_sweeps(h, xyz_pad4, n));   // before anything is enqueued: a refusal has no side effects (c_api.h)
  TRY(check_host_image(h, width, height, stride));
  HIPCHK(hipSetDevice(h->device));
  const void* d[kMaxBatch];
  const void* d_img[kMaxBatch];
  for (int b = 0; b < h->se.B; b++) {
    TRY(stage_inline(h, b, xyz_pad4[b], n[b], &d[b]));
    TRY(upload_image(h, gray[b], width, height, stride, b));
    d_img[b] = h->img.staging + (size_t)b * h->se.ss;
  }
  return vloam_batch_process_frame_image_device(h, d, n, d_img, width, height, width);
}

vloam_status vloam_process_frame_image(vloam_handle* h, const float* xyz_pad4, int n, const unsigned char* gray, int width, int height, int stride) {
  if (!h || !xyz_pad4 || !gray) return VLOAM_ERR_INVALID;
  SINGLE_SESSION_ONLY(h);
  return vloam_batch_process_frame_image(h, &xyz_pad4, &n, &gray, width, height, stride);
}

// ---- the image front-end on its own (VisualOdometry::processImage, optical_flow_match = true)
vloam_status vloam_vo_process_image_device(vloam_handle* h, const void* d_gray, int width, int height, int stride) {
  if (!h || !d_gray) return VLOAM_ERR_INVALID;
  h->vo_used = true;
  SINGLE_SESSION_ONLY(h);
  TRY(require_image_front_end(h));
  HIPCHK(hipSetDevice(h->device));
  // (no match outputs here: vloam_vo_solve uploads host matches into d_prev / d_curr on another stream; nothing consumes device-side matches in standalone mode)
  const vloam_status s = img_process(&h->img, h->s_img, (const unsigned char*)d_gray, width, height, stride, nullptr, nullptr, &h->prof);
  if (s != VLOAM_OK) set_image_size_err(h, width, height, stride);
  return s;
}

vloam_status vloam_vo_process_image(vloam_handle* h, const unsigned char* gray, int width, int height, int stride) {
  if (!h || !gray) return VLOAM_ERR_INVALID;
  h->vo_used = true;
  TRY(check_host_image(h, width, height, stride));
  HIPCHK(hipSetDevice(h->device));
  TRY(upload_image(h, gray, width, height, stride));
  return vloam_vo_process_image_device(h, h->img.staging, width, height, width);
}

// ImageUtil::matchDescriptors (image_util.cpp:221-296) for binary descriptors: BFMatcher(NORM_HAMMING), knnMatch k = 2 + ratio 0.8 (select_knn != 0,
// the reference's SelectType::KNN) or match with crossCheck (select_knn == 0, SelectType::NN).  Descriptors in host memory, n x bytes_per_desc.
vloam_status vloam_vo_match_descriptors(vloam_handle* h, const unsigned char* desc_prev, int n_prev, const unsigned char* desc_curr, int n_curr, int bytes_per_desc,
                                        int select_knn, int* query_idx, int* train_idx, int cap, int* n_matches) {
  if (!h || !n_matches || cap < 0 || (n_prev > 0 && !desc_prev) || (n_curr > 0 && !desc_curr) || (cap > 0 && (!query_idx || !train_idx))) return VLOAM_ERR_INVALID;
  h->vo_used = true;
  SINGLE_SESSION_ONLY(h);
  TRY(require_image_front_end(h));
  HIPCHK(hipSetDevice(h->device));
  vloam_status s = img_match_descriptors(&h->img, h->s_img, desc_prev, n_prev, desc_curr, n_curr, bytes_per_desc, select_knn != 0, query_idx, train_idx, cap, n_matches);
  if (s == VLOAM_ERR_CAPACITY) set_err("more than %d descriptors", kImgMaxDesc);
  if (s == VLOAM_ERR_INVALID) set_err("bytes_per_desc must be a multiple of 4 up to %d", kImgMaxDescBytes);
  return s;
}

static vloam_status img_results(vloam_handle* h, std::vector<float2>* corners, std::vector<float2>* tracked, std::vector<unsigned char>* status, int* n_corners,
                                bool* have_flow) {
  if (h->img.max_w == 0 || h->img.count < 0) { set_err("no image processed yet"); return VLOAM_ERR_ORDER; }
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  const ImgContext img = h->img.rebased((size_t)h->sel * h->se.ss);   // the session vloam_select_session chose
  int ierr = 0;
  HIPCHK(hipMemcpy(&ierr, img.error, sizeof(int), hipMemcpyDeviceToHost));
  if (ierr) { set_err("image front-end capacity exceeded (bits %d: 1 candidates > %d, 2 neighbours > %d, 4 corners > %d)", ierr, kImgCandCap, kImgNbrCap, kImgAccCap); return VLOAM_ERR_CAPACITY; }
  const int cur = h->img.count % 2;
  HIPCHK(hipMemcpy(n_corners, img.n_corners[cur], sizeof(int), hipMemcpyDeviceToHost));
  corners->resize((size_t)*n_corners + 1);
  if (*n_corners) HIPCHK(hipMemcpy(corners->data(), img.corners[cur], sizeof(float2) * (size_t)*n_corners, hipMemcpyDeviceToHost));
  *have_flow = h->img.count > 0 && !h->img.orb;   // ORB + brute-force tracks nothing: matches come from vloam_vo_get_flow_matches
  if (tracked && *have_flow && *n_corners) {
    tracked->resize((size_t)*n_corners); status->resize((size_t)*n_corners);
    HIPCHK(hipMemcpy(tracked->data(), img.tracked, sizeof(float2) * (size_t)*n_corners, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(status->data(), img.status, (size_t)*n_corners, hipMemcpyDeviceToHost));
  }
  return VLOAM_OK;
}

vloam_status vloam_vo_get_keypoints(vloam_handle* h, float* xy, int cap, int* n) {
  if (!h || !n || cap < 0 || (cap > 0 && !xy)) return VLOAM_ERR_INVALID;
  std::vector<float2> c;
  int nc = 0;
  bool flow = false;
  TRY(img_results(h, &c, nullptr, nullptr, &nc, &flow));
  *n = nc;
  for (int k = 0; k < nc && k < cap; k++) { xy[2 * k] = c[(size_t)k].x; xy[2 * k + 1] = c[(size_t)k].y; }
  return VLOAM_OK;
}

vloam_status vloam_vo_get_flow(vloam_handle* h, float* prev_xy, float* curr_xy, unsigned char* status, int cap, int* n) {
  if (!h || !n || cap < 0 || (cap > 0 && (!prev_xy || !curr_xy || !status))) return VLOAM_ERR_INVALID;
  std::vector<float2> c, t;
  std::vector<unsigned char> st;
  int nc = 0;
  bool flow = false;
  TRY(img_results(h, &c, &t, &st, &nc, &flow));
  *n = flow ? nc : 0;
  for (int k = 0; k < *n && k < cap; k++) {
    prev_xy[2 * k] = c[(size_t)k].x; prev_xy[2 * k + 1] = c[(size_t)k].y;
    curr_xy[2 * k] = t[(size_t)k].x; curr_xy[2 * k + 1] = t[(size_t)k].y;
    status[k] = st[(size_t)k];
  }
  return VLOAM_OK;
}

// ORB + brute-force configuration: the keypoints that survive ORB's border filter (what match indices refer to) and their descriptors
static vloam_status orb_results(vloam_handle* h, int which /* 0: the latest image, 1: the one before */, std::vector<float2>* kp, std::vector<unsigned char>* desc) {
  if (h->img.max_w == 0 || h->img.count < 0) { set_err("no image processed yet"); return VLOAM_ERR_ORDER; }
  if (!h->img.orb) { set_err("the handle runs the optical-flow configuration (no ORB pattern set: vloam_vo_set_orb_pattern)"); return VLOAM_ERR_ORDER; }
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  const ImgContext img = h->img.rebased((size_t)h->sel * h->se.ss);
  const int slot = (h->img.count + (which ? 1 : 0)) % 2;
  int n = 0;
  if (!(which && h->img.count == 0)) HIPCHK(hipMemcpy(&n, img.n_okp[slot], sizeof(int), hipMemcpyDeviceToHost));
  kp->resize((size_t)n);
  if (n) HIPCHK(hipMemcpy(kp->data(), img.okp[slot], sizeof(float2) * (size_t)n, hipMemcpyDeviceToHost));
  if (desc) {
    std::vector<unsigned> rows((size_t)n * (kImgMaxDescBytes / 4));
    if (n) HIPCHK(hipMemcpy(rows.data(), img.desc[slot], rows.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    desc->resize((size_t)n * 32);
    for (int k = 0; k < n; k++) memcpy(desc->data() + (size_t)k * 32, rows.data() + (size_t)k * (kImgMaxDescBytes / 4), 32);
  }
  return VLOAM_OK;
}

vloam_status vloam_vo_set_orb_pattern(vloam_handle* h, const signed char* pattern_256x4) {
  if (!h) return VLOAM_ERR_INVALID;
  TRY(require_image_front_end(h));
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  if (h->img.count >= 0 && (pattern_256x4 != nullptr) != h->img.orb) { set_err("the image configuration cannot change in the middle of a sequence"); return VLOAM_ERR_ORDER; }
  const vloam_status s = img_set_orb_pattern(&h->img, h->stream, pattern_256x4, h->se.B, h->se.ss);
  if (s == VLOAM_ERR_INVALID) set_err("ORB pattern: a steered offset leaves the 31-pixel border the keypoints keep (|x|, |y| <= 30)");
  return s;
}

vloam_status vloam_vo_get_descriptors(vloam_handle* h, float* xy, unsigned char* desc32, int cap, int* n) {
  if (!h || !n || cap < 0) return VLOAM_ERR_INVALID;
  std::vector<float2> kp;
  std::vector<unsigned char> d;
  TRY(orb_results(h, 0, &kp, &d));
  *n = (int)kp.size();
  const int m = *n < cap ? *n : cap;
  for (int k = 0; xy && k < m; k++) { xy[2 * k] = kp[(size_t)k].x; xy[2 * k + 1] = kp[(size_t)k].y; }
  if (desc32 && m > 0) memcpy(desc32, d.data(), (size_t)m * 32);
  return VLOAM_OK;
}

vloam_status vloam_vo_get_flow_matches(vloam_handle* h, int* prev_uv, int* curr_uv, int cap, int* n) {
  if (!h || !n || cap < 0 || (cap > 0 && (!prev_uv || !curr_uv))) return VLOAM_ERR_INVALID;
  if (h->img.max_w != 0 && h->img.orb) {
    // ORB + brute force: matchDescriptors(previous, latest) + the match loop's reads (visual_odometry.cpp:113-116,296-303), from what the device left
    std::vector<float2> kc, kp;
    vloam_status s = orb_results(h, 0, &kc, nullptr);
    if (s == VLOAM_OK) s = orb_results(h, 1, &kp, nullptr);
    if (s != VLOAM_OK) return s;
    *n = 0;
    if (h->img.count == 0 || kp.empty() || kc.size() < 2) return VLOAM_OK;
    const ImgContext img = h->img.rebased((size_t)h->sel * h->se.ss);
    std::vector<uint2> best(kp.size());
    HIPCHK(hipMemcpy(best.data(), img.best2[0], sizeof(uint2) * best.size(), hipMemcpyDeviceToHost));
    int m = 0;
    for (size_t q = 0; q < kp.size(); q++) {
      const uint2 b = best[q];
      if (b.y == 0xffffffffu || !((double)(float)(b.x >> 16) < 0.8 * (double)(float)(b.y >> 16))) continue;
      const float2 a = kp[q], c = kc[(size_t)(b.x & 0xffffu)];
      if (m < cap) { prev_uv[2 * m] = (int)a.x; prev_uv[2 * m + 1] = (int)a.y; curr_uv[2 * m] = (int)c.x; curr_uv[2 * m + 1] = (int)c.y; }
      m++;
    }
    *n = m;
    return VLOAM_OK;
  }
  std::vector<float2> c, t;
  std::vector<unsigned char> st;
  int nc = 0, m = 0;
  bool flow = false;
  TRY(img_results(h, &c, &t, &st, &nc, &flow));
  for (int k = 0; flow && k < nc; k++) {
    if (st[(size_t)k] != 1) continue;   // visual_odometry.cpp:298-308
    if (m < cap) {
      prev_uv[2 * m] = (int)c[(size_t)k].x; prev_uv[2 * m + 1] = (int)c[(size_t)k].y;
      curr_uv[2 * m] = (int)t[(size_t)k].x; curr_uv[2 * m + 1] = (int)t[(size_t)k].y;
    }
    m++;
  }
  *n = m;
  return VLOAM_OK;
}

// world_VOT_base_last of frames first..first+count-1 as {q xyzw, t} (what VO2Cam0StartFrame turns into VO rows, vloam_tf.cpp:77-101)
vloam_status vloam_get_vo_trajectory(vloam_handle* h, int first, int count, double* poses7) {
  if (!h || !poses7 || first < 0 || count < 0 || first + count > handed_over(h)) return VLOAM_ERR_INVALID;   // (a host sweep in flight is enqueued by the sync below)
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  if (count) HIPCHK(hipMemcpy(poses7, SEL(h, h->vo_traj) + (size_t)first * 7, sizeof(double) * 7 * (size_t)count, hipMemcpyDeviceToHost));
  return VLOAM_OK;
}

// the last frame's VO estimate (angles_0to1, t_0to1), its counter32 / counter22 and the LiDAR-odometry prior derived from it
vloam_status vloam_get_vo_result(vloam_handle* h, double angle_axis[3], double t[3], int counters32_22[2], double prior_q[4], double prior_t[3]) {
  if (!h) return VLOAM_ERR_INVALID;
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  double x[6];
  int cnt[2];
  LOState lo;
  HIPCHK(hipMemcpy(x, SEL(h, h->vo.x), sizeof(x), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(cnt, SEL(h, h->vo.counters), sizeof(cnt), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&lo, SEL(h, h->lo), sizeof(lo), hipMemcpyDeviceToHost));
  for (int k = 0; k < 3; k++) { if (angle_axis) angle_axis[k] = x[k]; if (t) t[k] = x[3 + k]; if (prior_t) prior_t[k] = lo.prior_t[k]; }
  if (counters32_22) { counters32_22[0] = cnt[0]; counters32_22[1] = cnt[1]; }
  if (prior_q) for (int k = 0; k < 4; k++) prior_q[k] = lo.prior_q[k];
  return VLOAM_OK;
}

// ------------------------------------------------------------------ VO
vloam_status vloam_vo_set_calib(vloam_handle* h, const vloam_calib* c) {
  if (!h || !c) return VLOAM_ERR_INVALID;
  HIPCHK(hipSetDevice(h->device));
  return vo_set_calib(&h->vo, h->stream, c) == VLOAM_OK ? VLOAM_OK : VLOAM_ERR_HIP;
}
vloam_status vloam_vo_process_point_cloud(vloam_handle* h, const float* xyz_pad4, int n) {
  if (!h || !xyz_pad4 || n <= 0) return VLOAM_ERR_INVALID;
  h->vo_used = true;
  SINGLE_SESSION_ONLY(h);
  if (n > h->cfg.max_points) return VLOAM_ERR_CAPACITY;
  HIPCHK(hipSetDevice(h->device));
  const void* d = nullptr;
  TRY(stage_inline(h, 0, xyz_pad4, n, &d));
  return vo_process_point_cloud(&h->vo, h->stream, (const float4*)d, n) == VLOAM_OK ? VLOAM_OK : VLOAM_ERR_HIP;
}
vloam_status vloam_vo_solve(vloam_handle* h, const int* prev_uv, const int* curr_uv, int n_match, double aa[3], double t[3], int counters[2]) {
  if (!h || !prev_uv || !curr_uv || !aa || !t || n_match < 0) return VLOAM_ERR_INVALID;
  h->vo_used = true;
  SINGLE_SESSION_ONLY(h);
  HIPCHK(hipSetDevice(h->device));
  vloam_status s = vo_solve(&h->vo, h->cfg, h->stream, prev_uv, curr_uv, n_match, aa, t, counters);
  if (s != VLOAM_OK) set_err("vo_solve failed: %s", hipGetErrorString(hipGetLastError()));
  return s;
}

}  // extern "C"
