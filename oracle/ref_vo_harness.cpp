// REFERENCE HARNESS — TEST INFRASTRUCTURE ONLY (our own text).
//
// A plain-C entry to the REFERENCE'S OWN vloam::VisualOdometry and its two vloam::PointCloudUtil objects (src/visual_odometry/src/
// visual_odometry.cpp, point_cloud_util.cpp — translation units of their own, compiled unmodified from the tree the make variable REF_DIR
// names), driven as the node drives them per frame: reset(); processPointCloud() (which fills point_cloud_3d_tilde from the sweep, hands
// it to point_cloud_utils[i] and calls projectPointCloud() and downsamplePointCloud()); from the second frame on solveNlsAll().
//
// What the harness sets instead of the ROS plumbing: the parameters (the stand-in parameter server, read by init()); the calibration
// matrices of both PointCloudUtil objects (setUpPointCloud copies them out of a CameraInfo message and two Eigen::Isometry3f, which are
// not restated); the public match containers — keypoints / matches (ORB configuration) or keypoints_2f / optical_flow_status
// (optical-flow configuration) —, which the OpenCV front-end (image_util.cpp, NOT built, not pinned) would fill; and
// vloam_tf->cam0_curr_LOT_cam0_prev, the prior solveNlsAll reads when reset_VO_to_identity is false.
//
// Everything is observed from outside: the public matrices of the PointCloudUtil objects, queryDepth itself, and — through the stand-in
// ceres::Problem's report of every AddResidualBlock — the functor's observations together with what the reference holds in its public
// members at that moment: depth0, point_3d_image0_0, point_3d_image0_1.  The loop's counters are locals that only reach ROS_INFO, so
// the counters returned here are the numbers of CostFunctor32 / CostFunctor22 blocks.  Which input match a block belongs to is found by
// walking both lists in order: a block belongs to the next match whose pixel pair, converted float -> int as C++ converts it, reproduces
// the block's point_3d_image0_0 / _1 exactly; the matches walked past were skipped by the reference.  A block that fits no match, or
// a match count that does not add up, is an error (-2): the harness never guesses.
//
// The ImageUtil member functions at the bottom are definitions of our own that abort: visual_odometry.cpp refers to them from
// processImage() / publish(), which are never called here, and the library has to load.
#include <visual_odometry/visual_odometry.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

namespace {

struct BlockRec {
  int kind;        // 32 / 22
  float depth0;
  float img0[3], img1[3];
  double obs[5];
};

struct Row {
  int kind;        // 32 / 22; 0: skipped by the outlier gate; -1: not a match (optical_flow_status != 1)
  float depth0;
  double obs[5];
  int uv[4];       // prev x, y, curr x, y as the reference's ints
};

struct Session {
  std::shared_ptr<vloam::VloamTF> tf;
  std::unique_ptr<vloam::VisualOdometry> vo;
  bool optical_flow = false;
  std::vector<BlockRec> blocks;
  std::vector<Row> rows;
  std::vector<double> before, after;   // the six parameters at ceres::Solve, when the problem had blocks
  double out[6] = {0, 0, 0, 0, 0, 0};
};

Session* g_observed = nullptr;

void on_add(const ceres::CostFunction* cf) {
  if (!g_observed) return;
  const vloam::VisualOdometry& vo = *g_observed->vo;
  BlockRec b;
  std::memset(&b, 0, sizeof b);
  if (auto* f = dynamic_cast<const ceres::AutoDiffCostFunction<vloam::CostFunctor32, 2, 3, 3>*>(cf)) {
    b.kind = 32;
    b.obs[0] = f->functor().observed_x0; b.obs[1] = f->functor().observed_y0; b.obs[2] = f->functor().observed_z0;
    b.obs[3] = f->functor().observed_x1_bar; b.obs[4] = f->functor().observed_y1_bar;
  } else if (auto* g = dynamic_cast<const ceres::AutoDiffCostFunction<vloam::CostFunctor22, 1, 3, 3>*>(cf)) {
    b.kind = 22;
    b.obs[0] = g->functor().observed_x0_bar; b.obs[1] = g->functor().observed_y0_bar;
    b.obs[2] = g->functor().observed_x1_bar; b.obs[3] = g->functor().observed_y1_bar;
  } else {
    b.kind = -99;   // a functor solveNlsAll does not create in the reference's text as it stands
  }
  b.depth0 = vo.depth0;
  for (int k = 0; k < 3; k++) { b.img0[k] = vo.point_3d_image0_0(k); b.img1[k] = vo.point_3d_image0_1(k); }
  g_observed->blocks.push_back(b);
}

void on_solve(const ceres::refshim::SolveRecord& rec) {
  if (!g_observed) return;
  g_observed->before = rec.before;
  g_observed->after = rec.after;
}

const vloam::PointCloudUtil& pcu(Session* s, int which) { return s->vo->point_cloud_utils[(size_t)(which == 0 ? s->vo->i : 1 - s->vo->i)]; }

int copy_rows3(const Eigen::MatrixXf& m, float* out, int cap_rows) {
  const int n = m.rows();
  if (out) for (int r = 0; r < n && r < cap_rows; r++) for (int c = 0; c < 3; c++) out[3 * r + c] = m(r, c);
  return n;
}

}  // namespace

extern "C" {

void* ref_vo_create(const float* cam_T_velo16, const float* rect0_T_cam16, const float* P_rect0_12, int remove_VO_outlier, int reset_VO_to_identity,
                    int optical_flow_match) {
  std::map<std::string, double>& store = ros::param::shim_store();
  store["loam_verbose_level"] = 0;
  store["reset_VO_to_identity"] = reset_VO_to_identity;
  store["remove_VO_outlier"] = remove_VO_outlier;
  store["keypoint_NMS"] = 0;
  store["CLAHE"] = 0;
  store["visualize_optical_flow"] = 0;
  store["optical_flow_match"] = optical_flow_match;
  ceres::refshim::add_observer() = on_add;
  ceres::refshim::observer() = on_solve;
  Session* s = new Session;
  s->optical_flow = optical_flow_match != 0;
  s->tf = std::make_shared<vloam::VloamTF>();
  s->vo.reset(new vloam::VisualOdometry());
  s->vo->init(s->tf);
  for (vloam::PointCloudUtil& u : s->vo->point_cloud_utils) {
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { u.cam_T_velo(r, c) = cam_T_velo16[4 * r + c]; u.rect0_T_cam(r, c) = rect0_T_cam16[4 * r + c]; }
    for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) u.P_rect0(r, c) = P_rect0_12[4 * r + c];
  }
  return s;
}
void ref_vo_destroy(void* h) {
  if (g_observed == h) g_observed = nullptr;
  delete static_cast<Session*>(h);
}

// one frame's sweep: VisualOdometry::reset, then processPointCloud (no visualisation, nothing published)
void ref_vo_frame(void* h, const float* xyz_pad4, int n) {
  Session* s = static_cast<Session*>(h);
  pcl::PointCloud<pcl::PointXYZ> cloud;
  cloud.points.resize((size_t)n);
  for (int k = 0; k < n; k++) cloud.points[(size_t)k] = pcl::PointXYZ(xyz_pad4[4 * k], xyz_pad4[4 * k + 1], xyz_pad4[4 * k + 2]);
  cloud.width = (uint32_t)n;
  cloud.height = 1;
  s->vo->reset();
  s->vo->processPointCloud(sensor_msgs::PointCloud2ConstPtr(), cloud, false, false);
}

int ref_vo_count(void* h) { return static_cast<Session*>(h)->vo->count; }

// which: 0 the current frame's PointCloudUtil (point_cloud_utils[i]), 1 the previous frame's
int ref_vo_get_points2d(void* h, int which, float* uvd, int cap_rows) { return copy_rows3(pcu(static_cast<Session*>(h), which).point_cloud_2d, uvd, cap_rows); }
int ref_vo_get_dnsp(void* h, int which, float* uvd, int cap_rows) { return copy_rows3(pcu(static_cast<Session*>(h), which).point_cloud_2d_dnsp, uvd, cap_rows); }
// the four bucket matrices, flattened index_x * new_height + index_y; dims = (new_width, new_height); returns their product
int ref_vo_get_buckets(void* h, int which, float* bx, float* by, float* bd, int* bc, int cap, int* dims) {
  const vloam::PointCloudUtil& u = pcu(static_cast<Session*>(h), which);
  const int w = u.bucket_x.rows(), hh = u.bucket_x.cols();
  if (dims) { dims[0] = w; dims[1] = hh; }
  for (int x = 0; x < w; x++)
    for (int y = 0; y < hh; y++) {
      const int k = x * hh + y;
      if (k >= cap) continue;
      bx[k] = u.bucket_x(x, y); by[k] = u.bucket_y(x, y); bd[k] = u.bucket_depth(x, y); bc[k] = u.bucket_count(x, y);
    }
  return w * hh;
}

// queryDepth(x, y) for n pixels.  tie[k] = 1 when the third and the fourth smallest neighbour distance of pixel k are equal: the
// reference's std::sort leaves their order open, so which three neighbours it averages is not defined by its text.  The distances are
// computed with the expression of point_cloud_util.cpp:329 over the neighbourhood of :319-324 (a restatement, used for this flag only).
void ref_vo_query_depth(void* h, int which, const float* xy, int n, float* depth, unsigned char* tie) {
  const vloam::PointCloudUtil& u = pcu(static_cast<Session*>(h), which);
  const int w = u.bucket_x.rows(), hh = u.bucket_x.cols();
  for (int k = 0; k < n; k++) {
    const float x = xy[2 * k], y = xy[2 * k + 1];
    depth[k] = u.queryDepth(x, y);
    if (!tie) continue;
    const int ix = static_cast<int>(x / u.downsample_grid_size), iy = static_cast<int>(y / u.downsample_grid_size);
    std::vector<float> d;
    for (int a = ix - 2; a <= ix + 2; a++)
      for (int b = iy - 2; b <= iy + 2; b++)
        if (a >= 0 && a < w && b >= 0 && b < hh && u.bucket_count(a, b) > 0) {
          const float dist = std::sqrt(std::pow(x - u.bucket_x(a, b), 2) + std::pow(y - u.bucket_y(a, b), 2));
          d.push_back(dist);
        }
    std::sort(d.begin(), d.end());
    tie[k] = (d.size() >= 10 && d[2] == d[3]) ? 1 : 0;
  }
}

// solveNlsAll on the current frame.  ORB configuration: kp_prev [n_prev, 2] / kp_curr [n_curr, 2] fill keypoints[1 - i] / keypoints[i],
// (query_idx, train_idx) [n_match] fill matches.  Optical-flow configuration: kp_prev / kp_curr [n_match, 2] fill keypoints_2f[1 - i] /
// keypoints_2f[i], status [n_match] fills optical_flow_status.  prior_q_xyzw / prior_t, when given, are stored in
// vloam_tf->cam0_curr_LOT_cam0_prev first.  0, or -2 when the blocks cannot be attributed to the matches (see the top of this file).
int ref_vo_solve(void* h, const float* kp_prev, int n_prev, const float* kp_curr, int n_curr, const int* query_idx, const int* train_idx,
                 const unsigned char* status, int n_match, const double* prior_q_xyzw, const double* prior_t) {
  Session* s = static_cast<Session*>(h);
  vloam::VisualOdometry& vo = *s->vo;
  const int i = vo.i;
  if (prior_q_xyzw && prior_t) {
    s->tf->cam0_curr_LOT_cam0_prev.setOrigin(tf2::Vector3(prior_t[0], prior_t[1], prior_t[2]));
    s->tf->cam0_curr_LOT_cam0_prev.setRotation(tf2::Quaternion(prior_q_xyzw[0], prior_q_xyzw[1], prior_q_xyzw[2], prior_q_xyzw[3]));
  }
  if (s->optical_flow) {
    vo.keypoints_2f[(size_t)(1 - i)].resize((size_t)n_match);
    vo.keypoints_2f[(size_t)i].resize((size_t)n_match);
    vo.optical_flow_status.resize((size_t)n_match);
    for (int k = 0; k < n_match; k++) {
      vo.keypoints_2f[(size_t)(1 - i)][(size_t)k] = cv::Point2f(kp_prev[2 * k], kp_prev[2 * k + 1]);
      vo.keypoints_2f[(size_t)i][(size_t)k] = cv::Point2f(kp_curr[2 * k], kp_curr[2 * k + 1]);
      vo.optical_flow_status[(size_t)k] = status[k];
    }
  } else {
    vo.keypoints[(size_t)(1 - i)].assign((size_t)n_prev, cv::KeyPoint());
    vo.keypoints[(size_t)i].assign((size_t)n_curr, cv::KeyPoint());
    for (int k = 0; k < n_prev; k++) vo.keypoints[(size_t)(1 - i)][(size_t)k].pt = cv::Point2f(kp_prev[2 * k], kp_prev[2 * k + 1]);
    for (int k = 0; k < n_curr; k++) vo.keypoints[(size_t)i][(size_t)k].pt = cv::Point2f(kp_curr[2 * k], kp_curr[2 * k + 1]);
    vo.matches.assign((size_t)n_match, cv::DMatch());
    for (int k = 0; k < n_match; k++) { vo.matches[(size_t)k].queryIdx = query_idx[k]; vo.matches[(size_t)k].trainIdx = train_idx[k]; }
  }
  s->blocks.clear();
  s->before.clear();
  s->after.clear();
  g_observed = s;
  vo.solveNlsAll();
  g_observed = nullptr;
  for (int k = 0; k < 3; k++) { s->out[k] = vo.angles_0to1[k]; s->out[3 + k] = vo.t_0to1[k]; }

  // attribute the blocks to the matches
  s->rows.assign((size_t)n_match, Row());
  size_t nb = 0;
  for (int k = 0; k < n_match; k++) {
    Row& r = s->rows[(size_t)k];
    std::memset(&r, 0, sizeof r);
    const float* a = s->optical_flow ? kp_prev + 2 * k : kp_prev + 2 * query_idx[k];
    const float* b = s->optical_flow ? kp_curr + 2 * k : kp_curr + 2 * train_idx[k];
    const int px = a[0], py = a[1], cx = b[0], cy = b[1];   // float -> int, as the assignments of visual_odometry.cpp:291-303
    r.uv[0] = px; r.uv[1] = py; r.uv[2] = cx; r.uv[3] = cy;
    if (s->optical_flow && status[k] != 1) { r.kind = -1; continue; }
    if (nb == s->blocks.size()) continue;   // kind 0
    const BlockRec& bl = s->blocks[nb];
    bool fits = bl.img1[0] == (float)cx && bl.img1[1] == (float)cy && bl.img1[2] == 1.0f;
    if (bl.kind == 32) fits = fits && bl.img0[0] == px * bl.depth0 && bl.img0[1] == py * bl.depth0 && bl.img0[2] == bl.depth0;
    else if (bl.kind == 22) fits = fits && bl.img0[0] == (float)px && bl.img0[1] == (float)py && bl.img0[2] == 1.0f;
    else return -2;
    if (!fits) continue;
    r.kind = bl.kind;
    r.depth0 = bl.depth0;
    std::memcpy(r.obs, bl.obs, sizeof r.obs);
    nb++;
  }
  return nb == s->blocks.size() ? 0 : -2;
}

// angles_0to1 / t_0to1 after the solve (out6) and as ceres::Solve found them (in6: what the reset or the prior had put there; for a
// problem without blocks, which Solve leaves alone, the same as out6); counters: CostFunctor32 blocks, CostFunctor22 blocks
void ref_vo_get_result(void* h, double* out6, double* in6, int* counters2) {
  Session* s = static_cast<Session*>(h);
  std::memcpy(out6, s->out, sizeof s->out);
  if (s->before.size() == 6) std::memcpy(in6, s->before.data(), 6 * sizeof(double));
  else std::memcpy(in6, s->out, sizeof s->out);
  counters2[0] = counters2[1] = 0;
  for (const BlockRec& b : s->blocks) counters2[b.kind == 32 ? 0 : 1]++;
}

// per input match 11 doubles: kind, depth0, obs[5], prev x, prev y, curr x, curr y
int ref_vo_get_match_rows(void* h, double* rows11, int cap) {
  Session* s = static_cast<Session*>(h);
  const int n = (int)s->rows.size();
  for (int k = 0; k < n && k < cap; k++) {
    const Row& r = s->rows[(size_t)k];
    double* d = rows11 + 11 * k;
    d[0] = r.kind; d[1] = r.depth0;
    for (int j = 0; j < 5; j++) d[2 + j] = r.obs[j];
    for (int j = 0; j < 4; j++) d[7 + j] = r.uv[j];
  }
  return n;
}

}  // extern "C"

// ---- image_util.cpp is not built: see the top of this file
namespace vloam {
std::vector<cv::KeyPoint> ImageUtil::detKeypoints(cv::Mat&) { std::abort(); }
cv::Mat ImageUtil::descKeypoints(std::vector<cv::KeyPoint>&, cv::Mat&) { std::abort(); }
std::vector<cv::DMatch> ImageUtil::matchDescriptors(cv::Mat&, cv::Mat&) { std::abort(); }
cv::Mat ImageUtil::visualizeMatches(const cv::Mat&, const cv::Mat&, const std::vector<cv::KeyPoint>&, const std::vector<cv::KeyPoint>&,
                                    const std::vector<cv::DMatch>&) { std::abort(); }
std::tuple<std::vector<cv::Point2f>, std::vector<cv::Point2f>, std::vector<uchar>> ImageUtil::calculateOpticalFlow(const cv::Mat&, const cv::Mat&,
                                                                                                                   const std::vector<cv::KeyPoint>&) { std::abort(); }
cv::Mat ImageUtil::visualizeOpticalFlow(const cv::Mat&, const std::vector<cv::Point2f>&, const std::vector<cv::Point2f>&, const std::vector<uchar>&) { std::abort(); }
cv::Mat ImageUtil::visualizeOpticalFlow(const cv::Mat&, const std::vector<cv::KeyPoint>&, const std::vector<cv::KeyPoint>&, const std::vector<cv::DMatch>&) {
  std::abort();
}
}  // namespace vloam
