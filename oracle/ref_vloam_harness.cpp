// REFERENCE HARNESS — TEST INFRASTRUCTURE ONLY (our own text).
//
// A plain-C entry to the REFERENCE'S OWN coupled frame loop: one vloam::VloamTF (src/vloam_tf/src/vloam_tf.cpp), one vloam::VisualOdometry
// (visual_odometry.cpp, point_cloud_util.cpp) and one vloam::LidarOdometryMapping (lidar_odometry_mapping.cpp, the façade, over
// scan_registration.cpp, laser_odometry.cpp, laser_mapping.cpp) — each a translation unit of its own, compiled unmodified from the tree the
// make variable REF_DIR names — sharing the one VloamTF as the node's init() wires them (vloam_main_node.cpp:116-122), so that the VO's
// result reaches the odometry through VO2VeloAndBase and the odometry's result reaches the next frame's VO through LaserOdometry::publish.
//
// The node's callback() (vloam_main_node.cpp:131-178) is RESTATED in ref_vloam_frame below, call for call: compiling vloam_main_node.cpp
// itself would need actionlib, rosbag, message_filters, boost::bind and generated action headers stubbed, and its callback() calls
// VO->processImage and VO->setUpPointCloud, i. e. OpenCV and a 4 x 4 f32 inverse, neither of which exists here.  What is left out of the
// restated callback: processImage (the harness fills the public match containers instead, as ref_vo_harness.cpp does), setUpPointCloud
// (cam_T_velo, rect0_T_cam, P_rect0 are set directly), the two sendTransform calls and VO->publish() (visualisation only; publish() is
// still called, the stand-in publishers keep the message).
//
// What the harness sets in place of ROS: the parameters (stand-in parameter server); the transforms tf2_ros::Buffer::lookupTransform
// returns (imu_link <- velo_link, imu_link <- camera_gray_left, base_link <- imu_link, and base_link <- velo_link, which the reference only
// re-broadcasts); the match containers keypoints[1 - i] / keypoints[i] / matches (ORB configuration, one keypoint pair per match).
//
// Observed from outside: every public tf2::Transform of VloamTF; the stand-in Problem's reports (AddResidualBlock and Solve), tagged with
// the stage that was running; the stand-in publishers' last messages; the rows the three *2Cam0StartFrame writers print into tmpfile()s.
// ONE thing is read through a door of our own: the façade keeps the hand-over clouds, q_wodom_curr / t_wodom_curr and skip_frame in private
// members, so this file — and only this file; lidar_odometry_mapping.cpp is compiled as it is — reads the class definition with `private`
// spelled `public` (after every other header has been read unchanged).  Access specifiers do not change the Itanium-ABI layout.
//
// The harness never lets the reference run into undefined behaviour; it returns a status and closes the session instead:
//   -1  no point survives the input filters (scan_registration.cpp would index an empty cloud);
//   -2  a kd-tree of the odometry is empty while there are features to look up (laser_odometry.cpp:272 / :359);
//   -5  t_wodom_curr is not finite and this frame is mapped: laser_mapping.cpp:207-209 converts it to int (undefined; INT_MIN on x86-64,
//       after which the `while (centerCubeI < 3)` roll of :218 runs for 2^31 rounds).  Everything up to laserOdometryIO has run and can be read.
#include <lidar_odometry_mapping/laser_mapping.h>
#include <lidar_odometry_mapping/laser_odometry.h>
#include <lidar_odometry_mapping/scan_registration.h>
#include <visual_odometry/visual_odometry.h>
#include <vloam_tf/vloam_tf.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

// Everything the façade's header includes — laser_mapping.h, laser_odometry.h, scan_registration.h, vloam_tf.h and through them the
// stand-ins and every standard header they pull in (<memory>, <string>, <vector>, <map>, <cstdio>, ...) — MUST have been included above, with
// `private` meaning private: all of them carry `#pragma once` or include guards, so below only the body of class LidarOdometryMapping is read
// with the keyword respelled.  A new include in lidar_odometry_mapping.h has to be added to the list above first.
#define private public
#include <lidar_odometry_mapping/lidar_odometry_mapping.h>
#undef private

namespace {

enum Stage { ST_VO = 0, ST_LO = 1, ST_MAP = 2 };

struct Block { int type; double payload[13]; };
struct Solve {
  int stage;
  std::vector<double> before, after, raw;
  std::vector<int> nres;
  std::vector<Block> blocks;
  int max_num_iterations;
};

struct VoBlock { int kind; float depth0; float img0[3], img1[3]; double obs[5]; };
struct Row { int kind; float depth0; double obs[5]; int uv[4]; };

struct Session {
  std::shared_ptr<vloam::VloamTF> tf;
  std::shared_ptr<vloam::VisualOdometry> vo;
  std::shared_ptr<vloam::LidarOdometryMapping> loam;
  int count = 0, start_frame = 0, end_frame = -1;
  bool save_traj = false, dead = false, lo_inited = false, map_ran = false;
  float thres = 0.f;
  size_t tree_corner = 0, tree_surf = 0;
  FILE* files[3] = {nullptr, nullptr, nullptr};   // VO, LO, MO
  std::vector<Solve> solves;      // of the last frame, in call order
  std::vector<VoBlock> vo_blocks;
  std::vector<Row> rows;
  double vo_in[6] = {0, 0, 0, 0, 0, 0}, vo_out[6] = {0, 0, 0, 0, 0, 0};
  bool vo_ran = false;
  std::shared_ptr<const void> odom_msg, map_odom_msg;
};

Session* g_observed = nullptr;
int g_stage = ST_VO;

void put3(double* d, const Eigen::Vector3d& v) { d[0] = v.x(); d[1] = v.y(); d[2] = v.z(); }

void on_add(const ceres::CostFunction* cf) {
  if (!g_observed || g_stage != ST_VO) return;
  const vloam::VisualOdometry& vo = *g_observed->vo;
  VoBlock b;
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
    b.kind = -99;
  }
  b.depth0 = vo.depth0;
  for (int k = 0; k < 3; k++) { b.img0[k] = vo.point_3d_image0_0(k); b.img1[k] = vo.point_3d_image0_1(k); }
  g_observed->vo_blocks.push_back(b);
}

void on_solve(const ceres::refshim::SolveRecord& rec) {
  if (!g_observed) return;
  Solve s;
  s.stage = g_stage;
  s.before = rec.before; s.after = rec.after; s.raw = rec.raw_residuals0; s.nres = rec.num_residuals;
  s.max_num_iterations = rec.max_num_iterations;
  for (const ceres::Problem::ResidualBlock& rb : rec.problem->residual_blocks()) {
    Block b;
    b.type = -1;
    std::memset(b.payload, 0, sizeof b.payload);
    if (auto* e = dynamic_cast<const ceres::AutoDiffCostFunction<LidarEdgeFactor, 3, 4, 3>*>(rb.cost)) {
      b.type = 0;
      put3(b.payload, e->functor().curr_point); put3(b.payload + 3, e->functor().last_point_a); put3(b.payload + 6, e->functor().last_point_b);
      b.payload[9] = e->functor().s;
    } else if (auto* p = dynamic_cast<const ceres::AutoDiffCostFunction<LidarPlaneFactor, 1, 4, 3>*>(rb.cost)) {
      b.type = 1;
      put3(b.payload, p->functor().curr_point); put3(b.payload + 3, p->functor().last_point_j); put3(b.payload + 6, p->functor().last_point_l);
      put3(b.payload + 9, p->functor().last_point_m);
      b.payload[12] = p->functor().s;
    } else if (auto* n = dynamic_cast<const ceres::AutoDiffCostFunction<LidarPlaneNormFactor, 1, 4, 3>*>(rb.cost)) {
      b.type = 2;
      put3(b.payload, n->functor().curr_point); put3(b.payload + 3, n->functor().plane_unit_norm);
      b.payload[6] = n->functor().negative_OA_dot_norm;
    } else if (auto* f = dynamic_cast<const ceres::AutoDiffCostFunction<vloam::CostFunctor32, 2, 3, 3>*>(rb.cost)) {
      b.type = 32;
      b.payload[0] = f->functor().observed_x0; b.payload[1] = f->functor().observed_y0; b.payload[2] = f->functor().observed_z0;
      b.payload[3] = f->functor().observed_x1_bar; b.payload[4] = f->functor().observed_y1_bar;
    } else if (auto* g = dynamic_cast<const ceres::AutoDiffCostFunction<vloam::CostFunctor22, 1, 3, 3>*>(rb.cost)) {
      b.type = 22;
      b.payload[0] = g->functor().observed_x0_bar; b.payload[1] = g->functor().observed_y0_bar;
      b.payload[2] = g->functor().observed_x1_bar; b.payload[3] = g->functor().observed_y1_bar;
    }
    s.blocks.push_back(b);
  }
  g_observed->solves.push_back(s);
}

geometry_msgs::Transform msg_of(const double* q_xyzw_t) {
  geometry_msgs::Transform m;
  m.rotation.x = q_xyzw_t[0]; m.rotation.y = q_xyzw_t[1]; m.rotation.z = q_xyzw_t[2]; m.rotation.w = q_xyzw_t[3];
  m.translation.x = q_xyzw_t[4]; m.translation.y = q_xyzw_t[5]; m.translation.z = q_xyzw_t[6];
  return m;
}

int copy_cloud(const pcl::PointCloud<PointType>::Ptr& c, float* buf, int cap) {
  if (!c) return -1;
  const int n = (int)c->points.size();
  if (buf)
    for (int i = 0; i < n && i < cap; i++) {
      const PointType& p = c->points[(size_t)i];
      buf[4 * i] = p.x; buf[4 * i + 1] = p.y; buf[4 * i + 2] = p.z; buf[4 * i + 3] = p.intensity;
    }
  return n;
}

// attribute the VO's residual blocks to the input matches: see ref_vo_harness.cpp
int attribute(Session* s, const int* prev_uv, const int* curr_uv, int n_match) {
  s->rows.assign((size_t)n_match, Row());
  size_t nb = 0;
  for (int k = 0; k < n_match; k++) {
    Row& r = s->rows[(size_t)k];
    std::memset(&r, 0, sizeof r);
    const int px = prev_uv[2 * k], py = prev_uv[2 * k + 1], cx = curr_uv[2 * k], cy = curr_uv[2 * k + 1];
    r.uv[0] = px; r.uv[1] = py; r.uv[2] = cx; r.uv[3] = cy;
    if (nb == s->vo_blocks.size()) continue;
    const VoBlock& bl = s->vo_blocks[nb];
    bool fits = bl.img1[0] == (float)cx && bl.img1[1] == (float)cy && bl.img1[2] == 1.0f;
    if (bl.kind == 32) fits = fits && bl.img0[0] == px * bl.depth0 && bl.img0[1] == py * bl.depth0 && bl.img0[2] == bl.depth0;
    else if (bl.kind == 22) fits = fits && bl.img0[0] == (float)px && bl.img0[1] == (float)py && bl.img0[2] == 1.0f;
    else return -4;
    if (!fits) continue;
    r.kind = bl.kind;
    r.depth0 = bl.depth0;
    std::memcpy(r.obs, bl.obs, sizeof r.obs);
    nb++;
  }
  return nb == s->vo_blocks.size() ? 0 : -4;
}

void put_tf(double* d, const tf2::Transform& T) {
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) d[3 * r + c] = T.getBasis()[r][c];
  d[9] = T.getOrigin().x(); d[10] = T.getOrigin().y(); d[11] = T.getOrigin().z();
}

}  // namespace

extern "C" {

// statics21: imu_T_velo, imu_T_cam0, base_T_imu, each (q x, y, z, w, t x, y, z) as the three lookups return them.
// ints: scan_line, mapping_skip_frame, detach_VO_LO, reset_VO_to_identity, remove_VO_outlier, save_traj, start_frame, end_frame
void* ref_vloam_create(const float* cam_T_velo16, const float* rect0_T_cam16, const float* P_rect0_12, const double* statics21, const int* ints8,
                       double minimum_range, double line_res, double plane_res) {
  std::map<std::string, double>& store = ros::param::shim_store();
  store["loam_verbose_level"] = 0;
  store["scan_line"] = ints8[0];
  store["minimum_range"] = minimum_range;
  store["mapping_line_resolution"] = line_res;
  store["mapping_plane_resolution"] = plane_res;
  store["mapping_skip_frame"] = ints8[1];
  store["detach_VO_LO"] = ints8[2];
  store["map_pub_number"] = 1;
  store["reset_VO_to_identity"] = ints8[3];
  store["remove_VO_outlier"] = ints8[4];
  store["keypoint_NMS"] = 0;
  store["CLAHE"] = 0;
  store["visualize_optical_flow"] = 0;
  store["optical_flow_match"] = 0;
  ceres::refshim::add_observer() = on_add;
  ceres::refshim::observer() = on_solve;
  Session* s = new Session;
  s->save_traj = ints8[5] != 0;
  s->start_frame = ints8[6];
  s->end_frame = ints8[7];
  s->thres = (float)minimum_range;
  // vloam_main_node.cpp:114-122
  s->count = 0;
  s->tf = std::make_shared<vloam::VloamTF>();
  s->vo = std::make_shared<vloam::VisualOdometry>();
  s->loam = std::make_shared<vloam::LidarOdometryMapping>();
  s->tf->init();
  s->vo->init(s->tf);
  s->loam->init(s->tf);
  // in place of the tf tree
  const geometry_msgs::Transform imu_velo = msg_of(statics21), imu_cam0 = msg_of(statics21 + 7), base_imu = msg_of(statics21 + 14);
  s->tf->tf_buffer_ptr->shim_set("imu_link", "velo_link", imu_velo);
  s->tf->tf_buffer_ptr->shim_set("imu_link", "camera_gray_left", imu_cam0);
  s->tf->tf_buffer_ptr->shim_set("base_link", "imu_link", base_imu);
  tf2::Transform a, b;
  tf2::fromMsg(base_imu, a);
  tf2::fromMsg(imu_velo, b);
  s->tf->tf_buffer_ptr->shim_set("base_link", "velo_link", tf2::toMsg(a * b));
  // in place of setUpPointCloud
  for (vloam::PointCloudUtil& u : s->vo->point_cloud_utils) {
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { u.cam_T_velo(r, c) = cam_T_velo16[4 * r + c]; u.rect0_T_cam(r, c) = rect0_T_cam16[4 * r + c]; }
    for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) u.P_rect0(r, c) = P_rect0_12[4 * r + c];
  }
  if (s->save_traj) for (FILE*& f : s->files) f = std::tmpfile();   // vloam_main_node.cpp:101-103
  return s;
}

void ref_vloam_destroy(void* h) {
  Session* s = static_cast<Session*>(h);
  if (g_observed == s) g_observed = nullptr;
  for (FILE* f : s->files) if (f) std::fclose(f);
  delete s;
}

// One callback().  prev_uv / curr_uv: n_match integer pixel pairs, previous frame -> this frame (read when count > 0).
int ref_vloam_frame(void* h, const float* xyz_pad4, int n, const int* prev_uv, const int* curr_uv, int n_match) {
  Session* s = static_cast<Session*>(h);
  if (s->dead) return -3;
  pcl::PointCloud<pcl::PointXYZ> cloud;
  cloud.points.resize((size_t)n);
  bool any = false;
  for (int k = 0; k < n; k++) {
    const pcl::PointXYZ p(xyz_pad4[4 * k], xyz_pad4[4 * k + 1], xyz_pad4[4 * k + 2]);
    cloud.points[(size_t)k] = p;
    if (std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z) && !(p.x * p.x + p.y * p.y + p.z * p.z < s->thres * s->thres)) any = true;
  }
  cloud.width = (uint32_t)n;
  cloud.height = 1;
  cloud.is_dense = false;
  if (!any) { s->dead = true; return -1; }
  vloam::VisualOdometry& vo = *s->vo;
  vloam::LidarOdometryMapping& loam = *s->loam;
  s->solves.clear();
  s->vo_blocks.clear();
  s->rows.clear();
  s->vo_ran = false;
  s->map_ran = false;
  g_observed = s;
  int rc = 0;

  // ---- vloam_main_node.cpp:131-178
  vo.reset();
  loam.reset();
  if (s->count == 0) s->tf->processStaticTransform();
  vo.processPointCloud(sensor_msgs::PointCloud2ConstPtr(), cloud, false, false);
  if (s->count > 0) {
    const int i = vo.i;
    vo.keypoints[(size_t)(1 - i)].assign((size_t)n_match, cv::KeyPoint());
    vo.keypoints[(size_t)i].assign((size_t)n_match, cv::KeyPoint());
    vo.matches.assign((size_t)n_match, cv::DMatch());
    for (int k = 0; k < n_match; k++) {
      vo.keypoints[(size_t)(1 - i)][(size_t)k].pt = cv::Point2f((float)prev_uv[2 * k], (float)prev_uv[2 * k + 1]);
      vo.keypoints[(size_t)i][(size_t)k].pt = cv::Point2f((float)curr_uv[2 * k], (float)curr_uv[2 * k + 1]);
      vo.matches[(size_t)k].queryIdx = k;
      vo.matches[(size_t)k].trainIdx = k;
    }
    g_stage = ST_VO;
    vo.solveNlsAll();
    s->vo_ran = true;
    for (int k = 0; k < 3; k++) { s->vo_out[k] = vo.angles_0to1[k]; s->vo_out[3 + k] = vo.t_0to1[k]; }
    const Solve& sv = s->solves.back();
    if (sv.before.size() == 6) std::memcpy(s->vo_in, sv.before.data(), sizeof s->vo_in);
    else std::memcpy(s->vo_in, s->vo_out, sizeof s->vo_in);   // no block: Solve left the parameters alone
    rc = attribute(s, prev_uv, curr_uv, n_match);
  }
  s->tf->VO2VeloAndBase(vo.cam0_curr_T_cam0_last);
  vo.publish();

  g_stage = ST_LO;
  loam.scanRegistrationIO(cloud);
  if (s->lo_inited && ((s->tree_corner == 0 && !loam.cornerPointsSharp->points.empty()) || (s->tree_surf == 0 && !loam.surfPointsFlat->points.empty()))) {
    s->dead = true;
    g_observed = nullptr;
    return -2;
  }
  loam.laserOdometryIO();
  s->odom_msg = ros::shim_topics()["/laser_odom_to_init"];
  s->lo_inited = true;
  s->tree_corner = loam.cornerPointsLessSharp->points.size();
  s->tree_surf = loam.surfPointsLessFlat->points.size();
  if (!loam.skip_frame && !(std::isfinite(loam.t_wodom_curr.x()) && std::isfinite(loam.t_wodom_curr.y()) && std::isfinite(loam.t_wodom_curr.z()))) {
    s->dead = true;
    g_observed = nullptr;
    return -5;
  }
  g_stage = ST_MAP;
  loam.laserMappingIO();
  s->map_ran = !loam.skip_frame;
  s->map_odom_msg = ros::shim_topics()["/aft_mapped_to_init"];

  if (s->save_traj && s->count >= s->start_frame && s->count <= s->end_frame) {
    s->tf->VO2Cam0StartFrame(s->files[0], s->count - s->start_frame);
    s->tf->LO2Cam0StartFrame(s->files[1], s->count - s->start_frame);
    s->tf->MO2Cam0StartFrame(s->files[2], s->count - s->start_frame);
  }
  ++s->count;
  // ----
  g_observed = nullptr;
  return rc;
}

int ref_vloam_count(void* h) { return static_cast<Session*>(h)->count; }

// The public tf2::Transform members of VloamTF in declaration order, 12 doubles each (basis row-major, origin):
// 0 imu_T_velo, 1 imu_T_cam0, 2 base_T_imu, 3 base_T_cam0, 4 velo_T_cam0, 5 world_VOT_base_last, 6 base_last_VOT_base_curr,
// 7 cam0_curr_VOT_cam0_last, 8 velo_last_VOT_velo_curr, 9 cam0_init_VOT_cam0_last, 10 cam0_init_VOT_cam0_start, 11 cam0_start_VOT_cam0_last,
// 12 world_LOT_base_last, 13 cam0_init_LOT_cam0_last, 14 cam0_init_LOT_cam0_start, 15 cam0_start_LOT_cam0_last, 16 base_prev_LOT_base_curr,
// 17 cam0_curr_LOT_cam0_prev, 18 world_MOT_base_last, 19 cam0_init_MOT_cam0_last, 20 cam0_init_MOT_cam0_start, 21 cam0_start_MOT_cam0_last;
// 22 is VisualOdometry::cam0_curr_T_cam0_last.
int ref_vloam_get_tfs(void* h, double* out23x12) {
  Session* s = static_cast<Session*>(h);
  const vloam::VloamTF& t = *s->tf;
  const tf2::Transform* all[23] = {&t.imu_T_velo, &t.imu_T_cam0, &t.base_T_imu, &t.base_T_cam0, &t.velo_T_cam0, &t.world_VOT_base_last,
                                   &t.base_last_VOT_base_curr, &t.cam0_curr_VOT_cam0_last, &t.velo_last_VOT_velo_curr, &t.cam0_init_VOT_cam0_last,
                                   &t.cam0_init_VOT_cam0_start, &t.cam0_start_VOT_cam0_last, &t.world_LOT_base_last, &t.cam0_init_LOT_cam0_last,
                                   &t.cam0_init_LOT_cam0_start, &t.cam0_start_LOT_cam0_last, &t.base_prev_LOT_base_curr, &t.cam0_curr_LOT_cam0_prev,
                                   &t.world_MOT_base_last, &t.cam0_init_MOT_cam0_last, &t.cam0_init_MOT_cam0_start, &t.cam0_start_MOT_cam0_last,
                                   &s->vo->cam0_curr_T_cam0_last};
  for (int k = 0; k < 23; k++) put_tf(out23x12 + 12 * k, *all[k]);
  return 23;
}

// a transform's rotation as tf2 hands it back (getRotation), for the quaternion the odometry reads out of velo_last_VOT_velo_curr (index 8)
void ref_vloam_get_tf_rotation(void* h, int which, double* q_xyzw) {
  Session* s = static_cast<Session*>(h);
  const tf2::Transform& T = which == 8 ? s->tf->velo_last_VOT_velo_curr : which == 17 ? s->tf->cam0_curr_LOT_cam0_prev : s->tf->world_VOT_base_last;
  const tf2::Quaternion q = T.getRotation();
  q_xyzw[0] = q.x(); q_xyzw[1] = q.y(); q_xyzw[2] = q.z(); q_xyzw[3] = q.w();
}

// imu_eigen_T_velo / imu_eigen_T_cam0 (f32, row-major 4 x 4) as processStaticTransform left them
void ref_vloam_get_eigen_statics(void* h, float* out2x16) {
  Session* s = static_cast<Session*>(h);
  for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { out2x16[4 * r + c] = s->tf->imu_eigen_T_velo(r, c); out2x16[16 + 4 * r + c] = s->tf->imu_eigen_T_cam0(r, c); }
}

// 1 when solveNlsAll ran in the last frame; in6 / out6 the six parameters before / after the solve; counters: CostFunctor32 / 22 blocks
int ref_vloam_get_vo(void* h, double* in6, double* out6, int* counters2) {
  Session* s = static_cast<Session*>(h);
  std::memcpy(in6, s->vo_in, sizeof s->vo_in);
  std::memcpy(out6, s->vo_out, sizeof s->vo_out);
  counters2[0] = counters2[1] = 0;
  for (const VoBlock& b : s->vo_blocks) counters2[b.kind == 32 ? 0 : 1]++;
  return s->vo_ran ? 1 : 0;
}
// per input match 11 doubles: kind (32 / 22; 0 skipped by the outlier gate), depth0, obs[5], prev x, prev y, curr x, curr y
int ref_vloam_get_vo_rows(void* h, double* rows11, int cap) {
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

// the four bucket matrices of the current frame's PointCloudUtil (point_cloud_utils[i]), flattened index_x * new_height + index_y
int ref_vloam_get_buckets(void* h, float* bx, float* by, float* bd, int* bc, int cap, int* dims) {
  Session* s = static_cast<Session*>(h);
  const vloam::PointCloudUtil& u = s->vo->point_cloud_utils[(size_t)s->vo->i];
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

// which: 0-4 the façade's scan-registration clouds; 5 / 6 / 7 laserCloudCornerLast / SurfLast / FullRes as output() handed them over
int ref_vloam_get_cloud(void* h, int which, float* buf, int cap) {
  vloam::LidarOdometryMapping& l = *static_cast<Session*>(h)->loam;
  const pcl::PointCloud<PointType>::Ptr* c[8] = {&l.laserCloud, &l.cornerPointsSharp, &l.cornerPointsLessSharp, &l.surfPointsFlat, &l.surfPointsLessFlat,
                                                 &l.laserCloudCornerLast, &l.laserCloudSurfLast, &l.laserCloudFullRes};
  if (which < 0 || which > 7) return -1;
  return copy_cloud(*c[which], buf, cap);
}
int ref_vloam_skip_frame(void* h) { return static_cast<Session*>(h)->loam->skip_frame ? 1 : 0; }
int ref_vloam_map_ran(void* h) { return static_cast<Session*>(h)->map_ran ? 1 : 0; }

// q_wodom_curr (x, y, z, w) / t_wodom_curr as LaserOdometry::output() handed them to the façade
void ref_vloam_get_lo_pose(void* h, double* q, double* t) {
  vloam::LidarOdometryMapping& l = *static_cast<Session*>(h)->loam;
  q[0] = l.q_wodom_curr.x(); q[1] = l.q_wodom_curr.y(); q[2] = l.q_wodom_curr.z(); q[3] = l.q_wodom_curr.w();
  put3(t, l.t_wodom_curr);
}
// topic 0: /laser_odom_to_init, 1: /aft_mapped_to_init — this session's last message; -1 when there is none
int ref_vloam_get_published_pose(void* h, int topic, double* q, double* t) {
  Session* s = static_cast<Session*>(h);
  const nav_msgs::Odometry* m = static_cast<const nav_msgs::Odometry*>((topic == 0 ? s->odom_msg : s->map_odom_msg).get());
  if (!m) return -1;
  q[0] = m->pose.pose.orientation.x; q[1] = m->pose.pose.orientation.y; q[2] = m->pose.pose.orientation.z; q[3] = m->pose.pose.orientation.w;
  t[0] = m->pose.pose.position.x; t[1] = m->pose.pose.position.y; t[2] = m->pose.pose.position.z;
  return 0;
}

// every ceres::Solve of the last frame in call order.  info: stage (0 VO, 1 odometry, 2 mapping), residual blocks, residuals,
// max_num_iterations, parameters (6 for the VO, 7 otherwise; 0 when the problem had no block at all)
int ref_vloam_num_solves(void* h) { return (int)static_cast<Session*>(h)->solves.size(); }
int ref_vloam_get_solve(void* h, int k, double* before7, double* after7, int* info5) {
  Session* s = static_cast<Session*>(h);
  if (k < 0 || k >= (int)s->solves.size()) return -1;
  const Solve& v = s->solves[(size_t)k];
  if (v.before.size() > 7 || v.after.size() != v.before.size()) return -2;
  std::memcpy(before7, v.before.data(), v.before.size() * sizeof(double));
  std::memcpy(after7, v.after.data(), v.after.size() * sizeof(double));
  info5[0] = v.stage; info5[1] = (int)v.blocks.size(); info5[2] = (int)v.raw.size(); info5[3] = v.max_num_iterations; info5[4] = (int)v.before.size();
  return 0;
}
// types[blocks] (0 LidarEdgeFactor, 1 LidarPlaneFactor, 2 LidarPlaneNormFactor, 32 CostFunctor32, 22 CostFunctor22), nres[blocks],
// payload[blocks][13], raw[residuals]
int ref_vloam_get_solve_blocks(void* h, int k, int* types, int* nres, double* payload, double* raw) {
  Session* s = static_cast<Session*>(h);
  if (k < 0 || k >= (int)s->solves.size()) return -1;
  const Solve& v = s->solves[(size_t)k];
  for (size_t i = 0; i < v.blocks.size(); i++) {
    types[i] = v.blocks[i].type;
    nres[i] = v.nres[i];
    std::memcpy(payload + 13 * i, v.blocks[i].payload, 13 * sizeof(double));
  }
  if (!v.raw.empty()) std::memcpy(raw, v.raw.data(), v.raw.size() * sizeof(double));
  return 0;
}

// the text written so far into file `which` (0 VO, 1 LO, 2 MO), byte for byte; returns its length (-1: save_traj is off)
long ref_vloam_get_rows_text(void* h, int which, char* buf, long cap) {
  Session* s = static_cast<Session*>(h);
  FILE* f = (which >= 0 && which < 3) ? s->files[which] : nullptr;
  if (!f) return -1;
  std::fflush(f);
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  if (buf && cap > 0) {
    std::rewind(f);
    const size_t got = std::fread(buf, 1, (size_t)(n < cap ? n : cap), f);
    (void)got;
    std::fseek(f, 0, SEEK_END);
  }
  return n;
}

}  // extern "C"

// ---- image_util.cpp is not built: visual_odometry.cpp refers to these from processImage() / publish() (verbose_level > 0 only), never called here
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
