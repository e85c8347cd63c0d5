// REFERENCE HARNESS — TEST INFRASTRUCTURE ONLY (our own text).
//
// A plain-C entry to the REFERENCE'S OWN vloam::LaserOdometry and vloam::LaserMapping (src/lidar_odometry_mapping/src/
// laser_odometry.cpp, laser_mapping.cpp — translation units of their own, compiled unmodified from the tree the make variable REF_DIR
// names) next to its ScanRegistration, chained as the façade chains them (lidar_odometry_mapping.cpp:65-150: reset, scanRegistrationIO,
// laserOdometryIO = input / solveLO / publish / output, laserMappingIO = input / solveMapping unless skip_frame / publish).  The façade
// class itself keeps the hand-over clouds in private members, so the chaining is restated here, call for call.
//
// Everything is observed from OUTSIDE — no private member is touched:
//   * output() hands over q_w_curr / t_w_curr, the three last clouds and skip_frame;
//   * the stand-in ceres::Solve reports each problem (ref_shim/ceres/ceres.h): parameters before / after, the residual blocks in
//     AddResidualBlock order with their functors' points (public members of the reference's functor structs), raw residuals;
//   * the stand-in publishers keep the last message per topic: /aft_mapped_to_init, /laser_cloud_map (with the point count of every
//     cube: ref_shim/pcl/point_cloud.h), /velodyne_cloud_registered;
//   * the stand-in VoxelGrid logs the sizes of what it filtered: the first two calls of solveMapping are the two stacks.
// What this pins is the reference's control flow, constants, index arithmetic, argument order and evaluation order.  The minimizer, the
// kd-tree, the eigen-solver and the QR behind it are the ORACLE'S restatements (ref_bridge.cpp, ref_shim/): not pinned, on purpose.
// The harness never lets the reference run into undefined behaviour: where it would index an empty search result it returns a status.
#include <lidar_odometry_mapping/laser_mapping.h>
#include <lidar_odometry_mapping/laser_odometry.h>
#include <lidar_odometry_mapping/scan_registration.h>

#include <cstring>
#include <memory>

namespace {

struct Block { int type; double payload[13]; };
struct Solve {
  std::vector<double> before, after, raw;
  std::vector<int> nres;
  std::vector<Block> blocks;
  int max_num_iterations;
};

struct Session {
  std::shared_ptr<vloam::VloamTF> tf;
  std::unique_ptr<vloam::ScanRegistration> sr;
  std::unique_ptr<vloam::LaserOdometry> lo;
  std::unique_ptr<vloam::LaserMapping> lm;
  float thres = 0.f;
  pcl::PointCloud<PointType>::Ptr srout[5];
  // what laserOdometryIO hands to laserMappingIO (members of the façade in the reference)
  Eigen::Quaterniond q_wodom_curr;
  Eigen::Vector3d t_wodom_curr;
  pcl::PointCloud<PointType>::Ptr cornerLast, surfLast, fullRes;
  bool skip_frame = false;
  // bookkeeping for the undefined-behaviour guard: sizes of the clouds the odometry's kd-trees currently hold
  bool lo_inited = false, dead = false;
  size_t tree_corner = 0, tree_surf = 0;
  std::vector<Solve> solves[2];   // of the last laserOdometryIO / laserMappingIO
  std::vector<std::pair<int, int>> map_filter_log;
  bool map_ran = false;
  // this session's own copies of the last messages (the stand-in topics are process-wide: taken right after each publish())
  std::shared_ptr<const void> odom_msg, map_odom_msg, map_msg, registered_msg;
};

Session* g_observed = nullptr;
int g_stage = 0;

void put3(double* d, const Eigen::Vector3d& v) { d[0] = v.x(); d[1] = v.y(); d[2] = v.z(); }

void observe(const ceres::refshim::SolveRecord& rec) {
  if (!g_observed) return;
  Solve s;
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
    } else if (auto* d = dynamic_cast<const ceres::AutoDiffCostFunction<LidarDistanceFactor, 3, 4, 3>*>(rb.cost)) {
      b.type = 3;
      put3(b.payload, d->functor().curr_point); put3(b.payload + 3, d->functor().closed_point);
    }
    s.blocks.push_back(b);
  }
  g_observed->solves[g_stage].push_back(s);
}

int copy_cloud(const std::vector<PointType>& p, float* buf, int cap) {
  const int n = (int)p.size();
  if (buf)
    for (int i = 0; i < n && i < cap; i++) {
      buf[4 * i] = p[(size_t)i].x; buf[4 * i + 1] = p[(size_t)i].y; buf[4 * i + 2] = p[(size_t)i].z; buf[4 * i + 3] = p[(size_t)i].intensity;
    }
  return n;
}

}  // namespace

extern "C" {

void* ref_loam_create(int scan_line, double minimum_range, double line_res, double plane_res, int mapping_skip_frame, int detach_vo_lo) {
  std::map<std::string, double>& store = ros::param::shim_store();
  store["loam_verbose_level"] = 0;
  store["scan_line"] = scan_line;
  store["minimum_range"] = minimum_range;
  store["mapping_line_resolution"] = line_res;
  store["mapping_plane_resolution"] = plane_res;
  store["mapping_skip_frame"] = mapping_skip_frame;
  store["detach_VO_LO"] = detach_vo_lo;
  store["map_pub_number"] = 1;   // (frameCount * mapping_skip_frame) % 1 == 0: the map is published on every call of publish()
  ceres::refshim::observer() = observe;
  Session* s = new Session;
  s->tf = std::make_shared<vloam::VloamTF>();
  s->sr.reset(new vloam::ScanRegistration());
  s->lo.reset(new vloam::LaserOdometry());
  s->lm.reset(new vloam::LaserMapping());
  s->sr->init();
  s->lo->init(s->tf);
  s->lm->init(s->tf);
  s->thres = (float)minimum_range;
  // the façade's init() (lidar_odometry_mapping.cpp:52-54)
  s->cornerLast = boost::make_shared<pcl::PointCloud<PointType>>();
  s->surfLast = boost::make_shared<pcl::PointCloud<PointType>>();
  s->fullRes = boost::make_shared<pcl::PointCloud<PointType>>();
  return s;
}
void ref_loam_destroy(void* h) {
  if (g_observed == h) g_observed = nullptr;
  delete static_cast<Session*>(h);
}

// vloam_tf->velo_last_VOT_velo_curr, which laser_odometry.cpp:225-232 reads when detach_VO_LO is false.  A tf2::Transform keeps the
// rotation as a matrix: q_back / t_back receive what the reference will read from it (not bit for bit q).
void ref_loam_set_vo_prior(void* h, const double* q_xyzw, const double* t, double* q_back, double* t_back) {
  Session* s = static_cast<Session*>(h);
  s->tf->velo_last_VOT_velo_curr.setOrigin(tf2::Vector3(t[0], t[1], t[2]));
  s->tf->velo_last_VOT_velo_curr.setRotation(tf2::Quaternion(q_xyzw[0], q_xyzw[1], q_xyzw[2], q_xyzw[3]));
  const tf2::Quaternion q = s->tf->velo_last_VOT_velo_curr.getRotation();
  const tf2::Vector3& o = s->tf->velo_last_VOT_velo_curr.getOrigin();
  q_back[0] = q.x(); q_back[1] = q.y(); q_back[2] = q.z(); q_back[3] = q.w();
  t_back[0] = o.x(); t_back[1] = o.y(); t_back[2] = o.z();
}

// LidarOdometryMapping::reset + scanRegistrationIO.  -1 (nothing called) when no point survives the input filters: see ref_sr_run.
int ref_loam_stage_sr(void* h, const float* xyz_pad4, int n) {
  Session* s = static_cast<Session*>(h);
  if (s->dead) return -3;
  pcl::PointCloud<pcl::PointXYZ> in;
  in.points.resize((size_t)n);
  for (int i = 0; i < n; i++) in.points[(size_t)i] = pcl::PointXYZ(xyz_pad4[4 * i], xyz_pad4[4 * i + 1], xyz_pad4[4 * i + 2]);
  in.width = (uint32_t)n;
  in.height = 1;
  in.is_dense = false;
  bool any = false;
  for (int i = 0; i < n && !any; i++) {
    const pcl::PointXYZ& p = in.points[(size_t)i];
    if (!(std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z))) continue;
    if (p.x * p.x + p.y * p.y + p.z * p.z < s->thres * s->thres) continue;
    any = true;
  }
  if (!any) return -1;
  s->sr->reset();
  s->lm->reset();
  s->sr->input(in);
  s->sr->output(s->srout[0], s->srout[1], s->srout[2], s->srout[3], s->srout[4]);
  return 0;
}

// replaces one of the five clouds between the stages (which: 0 laserCloud ... 4 surfPointsLessFlat)
int ref_loam_set_sr_cloud(void* h, int which, const float* pts, int n) {
  Session* s = static_cast<Session*>(h);
  if (which < 0 || which > 4) return -1;
  auto c = boost::make_shared<pcl::PointCloud<PointType>>();
  for (int i = 0; i < n; i++) {
    PointType p;
    p.x = pts[4 * i]; p.y = pts[4 * i + 1]; p.z = pts[4 * i + 2]; p.intensity = pts[4 * i + 3];
    c->push_back(p);
  }
  s->srout[which] = c;
  return 0;
}

// laserOdometryIO.  -2 (nothing called, the session is closed) when a kd-tree of the odometry is empty while there are features to look up:
// nearestKSearch then returns nothing and laser_odometry.cpp:272 / :359 reads pointSearchSqDis[0] of an empty vector.
int ref_loam_stage_lo(void* h) {
  Session* s = static_cast<Session*>(h);
  if (s->dead) return -3;
  for (int w = 0; w < 5; w++) if (!s->srout[w]) return -1;
  if (s->lo_inited && ((s->tree_corner == 0 && !s->srout[1]->points.empty()) || (s->tree_surf == 0 && !s->srout[3]->points.empty()))) {
    s->dead = true;
    return -2;
  }
  g_observed = s;
  g_stage = 0;
  s->solves[0].clear();
  s->lo->input(s->srout[0], s->srout[1], s->srout[2], s->srout[3], s->srout[4]);
  s->lo->solveLO();
  s->lo->publish();
  s->odom_msg = ros::shim_topics()["/laser_odom_to_init"];
  s->lo->output(s->q_wodom_curr, s->t_wodom_curr, s->cornerLast, s->surfLast, s->fullRes, s->skip_frame);
  g_observed = nullptr;
  s->lo_inited = true;
  s->tree_corner = s->srout[2]->points.size();   // laser_odometry.cpp:511-526: the less-sharp / less-flat clouds become the trees
  s->tree_surf = s->srout[4]->points.size();
  return 0;
}

// replaces what laserOdometryIO handed over, before laserMappingIO: which 5 / 6 / 7 = laserCloudCornerLast / SurfLast / FullRes
int ref_loam_set_map_cloud(void* h, int which, const float* pts, int n) {
  Session* s = static_cast<Session*>(h);
  if (which < 5 || which > 7) return -1;
  auto c = boost::make_shared<pcl::PointCloud<PointType>>();
  for (int i = 0; i < n; i++) {
    PointType p;
    p.x = pts[4 * i]; p.y = pts[4 * i + 1]; p.z = pts[4 * i + 2]; p.intensity = pts[4 * i + 3];
    c->push_back(p);
  }
  (which == 5 ? s->cornerLast : which == 6 ? s->surfLast : s->fullRes) = c;
  return 0;
}

// laserMappingIO; q_xyzw / t, when given, replace the odometry pose handed over (LaserMapping::input takes whatever its caller has)
int ref_loam_stage_map(void* h, const double* q_xyzw, const double* t) {
  Session* s = static_cast<Session*>(h);
  if (s->dead) return -3;
  if (q_xyzw) s->q_wodom_curr = Eigen::Quaterniond(q_xyzw[3], q_xyzw[0], q_xyzw[1], q_xyzw[2]);
  if (t) s->t_wodom_curr = Eigen::Vector3d(t[0], t[1], t[2]);
  g_observed = s;
  g_stage = 1;
  s->solves[1].clear();
  pcl::refshim::filter_log().clear();
  s->lm->input(s->cornerLast, s->surfLast, s->fullRes, s->q_wodom_curr, s->t_wodom_curr, s->skip_frame);
  s->map_ran = !s->skip_frame;
  pcl::refshim::filter_log_on() = true;    // only around this call: other sessions and scan registration log nothing
  if (!s->skip_frame) s->lm->solveMapping();
  pcl::refshim::filter_log_on() = false;
  s->map_filter_log = pcl::refshim::filter_log();
  pcl::refshim::filter_log().clear();
  s->lm->publish();
  s->map_odom_msg = ros::shim_topics()["/aft_mapped_to_init"];
  s->map_msg = ros::shim_topics()["/laser_cloud_map"];
  s->registered_msg = ros::shim_topics()["/velodyne_cloud_registered"];
  g_observed = nullptr;
  return 0;
}

int ref_loam_skip_frame(void* h) { return static_cast<Session*>(h)->skip_frame ? 1 : 0; }

// which: 0-4 the scan registration's clouds; 5 / 6 / 7 laserCloudCornerLast / SurfLast / FullRes as output() handed them over;
// 8 /laser_cloud_map; 9 /velodyne_cloud_registered
int ref_loam_get_cloud(void* h, int which, float* buf, int cap) {
  Session* s = static_cast<Session*>(h);
  if (which >= 0 && which <= 4) return s->srout[which] ? copy_cloud(s->srout[which]->points, buf, cap) : -1;
  if (which == 5) return copy_cloud(s->cornerLast->points, buf, cap);
  if (which == 6) return copy_cloud(s->surfLast->points, buf, cap);
  if (which == 7) return copy_cloud(s->fullRes->points, buf, cap);
  if (which == 8 || which == 9) {
    const sensor_msgs::PointCloud2* m = static_cast<const sensor_msgs::PointCloud2*>((which == 8 ? s->map_msg : s->registered_msg).get());
    if (!m) return -1;
    const int n = (int)(m->xyzi.size() / 4);
    if (buf) std::memcpy(buf, m->xyzi.data(), sizeof(float) * 4 * (size_t)(n < cap ? n : cap));
    return n;
  }
  return -1;
}

// point counts of the 4851 cubes of the last published map, corner and surface alternating (2 * 4851 numbers)
int ref_loam_get_map_cube_counts(void* h, unsigned* buf, int cap) {
  const sensor_msgs::PointCloud2* m = static_cast<const sensor_msgs::PointCloud2*>(static_cast<Session*>(h)->map_msg.get());
  if (!m) return -1;
  const int n = (int)m->appended.size();
  if (buf) for (int i = 0; i < n && i < cap; i++) buf[i] = m->appended[(size_t)i];
  return n;
}

// q_w_curr (x, y, z, w) / t_w_curr as output() handed them over
void ref_loam_get_lo_pose(void* h, double* q, double* t) {
  Session* s = static_cast<Session*>(h);
  q[0] = s->q_wodom_curr.x(); q[1] = s->q_wodom_curr.y(); q[2] = s->q_wodom_curr.z(); q[3] = s->q_wodom_curr.w();
  put3(t, s->t_wodom_curr);
}

// topic 0: /laser_odom_to_init, 1: /aft_mapped_to_init — the pose of the last message, 0 when there is one
int ref_loam_get_published_pose(void* h, int topic, double* q, double* t) {
  Session* s = static_cast<Session*>(h);
  const nav_msgs::Odometry* m = static_cast<const nav_msgs::Odometry*>((topic == 0 ? s->odom_msg : s->map_odom_msg).get());
  if (!m) return -1;
  q[0] = m->pose.pose.orientation.x; q[1] = m->pose.pose.orientation.y; q[2] = m->pose.pose.orientation.z; q[3] = m->pose.pose.orientation.w;
  t[0] = m->pose.pose.position.x; t[1] = m->pose.pose.position.y; t[2] = m->pose.pose.position.z;
  return 0;
}

// which: 0 base_prev_LOT_base_curr, 1 world_LOT_base_last, 2 world_MOT_base_last — as tf2 hands them back (rotation through a matrix)
void ref_loam_get_tf(void* h, int which, double* q, double* t) {
  Session* s = static_cast<Session*>(h);
  const tf2::Transform& T = which == 0 ? s->tf->base_prev_LOT_base_curr : which == 1 ? s->tf->world_LOT_base_last : s->tf->world_MOT_base_last;
  const tf2::Quaternion r = T.getRotation();
  q[0] = r.x(); q[1] = r.y(); q[2] = r.z(); q[3] = r.w();
  t[0] = T.getOrigin().x(); t[1] = T.getOrigin().y(); t[2] = T.getOrigin().z();
}

// did the last laserMappingIO call solveMapping; the (in, out) sizes of its VoxelGrid calls
int ref_loam_map_ran(void* h) { return static_cast<Session*>(h)->map_ran ? 1 : 0; }
int ref_loam_get_map_filter_log(void* h, int* buf, int cap) {
  Session* s = static_cast<Session*>(h);
  const int n = (int)s->map_filter_log.size();
  if (buf) for (int i = 0; i < n && i < cap; i++) { buf[2 * i] = s->map_filter_log[(size_t)i].first; buf[2 * i + 1] = s->map_filter_log[(size_t)i].second; }
  return n;
}

// stage: 0 odometry, 1 mapping.  Number of ceres::Solve calls of the last stage call
int ref_loam_num_solves(void* h, int stage) { return (int)static_cast<Session*>(h)->solves[stage].size(); }
// before / after: 7 doubles (q x, y, z, w, t); counts: residual blocks, residuals, max_num_iterations
int ref_loam_get_solve(void* h, int stage, int k, double* before, double* after, int* counts) {
  Session* s = static_cast<Session*>(h);
  if (k < 0 || k >= (int)s->solves[stage].size()) return -1;
  const Solve& v = s->solves[stage][(size_t)k];
  if (v.before.size() != 7 || v.after.size() != 7) return -2;
  std::memcpy(before, v.before.data(), 7 * sizeof(double));
  std::memcpy(after, v.after.data(), 7 * sizeof(double));
  counts[0] = (int)v.blocks.size(); counts[1] = (int)v.raw.size(); counts[2] = v.max_num_iterations;
  return 0;
}
// types[blocks], nres[blocks], payload[blocks][13], raw[residuals]
int ref_loam_get_solve_blocks(void* h, int stage, int k, int* types, int* nres, double* payload, double* raw) {
  Session* s = static_cast<Session*>(h);
  if (k < 0 || k >= (int)s->solves[stage].size()) return -1;
  const Solve& v = s->solves[stage][(size_t)k];
  for (size_t i = 0; i < v.blocks.size(); i++) {
    types[i] = v.blocks[i].type;
    nres[i] = v.nres[i];
    std::memcpy(payload + 13 * i, v.blocks[i].payload, 13 * sizeof(double));
  }
  if (!v.raw.empty()) std::memcpy(raw, v.raw.data(), v.raw.size() * sizeof(double));
  return 0;
}

}  // extern "C"
