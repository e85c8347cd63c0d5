// REFERENCE HARNESS — TEST INFRASTRUCTURE ONLY (our own text).
//
// A plain-C entry to the REFERENCE'S OWN program text, compiled unmodified from the reference tree named by the make variable REF_DIR
// (oracle/Makefile, target `ref`) against the functional stand-in headers of oracle/ref_shim/:
//   * vloam::ScanRegistration (src/lidar_odometry_mapping/src/scan_registration.cpp, a translation unit of its own): init with
//     scan_line / minimum_range, then per sweep reset(), input() with a caller-chosen is_dense, output() — the five clouds;
//   * the eight cost functors of lidarFactor.hpp and ceres_cost_function.h: residuals and the full Jacobian with respect to the raw
//     parameter blocks (4 + 3 or 3 + 3 ambient parameters), in double through the functor's own Create() and in long double through
//     Jet<long double, N>.
// What this pins is the reference's control flow, constants, index arithmetic, overload resolution and evaluation order.  PCL, Eigen,
// Ceres and ROS behind it are stand-ins (each header says what it restates).  Nothing of the reference is copied here.
#include <lidar_odometry_mapping/scan_registration.h>
// Right after the reference's own includes, before anything else can add a declaration: the overloads that the unqualified calls of
// scan_registration.cpp:192 (`atan(point.z / sqrt(...))` on floats) see in their translation unit.
static const int kAtanOfFloatIsFloat = sizeof(atan(1.0f)) == sizeof(float) ? 1 : 0;
static const int kSqrtOfFloatIsFloat = sizeof(sqrt(1.0f)) == sizeof(float) ? 1 : 0;

#include <lidar_odometry_mapping/lidarFactor.hpp>
#include <visual_odometry/ceres_cost_function.h>

#include <cstring>
#include <memory>

namespace {

struct SrSession {
  std::unique_ptr<vloam::ScanRegistration> sr;  // 6.4 MB of member arrays: on the heap
  pcl::PointCloud<PointType>::Ptr out[5];
  float thres = 0.f;  // MINIMUM_RANGE as removeClosedPointCloud receives it (a double passed as float)
};

// residuals and Jacobian of one functor in scalar type S, by one Jet<S, N0 + N1> evaluation (what ceres::AutoDiffCostFunction does)
template <class S, int kRes, int N0, int N1, class F>
int eval_jet(const F& f, const double* p0, const double* p1, S* res, S* jac) {
  typedef ceres::Jet<S, N0 + N1> J;
  J x0[N0], x1[N1], r[kRes];
  for (int i = 0; i < N0; i++) x0[i] = J(S(p0[i]), i);
  for (int i = 0; i < N1; i++) x1[i] = J(S(p1[i]), N0 + i);
  if (!f(x0, x1, r)) return -1;
  for (int k = 0; k < kRes; k++) {
    res[k] = r[k].a;
    for (int i = 0; i < N0 + N1; i++) jac[k * (N0 + N1) + i] = r[k].v[i];
  }
  return kRes;
}

// the double path goes through the reference's own Create(): its residual / block-size template arguments are part of what is pinned
template <int N0, int N1>
int eval_created(ceres::CostFunction* cf, const double* p0, const double* p1, double* res, double* jac) {
  std::unique_ptr<ceres::CostFunction> own(cf);
  const int n = own->num_residuals();
  double j0[3 * N0], j1[3 * N1];
  const double* params[2] = {p0, p1};
  double* jacs[2] = {j0, j1};
  if (!own->Evaluate(params, res, jacs)) return -1;
  for (int k = 0; k < n; k++) {
    for (int i = 0; i < N0; i++) jac[k * (N0 + N1) + i] = j0[k * N0 + i];
    for (int i = 0; i < N1; i++) jac[k * (N0 + N1) + N0 + i] = j1[k * N1 + i];
  }
  return n;
}

Eigen::Vector3d v3(const double* p) { return Eigen::Vector3d(p[0], p[1], p[2]); }

}  // namespace

extern "C" {

// 1 when the reference's translation unit resolves atan(float) and sqrt(float) to the float overloads
int ref_math_overloads_are_float() { return kAtanOfFloatIsFloat && kSqrtOfFloatIsFloat; }

// false: VoxelGrid sorts with std::sort as PCL does; true: the project's canonical order (see ref_shim/pcl/filters/voxel_grid.h)
void ref_set_voxel_stable_order(int stable) { pcl::refshim::voxel_stable_order() = stable != 0; }

void* ref_sr_create(int scan_line, double minimum_range) {
  std::map<std::string, double>& store = ros::param::shim_store();
  store["loam_verbose_level"] = 0;  // (read without a check at scan_registration.cpp:42: the member stays uninitialised if unset)
  store["scan_line"] = scan_line;
  store["minimum_range"] = minimum_range;
  SrSession* s = new SrSession;
  s->sr.reset(new vloam::ScanRegistration());
  s->sr->init();
  s->thres = (float)minimum_range;
  return s;
}
void ref_sr_destroy(void* h) { delete static_cast<SrSession*>(h); }

// One sweep: reset(), input(), output().  xyz_pad4: n points of 4 floats, the fourth ignored (the input type is pcl::PointXYZ).
// Returns -1 WITHOUT calling input() when no point would survive the two input filters: the reference then reads points[0] of an empty
// vector (scan_registration.cpp:166), which is undefined behaviour and not a result to record.
int ref_sr_run(void* h, const float* xyz_pad4, int n, int is_dense) {
  SrSession* s = static_cast<SrSession*>(h);
  pcl::PointCloud<pcl::PointXYZ> in;
  in.points.resize((size_t)n);
  for (int i = 0; i < n; i++) in.points[(size_t)i] = pcl::PointXYZ(xyz_pad4[4 * i], xyz_pad4[4 * i + 1], xyz_pad4[4 * i + 2]);
  in.width = (uint32_t)n;
  in.height = 1;
  in.is_dense = is_dense != 0;
  const float thres = s->thres;
  bool any = false;
  for (int i = 0; i < n && !any; i++) {
    const pcl::PointXYZ& p = in.points[(size_t)i];
    if (!is_dense && !(std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z))) continue;
    if (p.x * p.x + p.y * p.y + p.z * p.z < thres * thres) continue;
    any = true;
  }
  if (!any) return -1;
  s->sr->reset();
  s->sr->input(in);
  s->sr->output(s->out[0], s->out[1], s->out[2], s->out[3], s->out[4]);
  return 0;
}

// which: 0 laserCloud, 1 cornerPointsSharp, 2 cornerPointsLessSharp, 3 surfPointsFlat, 4 surfPointsLessFlat; returns the point count
int ref_sr_get_cloud(void* h, int which, float* buf, int cap) {
  SrSession* s = static_cast<SrSession*>(h);
  if (which < 0 || which > 4 || !s->out[which]) return -1;
  const std::vector<PointType>& p = s->out[which]->points;
  const int n = (int)p.size();
  if (buf)
    for (int i = 0; i < n && i < cap; i++) {
      buf[4 * i] = p[(size_t)i].x; buf[4 * i + 1] = p[(size_t)i].y; buf[4 * i + 2] = p[(size_t)i].z; buf[4 * i + 3] = p[(size_t)i].intensity;
    }
  return n;
}

// type / payload d[] / parameter blocks:
//   0 LidarEdgeFactor      curr[3] a[3] b[3] s        q[4] (x, y, z, w), t[3]
//   1 LidarPlaneFactor     curr[3] j[3] l[3] m[3] s   q[4], t[3]
//   2 LidarPlaneNormFactor curr[3] n[3] d             q[4], t[3]
//   3 LidarDistanceFactor  curr[3] closed[3]          q[4], t[3]
//   4 CostFunctor33        x0 y0 z0 x1 y1 z1          angles[3], t[3]
//   5 CostFunctor32        x0 y0 z0 x1_bar y1_bar     angles[3], t[3]
//   6 CostFunctor23        x0_bar y0_bar x1 y1 z1     angles[3], t[3]
//   7 CostFunctor22        x0_bar y0_bar x1_bar y1_bar angles[3], t[3]
// Returns the number of residuals; res[nres]; jac[nres][n0 + 3] row-major, derivatives with respect to the raw parameters.
int ref_eval_factor(int type, const double* d, const double* p0, const double* p1, double* res, double* jac) {
  switch (type) {
    case 0: return eval_created<4, 3>(LidarEdgeFactor::Create(v3(d), v3(d + 3), v3(d + 6), d[9]), p0, p1, res, jac);
    case 1: return eval_created<4, 3>(LidarPlaneFactor::Create(v3(d), v3(d + 3), v3(d + 6), v3(d + 9), d[12]), p0, p1, res, jac);
    case 2: return eval_created<4, 3>(LidarPlaneNormFactor::Create(v3(d), v3(d + 3), d[6]), p0, p1, res, jac);
    case 3: return eval_created<4, 3>(LidarDistanceFactor::Create(v3(d), v3(d + 3)), p0, p1, res, jac);
    case 4: return eval_created<3, 3>(vloam::CostFunctor33::Create(d[0], d[1], d[2], d[3], d[4], d[5]), p0, p1, res, jac);
    case 5: return eval_created<3, 3>(vloam::CostFunctor32::Create(d[0], d[1], d[2], d[3], d[4]), p0, p1, res, jac);
    case 6: return eval_created<3, 3>(vloam::CostFunctor23::Create(d[0], d[1], d[2], d[3], d[4]), p0, p1, res, jac);
    case 7: return eval_created<3, 3>(vloam::CostFunctor22::Create(d[0], d[1], d[2], d[3]), p0, p1, res, jac);
  }
  return -1;
}

// the same functors evaluated in long double (inputs are the same doubles, widened): the yardstick for the double evaluation's own error
int ref_eval_factor_ld(int type, const double* d, const double* p0, const double* p1, long double* res, long double* jac) {
  typedef long double L;
  switch (type) {
    case 0: return eval_jet<L, 3, 4, 3>(LidarEdgeFactor(v3(d), v3(d + 3), v3(d + 6), d[9]), p0, p1, res, jac);
    case 1: return eval_jet<L, 1, 4, 3>(LidarPlaneFactor(v3(d), v3(d + 3), v3(d + 6), v3(d + 9), d[12]), p0, p1, res, jac);
    case 2: return eval_jet<L, 1, 4, 3>(LidarPlaneNormFactor(v3(d), v3(d + 3), d[6]), p0, p1, res, jac);
    case 3: return eval_jet<L, 3, 4, 3>(LidarDistanceFactor(v3(d), v3(d + 3)), p0, p1, res, jac);
    case 4: return eval_jet<L, 3, 3, 3>(vloam::CostFunctor33(d[0], d[1], d[2], d[3], d[4], d[5]), p0, p1, res, jac);
    case 5: return eval_jet<L, 2, 3, 3>(vloam::CostFunctor32(d[0], d[1], d[2], d[3], d[4]), p0, p1, res, jac);
    case 6: return eval_jet<L, 2, 3, 3>(vloam::CostFunctor23(d[0], d[1], d[2], d[3], d[4]), p0, p1, res, jac);
    case 7: return eval_jet<L, 1, 3, 3>(vloam::CostFunctor22(d[0], d[1], d[2], d[3]), p0, p1, res, jac);
  }
  return -1;
}

}  // extern "C"
