// Test probe (tests/test_ref_factors.py): the PRODUCT header include/vloam_hip/factors.hpp evaluated with a dual number, behind the same
// C entry as oracle/ref_harness.cpp's ref_eval_factor — residuals and the Jacobian with respect to the raw parameter blocks.
// The dual number is oracle/ref_shim/ceres/jet.h (our stand-in for ceres::Jet; found by ADL exactly as factors.hpp's header promises for
// the real one).  Nothing of the reference is included here.
#include <ceres/jet.h>
#include "vloam_hip/factors.hpp"

namespace {
template <int kRes, int N0, class F>
int eval(const F& f, const double* p0, const double* p1, double* res, double* jac) {
  typedef ceres::Jet<double, N0 + 3> J;
  J x0[N0], x1[3], r[kRes];
  for (int i = 0; i < N0; i++) x0[i] = J(p0[i], i);
  for (int i = 0; i < 3; i++) x1[i] = J(p1[i], N0 + i);
  if (!f(x0, x1, r)) return -1;
  for (int k = 0; k < kRes; k++) {
    res[k] = r[k].a;
    for (int i = 0; i < N0 + 3; i++) jac[k * (N0 + 3) + i] = r[k].v[i];
  }
  return kRes;
}
}  // namespace

// types and payloads as ref_eval_factor's (0 edge, 1 plane, 2 plane-norm, 5 CostFunctor32, 7 CostFunctor22); -2 = the header has no such functor
extern "C" int fac_eval_factor(int type, const double* d, const double* p0, const double* p1, double* res, double* jac) {
  using namespace vloam::factors;
  switch (type) {
    case 0: return eval<3, 4>(LidarEdgeFactor(d, d + 3, d + 6, d[9]), p0, p1, res, jac);
    case 1: return eval<1, 4>(LidarPlaneFactor(d, d + 3, d + 6, d + 9, d[12]), p0, p1, res, jac);
    case 2: return eval<1, 4>(LidarPlaneNormFactor(d, d + 3, d[6]), p0, p1, res, jac);
    case 5: return eval<2, 3>(CostFunctor32(d[0], d[1], d[2], d[3], d[4]), p0, p1, res, jac);
    case 7: return eval<1, 3>(CostFunctor22(d[0], d[1], d[2], d[3]), p0, p1, res, jac);
  }
  return -2;
}
