// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text; functional).
//
// ceres::AngleAxisRotatePoint, CrossProduct, DotProduct of Ceres Solver 2.0 include/ceres/rotation.h, restated.  AngleAxisRotatePoint
// has two branches: theta^2 = w . w > std::numeric_limits<double>::epsilon() -> Rodrigues' formula with the unit axis w / theta
// (pt cos(theta) + (w x pt) sin(theta) + w (w . pt) (1 - cos(theta))); otherwise the first-order form pt + w x pt, which keeps the
// derivative finite at zero rotation.  A second entry next to oracle/orc_ceres.h, sharing no code with it.
#pragma once
#include <cmath>
#include <limits>
#include <ceres/jet.h>

namespace ceres {

template <class T> inline T DotProduct(const T x[3], const T y[3]) { return (x[0] * y[0] + x[1] * y[1] + x[2] * y[2]); }

template <class T> inline void CrossProduct(const T x[3], const T y[3], T x_cross_y[3]) {
  x_cross_y[0] = x[1] * y[2] - x[2] * y[1];
  x_cross_y[1] = x[2] * y[0] - x[0] * y[2];
  x_cross_y[2] = x[0] * y[1] - x[1] * y[0];
}

template <class T> inline void AngleAxisRotatePoint(const T angle_axis[3], const T pt[3], T result[3]) {
  using std::sqrt;
  using std::cos;
  using std::sin;
  const T theta2 = DotProduct(angle_axis, angle_axis);
  if (theta2 > T(std::numeric_limits<double>::epsilon())) {
    const T theta = sqrt(theta2);
    const T costheta = cos(theta);
    const T sintheta = sin(theta);
    const T theta_inverse = T(1.0) / theta;
    const T w[3] = {angle_axis[0] * theta_inverse, angle_axis[1] * theta_inverse, angle_axis[2] * theta_inverse};
    T w_cross_pt[3];
    CrossProduct(w, pt, w_cross_pt);
    const T tmp = DotProduct(w, pt) * (T(1.0) - costheta);
    for (int i = 0; i < 3; i++) result[i] = pt[i] * costheta + w_cross_pt[i] * sintheta + w[i] * tmp;
  } else {
    T w_cross_pt[3];
    CrossProduct(angle_axis, pt, w_cross_pt);
    for (int i = 0; i < 3; i++) result[i] = pt[i] + w_cross_pt[i];
  }
}

}  // namespace ceres
