// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// ceres::LossFunction / HuberLoss: declarations for the files that will need them (laser_odometry.cpp, laser_mapping.cpp,
// visual_odometry.cpp — not built against this tree yet).  ceres_cost_function.h includes the header and uses nothing of it.
#pragma once

namespace ceres {
class LossFunction {
 public:
  virtual ~LossFunction() {}
  virtual void Evaluate(double sq_norm, double out[3]) const = 0;
};
}  // namespace ceres
