// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text).
// ceres::LossFunction / HuberLoss(a) (Ceres 2.0 loss_function.cc: rho = s for s <= a^2, else 2 a sqrt(s) - a^2).  The minimizer the
// residual blocks end up in is the oracle's (ceres/ceres.h says how), which applies its own Huber from a(): Evaluate is here for
// completeness.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>

namespace ceres {
class LossFunction {
 public:
  virtual ~LossFunction() {}
  virtual void Evaluate(double sq_norm, double out[3]) const = 0;
};
class HuberLoss : public LossFunction {
 public:
  explicit HuberLoss(double a) : a_(a), b_(a * a) {}
  double a() const { return a_; }
  void Evaluate(double s, double rho[3]) const override {
    if (s > b_) {
      const double r = std::sqrt(s);
      rho[0] = 2.0 * a_ * r - b_;
      rho[1] = std::max(std::numeric_limits<double>::min(), a_ / r);
      rho[2] = -rho[1] / (2.0 * s);
    } else {
      rho[0] = s; rho[1] = 1.0; rho[2] = 0.0;
    }
  }

 private:
  double a_, b_;
};
}  // namespace ceres
