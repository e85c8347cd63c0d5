// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text; functional).
//
// What the reference's functor headers need of <ceres/ceres.h>: Jet (ceres/jet.h), CostFunction and an AutoDiffCostFunction<Functor,
// kNumResiduals, N0, N1> that does what Ceres 2.0's does for two parameter blocks — seeds one Jet<double, N0 + N1> per parameter with
// a unit partial, calls the functor once, and hands back the residuals and one row-major kNumResiduals x Ni Jacobian per block, in
// the AMBIENT parameters (no local parameterization; that is the solver's business).  The minimizer (Problem / Solve) is NOT here.
#pragma once
#include <ceres/jet.h>

namespace ceres {

class CostFunction {
 public:
  virtual ~CostFunction() {}
  virtual bool Evaluate(double const* const* parameters, double* residuals, double** jacobians) const = 0;
  virtual int num_residuals() const = 0;
};

template <class Functor, int kNumResiduals, int N0, int N1>
class AutoDiffCostFunction : public CostFunction {
 public:
  explicit AutoDiffCostFunction(Functor* f) : f_(f) {}
  ~AutoDiffCostFunction() override { delete f_; }
  int num_residuals() const override { return kNumResiduals; }
  bool Evaluate(double const* const* parameters, double* residuals, double** jacobians) const override {
    if (!jacobians) return (*f_)(parameters[0], parameters[1], residuals);
    typedef Jet<double, N0 + N1> J;
    J x0[N0], x1[N1], r[kNumResiduals];
    for (int i = 0; i < N0; i++) x0[i] = J(parameters[0][i], i);
    for (int i = 0; i < N1; i++) x1[i] = J(parameters[1][i], N0 + i);
    if (!(*f_)(x0, x1, r)) return false;
    for (int k = 0; k < kNumResiduals; k++) {
      residuals[k] = r[k].a;
      if (jacobians[0]) for (int i = 0; i < N0; i++) jacobians[0][k * N0 + i] = r[k].v[i];
      if (jacobians[1]) for (int i = 0; i < N1; i++) jacobians[1][k * N1 + i] = r[k].v[N0 + i];
    }
    return true;
  }

 private:
  Functor* f_;
};

}  // namespace ceres
