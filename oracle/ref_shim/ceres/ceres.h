// REFERENCE-BUILD STAND-IN — TEST INFRASTRUCTURE ONLY (our own text; functional).
//
// What the reference's functor headers need of <ceres/ceres.h>: Jet (ceres/jet.h), CostFunction and an AutoDiffCostFunction<Functor,
// kNumResiduals, N0, N1> that does what Ceres 2.0's does for two parameter blocks — seeds one Jet<double, N0 + N1> per parameter with
// a unit partial, calls the functor once, and hands back the residuals and one row-major kNumResiduals x Ni Jacobian per block, in
// the AMBIENT parameters (no local parameterization; that is the solver's business).  AutoDiffCostFunction::functor() exposes the
// functor, as Ceres 2.0's does.
//
// Problem / Solve, as laser_odometry.cpp:217-221,257-258,347,440,458-463 and laser_mapping.cpp:461-467,514,578,610-617 drive them:
// Problem(Options), AddParameterBlock(values, size[, parameterization]), AddResidualBlock(cost, loss, block0, block1),
// Solver::Options / Summary, Solve.  visual_odometry.cpp:258-259,366,413,423 adds no parameter block of its own: like Ceres,
// AddResidualBlock then registers the two blocks it is given, with the sizes the cost function states (parameter_block_size), in the
// order it first sees them.  Every AddResidualBlock is also reported to ceres::refshim::add_observer(), at the moment of the call, so
// that a harness can read what the reference holds in its public members right then (VisualOdometry::depth0, point_3d_image0_0 / _1).
// The Problem owns what it is given, like Ceres' default Options.  The MINIMIZER IS NOT RESTATED
// HERE: Solve (oracle/ref_bridge.cpp) hands the residual blocks, in AddResidualBlock order, to the oracle's restatement of Ceres'
// trust-region loop (orc::Problem::Solve, oracle/orc_ceres.cpp, linked into the reference library) — pinning Ceres is not the aim.
// What is pinned is what the reference PUTS INTO the problem: which blocks, in which order, from which points, at which parameters.
// For that, Solve reports every call to ceres::refshim::observer(): the problem while it is still alive, the parameter values before
// and after, and the raw residuals of every block at the initial point.
#pragma once
#include <functional>
#include <string>
#include <vector>
#include <ceres/jet.h>
#include <ceres/loss_function.h>

namespace ceres {

class CostFunction {
 public:
  virtual ~CostFunction() {}
  virtual bool Evaluate(double const* const* parameters, double* residuals, double** jacobians) const = 0;
  virtual int num_residuals() const = 0;
  virtual int parameter_block_size(int k) const = 0;
};

namespace refshim {
inline std::function<void(const CostFunction*)>& add_observer() { static std::function<void(const CostFunction*)> f; return f; }
}  // namespace refshim

template <class Functor, int kNumResiduals, int N0, int N1>
class AutoDiffCostFunction : public CostFunction {
 public:
  explicit AutoDiffCostFunction(Functor* f) : f_(f) {}
  ~AutoDiffCostFunction() override { delete f_; }
  int num_residuals() const override { return kNumResiduals; }
  int parameter_block_size(int k) const override { return k == 0 ? N0 : N1; }
  const Functor& functor() const { return *f_; }
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

class LocalParameterization {
 public:
  virtual ~LocalParameterization() {}
};
class EigenQuaternionParameterization : public LocalParameterization {};

enum LinearSolverType { DENSE_QR };

class Solver {
 public:
  struct Options {
    LinearSolverType linear_solver_type = DENSE_QR;
    int max_num_iterations = 50;
    bool minimizer_progress_to_stdout = false;
    bool check_gradients = false;
    double gradient_check_relative_precision = 1e-8;
  };
  struct Summary {
    double initial_cost = 0, final_cost = 0;
    int num_residual_blocks = 0, num_residuals = 0;
    std::string FullReport() const { return std::string(); }
  };
};

class Problem {
 public:
  struct Options {};
  struct ParameterBlock { double* values; int size; LocalParameterization* parameterization; };
  struct ResidualBlock { CostFunction* cost; LossFunction* loss; double* p0; double* p1; };

  Problem() {}
  explicit Problem(const Options&) {}
  Problem(const Problem&) = delete;
  Problem& operator=(const Problem&) = delete;
  ~Problem() {
    std::vector<const void*> freed;   // one loss / parameterization object may be shared by many blocks
    auto once = [&](const void* p) { for (const void* q : freed) if (q == p) return false; freed.push_back(p); return true; };
    for (ResidualBlock& r : residual_blocks_) {
      delete r.cost;
      if (r.loss && once(r.loss)) delete r.loss;
    }
    for (ParameterBlock& b : parameter_blocks_) if (b.parameterization && once(b.parameterization)) delete b.parameterization;
  }
  void AddParameterBlock(double* values, int size, LocalParameterization* parameterization = nullptr) {
    parameter_blocks_.push_back({values, size, parameterization});
  }
  void AddResidualBlock(CostFunction* cost, LossFunction* loss, double* p0, double* p1) {
    double* const p[2] = {p0, p1};
    for (int k = 0; k < 2; k++) {
      bool known = false;
      for (const ParameterBlock& b : parameter_blocks_) known = known || b.values == p[k];
      if (!known) parameter_blocks_.push_back({p[k], cost->parameter_block_size(k), nullptr});
    }
    residual_blocks_.push_back({cost, loss, p0, p1});
    if (refshim::add_observer()) refshim::add_observer()(cost);
  }
  const std::vector<ParameterBlock>& parameter_blocks() const { return parameter_blocks_; }
  const std::vector<ResidualBlock>& residual_blocks() const { return residual_blocks_; }

 private:
  std::vector<ParameterBlock> parameter_blocks_;
  std::vector<ResidualBlock> residual_blocks_;
};

namespace refshim {
struct SolveRecord {
  const Problem* problem;                  // alive during the call only
  int max_num_iterations;
  std::vector<double> before, after;       // the parameter blocks in AddParameterBlock order, concatenated
  std::vector<int> num_residuals;          // per residual block
  std::vector<double> raw_residuals0;      // of all blocks at the initial point, concatenated (no loss applied)
};
inline std::function<void(const SolveRecord&)>& observer() { static std::function<void(const SolveRecord&)> f; return f; }
}  // namespace refshim

void Solve(const Solver::Options& options, Problem* problem, Solver::Summary* summary);   // oracle/ref_bridge.cpp

}  // namespace ceres
