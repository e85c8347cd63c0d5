// REFERENCE HARNESS — TEST INFRASTRUCTURE ONLY (our own text).
//
// ceres::Solve of the stand-in <ceres/ceres.h> (ref_shim/): the reference's Problem, exactly as laser_odometry.cpp / laser_mapping.cpp
// built it, handed to the ORACLE'S minimizer (orc::Problem::Solve, orc_ceres.cpp).  The minimizer is delegated on purpose — Ceres
// does not exist on the build machine and pinning it is not the aim; see ref_shim/ceres/ceres.h.  Every residual block keeps the
// reference's own cost function (its AutoDiffCostFunction around its own functor): the oracle's solver only calls Evaluate on it.
// Checked rather than assumed: two parameter blocks of sizes (4 with a quaternion parameterization | 3, 3), every residual block on
// exactly those two in that order, one HuberLoss shared by all (or none).  Anything else aborts: it would mean the reference drives
// Ceres in a way this bridge does not express.  A problem without any block (VisualOdometry::solveNlsAll on a frame without a usable
// match) is left alone, as Ceres leaves it: no parameter block, nothing to minimise, the parameters keep their values.
//
// Also here: Eigen::refshim::qr3_f32, what the stand-in Eigen's colPivHouseholderQr().solve on a 3 x 3 f32 block delegates to — the
// oracle's own f32 restatement (orc::solve3x3_colpiv_qr_f32, orc_vo.cpp).  Eigen's QR is not pinned either.
#include <cstdio>
#include <cstdlib>
#include <ceres/ceres.h>
#include "orc_ceres.h"
#include "orc_vo.h"

namespace Eigen {
namespace refshim {
void qr3_f32(const float A_row_major[9], const float b[3], float x[3]) { orc::solve3x3_colpiv_qr_f32(A_row_major, b, x); }
}  // namespace refshim
}  // namespace Eigen

namespace {

struct Adapter : orc::CostFunction {
  const ceres::CostFunction* cf;
  explicit Adapter(const ceres::CostFunction* c) : cf(c) { nres = c->num_residuals(); }
  void Evaluate(const double* p0, const double* p1, double* residuals, double* jac0, double* jac1) const override {
    const double* params[2] = {p0, p1};
    double* jacs[2] = {jac0, jac1};
    if (!cf->Evaluate(params, residuals, (jac0 || jac1) ? jacs : nullptr)) { std::fprintf(stderr, "ref_bridge: a cost function failed\n"); std::abort(); }
  }
};

void require(bool ok, const char* what) {
  if (!ok) { std::fprintf(stderr, "ref_bridge: %s\n", what); std::abort(); }
}

}  // namespace

namespace ceres {

void Solve(const Solver::Options& options, Problem* problem, Solver::Summary* summary) {
  const std::vector<Problem::ParameterBlock>& pb = problem->parameter_blocks();
  const std::vector<Problem::ResidualBlock>& rb = problem->residual_blocks();
  if (pb.empty() && rb.empty()) {
    refshim::SolveRecord rec;
    rec.problem = problem;
    rec.max_num_iterations = options.max_num_iterations;
    if (summary) *summary = Solver::Summary();
    if (refshim::observer()) refshim::observer()(rec);
    return;
  }
  require(pb.size() == 2 && pb[1].size == 3 && !pb[1].parameterization, "expected two parameter blocks, the second a plain 3-vector");
  const bool quat = dynamic_cast<EigenQuaternionParameterization*>(pb[0].parameterization) != nullptr;
  require(quat ? pb[0].size == 4 : (pb[0].size == 3 && !pb[0].parameterization), "first block: 4 with EigenQuaternionParameterization, or a plain 3");
  require(options.linear_solver_type == DENSE_QR, "DENSE_QR expected");

  orc::SolveOptions opt;
  opt.max_num_iterations = options.max_num_iterations;
  opt.quaternion_block0 = quat;
  opt.huber_a = 0.0;
  orc::Problem p;
  refshim::SolveRecord rec;
  rec.problem = problem;
  rec.max_num_iterations = options.max_num_iterations;
  for (size_t i = 0; i < rb.size(); i++) {
    require(rb[i].p0 == pb[0].values && rb[i].p1 == pb[1].values, "a residual block on other parameter blocks, or in another order");
    require(rb[i].loss == rb[0].loss, "one loss function shared by all residual blocks expected");
    p.Add(new Adapter(rb[i].cost));
    const int n = rb[i].cost->num_residuals();
    require(n >= 1 && n <= 3, "1 to 3 residuals per block");
    double r[3];
    const double* params[2] = {pb[0].values, pb[1].values};
    require(rb[i].cost->Evaluate(params, r, nullptr), "a cost function failed at the initial point");
    rec.num_residuals.push_back(n);
    rec.raw_residuals0.insert(rec.raw_residuals0.end(), r, r + n);
  }
  if (!rb.empty() && rb[0].loss) {
    const HuberLoss* h = dynamic_cast<const HuberLoss*>(rb[0].loss);
    require(h != nullptr, "HuberLoss expected");
    opt.huber_a = h->a();
  } else if (rb.empty()) {
    opt.huber_a = 0.1;   // no block, no loss to ask: immaterial
  }
  for (const Problem::ParameterBlock& b : pb) rec.before.insert(rec.before.end(), b.values, b.values + b.size);
  orc::SolveSummary s;
  p.Solve(opt, pb[0].values, pb[1].values, &s);
  for (const Problem::ParameterBlock& b : pb) rec.after.insert(rec.after.end(), b.values, b.values + b.size);
  if (summary) {
    summary->initial_cost = s.initial_cost;
    summary->final_cost = s.final_cost;
    summary->num_residual_blocks = s.num_residual_blocks;
    summary->num_residuals = s.num_residuals;
  }
  if (refshim::observer()) refshim::observer()(rec);
}

}  // namespace ceres
