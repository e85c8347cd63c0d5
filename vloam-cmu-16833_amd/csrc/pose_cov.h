// Per-sweep pose covariance rows (vloam_pose_cov_enable, c_api.h: vloam_pose_cov_record) — host-visible interface of pose_cov.hip.
// An add-on of the pose information product (pose_info.h): one row per sweep and session, an allocation of its own OUTSIDE the session arenas.
// Each LiDAR stage writes its half with ONE one-wavefront launch on its own stream directly behind k_pose_info_lo / k_pose_info_map of the same
// sweep: it reads the H, cost, counts and valid bit that kernel just wrote (no second walk over the factor table), runs a lane-parallel cyclic
// Jacobi WITH eigenvectors on it and writes eigenvalues, eigenvectors, rank, sigma^2 and the pseudo-inverse covariance.  The VO half is written
// by a reduction kernel behind the VO solve of a coupled frame (vloam_process_frame*): sum rho' J^T J of CostFunctor32 / CostFunctor22 over the
// VO stage's factor storage at the returned (angle-axis, t), then the same decomposition.  Nothing here is allocated or launched on a handle
// that did not enable the product.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/vloam_hip/c_api.h"
#include "vloam_device.h"

namespace vloam {

constexpr int kPcThreads = 256;        // the VO reduction's workgroup
constexpr int kPcSlotsPerBlock = 512;  // VO table slots a workgroup takes per trip (2 per lane: the dual-number evaluation is long)
constexpr int kPcMaxBlocks = 16;       // workgroups of the VO reduction at most (their partials are added in workgroup order)
// per session: the ticket the workgroups of a VO launch draw and their partial sums (pose_rows_dev.h, which only the kernels' units see)
template <int MaxBlocks> struct PoseRowsScratch;
using PoseCovScratch = PoseRowsScratch<kPcMaxBlocks>;

struct PoseCov {   // device memory of the product, one allocation each, not in the arenas
  vloam_pose_cov_record* rows = nullptr;   // [B][max_frames]
  PoseCovScratch* scratch = nullptr;       // [B]
  int max_frames = 0;
  double min_eig[3] = {0.0, 0.0, 0.0};     // pseudo-inverse thresholds: odometry, mapping, VO (0: only lambda <= 1e-12 lambda_max is dropped)
};

inline int pose_cov_vo_blocks(int cap) { const int g = (cap + kPcSlotsPerBlock - 1) / kPcSlotsPerBlock; return g < 1 ? 1 : (g > kPcMaxBlocks ? kPcMaxBlocks : g); }

size_t pose_cov_scratch_bytes(int n_sessions);
// rows of a fresh product: zero, frame = -1 (all sessions); scratch zero
hipError_t pose_cov_init(hipStream_t st, const PoseCov& P, int n_sessions);
// stage 0 (odometry) / 1 (mapping) of sweep `frame`, on that stage's stream directly behind pose_info_launch of the same stage and sweep.
// info_rows: the pose information rows ([B][max_frames], same indexing).  stamp: this launch completes the row (writes `frame`).
void pose_cov_launch(hipStream_t st, Sess se, const PoseCov& P, const vloam_pose_info_record* info_rows, int stage, int frame, bool stamp, hipEvent_t done);
// the VO half of sweep `frame`, on the stream that ran the VO solve, behind it.  F: the VO stage's table (read by slot: type, p, A; session 0's
// addresses); x: the (angle-axis, t) the solve returned.
void pose_cov_vo_launch(hipStream_t st, Sess se, const PoseCov& P, int frame, const FactorTable& F, const double* x);

}  // namespace vloam
