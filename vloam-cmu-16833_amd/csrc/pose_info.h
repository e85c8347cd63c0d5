// Per-sweep pose information matrices (vloam_pose_info_enable, c_api.h: vloam_pose_info_record) — host-visible interface of pose_info.hip.
// One row per sweep and session, OUTSIDE the session arenas (arena layout and checkpoints are what they are without the product).  Each
// LiDAR stage writes its half of the row with ONE launch on its own stream behind its last solve: the Gauss–Newton information matrix of the
// last outer round's problem at the pose that round returned, its eigenvalues, cost, factor counts and flags.  Nothing here is allocated or
// launched on a handle that did not enable the product.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/vloam_hip/c_api.h"
#include "vloam_device.h"

namespace vloam {

constexpr int kPiThreads = 256;
constexpr int kPiMaxBlocks = 64;       // workgroups of one reduce launch at most (their partials are added in workgroup order)
constexpr int kPiSlotsPerBlock = 2048; // table slots a workgroup takes per trip (8 per lane)
// per (stage, session): the ticket the workgroups of a launch draw and their partial sums (pose_rows_dev.h, which only the kernels' units see)
template <int MaxBlocks> struct PoseRowsScratch;
using PoseInfoScratch = PoseRowsScratch<kPiMaxBlocks>;

struct PoseInfo {   // device memory of the product, one allocation each, not in the arenas
  vloam_pose_info_record* rows = nullptr;   // [B][max_frames]
  PoseInfoScratch* scratch = nullptr;       // [2 stages][B]
  int max_frames = 0;
  double min_eig[2] = {0.0, 0.0};           // degeneracy thresholds: odometry, mapping (0 = never)
};

inline int pose_info_blocks(int cap) { const int g = (cap + kPiSlotsPerBlock - 1) / kPiSlotsPerBlock; return g < 1 ? 1 : (g > kPiMaxBlocks ? kPiMaxBlocks : g); }

size_t pose_info_scratch_bytes(int n_sessions);
// rows of a fresh product: zero, frame = -1 (all sessions); scratch zero
hipError_t pose_info_init(hipStream_t st, const PoseInfo& P, int n_sessions);
// stage 0 (odometry) / 1 (mapping) of sweep `frame`, on that stage's stream behind its last solve.  F: the table of the last outer round (read by
// slot: type, p, dg; session 0's addresses); rec: that round's LMRecord (x_out is the point of evaluation, n_factors is not trusted but
// recounted).  ran: the host's knowledge that the stage solved at all (0: first sweep / skipped sweep -> the zero half, no VALID bit, the
// table and the record are not read); d_enable (may be null): the device's gate of the solve (MapState::do_optimize), 0 -> the same.
// stamp: this launch completes the row (writes `frame`).
void pose_info_launch(hipStream_t st, Sess se, const PoseInfo& P, int stage, int frame, const FactorTable& F, const LMRecord* rec, bool ran,
                      const int* d_enable, bool stamp, ProfHook* ph, hipEvent_t done);

}  // namespace vloam
