// Per-sweep diagnostics log (vloam_limits_ext::sweep_log, c_api.h: vloam_sweep_record) — host-visible interface of sweep_log.hip.
// One row per sweep and session beside the trajectory log.  Each stage stream writes its slice of the row behind its own work for that
// sweep with one single-workgroup launch (two on the mapping stream), so no stream waits for another; the last stage stamps `frame`.
// Nothing here is allocated or launched on a handle without the log.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/vloam_hip/c_api.h"
#include "map_kernels.h"
#include "vloam_device.h"

namespace vloam {

// what the log kernels carry from one launch to a later one (per session, in the arena; zero at creation)
struct SweepLogScratch {
  int vo_nan_seen;      // LOState::tf.vo_nan_frames as of the last odometry row: a rise is this frame's zero-angle VO solve
  int fallback_seen;    // MapFrame::fallback_solves as claimed by a row so far (atomicMax: the odometry and mapping streams share the counter)
  int map_err_before;   // the handle's sticky error word in front of this sweep's mapping (k_sweep_log_map_begin)
  int stack_err;        // the error word of this sweep's scan-feature VoxelGrid, read before k_map_prepare folds and clears it
};

struct SweepLogN { int n[kMaxBatch]; };   // points handed in, per session

// behind the sweep's scan registration (scan-registration stream): counts + kErrEmpty / kErrRingTooLong of this sweep (FrameScalars::error is per sweep)
void sweep_log_sr_launch(hipStream_t st, Sess se, vloam_sweep_record* rows, int frame, const FrameScalars* S, const BatchIn& bi, ProfHook* ph, hipEvent_t done);
// behind the sweep's odometry (odometry stream).  corr0 / corr1: the correspondence arrays the two solves' factors were emitted with ([kMaxLoFactors][4],
// first int -1 = no factor); rec: LMRecord[2]; complete: the handle has no mapping stage, this launch stamps `frame`
void sweep_log_lo_launch(hipStream_t st, Sess se, vloam_sweep_record* rows, int frame, SweepLogScratch* scratch, const LOState* lo, const int* corr0,
                         const int* corr1, const LMRecord* rec, const int* fallbacks, bool complete, ProfHook* ph, hipEvent_t done);
// in front of / behind the sweep's mapping (mapping stream)
void sweep_log_map_begin_launch(hipStream_t st, Sess se, SweepLogScratch* scratch, const MapFrame* fr, const StackInfo* si, bool skip_frame, ProfHook* ph);
void sweep_log_map_launch(hipStream_t st, Sess se, vloam_sweep_record* rows, int frame, SweepLogScratch* scratch, const MapState* ms, const MapFrame* fr,
                          const LMRecord* rec, bool skip_frame, ProfHook* ph, hipEvent_t done);
// rows of a fresh log: zero, frame = -1 (one session; the others are copied from it)
hipError_t sweep_log_init(hipStream_t st, vloam_sweep_record* rows, int n_rows);

}  // namespace vloam
