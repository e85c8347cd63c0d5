// Per-sweep diagnostics log: the kernels that write vloam_sweep_record rows (sweep_log.h).  gfx950, wave64.
// Every launch is ONE workgroup per session (session in blockIdx.z, VL_SESSION) that reads a few scalars its stage has just left in HBM and
// writes a slice of one 192-byte row with plain vector stores; error_bits and flags are shared by the stages and therefore OR-ed atomically.
#include "sweep_log.h"

namespace vloam {

__global__ __launch_bounds__(64) void k_sweep_log_init(vloam_sweep_record* rows, int n_rows) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= n_rows) return;
  int* w = reinterpret_cast<int*>(rows + r);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(vloam_sweep_record) / sizeof(int)); k++) w[k] = 0;
  rows[r].frame = -1;
}

__global__ __launch_bounds__(64) void k_sweep_log_sr(vloam_sweep_record* rows, int frame, const FrameScalars* S, SweepLogN nin, size_t ss) {
  VL_SESSION(ss); RB(rows); RB(S);
  if (threadIdx.x != 0) return;
  vloam_sweep_record* row = rows + frame;
  row->n_in = nin.n[blockIdx.z];
  row->n_cloud = S->N2;
  row->n_sharp = S->n_sharp; row->n_less_sharp = S->n_less_sharp; row->n_flat = S->n_flat; row->n_less_flat = S->n_less_flat;
  const int e = S->error & (kErrEmpty | kErrRingTooLong);
  if (e) atomicOr(&row->error_bits, e);
}

// a cooperative solve that degraded bumped the handle's counter: the first row to see the rise claims it
__device__ __forceinline__ int claim_fallbacks(SweepLogScratch* sc, const int* fallbacks) {
  const int now = *fallbacks;
  return now > atomicMax(&sc->fallback_seen, now) ? VLOAM_SWEEP_FLAG_SOLVE_DEGRADED : 0;
}

__global__ __launch_bounds__(256) void k_sweep_log_lo(vloam_sweep_record* rows, int frame, SweepLogScratch* sc, const LOState* lo, const int* corr0,
                                                      const int* corr1, const LMRecord* rec, const int* fallbacks, int complete, size_t ss) {
  VL_SESSION(ss); RB(rows); RB(sc); RB(lo); RB(corr0); RB(corr1); RB(rec); RB(fallbacks);
  __shared__ int cnt[4];   // [round][corner, plane]
  const int tid = threadIdx.x;
  if (tid < 4) cnt[tid] = 0;
  __syncthreads();
  if (frame > 0) {
    // factors per round and kind, from the correspondence arrays k_lo_assoc* filled for the solves: a wavefront's ballot per 64 slots
    // (kMaxSharp is a multiple of 64, so a wavefront never straddles the corner / plane boundary)
    static_assert(kMaxSharp % 64 == 0 && kMaxLoFactors % 256 == 0, "one kind per wavefront, no tail");
    for (int slot = tid; slot < kMaxLoFactors; slot += 256) {
      const unsigned long long m0 = __ballot(corr0[slot * 4] >= 0), m1 = __ballot(corr1[slot * 4] >= 0);
      if ((tid & 63) == 0) {
        const int kind = slot < kMaxSharp ? 0 : 1;
        if (m0) atomicAdd(&cnt[kind], __popcll(m0));
        if (m1) atomicAdd(&cnt[2 + kind], __popcll(m1));
      }
    }
  }
  __syncthreads();
  if (tid != 0) return;
  vloam_sweep_record* row = rows + frame;
  int flags = claim_fallbacks(sc, fallbacks);
  if (frame == 0) flags |= VLOAM_SWEEP_FLAG_FIRST;   // LO:196-204: the first sweep only initialises
  else {
    for (int o = 0; o < 2; o++) {
      row->lo_corner_factors[o] = cnt[2 * o]; row->lo_plane_factors[o] = cnt[2 * o + 1];
      row->lo_iterations[o] = (int)rec[o].n_iterations; row->lo_termination[o] = (int)rec[o].termination;
      row->lo_initial_cost[o] = rec[o].initial_cost; row->lo_final_cost[o] = rec[o].final_cost;
      if (cnt[2 * o] + cnt[2 * o + 1] < 10) flags |= o ? VLOAM_SWEEP_FLAG_LO_LESS_CORR_1 : VLOAM_SWEEP_FLAG_LO_LESS_CORR_0;   // LO:452-455
    }
  }
  const int nan_frames = lo->tf.vo_nan_frames;
  if (nan_frames > sc->vo_nan_seen) { atomicOr(&row->error_bits, kErrVoDegenerate); sc->vo_nan_seen = nan_frames; }
  if (flags) atomicOr(&row->flags, flags);
  if (complete) row->frame = frame;
}

__global__ __launch_bounds__(64) void k_sweep_log_map_begin(SweepLogScratch* sc, const MapFrame* fr, const StackInfo* si, int skip_frame, size_t ss) {
  VL_SESSION(ss); RB(sc); RB(fr); RB(si);
  if (threadIdx.x != 0) return;
  sc->map_err_before = fr->error;
  sc->stack_err = skip_frame ? 0 : si->error;   // (a skipped sweep has no scan-feature VoxelGrid)
}

__global__ __launch_bounds__(64) void k_sweep_log_map(vloam_sweep_record* rows, int frame, SweepLogScratch* sc, const MapState* ms, const MapFrame* fr,
                                                      const LMRecord* rec, int skip_frame, size_t ss) {
  VL_SESSION(ss); RB(rows); RB(sc); RB(ms); RB(fr); RB(rec);
  if (threadIdx.x != 0) return;
  vloam_sweep_record* row = rows + frame;
  int flags = claim_fallbacks(sc, &fr->fallback_solves);
  if (skip_frame) flags |= VLOAM_SWEEP_FLAG_MAP_SKIPPED;
  else {
    const int opt = ms->do_optimize;
    row->n_corner_stack = ms->n_corner_stack; row->n_surf_stack = ms->n_surf_stack;
    row->n_map_corner = ms->n_map_corner; row->n_map_surf = ms->n_map_surf;
    if (!opt) flags |= VLOAM_SWEEP_FLAG_MAP_NOT_OPTIMIZED;   // LM:448,631-635: the records still hold an earlier sweep's solves
    else {
      for (int o = 0; o < 2; o++) {
        row->map_corner_factors[o] = fr->n_factors[o][0]; row->map_surf_factors[o] = fr->n_factors[o][1];
        row->map_iterations[o] = (int)rec[o].n_iterations; row->map_termination[o] = (int)rec[o].termination;
        row->map_initial_cost[o] = rec[o].initial_cost; row->map_final_cost[o] = rec[o].final_cost;
      }
    }
    // the map's own bits stay in the sticky word for good: what this sweep's mapping ADDED to it; the VoxelGrid's bits are this sweep's own word
    const int e = ((fr->error & ~sc->map_err_before) & (kErrMapFull | kErrMapDeferred)) | (sc->stack_err & (kErrStackFull | kErrSolverSync));
    if (e) atomicOr(&row->error_bits, e);
  }
  if (flags) atomicOr(&row->flags, flags);
  row->frame = frame;
}

static_assert(VLOAM_SWEEP_EMPTY == kErrEmpty && VLOAM_SWEEP_RING_TOO_LONG == kErrRingTooLong && VLOAM_SWEEP_MAP_FULL == kErrMapFull &&
              VLOAM_SWEEP_MAP_RAW_CAPACITY == kErrMapDeferred && VLOAM_SWEEP_STACK_FULL == kErrStackFull && VLOAM_SWEEP_DS_TIMEOUT == kErrSolverSync &&
              VLOAM_SWEEP_VO_DEGENERATE == kErrVoDegenerate, "the public bits are the device's");

void sweep_log_sr_launch(hipStream_t st, Sess se, vloam_sweep_record* rows, int frame, const FrameScalars* S, const BatchIn& bi, ProfHook* ph, hipEvent_t done) {
  SweepLogN nin;
  for (int b = 0; b < kMaxBatch; b++) nin.n[b] = b < se.B ? bi.n[b] : 0;
  VLOAM_LAUNCH_EV(ph, kKSweepLogSr, st, done, k_sweep_log_sr, dim3(1, 1, se.B), dim3(64), 0, st, rows, frame, S, nin, se.ss);
}
void sweep_log_lo_launch(hipStream_t st, Sess se, vloam_sweep_record* rows, int frame, SweepLogScratch* scratch, const LOState* lo, const int* corr0,
                         const int* corr1, const LMRecord* rec, const int* fallbacks, bool complete, ProfHook* ph, hipEvent_t done) {
  VLOAM_LAUNCH_EV(ph, kKSweepLogLo, st, done, k_sweep_log_lo, dim3(1, 1, se.B), dim3(256), 0, st, rows, frame, scratch, lo, corr0, corr1, rec, fallbacks,
                  complete ? 1 : 0, se.ss);
}
void sweep_log_map_begin_launch(hipStream_t st, Sess se, SweepLogScratch* scratch, const MapFrame* fr, const StackInfo* si, bool skip_frame, ProfHook* ph) {
  VLOAM_LAUNCH(ph, kKSweepLogMapBegin, st, k_sweep_log_map_begin, dim3(1, 1, se.B), dim3(64), 0, st, scratch, fr, si, skip_frame ? 1 : 0, se.ss);
}
void sweep_log_map_launch(hipStream_t st, Sess se, vloam_sweep_record* rows, int frame, SweepLogScratch* scratch, const MapState* ms, const MapFrame* fr,
                          const LMRecord* rec, bool skip_frame, ProfHook* ph, hipEvent_t done) {
  VLOAM_LAUNCH_EV(ph, kKSweepLogMap, st, done, k_sweep_log_map, dim3(1, 1, se.B), dim3(64), 0, st, rows, frame, scratch, ms, fr, rec, skip_frame ? 1 : 0, se.ss);
}
hipError_t sweep_log_init(hipStream_t st, vloam_sweep_record* rows, int n_rows) {
  VL_RAW_LAUNCH(k_sweep_log_init, dim3((n_rows + 63) / 64), dim3(64), 0, st, rows, n_rows);
  return hipGetLastError();
}

}  // namespace vloam
