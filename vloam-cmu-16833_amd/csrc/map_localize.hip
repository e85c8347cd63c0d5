// Localisation on gfx950: a dry run of the mapping chain against the persistent map (vloam_map_localize / vloam_map_localize_device).
// A code object of its own, like map_query.hip: a handle that never localises launches nothing of this, and no kernel of a sweep changes.
// The chain (map_localize_enqueue, map_kernels.hip) is the sweep's own — the scan-feature VoxelGrid for foreign clouds, then two rounds of
// k_map_assoc, k_map_fit and the LM solve, same template arguments and grids — but every pointer to per-sweep state names the SCRATCH
// (MapLocalize, map_kernels.h).  The voxel tables and the live cube counters are only read.  There is no k_map_insert and no k_map_finalize.
//   k_map_loc_prepare  1 WG   scratch MapState = the live one; the guess (LM:182-195, or the caller's); centre cube and the six window-shift
//                             loops (LM:207-402) into the scratch centre offsets; the valid block's point counts through the shifted index
//                             (LM:404-430: cubes a roll would bring in count 0); the gate (LM:448)
//   k_map_loc_finish   1 WG   packs vloam_localize_result from the scratch state, counters and solve records
// What k_map_prepare does and this does NOT: merge newraw into deferred, bump sweep_no, consume StackInfo::error, write the live MapFrame,
// host flags, a trajectory row or a time stamp.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "map_kernels.h"
#include "map_device.h"

namespace vloam {

struct LocPose { double v[7]; };   // (q xyzw, t) by value: the host's pose needs no upload

__global__ __launch_bounds__(256) void k_map_loc_prepare(const MapState* __restrict__ live_ms, const MapFrame* __restrict__ live_fr,
                                                         const int* __restrict__ cube_cnt, const StackInfo* __restrict__ si,
                                                         const double* __restrict__ row7, LocPose pose, int pose_frame, MapState* ms, MapFrame* fr,
                                                         LocAux* aux) {
  __shared__ int s_shift[3], s_cen[3];
  const int tid = threadIdx.x;
  if (tid == 0) {
    MapState s = *live_ms;
    double row[7];
    for (int k = 0; k < 7; k++) row[k] = row7 ? row7[k] : pose.v[k];
    double q[4], t[3];
    if (pose_frame == 0) {
      // LaserMapping::input LM:182-195, as k_map_prepare: q_w_curr = q_wmap_wodom * q_wodom_curr, t_w_curr = q_wmap_wodom * t_wodom_curr + t_wmap_wodom
      for (int k = 0; k < 4; k++) s.q_wodom_curr[k] = row[k];
      for (int k = 0; k < 3; k++) s.t_wodom_curr[k] = row[4 + k];
      dquat_mul(s.q_wmap_wodom, row, q);
      dquat_rot(s.q_wmap_wodom, row + 4, t);
      for (int k = 0; k < 3; k++) t[k] = t[k] + s.t_wmap_wodom[k];
    } else {
      for (int k = 0; k < 4; k++) q[k] = row[k];
      for (int k = 0; k < 3; k++) t[k] = row[4 + k];
    }
    for (int k = 0; k < 4; k++) { s.parameters[k] = q[k]; aux->guess[k] = q[k]; }
    for (int k = 0; k < 3; k++) { s.parameters[4 + k] = t[k]; aux->guess[4 + k] = t[k]; }
    // LM:207-216, LM:218-402: the six while loops, on the scratch centre offsets only
    int cen[3] = {s.cenW, s.cenH, s.cenD}, shift[3] = {0, 0, 0};
    int cI = cube_abs(t[0]) + cen[0], cJ = cube_abs(t[1]) + cen[1], cK = cube_abs(t[2]) + cen[2];
    while (cI < 3) { cI++; cen[0]++; shift[0]++; }
    while (cI >= kCubeW - 3) { cI--; cen[0]--; shift[0]--; }
    while (cJ < 3) { cJ++; cen[1]++; shift[1]++; }
    while (cJ >= kCubeH - 3) { cJ--; cen[1]--; shift[1]--; }
    while (cK < 3) { cK++; cen[2]++; shift[2]++; }
    while (cK >= kCubeD - 3) { cK--; cen[2]--; shift[2]--; }
    s.centerCube[0] = cI; s.centerCube[1] = cJ; s.centerCube[2] = cK;
    s.cenW = cen[0]; s.cenH = cen[1]; s.cenD = cen[2];
    for (int k = 0; k < 3; k++) { s_shift[k] = shift[k]; aux->shift[k] = shift[k]; }
    s_cen[0] = cI; s_cen[1] = cJ; s_cen[2] = cK;
    // the stack: the mapping would not take it with a full table or a VoxelGrid that timed out (k_map_prepare); the live words are only read
    int nst[2] = {si->n_stack[0], si->n_stack[1]};
    const int si_err = si->error;
    if ((live_fr->error | si_err) & (kErrMapFull | kErrSolverSync)) nst[0] = nst[1] = 0;
    aux->si_error = si_err;
    s.n_corner_stack = nst[0]; s.n_surf_stack = nst[1];
    s.do_optimize = 0; s.n_map_corner = 0; s.n_map_surf = 0;
    *ms = s;
    MapFrame f;
    memset(&f, 0, sizeof(f));
    f.n_stack[0] = nst[0]; f.n_stack[1] = nst[1];
    f.rolled = (shift[0] | shift[1] | shift[2]) ? 1 : 0;
    *fr = f;
  }
  __syncthreads();
  // LM:404-430,448: points in the valid 5x5x3 block; cube (i, j, k) of the shifted window is cube (i, j, k) - shift of the live counters
  if (tid < 64) {
    int s0 = 0, s1 = 0;
    for (int c = tid; c < 75; c += 64) {
      const int i = s_cen[0] - 2 + c / 15, j = s_cen[1] - 2 + (c / 3) % 5, k = s_cen[2] - 1 + c % 3;
      if (i >= 0 && i < kCubeW && j >= 0 && j < kCubeH && k >= 0 && k < kCubeD) {
        const int oi = i - s_shift[0], oj = j - s_shift[1], ok = k - s_shift[2];
        if (oi >= 0 && oi < kCubeW && oj >= 0 && oj < kCubeH && ok >= 0 && ok < kCubeD) {
          const int ci = oi + kCubeW * oj + kCubeW * kCubeH * ok;
          s0 += cube_cnt[ci]; s1 += cube_cnt[kCubeNum + ci];
        }
      }
    }
    for (int d = 32; d > 0; d >>= 1) { s0 += __shfl_xor(s0, d); s1 += __shfl_xor(s1, d); }
    if (tid == 0) {
      ms->n_map_corner = s0; ms->n_map_surf = s1;
      ms->do_optimize = (s0 > 10 && s1 > 50) ? 1 : 0;
    }
  }
}

__global__ __launch_bounds__(64) void k_map_loc_finish(const MapState* __restrict__ ms, const MapFrame* __restrict__ fr, const LocAux* __restrict__ aux,
                                                       const LMRecord* __restrict__ rec, vloam_localize_result* out) {
  if (threadIdx.x != 0) return;
  vloam_localize_result r;
  memset(&r, 0, sizeof(r));
  const int opt = ms->do_optimize;
  r.flags = (opt ? VLOAM_LOC_SOLVED : VLOAM_LOC_NOT_OPTIMIZED) | ((aux->shift[0] | aux->shift[1] | aux->shift[2]) ? VLOAM_LOC_WOULD_ROLL : 0) |
            (fr->fallback_solves > 0 ? VLOAM_LOC_DEGRADED : 0);
  r.error_bits = fr->error | aux->si_error;   // ErrorBits == VLOAM_SWEEP_* bit for bit
  for (int k = 0; k < 3; k++) r.center_cube[k] = ms->centerCube[k];
  r.n_stack[0] = ms->n_corner_stack; r.n_stack[1] = ms->n_surf_stack;
  r.n_map[0] = ms->n_map_corner; r.n_map[1] = ms->n_map_surf;
  for (int o = 0; o < 2; o++) {
    r.n_factors[o][0] = fr->n_factors[o][0]; r.n_factors[o][1] = fr->n_factors[o][1];
    if (opt) {   // (a gated solve leaves its record alone)
      r.iterations[o] = (int)rec[o].n_iterations; r.termination[o] = (int)rec[o].termination;
      r.initial_cost[o] = rec[o].initial_cost; r.final_cost[o] = rec[o].final_cost;
    }
  }
  for (int k = 0; k < 4; k++) { r.q_guess[k] = aux->guess[k]; r.q_map[k] = ms->parameters[k]; }
  for (int k = 0; k < 3; k++) { r.t_guess[k] = aux->guess[4 + k]; r.t_map[k] = ms->parameters[4 + k]; }
  *out = r;
}

void map_loc_prepare_launch(hipStream_t st, const MapContext* m, const StackInfo* si, const double* row7, const double pose7[7], int pose_frame) {
  const MapLocalize* L = m->loc;
  LocPose pose;
  for (int k = 0; k < 7; k++) pose.v[k] = pose7 ? pose7[k] : 0.0;
  VL_RAW_LAUNCH(k_map_loc_prepare, dim3(1, 1, 1), dim3(256), 0, st, m->state, m->frame, m->cube_cnt, si, row7, pose, pose_frame, L->state, L->frame, L->aux);
}

void map_loc_finish_launch(hipStream_t st, const MapContext* m, vloam_localize_result* d_result) {
  const MapLocalize* L = m->loc;
  VL_RAW_LAUNCH(k_map_loc_finish, dim3(1, 1, 1), dim3(64), 0, st, L->state, L->frame, L->aux, L->rec, d_result);
}

// One allocation, laid out by the arena helper the session arenas use (dry pass to measure), zeroed: the VoxelGrid's counters and look-back
// words start clean, as in a fresh arena.
static bool loc_layout(const MapContext* m, MapLocalize* L, Arena& A) {
  bool ok = A.take(&L->state, 1) && A.take(&L->frame, 1) && A.take(&L->aux, 1) && A.take(&L->si, 1) && A.take(&L->S, 1) && A.take(&L->result, 1) &&
            A.take(&L->in[0], (size_t)kMaxLessSharp) && A.take(&L->in[1], (size_t)m->max_points);
  for (int k = 0; k < 2 && ok; k++) {
    DsScratch& D = L->ds[k];
    D.stack_cap = k ? kStackCapSurf : kStackCapCorner;
    ok = A.take(&D.region, (size_t)kDsMaxBins * kDsBinCap) && A.take(&D.over, (size_t)m->max_points) && A.take(&D.tmp, (size_t)m->max_points) &&
         A.take(&D.sorted, (size_t)m->max_points) && A.take(&D.splitters, (size_t)kDsMaxBins) && A.take(&D.cursor, (size_t)kDsMaxBins + 4) &&
         A.take(&D.done, (size_t)kDsMaxBins) && A.take(&L->stack[k], (size_t)D.stack_cap);
    FactorTable& F = L->F[k];
    F = m->F[k];   // the handle's sync words, patience and generation rules; every array below is the scratch's own
    F.cap = kMapFactorCap;
    ok = ok && A.take(&F.type, (size_t)F.cap) && A.take(&F.p, 3 * (size_t)F.cap) && A.take(&F.A, 3 * (size_t)F.cap) && A.take(&F.B, 3 * (size_t)F.cap) &&
         A.take(&F.resid, 3 * (size_t)F.cap) && A.take(&F.ctype, (size_t)F.cap) && A.take(&F.cslot, (size_t)F.cap) && A.take(&F.cpack, 11 * (size_t)F.cap) &&
         A.take(&F.dg, 8 * (size_t)F.cap) && A.take(&F.rowcnt, (size_t)F.cap / 64 + 1) && A.take(&F.rowmask, (size_t)F.cap / 64 + 2);
    F.err = &L->frame->error;
    F.fallbacks = &L->frame->fallback_solves;
    F.host_degraded = nullptr;   // a localisation that degrades says so in its record; the handle's sweeps keep their cooperative solves
  }
  return ok && A.take(&L->rec, 2) && A.take(&L->nbr, 5 * (size_t)kMapFactorCap) && A.take(&L->cbox, 2 * (size_t)kMapFactorCap) &&
         A.take(&L->ccand, (size_t)kMapFactorCap * kCandCache);
}

vloam_status map_localize_alloc(MapContext* m, hipStream_t st) {
  if (m->loc) return VLOAM_OK;
  MapLocalize* L = new MapLocalize;
  Arena dry;
  loc_layout(m, L, dry);
  Arena A;
  A.cap = dry.off; A.dry = false;
  if (hipMalloc((void**)&L->base, A.cap) != hipSuccess) { delete L; return VLOAM_ERR_HIP; }
  A.base = L->base;
  if (!loc_layout(m, L, A) || hipMemsetAsync(L->base, 0, A.cap, st) != hipSuccess) { (void)hipFree(L->base); delete L; return VLOAM_ERR_HIP; }
  m->loc = L;
  return VLOAM_OK;
}

void map_localize_free(MapContext* m) {
  if (!m->loc) return;
  (void)hipFree(m->loc->base);
  delete m->loc;
  m->loc = nullptr;
}

}  // namespace vloam
