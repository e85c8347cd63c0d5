// k_map_prepare and k_map_fit — written once, compiled twice (map_kernels.hip includes this file two times):
//   default form   VL_MAP_TIER 0: the surf stack capacity is the constant kStackCapSurf, exactly the kernels a default handle always launched
//   large tier     VL_MAP_TIER 1: k_map_prepare_tier / k_map_fit_tier take the handle's capacity at run time (vloam_limits::max_surf_stack_points)
// A textual include instead of a template: inlining a template body perturbs the register allocation of these two kernels' default forms,
// and the default code objects are to stay register for register what they are (profiles/r07_surf_stack_tier.txt).
// The name ends in .h because the Makefile's HDRS wildcard and the content hash of csrc/ (tools/pmc_summary.py) both go by suffix.
//   VL_MAP_KERNEL(name)  the kernel's name          VL_MAP_CAP_PARAM   the trailing parameter of the tier form (or nothing)
//   VL_MAP_SURF_CAP      surf stack capacity        VL_MAP_FACTOR_CAP  slots of the factor table: 8 192 corner + the surf capacity

__global__ __launch_bounds__(256) void VL_MAP_KERNEL(k_map_prepare)(MapState* ms, MapFrame* fr, const LOState* lo, int* cube_cnt, int skip_frame,
                                                     double* traj_row14, StackInfo* si, int* deferred0, int* deferred1, const int* newraw0,
                                                     const int* newraw1, long long* ts_log, size_t ss VL_MAP_CAP_PARAM) {
  VL_SESSION(ss); RB(ms); RB(fr); RB(lo); RB(cube_cnt); RB(traj_row14); RB(si); RB(deferred0); RB(deferred1); RB(newraw0); RB(newraw1); RB(ts_log);
  const long long ts_begin = ts_log ? (long long)wall_clock64() : 0;
  __shared__ int shift[3], s_cen[3];
  const int tid = threadIdx.x;
  // Every load that does not depend on another one is issued up front (one memory round trip for the lot): this launch is a single
  // workgroup at the head of the stream that bounds the throughput, and each dependent trip costs ~1 us there.
  const int nn0 = min(fr->n_newraw[0], kStackCapCorner), nn1 = min(fr->n_newraw[1], VL_MAP_SURF_CAP);
  const int nd0 = fr->n_deferred[0], nd1 = fr->n_deferred[1];
  double row[7], qmw[4], tmw[3];
  int cen[3] = {0, 0, 0}, nst[2] = {0, 0}, si_err = 0, fr_err = 0, sweep_no = 0;
  if (tid == 0) {
    // the odometry pose of THIS sweep as k_lo_finish logged it (the live LOState may already belong to the next sweep: the
    // odometry stream runs ahead of the mapping stream)
    (void)lo;
    for (int k = 0; k < 7; k++) row[k] = traj_row14[k];
    for (int k = 0; k < 4; k++) qmw[k] = ms->q_wmap_wodom[k];
    for (int k = 0; k < 3; k++) tmw[k] = ms->t_wmap_wodom[k];
    cen[0] = ms->cenW; cen[1] = ms->cenH; cen[2] = ms->cenD;
    nst[0] = si->n_stack[0]; nst[1] = si->n_stack[1];
    si_err = si->error; fr_err = fr->error; sweep_no = ms->sweep_no;
  }
  // voxels that turned raw in the previous sweep join the list of raw voxels (k_map_finalize could not append to the list it compacts)
  if (nn0 > 0) for (int e = tid; e < nn0; e += 256) { if (nd0 + e < kStackCapCorner) deferred0[nd0 + e] = newraw0[e]; }
  if (nn1 > 0) for (int e = tid; e < nn1; e += 256) { if (nd1 + e < VL_MAP_SURF_CAP) deferred1[nd1 + e] = newraw1[e]; }
  // every wavefront holds its copy of the four counters (and has issued its share of the merge) before thread 0 rewrites them below:
  // the barrier's fence completes the loads above, so a wavefront that starts late can neither see the zeroed n_newraw nor the bumped n_deferred
  __syncthreads();
  if (tid == 0) {
    if (nd0 + nn0 > kStackCapCorner || nd1 + nn1 > VL_MAP_SURF_CAP) { atomicOr(&fr->error, kErrMapFull); fr_err |= kErrMapFull; }
    if (nn0 | nn1) {
      fr->n_deferred[0] = min(nd0 + nn0, kStackCapCorner); fr->n_deferred[1] = min(nd1 + nn1, VL_MAP_SURF_CAP);
      fr->n_newraw[0] = 0; fr->n_newraw[1] = 0;
    }
    // LaserMapping::input LM:182-195: q_w_curr = q_wmap_wodom * q_wodom_curr, t_w_curr = q_wmap_wodom * t_wodom_curr + t_wmap_wodom
    for (int k = 0; k < 4; k++) ms->q_wodom_curr[k] = row[k];
    for (int k = 0; k < 3; k++) ms->t_wodom_curr[k] = row[4 + k];
    double q[4], t[3];
    dquat_mul(qmw, row, q);
    dquat_rot(qmw, row + 4, t);
    for (int k = 0; k < 3; k++) t[k] = t[k] + tmw[k];
    shift[0] = shift[1] = shift[2] = 0;
    int rolled = 0;
    if (skip_frame) {  // only the high-frequency pose is produced (LM:186-190)
      if (traj_row14) { for (int k = 0; k < 4; k++) traj_row14[7 + k] = q[k]; for (int k = 0; k < 3; k++) traj_row14[11 + k] = t[k]; }
    } else {
      for (int k = 0; k < 4; k++) ms->parameters[k] = q[k];
      for (int k = 0; k < 3; k++) ms->parameters[4 + k] = t[k];
      // LM:207-216
      int cI = cube_abs(t[0]) + cen[0], cJ = cube_abs(t[1]) + cen[1], cK = cube_abs(t[2]) + cen[2];
      // LM:218-402: the six while loops only move cube pointers and the centre offsets
      while (cI < 3) { cI++; cen[0]++; shift[0]++; }
      while (cI >= kCubeW - 3) { cI--; cen[0]--; shift[0]--; }
      while (cJ < 3) { cJ++; cen[1]++; shift[1]++; }
      while (cJ >= kCubeH - 3) { cJ--; cen[1]--; shift[1]--; }
      while (cK < 3) { cK++; cen[2]++; shift[2]++; }
      while (cK >= kCubeD - 3) { cK--; cen[2]--; shift[2]--; }
      ms->centerCube[0] = cI; ms->centerCube[1] = cJ; ms->centerCube[2] = cK;
      s_cen[0] = cI; s_cen[1] = cJ; s_cen[2] = cK;
      if (shift[0] | shift[1] | shift[2]) { rolled = 1; ms->cenW = cen[0]; ms->cenH = cen[1]; ms->cenD = cen[2]; }
      // the scan features were voxelised on the scan-registration stream (k_map_ds_*): adopt this sweep's stack
      if (si_err) { atomicOr(&fr->error, si_err); fr_err |= si_err; si->error = 0; }
      if (fr_err & (kErrMapFull | kErrSolverSync)) nst[0] = nst[1] = 0;  // the map cannot take this sweep (table full), or its stack has holes (a bin of the scan-feature VoxelGrid timed out): no association, no insert; the pose stays the odometry guess (vloam_sync reports it)
      for (int k = 0; k < 2; k++) { fr->n_stack[k] = nst[k]; fr->n_touched[k] = 0; }
      ms->n_corner_stack = nst[0]; ms->n_surf_stack = nst[1];
      for (int k = 0; k < 4; k++) (&fr->n_factors[0][0])[k] = 0;
      ms->sweep_no = sweep_no + 1;
      if (ts_log) ts_log[2 * (sweep_no & 1023)] = ts_begin;
    }
    fr->rolled = rolled;
  }
  __syncthreads();
  if (skip_frame) return;
  // shift the per-cube point counters exactly like the reference shifts its cube arrays (cleared slabs -> 0)
  if (shift[0] | shift[1] | shift[2]) {
    for (int kind = 0; kind < 2; kind++) {
      int* cnt = cube_cnt + kind * kCubeNum;
      // gather-with-offset through registers: new[i][j][k] = old[i - sx][j - sy][k - sz] or 0
      int vals[(kCubeNum + 255) / 256];
      int n = 0;
      for (int c = tid; c < kCubeNum; c += 256, n++) {
        const int i = c % kCubeW, j = (c / kCubeW) % kCubeH, k = c / (kCubeW * kCubeH);
        const int si = i - shift[0], sj = j - shift[1], sk = k - shift[2];
        vals[n] = (si >= 0 && si < kCubeW && sj >= 0 && sj < kCubeH && sk >= 0 && sk < kCubeD) ? cnt[si + kCubeW * sj + kCubeW * kCubeH * sk] : 0;
      }
      __syncthreads();
      n = 0;
      for (int c = tid; c < kCubeNum; c += 256, n++) cnt[c] = vals[n];
      __syncthreads();
    }
  }
  // LM:404-430,448: points in the valid 5x5x3 block decide whether the optimisation runs
  if (tid < 64) {
    int s0 = 0, s1 = 0;
    for (int c = tid; c < 75; c += 64) {
      const int i = s_cen[0] - 2 + c / 15, j = s_cen[1] - 2 + (c / 3) % 5, k = s_cen[2] - 1 + c % 3;
      if (i >= 0 && i < kCubeW && j >= 0 && j < kCubeH && k >= 0 && k < kCubeD) {
        const int ci = i + kCubeW * j + kCubeW * kCubeH * k;
        s0 += cube_cnt[ci]; s1 += cube_cnt[kCubeNum + ci];
      }
    }
    for (int d = 32; d > 0; d >>= 1) { s0 += __shfl_xor(s0, d); s1 += __shfl_xor(s1, d); }
    if (tid == 0) {
      ms->n_map_corner = s0; ms->n_map_surf = s1;
      ms->do_optimize = (s0 > 10 && s1 > 50) ? 1 : 0;
    }
  }
}

__global__ __launch_bounds__(256) void VL_MAP_KERNEL(k_map_fit)(const float4* __restrict__ stack0, const float4* __restrict__ stack1, VoxelTable T0,
                                                 VoxelTable T1, const MapState* __restrict__ ms, MapFrame* fr, const float4* __restrict__ nbr,
                                                 FactorTable F, int outer, size_t ss) {
  VL_SESSION(ss); RB(stack0); RB(stack1); RB(ms); RB(fr); RB(nbr); F.rebase(so_);
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= VL_MAP_FACTOR_CAP) return;
  const int kind = slot < kStackCapCorner ? 0 : 1;
  const int i = kind ? slot - kStackCapCorner : slot;
  const int nst = kind ? ms->n_surf_stack : ms->n_corner_stack;
  int type = 0;
  (void)T0; (void)T1;
  if (ms->do_optimize && i < nst && nbr[slot * 5].w != 0.0f) {
    const float4 pointOri = kind ? stack1[i] : stack0[i];
    double P[5][3];
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const float4 p = nbr[slot * 5 + j];
      P[j][0] = p.x; P[j][1] = p.y; P[j][2] = p.z;
    }
    double A3[3] = {0, 0, 0}, B3[3] = {0, 0, 0};
    if (kind == 0) {  // LM:481-517
      double center[3] = {0, 0, 0};
#pragma unroll
      for (int j = 0; j < 5; j++) for (int a = 0; a < 3; a++) center[a] = center[a] + P[j][a];
      for (int a = 0; a < 3; a++) center[a] = center[a] / 5.0;
      double cov[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
      for (int j = 0; j < 5; j++) {
        const double z[3] = {P[j][0] - center[0], P[j][1] - center[1], P[j][2] - center[2]};
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) cov[a][b] = cov[a][b] + z[a] * z[b];
      }
      double e_mid, e_max, dir[3];
      sym_eig3_top(cov, &e_mid, &e_max, dir);
      if (e_max > 3 * e_mid) {
        for (int a = 0; a < 3; a++) { A3[a] = 0.1 * dir[a] + center[a]; B3[a] = -0.1 * dir[a] + center[a]; }
        type = 1;
      }
    } else {          // LM:545-581
      double matA0[15], matB0[5], nrm[3];
#pragma unroll
      for (int j = 0; j < 5; j++) { matA0[j * 3] = P[j][0]; matA0[j * 3 + 1] = P[j][1]; matA0[j * 3 + 2] = P[j][2]; matB0[j] = -1.0; }
      if (householder_ls_5x3(matA0, matB0, nrm)) {
        const double nn_ = sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
        const double negative_OA_dot_norm = 1 / nn_;
        nrm[0] = nrm[0] / nn_; nrm[1] = nrm[1] / nn_; nrm[2] = nrm[2] / nn_;
        bool planeValid = true;
#pragma unroll
        for (int j = 0; j < 5; j++)
          if (fabs(nrm[0] * P[j][0] + nrm[1] * P[j][1] + nrm[2] * P[j][2] + negative_OA_dot_norm) > 0.2) planeValid = false;
        if (planeValid) { A3[0] = nrm[0]; A3[1] = nrm[1]; A3[2] = nrm[2]; B3[0] = negative_OA_dot_norm; type = 3; }
      }
    }
    if (type) {
      const int cap = F.cap;
      F.p[slot] = pointOri.x; F.p[cap + slot] = pointOri.y; F.p[2 * cap + slot] = pointOri.z;
      F.A[slot] = A3[0]; F.A[cap + slot] = A3[1]; F.A[2 * cap + slot] = A3[2];
      F.B[slot] = B3[0]; F.B[cap + slot] = B3[1]; F.B[2 * cap + slot] = B3[2];
      factor_digest(F, slot, type, A3, B3);   // the solve's form of the factor, ready when the solve starts (lm_solve.hip)
    }
  }
  F.type[slot] = type;
  // a wavefront == one 64-slot row of the table: its accepted slots as one mask (every row, every launch: nothing to clear); the solve
  // compacts from the masks on its own
  const unsigned long long m = __ballot(type != 0);
  if ((threadIdx.x & 63) == 0) {
#if VL_MAP_TIER
    F.rowcnt[slot >> 6] = __popcll(m);   // a plain store (the wavefront owns the row): more than 512 rows are solved in the packed form, k_lm_compact reads the counts
#else
    F.rowmask[slot >> 6] = m;
#endif
    if (m) atomicAdd(&fr->n_factors[outer][kind], __popcll(m));
  }
}

#undef VL_MAP_TIER
#undef VL_MAP_KERNEL
#undef VL_MAP_CAP_PARAM
#undef VL_MAP_SURF_CAP
#undef VL_MAP_FACTOR_CAP
