// Per-sweep pose covariance rows: the kernels that write vloam_pose_cov_record rows (pose_cov.h).  gfx950, wave64.
//   k_pose_cov_lo / k_pose_cov_map   one wavefront per session, directly behind k_pose_info_lo / k_pose_info_map of the same sweep on the same stream:
//            reads the H, cost, counts and valid bit of the pose information row, decomposes H and writes eig, V, rank, sigma2 and cov.
//   k_pose_cov_vo   behind the VO solve of a coupled frame.  reduce: every workgroup walks its share of the VO stage's FactorTable BY SLOT (type, p, A),
//            evaluates CostFunctor32 / CostFunctor22 at the returned (angle-axis, t) with forward-mode duals (what ceres::AutoDiffCostFunction
//            computes) and accumulates rho' J^T J (upper triangle), 0.5 rho and the two block counts in f64 registers; lanes are added by cross-lane
//            shuffles, wavefronts through LDS in wavefront order, ONE partial per workgroup goes to HBM.  finish: the workgroup that draws the last
//            integer ticket adds the partials in workgroup order (no floating-point atomics anywhere) and decomposes like the other two.
// The decomposition is a cyclic Jacobi in f64 on ONE wavefront in the round-robin ordering of pose_info.hip: lane 6 r + c holds element (r, c) of
// the matrix and of the accumulated rotations V in registers, neighbours are fetched by cross-lane shuffles, and the three disjoint rotations of
// a step are applied to all 36 elements at once (A <- J^T A J in one pass of four products per element, V <- V J) — five dependent steps per
// sweep instead of the fifteen rotations' worth of work one lane does there.  Same stopping rule.
// The sums, their reduction and ticket, the Huber weight, the rotation and the rows' init are pose_rows_dev.h's, one text with pose_info.hip.  This
// unit keeps its OWN text of the two VO functors, for the reason pose_info.hip and map_grow.hip keep theirs: the code objects of
// the solver and of the sweep kernels stay what they are.
#include "pose_cov.h"
#include "pose_rows_dev.h"

namespace vloam {

static_assert(sizeof(vloam_pose_cov_record) == 2288 && offsetof(vloam_pose_cov_record, sigma2) == 32 && offsetof(vloam_pose_cov_record, lo_eig) == 64 &&
                  offsetof(vloam_pose_cov_record, map_eig) == 688 && offsetof(vloam_pose_cov_record, vo_x) == 1312 &&
                  offsetof(vloam_pose_cov_record, vo_eig) == 1664,
              "8 ints, 4 doubles, two halves of 78 doubles (eig[6], V[36], cov[36], contiguous), the VO half of 122");
static_assert(sizeof(PoseCovScratch) == 64 + sizeof(double) * kPcMaxBlocks * kPoseAcc && offsetof(PoseCovScratch, part) == 64,
              "the partials on a line of their own behind the ticket");

// ---------------------------------------------------------------------------------------------- lane-parallel Jacobi
// the partner of every index in the five steps of the round robin over six indices, 3 bits each:
// (0,5)(1,4)(2,3) | (0,4)(3,5)(1,2) | (0,3)(2,4)(1,5) | (0,2)(1,3)(4,5) | (0,1)(2,5)(3,4)
constexpr unsigned pc_pack(unsigned a, unsigned b, unsigned c, unsigned d, unsigned e, unsigned f) {
  return a | (b << 3) | (c << 6) | (d << 9) | (e << 12) | (f << 15);
}
__device__ __forceinline__ unsigned pc_partners(int step) {
  switch (step) {
    case 0: return pc_pack(5, 4, 3, 2, 1, 0);
    case 1: return pc_pack(4, 2, 1, 5, 0, 3);
    case 2: return pc_pack(3, 5, 4, 0, 2, 1);
    case 3: return pc_pack(2, 3, 0, 1, 5, 4);
    default: return pc_pack(1, 0, 5, 4, 3, 2);
  }
}
__device__ __forceinline__ double pc_wave_max(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = fmax(v, __shfl_xor(v, d));
  return v;
}

// One full wavefront.  Lane l < 36 holds a = A[r][c] and v = V[r][c], r = l / 6, c = l % 6 (lanes 36 .. 63 shadow lane 35).  In: a = the symmetric
// matrix, v = the identity.  Out: a's diagonal lanes hold the eigenvalues, v the eigenvectors by column, in the order the iteration left them.
// A lane below the diagonal computes its element exactly as its mirror lane does, so A stays bitwise symmetric.
__device__ __forceinline__ void pc_jacobi6(double& a, double& v, int r, int c) {
  const int ar = r < c ? r : c, ac = r < c ? c : r;   // the element of the upper triangle this lane's a mirrors
  for (int sweep = 0; sweep < 30; sweep++) {
    // converged when every off-diagonal element is below half an ulp of the largest diagonal element (pose_info.hip); a NaN runs into the cap
    const double off = pc_wave_max(r != c ? fabs(a) : 0.0), dmax = pc_wave_max(r == c ? fabs(a) : 0.0);
    if (off <= 0.5 * DBL_EPSILON * dmax) break;
#pragma unroll
    for (int step = 0; step < 5; step++) {
      const unsigned tab = pc_partners(step);
      const int rp = (int)((tab >> (3 * ar)) & 7u), cp = (int)((tab >> (3 * ac)) & 7u), vp = (int)((tab >> (3 * c)) & 7u);
      // the rotations of the row index's pair and of the column index's pair, from the elements as they are before the step
      const int rP = ar < rp ? ar : rp, rQ = ar < rp ? rp : ar, cP = ac < cp ? ac : cp, cQ = ac < cp ? cp : ac;
      const PoseRot Rr = pose_rot(__shfl(a, rP * 7), __shfl(a, rQ * 7), __shfl(a, rP * 6 + rQ));
      const PoseRot Rc = pose_rot(__shfl(a, cP * 7), __shfl(a, cQ * 7), __shfl(a, cP * 6 + cQ));
      const double sr = ar < rp ? -Rr.s : Rr.s, sc = ac < cp ? -Rc.s : Rc.s;   // J[rp][ar], J[cp][ac]
      // A'[r][c] = sum over i in {r, r'}, j in {c, c'} of J[i][r] A[i][j] J[j][c]
      const double a_rcp = __shfl(a, ar * 6 + cp), a_rpc = __shfl(a, rp * 6 + ac), a_rpcp = __shfl(a, rp * 6 + cp);
      const double an = Rr.c * (Rc.c * a + sc * a_rcp) + sr * (Rc.c * a_rpc + sc * a_rpcp);
      // V'[r][c] = V[r][c] J[c][c] + V[r][c'] J[c'][c]  (c's own pair: the same rotation as one of the two above)
      const PoseRot Rv = c == ac ? Rc : Rr;
      const double sv = c < vp ? -Rv.s : Rv.s;
      const double v_p = __shfl(v, r * 6 + vp);
      v = Rv.c * v + sv * v_p;
      a = ac == rp ? 0.0 : an;   // the rotated pair's own element
    }
  }
}

// The tail every kernel of this unit ends with; called by ALL threads of the workgroup (64 or kPcThreads), the work is wavefront 0's.
// s_H: the symmetric 6 x 6, row-major, in LDS (written before the call, a barrier in between).  out: eig[6], V[36], cov[36] of the half.
// which: 0 odometry, 1 mapping, 2 VO.  res_rows: residual rows of the problem.
__device__ __forceinline__ void pc_decompose(const double* s_H, double* s_e, double* s_V, double* out, vloam_pose_cov_record* row, int which, double cost,
                                             int res_rows, double min_eig, int tid) {
  if (tid < 64) {
    const int l = tid < 36 ? tid : 35, r = l / 6, c = l % 6;
    double a = s_H[l], v = r == c ? 1.0 : 0.0;
    pc_jacobi6(a, v, r, c);
    // ascending order: the rank of column c's eigenvalue among the six (ties by index)
    const double ec = __shfl(a, c * 7);
    int pos = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) {
      const double ej = __shfl(a, j * 7);
      pos += (ej < ec || (ej == ec && j < c)) ? 1 : 0;
    }
    // sign: the component of largest magnitude of the column is positive, ties go to the lowest row
    double big = __shfl(v, c);
#pragma unroll
    for (int j = 1; j < 6; j++) {
      const double vj = __shfl(v, j * 6 + c);
      if (fabs(vj) > fabs(big)) big = vj;
    }
    if (tid < 36) {
      s_V[r * 6 + pos] = big < 0.0 ? -v : v;
      if (r == 0) s_e[pos] = ec;
    }
  }
  __syncthreads();
  if (tid < 64) {
    const double lmax = s_e[5];
    const double floor_ = fmax(min_eig, 1e-12 * lmax);
    int rank = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) rank += (s_e[i] >= floor_ && s_e[i] > 0.0) ? 1 : 0;
    const int dof = res_rows - rank;
    const double sigma2 = dof > 0 ? 2.0 * cost / (double)dof : 0.0;
    if (tid < 6) out[tid] = s_e[tid];
    if (tid < 36) {
      const int r = tid / 6, c = tid % 6;
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < 6; i++)
        if (s_e[i] >= floor_ && s_e[i] > 0.0) s += s_V[r * 6 + i] * s_V[c * 6 + i] / s_e[i];
      out[6 + tid] = s_V[tid];
      out[42 + tid] = dof > 0 ? sigma2 * s : 0.0;
    }
    if (tid == 0) {
      row->rank[which] = rank;
      row->sigma2[which] = sigma2;
      const int flags = (dof > 0 ? (VLOAM_POSE_COV_LO_VALID << which) : 0) | (rank < 6 ? (VLOAM_POSE_COV_LO_TRUNCATED << which) : 0);
      if (flags) atomicOr(&row->flags, flags);   // the stages share the word
    }
  }
}

// ---------------------------------------------------------------------------------------------- the LiDAR halves
__device__ __forceinline__ void pose_cov_body(const vloam_pose_info_record* __restrict__ info_rows, vloam_pose_cov_record* rows, int max_frames, int frame,
                                              int stage, int stamp, double min_eig) {
  const int z = (int)blockIdx.z, tid = threadIdx.x;
  const vloam_pose_info_record* info = info_rows + (size_t)z * (size_t)max_frames + frame;
  vloam_pose_cov_record* row = rows + (size_t)z * (size_t)max_frames + frame;
  __shared__ double s_H[36], s_e[6], s_V[36];
  // the valid bit k_pose_info_* set on this stream in front of this launch (the other stage's stream may be setting its own bit meanwhile)
  const int info_flags = __hip_atomic_load(&info->flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int on = info_flags & (stage ? VLOAM_POSE_INFO_MAP_VALID : VLOAM_POSE_INFO_LO_VALID);
  if (on) {   // (uniform over the workgroup)
    const double* H = stage ? info->map_H : info->lo_H;
    const int* cnt = stage ? info->map_factors : info->lo_factors;
    if (tid < 36) s_H[tid] = H[tid];
    __syncthreads();
    pc_decompose(s_H, s_e, s_V, stage ? row->map_eig : row->lo_eig, row, stage, stage ? info->map_cost : info->lo_cost, 3 * cnt[0] + cnt[1], min_eig, tid);
  }
  // (an invalid half stays what pose_cov_init left: zero)
  if (stamp && tid == 0) row->frame = frame;
}

#define POSE_COV_ARGS const vloam_pose_info_record* info_rows, vloam_pose_cov_record* rows, int max_frames, int frame, int stamp, double min_eig
__global__ __launch_bounds__(64) void k_pose_cov_lo(POSE_COV_ARGS) { pose_cov_body(info_rows, rows, max_frames, frame, 0, stamp, min_eig); }
__global__ __launch_bounds__(64) void k_pose_cov_map(POSE_COV_ARGS) { pose_cov_body(info_rows, rows, max_frames, frame, 1, stamp, min_eig); }
#undef POSE_COV_ARGS

// ---------------------------------------------------------------------------------------------- the VO half
// forward-mode dual number with the 6 partials of (angle-axis, t)
struct PcDual { double a, v[6]; };
__device__ __forceinline__ PcDual pc_const(double a) { PcDual r; r.a = a; for (int i = 0; i < 6; i++) r.v[i] = 0.0; return r; }
__device__ __forceinline__ PcDual pc_var(double a, int k) { PcDual r = pc_const(a); r.v[k] = 1.0; return r; }
__device__ __forceinline__ PcDual operator+(PcDual f, PcDual g) { PcDual r; r.a = f.a + g.a; for (int i = 0; i < 6; i++) r.v[i] = f.v[i] + g.v[i]; return r; }
__device__ __forceinline__ PcDual operator-(PcDual f, PcDual g) { PcDual r; r.a = f.a - g.a; for (int i = 0; i < 6; i++) r.v[i] = f.v[i] - g.v[i]; return r; }
__device__ __forceinline__ PcDual operator*(PcDual f, PcDual g) { PcDual r; r.a = f.a * g.a; for (int i = 0; i < 6; i++) r.v[i] = f.a * g.v[i] + f.v[i] * g.a; return r; }
__device__ __forceinline__ PcDual operator*(PcDual f, double g) { PcDual r; r.a = f.a * g; for (int i = 0; i < 6; i++) r.v[i] = f.v[i] * g; return r; }
// ceres::AngleAxisRotatePoint (ceres/rotation.h) of a constant point
__device__ __forceinline__ void pc_rotate(const PcDual (&w_)[3], const double (&pt)[3], PcDual (&out)[3]) {
  const PcDual theta2 = w_[0] * w_[0] + w_[1] * w_[1] + w_[2] * w_[2];
  if (theta2.a > DBL_EPSILON) {
    PcDual theta, ti, ct, st;
    theta.a = sqrt(theta2.a);
    ti.a = 1.0 / theta.a;
    ct.a = cos(theta.a); st.a = sin(theta.a);
    for (int i = 0; i < 6; i++) {
      theta.v[i] = theta2.v[i] / (2.0 * theta.a);
      ti.v[i] = -theta.v[i] * ti.a * ti.a;
      ct.v[i] = -st.a * theta.v[i];
      st.v[i] = ct.a * theta.v[i];
    }
    const PcDual w[3] = {w_[0] * ti, w_[1] * ti, w_[2] * ti};
    const PcDual wxp[3] = {w[1] * pt[2] - w[2] * pt[1], w[2] * pt[0] - w[0] * pt[2], w[0] * pt[1] - w[1] * pt[0]};
    const PcDual tmp = (w[0] * pt[0] + w[1] * pt[1] + w[2] * pt[2]) * (pc_const(1.0) - ct);
    for (int k = 0; k < 3; k++) out[k] = ct * pt[k] + wxp[k] * st + w[k] * tmp;
  } else {   // first-order Taylor expansion near zero
    const PcDual wxp[3] = {w_[1] * pt[2] - w_[2] * pt[1], w_[2] * pt[0] - w_[0] * pt[2], w_[0] * pt[1] - w_[1] * pt[0]};
    for (int k = 0; k < 3; k++) out[k] = pc_const(pt[k]) + wxp[k];
  }
}

__global__ __launch_bounds__(kPcThreads) void k_pose_cov_vo(const int* __restrict__ type, const double* __restrict__ p, const double* __restrict__ A, int cap,
                                                            const double* __restrict__ x_, vloam_pose_cov_record* rows, PoseCovScratch* scratch,
                                                            int max_frames, int frame, double min_eig, size_t ss) {
  VL_SESSION(ss); RB(type); RB(p); RB(A); RB(x_);
  // rows and scratch are not in the arenas: indexed by the session, not rebased
  const int z = (int)blockIdx.z, G = (int)gridDim.x, wg = (int)blockIdx.x, tid = threadIdx.x;
  vloam_pose_cov_record* row = rows + (size_t)z * (size_t)max_frames + frame;
  PoseCovScratch* sc = scratch + z;
  __shared__ double s_tot[kPoseAcc];
  __shared__ double s_H[36], s_e[6], s_V[36];
  double x[6];
#pragma unroll
  for (int i = 0; i < 6; i++) x[i] = x_[i];
  // an estimate the reference cannot turn into a transform (zero angle: it divides by it, visual_odometry.cpp:427-430) or that is not finite:
  // the half stays zero, VO_VALID clear.  Uniform over the launch: every workgroup leaves before the ticket
  const double angle = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
  if (!(angle > 0.0) || !(angle <= DBL_MAX) || !(fabs(x[3]) <= DBL_MAX) || !(fabs(x[4]) <= DBL_MAX) || !(fabs(x[5]) <= DBL_MAX)) return;
  double acc[kPoseAcc];
#pragma unroll
  for (int i = 0; i < kPoseAcc; i++) acc[i] = 0.0;
  const PcDual w[3] = {pc_var(x[0], 0), pc_var(x[1], 1), pc_var(x[2], 2)};
  const PcDual t[3] = {pc_var(x[3], 3), pc_var(x[4], 4), pc_var(x[5], 5)};
  const double huber_a = 0.1;
  for (int slot = wg * kPcThreads + tid; slot < cap; slot += G * kPcThreads) {
    const int ty = type[slot];
    if (ty != 4 && ty != 5) continue;
    const double ox = A[slot], oy = A[cap + slot];   // x1_bar, y1_bar
    if (ty == 4) {
      // CostFunctor32 (ceres_cost_function.h:68-85): X1 = R X0 + t; r = (X1.x - X1.z x1_bar, X1.y - X1.z y1_bar)
      const double X0[3] = {p[slot], p[cap + slot], p[2 * cap + slot]};
      PcDual X1[3];
      pc_rotate(w, X0, X1);
      for (int k = 0; k < 3; k++) X1[k] = X1[k] + t[k];
      const PcDual q0 = X1[0] - X1[2] * ox, q1 = X1[1] - X1[2] * oy;
      const double wt = pose_huber(q0.a * q0.a + q1.a * q1.a, huber_a, &acc[0]);
      pose_add_row(acc, q0.v, wt);
      pose_add_row(acc, q1.v, wt);
      acc[22] += 1.0;
    } else {
      // CostFunctor22 (:159-174): r = (x1_bar, y1_bar, 1) . (t x R (x0_bar, y0_bar, 1))
      const double X0[3] = {p[slot], p[cap + slot], 1.0};
      PcDual RX[3];
      pc_rotate(w, X0, RX);
      const PcDual c0 = t[1] * RX[2] - t[2] * RX[1], c1 = t[2] * RX[0] - t[0] * RX[2], c2 = t[0] * RX[1] - t[1] * RX[0];
      const PcDual q0 = c0 * ox + c1 * oy + c2;
      const double wt = pose_huber(q0.a * q0.a, huber_a, &acc[0]);
      pose_add_row(acc, q0.v, wt);
      acc[23] += 1.0;
    }
  }
  if (!pose_rows_reduce<kPcThreads>(acc, sc, s_tot)) return;   // the workgroup with the last ticket finishes the half
  if (tid < 36) {   // mirror the upper triangle
    const double v = pose_rows_H(s_tot, tid);
    s_H[tid] = v;
    row->vo_H[tid] = v;
  }
  if (tid < 6) row->vo_x[tid] = x[tid];
  if (tid == 0) {
    row->vo_cost = s_tot[0];
    row->vo_factors[0] = (int)s_tot[22];
    row->vo_factors[1] = (int)s_tot[23];
  }
  __syncthreads();
  pc_decompose(s_H, s_e, s_V, row->vo_eig, row, 2, s_tot[0], 2 * (int)s_tot[22] + (int)s_tot[23], min_eig, tid);
}

size_t pose_cov_scratch_bytes(int n_sessions) { return sizeof(PoseCovScratch) * (size_t)n_sessions; }
hipError_t pose_cov_init(hipStream_t st, const PoseCov& P, int n_sessions) {
  return pose_rows_init(st, P.rows, (long long)P.max_frames * n_sessions, P.scratch, pose_cov_scratch_bytes(n_sessions));
}

// (the kernels of this unit carry no id of the per-kernel event timer: its table ends with k_pose_info_map, and the pose information launch in
// front keeps the stage's event when this product is off)
void pose_cov_launch(hipStream_t st, Sess se, const PoseCov& P, const vloam_pose_info_record* info_rows, int stage, int frame, bool stamp, hipEvent_t done) {
  const dim3 grid(1, 1, se.B);
  if (stage == 0)
    VLOAM_LAUNCH_EV((ProfHook*)nullptr, kKNone, st, done, k_pose_cov_lo, grid, dim3(64), 0, st, info_rows, P.rows, P.max_frames, frame, stamp ? 1 : 0, P.min_eig[0]);
  else
    VLOAM_LAUNCH_EV((ProfHook*)nullptr, kKNone, st, done, k_pose_cov_map, grid, dim3(64), 0, st, info_rows, P.rows, P.max_frames, frame, stamp ? 1 : 0, P.min_eig[1]);
}

void pose_cov_vo_launch(hipStream_t st, Sess se, const PoseCov& P, int frame, const FactorTable& F, const double* x) {
  const dim3 grid(pose_cov_vo_blocks(F.cap), 1, se.B);
  VL_RAW_LAUNCH(k_pose_cov_vo, grid, dim3(kPcThreads), 0, st, F.type, F.p, F.A, F.cap, x, P.rows, P.scratch, P.max_frames, frame, P.min_eig[2], se.ss);
}

}  // namespace vloam
