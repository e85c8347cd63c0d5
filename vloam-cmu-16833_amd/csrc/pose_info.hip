// Per-sweep pose information matrices: the kernels that write vloam_pose_info_record rows (pose_info.h).  gfx950, wave64.
// One launch per LiDAR stage and sweep, behind the stage's last solve on the stage's own stream, session in blockIdx.z (VL_SESSION).
//   reduce   every workgroup walks its share of the stage's FactorTable BY SLOT (type, p and the digest the solve itself consumed: FactorTable::dg),
//            evaluates the accepted factors at LMRecord::x_out with closed-form Jacobians in the tangent space of
//            EigenQuaternionParameterization, and accumulates rho' J^T J (upper triangle), the cost 0.5 rho and the two block counts in f64
//            registers; lanes are added by cross-lane shuffles, wavefronts through LDS in wavefront order, and ONE partial per workgroup goes to HBM.
//   finish   the workgroup that draws the last integer ticket adds the partials in workgroup order (no floating-point atomics anywhere:
//            a row is bit-identical from run to run), mirrors the 6 x 6, runs cyclic Jacobi on it in f64 to convergence (one lane, the matrix in registers), sorts the eigenvalues,
//            sets the flags and writes its half of the row with plain vector stores.
// This unit keeps its OWN text of the three LiDAR factor evaluations (edge, plane, plane-norm at s = 1), for the reason k_map_grow keeps its own
// (DESIGN.md §8): the code objects of the solver and of the association kernels stay what they are.  The sums, their reduction and ticket, the
// Huber weight, the rotation and the rows' init are pose_rows_dev.h's, one text with pose_cov.hip.
#include "pose_info.h"
#include "pose_rows_dev.h"

namespace vloam {

static_assert(sizeof(vloam_pose_info_record) == 832 && offsetof(vloam_pose_info_record, lo_x) == 32 && offsetof(vloam_pose_info_record, map_x) == 432,
              "8 ints, then two halves of 50 doubles");
static_assert(sizeof(PoseInfoScratch) == 64 + sizeof(double) * kPiMaxBlocks * kPoseAcc && offsetof(PoseInfoScratch, part) == 64,
              "the partials on a line of their own behind the ticket");
constexpr int kPiHalf = 50;   // doubles per stage: x[7], cost, H[36], eig[6]

// Eigenvalues of the symmetric 6 x 6 A (row-major in LDS) -> d[6] ascending.  Cyclic Jacobi in the parallel (round-robin) ordering: a sweep is five
// steps of three rotations in disjoint planes, 15 pairs in all; the matrix sits in the registers of ONE lane with every index a compile-time
// constant, and the three rotations of a step are written side by side so that their dependent f64 chains (one division, two reciprocal
// square roots each) overlap.  The rotation is pose_rot (pose_rows_dev.h).  Converged when every off-diagonal element
// is below half an ulp of the largest diagonal element (the eigenvalues are then the diagonal to ~1e-16 |A|; the convergence is quadratic,
// four to six sweeps); a matrix with a NaN runs into the sweep cap.
template <int P, int Q>
__device__ __forceinline__ void pi_apply(double (&a)[6][6], PoseRot R) {
#pragma unroll
  for (int i = 0; i < 6; i++) {   // columns p, q
    const double x = a[i][P], y = a[i][Q];
    a[i][P] = R.c * x - R.s * y;
    a[i][Q] = R.s * x + R.c * y;
  }
#pragma unroll
  for (int j = 0; j < 6; j++) {   // rows p, q
    const double x = a[P][j], y = a[Q][j];
    a[P][j] = R.c * x - R.s * y;
    a[Q][j] = R.s * x + R.c * y;
  }
  a[P][Q] = 0.0; a[Q][P] = 0.0;
}
template <int P0, int Q0, int P1, int Q1, int P2, int Q2>
__device__ __forceinline__ void pi_step(double (&a)[6][6]) {
  const PoseRot R0 = pose_rot(a[P0][P0], a[Q0][Q0], a[P0][Q0]), R1 = pose_rot(a[P1][P1], a[Q1][Q1], a[P1][Q1]), R2 = pose_rot(a[P2][P2], a[Q2][Q2], a[P2][Q2]);
  pi_apply<P0, Q0>(a, R0);   // disjoint planes: the three rotations commute
  pi_apply<P1, Q1>(a, R1);
  pi_apply<P2, Q2>(a, R2);
}
__device__ __forceinline__ void pi_jacobi6(const double* A, double* d) {
  double a[6][6];
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j < 6; j++) a[i][j] = A[i * 6 + j];
  for (int sweep = 0; sweep < 30; sweep++) {
    double off = 0.0, dmax = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      dmax = fmax(dmax, fabs(a[i][i]));
#pragma unroll
      for (int j = i + 1; j < 6; j++) off = fmax(off, fmax(fabs(a[i][j]), fabs(a[j][i])));
    }
    if (off <= 0.5 * DBL_EPSILON * dmax) break;
    pi_step<0, 5, 1, 4, 2, 3>(a);   // round robin over six indices: every pair once per sweep
    pi_step<0, 4, 3, 5, 1, 2>(a);
    pi_step<0, 3, 2, 4, 1, 5>(a);
    pi_step<0, 2, 1, 3, 4, 5>(a);
    pi_step<0, 1, 2, 5, 3, 4>(a);
  }
  double e[6];
#pragma unroll
  for (int i = 0; i < 6; i++) e[i] = a[i][i];
  // ascending: an odd-even transposition network (static indices)
#pragma unroll
  for (int pass = 0; pass < 6; pass++)
#pragma unroll
    for (int i = pass & 1; i + 1 < 6; i += 2) {
      const double lo = fmin(e[i], e[i + 1]), hi = fmax(e[i], e[i + 1]);
      e[i] = lo; e[i + 1] = hi;
    }
#pragma unroll
  for (int i = 0; i < 6; i++) d[i] = e[i];
}

__device__ __forceinline__ void pose_info_body(const int* __restrict__ type, const double* __restrict__ p, const double* __restrict__ dg, int cap,
                                               const LMRecord* __restrict__ rec, const int* __restrict__ enable, int ran, vloam_pose_info_record* rows,
                                               PoseInfoScratch* scratch, int max_frames, int frame, int stage, int stamp, double min_eig, size_t ss) {
  VL_SESSION(ss); RB(type); RB(p); RB(dg); RB(rec); RB(enable);
  // rows and scratch are not in the arenas: indexed by the session, not rebased
  const int z = (int)blockIdx.z, G = (int)gridDim.x, wg = (int)blockIdx.x, tid = threadIdx.x;
  vloam_pose_info_record* row = rows + (size_t)z * (size_t)max_frames + frame;
  PoseInfoScratch* sc = scratch + (size_t)stage * gridDim.z + z;
  __shared__ double s_tot[kPoseAcc];
  __shared__ double s_half[kPiHalf];
  __shared__ double s_a[36];
  // the solve ran: the host's knowledge (first sweep, skipped sweep) and the device's gate (MapState::do_optimize).  Otherwise neither the table
  // nor the record is this sweep's, and neither is read
  const int on = (ran && (enable ? *enable : 1)) ? 1 : 0;
  double acc[kPoseAcc];
#pragma unroll
  for (int i = 0; i < kPoseAcc; i++) acc[i] = 0.0;
  if (on) {
    double x[7];
#pragma unroll
    for (int i = 0; i < 7; i++) x[i] = rec->x_out[i];
    // rotation matrix of q = (x, y, z, w) as Eigen's toRotationMatrix() builds it
    double R[9];
    {
      const double tx = 2 * x[0], ty = 2 * x[1], tz = 2 * x[2];
      const double twx = tx * x[3], twy = ty * x[3], twz = tz * x[3];
      const double txx = tx * x[0], txy = ty * x[0], txz = tz * x[0], tyy = ty * x[1], tyz = tz * x[1], tzz = tz * x[2];
      R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
      R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
      R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
    }
    const double huber_a = 0.1;
    for (int slot = wg * kPiThreads + tid; slot < cap; slot += G * kPiThreads) {
      const int ty = type[slot];
      if (ty == 0) continue;
      const double px = p[slot], py = p[cap + slot], pz = p[2 * cap + slot];
      const double rx = R[0] * px + R[1] * py + R[2] * pz, ry = R[3] * px + R[4] * py + R[5] * pz, rz = R[6] * px + R[7] * py + R[8] * pz;
      const double lx = rx + x[4], ly = ry + x[5], lz = rz + x[6];
      if (ty == 1) {
        // LidarEdgeFactor (lidarFactor.hpp:21-45): r = v x (lp - a), v the line's unit direction; in the orthonormal pair (e1, e2) across the line
        // r = c1 e2 - c2 e1 with c_i = e_i . lp + d_i (vloam_device.h: edge_frame).  |r|^2 = c1^2 + c2^2 and J^T J are those of the two rows
        // c_i: d c_i / d t = e_i, d c_i / d theta = -2 (e_i x R p)  (q+ = exp(delta) * q turns by 2 |delta|)
        double e[8];
#pragma unroll
        for (int q = 0; q < 8; q++) e[q] = dg[q * cap + slot];
        const double c1 = (e[0] * lx + e[1] * ly + e[2] * lz) + e[6], c2 = (e[3] * lx + e[4] * ly + e[5] * lz) + e[7];
        const double w = pose_huber(c1 * c1 + c2 * c2, huber_a, &acc[0]);
        const double J1[6] = {-2.0 * (e[1] * rz - e[2] * ry), -2.0 * (e[2] * rx - e[0] * rz), -2.0 * (e[0] * ry - e[1] * rx), e[0], e[1], e[2]};
        const double J2[6] = {-2.0 * (e[4] * rz - e[5] * ry), -2.0 * (e[5] * rx - e[3] * rz), -2.0 * (e[3] * ry - e[4] * rx), e[3], e[4], e[5]};
        pose_add_row(acc, J1, w);
        pose_add_row(acc, J2, w);
        acc[22] += 1.0;
      } else {
        // LidarPlaneFactor (:72-93, (lp - j) . n) and LidarPlaneNormFactor (:115-127, n . lp + negative_OA_dot_norm) in the common form
        // r = n . lp + d
        const double nx = dg[slot], ny = dg[cap + slot], nz = dg[2 * cap + slot], d = dg[3 * cap + slot];
        const double r0 = (nx * lx + ny * ly + nz * lz) + d;
        const double w = pose_huber(r0 * r0, huber_a, &acc[0]);
        const double J[6] = {-2.0 * (ny * rz - nz * ry), -2.0 * (nz * rx - nx * rz), -2.0 * (nx * ry - ny * rx), nx, ny, nz};
        pose_add_row(acc, J, w);
        acc[23] += 1.0;
      }
    }
  }
  if (tid < kPiHalf) s_half[tid] = 0.0;   // (the barriers of the reduction stand between this and the next store)
  if (!pose_rows_reduce<kPiThreads>(acc, sc, s_tot)) return;   // the workgroup with the last ticket finishes the row
  if (on) {
    if (tid < 7) s_half[tid] = rec->x_out[tid];
    if (tid == 7) s_half[7] = s_tot[0];
    if (tid < 36) {   // mirror the upper triangle
      const double v = pose_rows_H(s_tot, tid);
      s_half[8 + tid] = v;
      s_a[tid] = v;
    }
  }
  __syncthreads();
  if (on && tid == 0) pi_jacobi6(s_a, &s_half[44]);
  __syncthreads();
  if (tid < kPiHalf) (reinterpret_cast<double*>(reinterpret_cast<char*>(row) + 32) + stage * kPiHalf)[tid] = s_half[tid];
  if (tid == 0) {
    int* cnt = stage ? row->map_factors : row->lo_factors;
    cnt[0] = on ? (int)s_tot[22] : 0;
    cnt[1] = on ? (int)s_tot[23] : 0;
    int flags = 0;
    if (on) {
      flags |= stage ? VLOAM_POSE_INFO_MAP_VALID : VLOAM_POSE_INFO_LO_VALID;
      if (min_eig > 0.0 && s_half[44] < min_eig) flags |= stage ? VLOAM_POSE_INFO_MAP_DEGENERATE : VLOAM_POSE_INFO_LO_DEGENERATE;
    }
    if (flags) atomicOr(&row->flags, flags);   // the two stages share the word
    if (stamp) row->frame = frame;
  }
}

#define POSE_INFO_ARGS const int* type, const double* p, const double* dg, int cap, const LMRecord* rec, const int* enable, int ran,            \
                       vloam_pose_info_record* rows, PoseInfoScratch* scratch, int max_frames, int frame, int stamp, double min_eig, size_t ss
__global__ __launch_bounds__(kPiThreads) void k_pose_info_lo(POSE_INFO_ARGS) {
  pose_info_body(type, p, dg, cap, rec, enable, ran, rows, scratch, max_frames, frame, 0, stamp, min_eig, ss);
}
__global__ __launch_bounds__(kPiThreads) void k_pose_info_map(POSE_INFO_ARGS) {
  pose_info_body(type, p, dg, cap, rec, enable, ran, rows, scratch, max_frames, frame, 1, stamp, min_eig, ss);
}
#undef POSE_INFO_ARGS

size_t pose_info_scratch_bytes(int n_sessions) { return sizeof(PoseInfoScratch) * 2 * (size_t)n_sessions; }
hipError_t pose_info_init(hipStream_t st, const PoseInfo& P, int n_sessions) {
  return pose_rows_init(st, P.rows, (long long)P.max_frames * n_sessions, P.scratch, pose_info_scratch_bytes(n_sessions));
}

void pose_info_launch(hipStream_t st, Sess se, const PoseInfo& P, int stage, int frame, const FactorTable& F, const LMRecord* rec, bool ran,
                      const int* d_enable, bool stamp, ProfHook* ph, hipEvent_t done) {
  const int G = ran ? pose_info_blocks(F.cap) : 1;
  const dim3 grid(G, 1, se.B);
  if (stage == 0)
    VLOAM_LAUNCH_EV(ph, kKPoseInfoLo, st, done, k_pose_info_lo, grid, dim3(kPiThreads), 0, st, F.type, F.p, F.dg, F.cap, rec, d_enable, ran ? 1 : 0, P.rows,
                    P.scratch, P.max_frames, frame, stamp ? 1 : 0, P.min_eig[0], se.ss);
  else
    VLOAM_LAUNCH_EV(ph, kKPoseInfoMap, st, done, k_pose_info_map, grid, dim3(kPiThreads), 0, st, F.type, F.p, F.dg, F.cap, rec, d_enable, ran ? 1 : 0, P.rows,
                    P.scratch, P.max_frames, frame, stamp ? 1 : 0, P.min_eig[1], se.ss);
}

}  // namespace vloam
