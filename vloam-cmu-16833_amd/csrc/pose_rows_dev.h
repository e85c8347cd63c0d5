// Device text that pose_info.hip and pose_cov.hip share, and nothing else includes: the sums of rho' J^T J and their reduction over a launch,
// the Jacobi rotation, and the init of a product's rows.  Both units are built with -ffp-contract=off -fno-fast-math and every function here is
// inlined, so a row is the same bits whichever unit the text is compiled into.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <stddef.h>
#include <algorithm>
#include "vloam_device.h"

namespace vloam {

// what a lane, a workgroup and a launch accumulate: [0] the cost, [1 .. 21] the upper triangle of sum rho' J^T J row by row, [22] and [23] the
// blocks of the two factor kinds (edge / plane; CostFunctor32 / CostFunctor22)
constexpr int kPoseAcc = 24;

// per reduction and session: the ticket the workgroups of a launch draw and their partial sums (at most MaxBlocks workgroups)
template <int MaxBlocks>
struct PoseRowsScratch {
  int ticket;
  int pad[15];
  double part[MaxBlocks][kPoseAcc];
};

// acc[1 .. 21] += w J J^T (upper triangle)
__device__ __forceinline__ void pose_add_row(double (&acc)[kPoseAcc], const double (&J)[6], double w) {
  int h = 1;
#pragma unroll
  for (int a = 0; a < 6; a++) {
    const double wj = w * J[a];
#pragma unroll
    for (int b = a; b < 6; b++) acc[h++] += wj * J[b];
  }
}

// ceres::HuberLoss(a) on s = |r|^2: rho (added to the cost as rho / 2) and rho'.  rho'' <= 0, so ceres' Corrector scales residual and Jacobian
// by sqrt(rho') and the Gauss-Newton matrix of the block is rho' J^T J.
__device__ __forceinline__ double pose_huber(double s, double a, double* cost) {
  if (s > a * a) {
    const double r = sqrt(s);
    *cost += 0.5 * (2.0 * a * r - a * a);
    return a / r;
  }
  *cost += 0.5 * s;
  return 1.0;
}

// Jacobi rotation in the (p, q) plane, p < q: d = (a_qq - a_pp) / 2, b = a_pq, t = tan(theta) = b sign(d) / (|d| + sqrt(d^2 + b^2)) (the smaller
// root: |theta| <= pi / 4), c = 1 / sqrt(1 + t^2), s = t c.  J has J_pp = J_qq = c, J_pq = s, J_qp = -s; A <- J^T A J zeroes a_pq.
struct PoseRot { double c, s; };
__device__ __forceinline__ PoseRot pose_rot(double app, double aqq, double apq) {
  const double d = 0.5 * (aqq - app), b = apq;
  const double r2 = d * d + b * b;
  const double r = r2 * rsqrt(fmax(r2, DBL_MIN));
  const double tt = (d < 0.0 ? -b : b) / (fabs(d) + r);
  const double t = b == 0.0 ? 0.0 : tt;
  PoseRot R;
  R.c = rsqrt(1.0 + t * t);
  R.s = t * R.c;
  return R;
}

// The sums of a launch.  Called by ALL Threads lanes of every workgroup of the launch (grid (G, 1, sessions), G <= MaxBlocks), each with its own
// sums in acc; sc: the launch's scratch slot.  Lanes are added by cross-lane shuffles, wavefronts through LDS in wavefront order, and ONE partial
// per workgroup goes to HBM.  The ticket: every workgroup publishes its partial (device-scope fence), then draws; false for all but the
// workgroup that drew the last one.  That one adds the partials in workgroup order (no floating-point atomics anywhere: the totals are
// bit-identical from run to run), resets the ticket for the next launch on the same slot (same stream, behind this one) and returns true with
// the totals in s_tot, behind a barrier.
template <int Threads, int MaxBlocks>
__device__ __forceinline__ bool pose_rows_reduce(double (&acc)[kPoseAcc], PoseRowsScratch<MaxBlocks>* sc, double (&s_tot)[kPoseAcc]) {
  __shared__ double s_w[Threads / 64][kPoseAcc];
  __shared__ int s_last;
  const int G = (int)gridDim.x, wg = (int)blockIdx.x, tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < kPoseAcc; i++) {
    double v = acc[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    acc[i] = v;
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < kPoseAcc; i++) s_w[tid >> 6][i] = acc[i];
  }
  __syncthreads();
  if (tid < kPoseAcc) {
    double v = s_w[0][tid];
    for (int w = 1; w < Threads / 64; w++) v += s_w[w][tid];
    sc->part[wg][tid] = v;
  }
  __threadfence();
  __syncthreads();
  if (tid == 0) s_last = atomicAdd(&sc->ticket, 1) == G - 1 ? 1 : 0;
  __syncthreads();
  if (!s_last) return false;
  __threadfence();
  if (tid < kPoseAcc) {
    double v = 0.0;
    for (int w = 0; w < G; w++) v += __hip_atomic_load(&sc->part[w][tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // workgroup order
    s_tot[tid] = v;
  }
  if (tid == 0) sc->ticket = 0;
  __syncthreads();
  return true;
}

// element e = 6 r + c of the symmetric 6 x 6 out of the totals: behind the cost the triangle's rows of 6, 5, .. 1 sums, (c, r) mirrors (r, c)
__device__ __forceinline__ double pose_rows_H(const double (&s_tot)[kPoseAcc], int e) {
  const int r = e / 6, c = e % 6, lo = r < c ? r : c, hi = r < c ? c : r;
  return s_tot[1 + lo * (13 - lo) / 2 + (hi - lo)];
}

// rows of a fresh product: zero, frame = -1; its scratch zero
template <class Rec>
__global__ __launch_bounds__(64) void k_pose_rows_init(Rec* rows, long long n_rows) {
  for (long long r = (long long)blockIdx.x * 64 + threadIdx.x; r < n_rows; r += (long long)gridDim.x * 64) {
    int* w = reinterpret_cast<int*>(rows + r);
    for (int k = 0; k < (int)(sizeof(Rec) / sizeof(int)); k++) w[k] = 0;
    rows[r].frame = -1;
  }
}
template <class Rec>
hipError_t pose_rows_init(hipStream_t st, Rec* rows, long long n_rows, void* scratch, size_t scratch_bytes) {
  hipLaunchKernelGGL(k_pose_rows_init<Rec>, vl_hw_grid(dim3((unsigned)std::min<long long>((n_rows + 63) / 64, 1024), 1, 1)), dim3(64), 0, st, rows, n_rows);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipMemsetAsync(scratch, 0, scratch_bytes, st);
}

}  // namespace vloam
