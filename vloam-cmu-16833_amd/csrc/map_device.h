// Device helpers of the mapping stage with callers in more than one of map_kernels.hip, map_output.hip and map_prepare_fit.inc.h: cube
// arithmetic of the 21 x 21 x 11 window, pointAssociateToMap, quaternion product and rotation in f64.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace vloam {

// LM:207-216 / LM:643-652: C int() truncation plus the "< 0" correction; absolute cube coordinate (no centre offset)
__device__ __forceinline__ int cube_abs(double v) {
  int c = int((v + 25.0) / 50.0);
  if (v + 25.0 < 0) c--;
  return c;
}
__device__ __forceinline__ int cube_lo(double v) { return (int)floor((v - 1e-3 + 25.0) * 0.02); }
__device__ __forceinline__ int cube_hi(double v) { return (int)floor((v + 1e-3 + 25.0) * 0.02); }
// first global voxel index that can belong to cube A (minus one cell of slack so the local index is never negative)
__device__ __forceinline__ int cube_voxel_base(int A, float inv) { return (int)floor((50.0 * (double)A - 25.0) * (double)inv) - 1; }

// Eigen q * v (see lm_solve.hip / lo_kernels.hip) followed by + t, rounded to f32: pointAssociateToMap, LM:146-155
__device__ __forceinline__ float4 associate_to_map(float4 pi, const double* q, const double* t) {
  const double ux = q[0], uy = q[1], uz = q[2], w = q[3];
  const double vx = pi.x, vy = pi.y, vz = pi.z;
  double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
  cx = cx + cx; cy = cy + cy; cz = cz + cz;
  const double dx = uy * cz - uz * cy, dy = uz * cx - ux * cz, dz = ux * cy - uy * cx;
  float4 o;
  o.x = (float)(((vx + w * cx) + dx) + t[0]);
  o.y = (float)(((vy + w * cy) + dy) + t[1]);
  o.z = (float)(((vz + w * cz) + dz) + t[2]);
  o.w = pi.w;
  return o;
}

__device__ __forceinline__ void dquat_mul(const double* a, const double* b, double* r) {
  r[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  r[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  r[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  r[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
__device__ __forceinline__ void dquat_rot(const double* q, const double* v, double* o) {
  const double ux = q[0], uy = q[1], uz = q[2], w = q[3];
  double cx = uy * v[2] - uz * v[1], cy = uz * v[0] - ux * v[2], cz = ux * v[1] - uy * v[0];
  cx = cx + cx; cy = cy + cy; cz = cz + cz;
  const double dx = uy * cz - uz * cy, dy = uz * cx - ux * cz, dz = ux * cy - uy * cx;
  o[0] = (v[0] + w * cx) + dx; o[1] = (v[1] + w * cy) + dy; o[2] = (v[2] + w * cz) + dz;
}

}  // namespace vloam
