// tf2::Transform restated (the algebra behind the vloam_tf blackboard of vloam_device.h): row-major 3x3 basis + origin, double precision, the
// same operation order as tf2/LinearMath (Transform::operator*, inverse(), Matrix3x3::setRotation / getRotation).  A header of its own so
// that a host compiler without HIP can build the same text: tests/cpp/dev_probe_host.cpp is the host statement the device probes
// (dev_probe.hip, tests/test_gpu_dev_probe.py) are compared with bit for bit.
#pragma once
#include <math.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace vloam {

struct TfDev { double m[9]; double o[3]; };
__host__ __device__ inline void tf_identity(TfDev* t) { for (int k = 0; k < 9; k++) t->m[k] = (k % 4 == 0) ? 1.0 : 0.0; t->o[0] = t->o[1] = t->o[2] = 0.0; }
__host__ __device__ inline void tf_mul(const TfDev& a, const TfDev& b, TfDev* r) {  // (a.m b.m, a.m b.o + a.o)
  TfDev t;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) t.m[i * 3 + j] = (a.m[i * 3] * b.m[j] + a.m[i * 3 + 1] * b.m[3 + j]) + a.m[i * 3 + 2] * b.m[6 + j];
  for (int i = 0; i < 3; i++) t.o[i] = ((a.m[i * 3] * b.o[0] + a.m[i * 3 + 1] * b.o[1]) + a.m[i * 3 + 2] * b.o[2]) + a.o[i];
  *r = t;
}
__host__ __device__ inline void tf_inverse(const TfDev& a, TfDev* r) {              // (m^T, m^T * -o)
  TfDev t;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) t.m[i * 3 + j] = a.m[j * 3 + i];
  const double n[3] = {-a.o[0], -a.o[1], -a.o[2]};
  for (int i = 0; i < 3; i++) t.o[i] = (t.m[i * 3] * n[0] + t.m[i * 3 + 1] * n[1]) + t.m[i * 3 + 2] * n[2];
  *r = t;
}
__host__ __device__ inline void tf_set_rotation(TfDev* t, const double q[4]) {      // Matrix3x3::setRotation
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double d = ((x * x + y * y) + z * z) + w * w;
  const double s = 2.0 / d;
  const double xs = x * s, ys = y * s, zs = z * s;
  const double wx = w * xs, wy = w * ys, wz = w * zs, xx = x * xs, xy = x * ys, xz = x * zs, yy = y * ys, yz = y * zs, zz = z * zs;
  t->m[0] = 1.0 - (yy + zz); t->m[1] = xy - wz; t->m[2] = xz + wy;
  t->m[3] = xy + wz; t->m[4] = 1.0 - (xx + zz); t->m[5] = yz - wx;
  t->m[6] = xz - wy; t->m[7] = yz + wx; t->m[8] = 1.0 - (xx + yy);
}
__host__ __device__ inline void tf_get_rotation(const TfDev& t, double q[4]) {      // Matrix3x3::getRotation
  const double* m = t.m;
  const double trace = (m[0] + m[4]) + m[8];
  if (trace > 0.0) {
    double s = sqrt(trace + 1.0);
    q[3] = s * 0.5;
    s = 0.5 / s;
    q[0] = (m[7] - m[5]) * s; q[1] = (m[2] - m[6]) * s; q[2] = (m[3] - m[1]) * s;
  } else {
    const int i = m[0] < m[4] ? (m[4] < m[8] ? 2 : 1) : (m[0] < m[8] ? 2 : 0);
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    double s = sqrt(((m[i * 4] - m[j * 4]) - m[k * 4]) + 1.0);
    q[i] = s * 0.5;
    s = 0.5 / s;
    q[3] = (m[k * 3 + j] - m[j * 3 + k]) * s;
    q[j] = (m[j * 3 + i] + m[i * 3 + j]) * s;
    q[k] = (m[k * 3 + i] + m[i * 3 + k]) * s;
  }
}

}  // namespace vloam
