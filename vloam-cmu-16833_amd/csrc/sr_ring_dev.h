// What the ring kernels of the scan registration share (SR:288-439 of the reference's scan_registration.cpp): the LDS tiers (k_sr_ring,
// sr_ring.hip) and the long tier (k_sr_ring_long, sr_ring_long.hip) read these rules from this one text.  Every piece is pinned bit for bit
// to the reference.  What differs on purpose stays with the kernels: the sector walks and the VoxelGrid's sort.
// `get` is how a tier reads point l of its ring as (x, y, z, intensity): from SoA floats in LDS, or from the ring-major cloud in HBM.  A
// component nobody uses is not loaded (the accessors are inlined).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include "vloam_device.h"
#include "sr_wave.h"

namespace vloam {

constexpr int kRingThreads = 512;   // a ring's workgroup: 8 wavefronts

// In-place exclusive scan of an int array (n <= 16 * kRingThreads); returns the total.  Per-thread chunk sums, a shuffle scan inside
// every wavefront, the eight wavefront totals through LDS: three workgroup barriers (a Hillis-Steele scan over 512 partial sums took 18).
__device__ inline int block_exclusive_scan(int* a, int n, int* scratch /* kRingThreads ints of LDS */) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int per = (n + kRingThreads - 1) / kRingThreads;
  const int lo = tid * per, hi = min(lo + per, n);
  int s = 0;
  for (int k = lo; k < hi; k++) s += a[k];
  int inc = s;
  for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d); if (lane >= d) inc += o; }
  __syncthreads();   // (scratch may still be read by the caller's previous use)
  if (lane == 63) scratch[wv] = inc;
  __syncthreads();
  int base = 0, total = 0;
  for (int w = 0; w < kRingThreads / 64; w++) { const int t = scratch[w]; base += w < wv ? t : 0; total += t; }
  int run = base + inc - s;
  for (int k = lo; k < hi; k++) { int v = a[k]; a[k] = run; run += v; }
  __syncthreads();
  return total;
}

// SR:288-303, the 11-tap curvature of point i
template <class Get>
__device__ __forceinline__ float sr_curvature(Get get, int i) {
  const float dX = get(i - 5).x + get(i - 4).x + get(i - 3).x + get(i - 2).x + get(i - 1).x - 10 * get(i).x + get(i + 1).x + get(i + 2).x + get(i + 3).x + get(i + 4).x + get(i + 5).x;
  const float dY = get(i - 5).y + get(i - 4).y + get(i - 3).y + get(i - 2).y + get(i - 1).y - 10 * get(i).y + get(i + 1).y + get(i + 2).y + get(i + 3).y + get(i + 4).y + get(i + 5).y;
  const float dZ = get(i - 5).z + get(i - 4).z + get(i - 3).z + get(i - 2).z + get(i - 1).z - 10 * get(i).z + get(i + 1).z + get(i + 2).z + get(i + 3).z + get(i + 4).z + get(i + 5).z;
  return dX * dX + dY * dY + dZ * dZ;
}

// SR:353-376: the neighbour suppression around a pick walks outwards and stops between two consecutive points further apart than this
__device__ __forceinline__ bool sr_gap(float4 a, float4 b) {
  const float dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
  return (double)(dx * dx + dy * dy + dz * dz) > 0.05;
}

// SR:330 / SR:383 compare the f32 curvature with the double 0.1, which lies between two neighbouring floats (0.099999994 and
// 0.1f = 0.100000001): (double)c > 0.1 <=> c >= 0.1f and (double)c < 0.1 <=> c < 0.1f — no f64 convert and compare per point.
// A curvature is >= 0, so its bit pattern orders like its value: the walks compare the bits.
__device__ __forceinline__ bool sr_sharp_cand(unsigned curv_bits) { return __uint_as_float(curv_bits) >= 0.1f; }
__device__ __forceinline__ bool sr_flat_cand(unsigned curv_bits) { return __uint_as_float(curv_bits) < 0.1f; }

__device__ __forceinline__ int sr_sector_lo(int start, int end, int s) { return start + (end - start) * s / 6; }            // SR:319
__device__ __forceinline__ int sr_sector_hi(int start, int end, int s) { return start + (end - start) * (s + 1) / 6 - 1; }  // SR:320

// One workgroup per ring (gridDim.x == kMaxRings) — or the catch-all: ONE workgroup per session, which looks at the ring lengths (one load
// per lane, the same answer in every wavefront) and works on the rings of more than `above` points one after the other (normally none: the
// launch ends here).  ONE call site of the ring body.
template <class Body>
__device__ __forceinline__ void sr_for_rings(const FrameScalars* S, int above, Body one_ring) {
  static_assert(kMaxRings == 64, "one ring per lane");
  unsigned long long todo = 1ull << (blockIdx.x & 63);
  if (gridDim.x != kMaxRings) todo = __ballot(S->ring_count[threadIdx.x & 63] > above);
  while (todo != 0ull) {
    const int r = __ffsll((long long)todo) - 1;
    todo &= todo - 1ull;
    one_ring(r);
    if (todo != 0ull) __syncthreads();   // the ring's LDS is no longer read
  }
}

// debug: cloudNeighborPicked and cloudLabel as the walks leave them
__device__ __forceinline__ void sr_dump_marks(int* __restrict__ dbg_picked, int* __restrict__ dbg_label, int off, int len,
                                              const unsigned char* picked, const signed char* label) {
  if (dbg_picked) for (int l = threadIdx.x; l < len; l += kRingThreads) { dbg_picked[off + l] = picked[l]; dbg_label[off + l] = label[l]; }
}

// ---- lessFlat (SR:424-430): every point of the six sectors — local indices [c_lo, c_hi] — that is neither sharp nor lessSharp
// Bounding box of the candidates (getMinMax3D) and their number, in every lane.  wred: [8 wavefronts][8] floats of LDS; ends behind a
// workgroup barrier.
struct SrBox {
  float mn[3], mx[3];
  int ncand;
};
template <class Get>
__device__ __forceinline__ SrBox sr_lessflat_box(Get get, const signed char* label, int c_lo, int c_hi, float* wred) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float mn[3] = {3.4e38f, 3.4e38f, 3.4e38f}, mx[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
  int mycnt = 0;
  for (int l = c_lo + tid; l <= c_hi; l += kRingThreads)
    if (label[l] <= 0) {
      const float4 q = get(l);
      mn[0] = fminf(mn[0], q.x); mx[0] = fmaxf(mx[0], q.x);
      mn[1] = fminf(mn[1], q.y); mx[1] = fmaxf(mx[1], q.y);
      mn[2] = fminf(mn[2], q.z); mx[2] = fmaxf(mx[2], q.z);
      mycnt++;
    }
  for (int a = 0; a < 3; a++) { mn[a] = wave_fminmax<false>(mn[a]); mx[a] = wave_fminmax<true>(mx[a]); }   // (DPP row steps: no LDS crossbar)
  mycnt = wave_sum_i32(mycnt);
  if (lane == 0) {
    for (int a = 0; a < 3; a++) { wred[wave * 8 + a] = mn[a]; wred[wave * 8 + 3 + a] = mx[a]; }
    ((int*)wred)[wave * 8 + 6] = mycnt;
  }
  __syncthreads();
  // (every lane folds the eight wavefronts' results itself — broadcast reads — instead of waiting for one lane behind a second barrier)
  SrBox b;
  b.ncand = 0;
  for (int a = 0; a < 3; a++) { b.mn[a] = wred[a]; b.mx[a] = wred[3 + a]; }
  for (int w = 0; w < kRingThreads / 64; w++) {
    for (int a = 0; a < 3; a++) { b.mn[a] = fminf(b.mn[a], wred[w * 8 + a]); b.mx[a] = fmaxf(b.mx[a], wred[w * 8 + 3 + a]); }
    b.ncand += ((int*)wred)[w * 8 + 6];
  }
  return b;
}

// ---- the per-ring pcl::VoxelGrid of leaf 0.2 (SR:433-437) over that box.  The cell index is PCL's own 32-bit integer arithmetic (the
// mapping stage's ds_grid / ds_cell of map_stack.hip compute in 64 bits: another rule, not to be merged with this one).
struct SrGrid {
  static constexpr float inv = 1.0f / 0.2f;  // inverse_leaf_size_
  int min_b[3], div_b[3];
  // PCL: "Leaf size is too small for the input dataset" -> the filter's output is its input
  __device__ __forceinline__ static bool too_fine(const SrBox& b) {
    const long long dx = (long long)((b.mx[0] - b.mn[0]) * inv) + 1, dy = (long long)((b.mx[1] - b.mn[1]) * inv) + 1, dz = (long long)((b.mx[2] - b.mn[2]) * inv) + 1;
    return dx * dy * dz > (long long)INT_MAX;
  }
  __device__ __forceinline__ explicit SrGrid(const SrBox& b) {
    for (int a = 0; a < 3; a++) {
      min_b[a] = (int)floorf(b.mn[a] * inv);
      div_b[a] = (int)floorf(b.mx[a] * inv) - min_b[a] + 1;
    }
  }
  __device__ __forceinline__ int voxel_of(float x, float y, float z) const {
    const int ijk0 = (int)(floorf(x * inv) - (float)min_b[0]);
    const int ijk1 = (int)(floorf(y * inv) - (float)min_b[1]);
    const int ijk2 = (int)(floorf(z * inv) - (float)min_b[2]);
    return ijk0 + ijk1 * div_b[0] + ijk2 * div_b[0] * div_b[1];
  }
};

// The too-fine grid's output: the ring's ncand candidates in input order.  iscr: [len] ints, scan_tmp: kRingThreads ints of LDS.
template <class Get>
__device__ __forceinline__ void sr_ds_passthrough(Get get, const signed char* label, int len, int c_lo, int c_hi, int* iscr, int* scan_tmp,
                                                  float4* out, FrameScalars* S, int r, int ncand) {
  const int tid = threadIdx.x;
  for (int l = tid; l < len; l += kRingThreads) iscr[l] = (l >= c_lo && l <= c_hi && label[l] <= 0) ? 1 : 0;
  __syncthreads();
  block_exclusive_scan(iscr, len, scan_tmp);
  for (int l = c_lo + tid; l <= c_hi; l += kRingThreads)
    if (label[l] <= 0) out[iscr[l]] = get(l);
  if (tid == 0) S->ring_ds_cnt[r] = ncand;
}

}  // namespace vloam
