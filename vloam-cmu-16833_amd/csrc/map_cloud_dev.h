// Device text that the two chains share which turn a caller's point cloud into voxel records, and nothing else includes: the import into a fresh
// handle (map_import.hip) and the merge into a live map (map_merge.hip).  Both key every point as k_map_insert keys a map-frame point, count the
// points per voxel, cut one segment of point indices per voxel (scan, scatter), order every segment ascending and fold it in INPUT order; what
// is the same in both is written here once.  Every function is inlined.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "map_kernels.h"
#include "map_device.h"
#include "map_table.h"
#include "bitonic.h"

namespace vloam {

constexpr int kImportLaneSort = 32;     // voxels of up to this many points are ordered and folded by one lane
constexpr int kImportLdsSort = 4096;    // ... up to this many by one workgroup in LDS
constexpr int kImportMaxGrid = 2048;    // k_map_grow's geometry: 256 CUs x 8 workgroups of 4 wavefronts, grid-stride beyond
constexpr float kImportReach = 1.0e6f;  // coordinates beyond this (metres) are outside any window: the cube arithmetic below stays inside int
constexpr int kImportScanPer = 8;       // consecutive list entries per thread and round of cloud_scan

// The start of a sequence at a map<-odometry transform, on a MapState whose cubes are all empty: the start pose (LM:182-195 with the odometry
// pose the state holds) and the six window-shift loops (LM:207-402), which then move the centre offsets only
__device__ __forceinline__ void cloud_place_start(MapState& s, const double* q_wmap_wodom, const double* t_wmap_wodom) {
  for (int k = 0; k < 4; k++) s.q_wmap_wodom[k] = q_wmap_wodom[k];
  for (int k = 0; k < 3; k++) s.t_wmap_wodom[k] = t_wmap_wodom[k];
  // LaserMapping::input LM:182-195 with the odometry pose of a fresh handle (identity): q_w_curr = q_wmap_wodom * q_wodom_curr, t_w_curr = q_wmap_wodom * t_wodom_curr + t_wmap_wodom
  double q[4], t[3];
  dquat_mul(s.q_wmap_wodom, s.q_wodom_curr, q);
  dquat_rot(s.q_wmap_wodom, s.t_wodom_curr, t);
  for (int k = 0; k < 3; k++) t[k] = t[k] + s.t_wmap_wodom[k];
  for (int k = 0; k < 4; k++) s.parameters[k] = q[k];
  for (int k = 0; k < 3; k++) s.parameters[4 + k] = t[k];
  // LM:207-216, LM:218-402: every cube is empty, so the six while loops move the centre offsets only
  int cen[3] = {s.cenW, s.cenH, s.cenD};
  int cI = cube_abs(t[0]) + cen[0], cJ = cube_abs(t[1]) + cen[1], cK = cube_abs(t[2]) + cen[2];
  while (cI < 3) { cI++; cen[0]++; }
  while (cI >= kCubeW - 3) { cI--; cen[0]--; }
  while (cJ < 3) { cJ++; cen[1]++; }
  while (cJ >= kCubeH - 3) { cJ--; cen[1]--; }
  while (cK < 3) { cK++; cen[2]++; }
  while (cK >= kCubeD - 3) { cK--; cen[2]--; }
  s.centerCube[0] = cI; s.centerCube[1] = cJ; s.centerCube[2] = cK;
  s.cenW = cen[0]; s.cenH = cen[1]; s.cenD = cen[2];
}

// An own text of k_map_insert's keying lines (map_kernels.hip): f64 cube test on the f32 point, f32 voxel index, pack_key.  The point's four
// floats are finite.  false: its cube lies outside the window (offsets cW, cH, cD) or outside the key's range
__device__ __forceinline__ bool cloud_key(const float4 p, float inv, int cW, int cH, int cD, u64* key) {
  if (!(fabsf(p.x) < kImportReach && fabsf(p.y) < kImportReach && fabsf(p.z) < kImportReach)) return false;
  const int Ai = cube_abs((double)p.x), Aj = cube_abs((double)p.y), Ak = cube_abs((double)p.z);
  const int wi = Ai + cW, wj = Aj + cH, wk = Ak + cD;   // == cubeI, cubeJ, cubeK of LM:643-652
  const int lx = (int)floorf(p.x * inv) - cube_voxel_base(Ai, inv), ly = (int)floorf(p.y * inv) - cube_voxel_base(Aj, inv),
            lz = (int)floorf(p.z * inv) - cube_voxel_base(Ak, inv);
  if (wi < 0 || wi >= kCubeW || wj < 0 || wj >= kCubeH || wk < 0 || wk >= kCubeD) return false;   // LM:654-655
  if ((unsigned)lx > (unsigned)kVoxMax || (unsigned)ly > (unsigned)kVoxMax || (unsigned)lz > (unsigned)kVoxMax || !cube_in_key_range(Ai, Aj, Ak)) return false;
  *key = pack_key(Ai, Aj, Ak, lx, ly, lz);
  return true;
}
__device__ __forceinline__ bool cloud_finite(const float4 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(p.w); }

// the two drop counters of a keying kernel: one add per wavefront
__device__ __forceinline__ void cloud_count_drops(int n_out, int n_bad, long long* outside, long long* nonfinite) {
  for (int d = 32; d > 0; d >>= 1) { n_out += __shfl_xor(n_out, d); n_bad += __shfl_xor(n_bad, d); }
  if ((threadIdx.x & 63) == 0) {
    if (n_out) atomicAdd((unsigned long long*)outside, (unsigned long long)n_out);
    if (n_bad) atomicAdd((unsigned long long*)nonfinite, (unsigned long long)n_bad);
  }
}

// One workgroup of 256 threads: the exclusive scan of the nv counters cnt_of(0 .. nv) into off[0 .. nv), off[v] the first place of voxel v's
// segment.  Returns their sum to every thread (the caller stores off[nv]); *most: the largest counter this thread's wavefront saw.
// part: 256 ints of LDS
template <class Cnt>
__device__ __forceinline__ int cloud_scan(int nv, Cnt cnt_of, int* __restrict__ off, int* part, int* most_out) {
  const int tid = threadIdx.x;
  int base = 0, most = 0;
  for (int c0 = 0; c0 < nv; c0 += 256 * kImportScanPer) {
    const int e0 = c0 + tid * kImportScanPer;
    int cnt[kImportScanPer], sum = 0;
#pragma unroll
    for (int e = 0; e < kImportScanPer; e++) {
      cnt[e] = e0 + e < nv ? cnt_of(e0 + e) : 0;
      sum += cnt[e];
      most = max(most, cnt[e]);
    }
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {   // inclusive scan of the 256 partial sums
      const int add = tid >= d ? part[tid - d] : 0;
      __syncthreads();
      part[tid] += add;
      __syncthreads();
    }
    int run = base + part[tid] - sum;
#pragma unroll
    for (int e = 0; e < kImportScanPer; e++) {
      if (e0 + e < nv) off[e0 + e] = run;
      run += cnt[e];
    }
    base += part[255];
    __syncthreads();
  }
  for (int d = 32; d > 0; d >>= 1) most = max(most, __shfl_xor(most, d));
  *most_out = most;
  return base;
}

// The three ordering paths of a voxel's segment of point indices.  One lane, up to kImportLaneSort indices, in place (insertion sort):
__device__ __forceinline__ void cloud_order_lane(int* idx, int cnt) {
  for (int a = 1; a < cnt; a++) {
    const int x = idx[a];
    int c = a - 1;
    while (c >= 0 && idx[c] > x) { idx[c + 1] = idx[c]; c--; }
    idx[c + 1] = x;
  }
}
// ... one workgroup of 256 threads, more: up to kImportLdsSort indices through the LDS bitonic network of bitonic.h (a: kImportLdsSort words of
// LDS), in place; beyond, an index's place is the number of smaller indices in the segment (as k_map_pub_rank), into seg2.  Returns where the
// ordered segment lies, visible to every thread of the workgroup; a[] is free again after the caller's next __syncthreads()
__device__ __forceinline__ const int* cloud_order_block(int* seg, int* seg2, int lo, int cnt, u64* a) {
  const int tid = threadIdx.x;
  const int* ordered = seg + lo;
  if (cnt <= kImportLdsSort) {
    int P2 = 256;
    while (P2 < cnt) P2 <<= 1;
    for (int e = tid; e < P2; e += 256) a[e] = e < cnt ? (u64)(unsigned)seg[lo + e] : ~0ull;
    __syncthreads();
    block_bitonic_sort_u64(a, P2, tid, 256);
    for (int e = tid; e < cnt; e += 256) seg[lo + e] = (int)a[e];
  } else {
    // indices are distinct: the number of smaller ones is the index's place
    for (int e = tid; e < cnt; e += 256) {
      const int x = seg[lo + e];
      int r = 0;
      for (int j = 0; j < cnt; j++) r += seg[lo + j] < x ? 1 : 0;
      seg2[lo + r] = x;
    }
    ordered = seg2 + lo;
  }
  __syncthreads();   // the ordered segment is visible to the folding lane
  return ordered;
}

// The input-order fold (map_finalize_body's arithmetic): acc + p[idx[0]] + p[idx[1]] + ..., one f32 addition at a time, then every component
// divided by (float)n.  acc starts at zero for a new voxel, at the centroid the voxel holds otherwise (n counts it)
__device__ __forceinline__ float4 cloud_fold(float4 acc, const float4* __restrict__ pts, const int* idx, int cnt, int n) {
  for (int a = 0; a < cnt; a++) { const float4 p = pts[idx[a]]; acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w; }
  const float nn = (float)n;
  acc.x = acc.x / nn; acc.y = acc.y / nn; acc.z = acc.z / nn; acc.w = acc.w / nn;
  return acc;
}
// ... and what a voxel that became live owes the map: its occupancy block and its cube's point count (the cube lies inside the window: nothing
// else was keyed)
__device__ __forceinline__ void cloud_new_voxel(const VoxelTable& T, u64 key, int kind, const MapState* ms, MapFrame* fr, int* __restrict__ cube_cnt) {
  int Ai, Aj, Ak;
  unpack_cube(key, &Ai, &Aj, &Ak);
  if (!map_publish_block(T, Ai, Aj, Ak, key_lx(key), key_ly(key), key_lz(key))) atomicOr(&fr->error, kErrMapFull);
  const int wi = Ai + ms->cenW, wj = Aj + ms->cenH, wk = Ak + ms->cenD;
  atomicAdd(&cube_cnt[kind * kCubeNum + wi + kCubeW * wj + kCubeW * kCubeH * wk], 1);
}

}  // namespace vloam
