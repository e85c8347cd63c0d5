// Map import on gfx950 (vloam_map_import / vloam_map_import_device): two point clouds in the map frame become the voxel tables of a fresh handle.
// A code object of its own, like map_ckpt.hip and map_query.hip: a handle that never imports launches and allocates nothing of this, and no
// kernel of a sweep changes.  The chain runs once per call on the mapping stream, with nothing of the handle in flight, on temporary allocations:
//   k_map_import_prepare  1 thread  the start pose (LM:182-195 with the identity odometry pose), the six window-shift loops (LM:207-402) on the
//                                   live MapState, the tables' counters and the result record start over
//   k_map_import_key      grid      per point: finite? cube (f64) and voxel (f32) as k_map_insert keys a map-frame point; find-or-insert with the
//                                   table's CAS and probe bound; integer atomicAdd of the record's point counter; the first claimant appends the
//                                   slot to the voxel list
//   k_map_import_scan     1 WG      exclusive scan of the voxel list's counters: one segment of point indices per voxel
//   k_map_import_scatter  grid      point index -> its voxel's segment (place inside the segment: arrival, fixed up next)
//   k_map_import_reduce   grid      per voxel of up to kImportLaneSort points: one lane orders the segment's indices ascending (insertion sort)
//                                   and folds; fuller voxels go onto the big list
//   k_map_import_big      1 WG/voxel  up to kImportLdsSort indices: the LDS bitonic network of bitonic.h; beyond: an index's place is the number
//                                   of smaller indices in the segment (as k_map_pub_rank); then one lane folds
//   k_map_import_finish   1 thread  60 % rule of k_map_finalize on the records and block keys created -> the sticky map-full error
// fold = f32 sum of the voxel's points in INPUT order, every component divided by (float)n, count 1, pend_cnt 0: the state k_map_finalize leaves
// behind a valid cube's VoxelGrid re-filter (map_kernels.hip, LM:689-702); then the voxel's occupancy block and its cube's point count.
// While the chain runs a claimed record holds scratch: count = the voxel's position in the list, pend_cnt = its point counter (back to zero once
// k_map_import_scatter has placed every point).  No floating-point atomics anywhere: the result is a function of the input arrays alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "map_kernels.h"
#include "map_device.h"
#include "map_table.h"
#include "bitonic.h"

namespace vloam {

constexpr int kImportLaneSort = 32;     // voxels of up to this many points are ordered and folded by one lane
constexpr int kImportLdsSort = 4096;    // ... up to this many by one workgroup in LDS
constexpr int kImportMaxGrid = 2048;    // k_map_grow's geometry: 256 CUs x 8 workgroups of 4 wavefronts, grid-stride beyond
constexpr float kImportReach = 1.0e6f;  // coordinates beyond this (metres) are outside any window: the cube arithmetic below stays inside int

struct ImportPose { double q[4], t[3]; };   // by value: the host's transform needs no upload
struct ImportCtr { int n_vox[2]; int n_big[2]; };

__global__ __launch_bounds__(64) void k_map_import_prepare(MapState* ms, MapFrame* fr, int* stats0, int* stats1, ImportPose pose, long long n0, long long n1,
                                                           ImportCtr* ctr, vloam_map_import_result* res) {
  if (threadIdx.x != 0) return;
  MapState s = *ms;
  for (int k = 0; k < 4; k++) s.q_wmap_wodom[k] = pose.q[k];
  for (int k = 0; k < 3; k++) s.t_wmap_wodom[k] = pose.t[k];
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
  *ms = s;
  for (int k = 0; k < 2; k++) { fr->n_deferred[k] = 0; fr->n_newraw[k] = 0; }
  for (int k = 0; k < 4; k++) { stats0[k] = 0; stats1[k] = 0; }
  ImportCtr c;
  memset(&c, 0, sizeof(c));
  *ctr = c;
  vloam_map_import_result r;
  memset(&r, 0, sizeof(r));
  r.n_in[0] = n0; r.n_in[1] = n1;
  for (int k = 0; k < 3; k++) r.center_cube[k] = cen[k];
  *res = r;
}

// An own text of k_map_insert's keying lines (map_kernels.hip): f64 cube test on the f32 point, f32 voxel index, pack_key
__global__ __launch_bounds__(256) void k_map_import_key(const float4* __restrict__ pts, int n, int kind, VoxelTable T, float inv, const MapState* __restrict__ ms,
                                                        MapFrame* fr, int* __restrict__ slot_of, int* __restrict__ vox_slot, ImportCtr* ctr,
                                                        vloam_map_import_result* res) {
  const int cW = ms->cenW, cH = ms->cenH, cD = ms->cenD;
  int n_out = 0, n_bad = 0;
  for (int i0 = (int)(blockIdx.x * 256u); i0 < n; i0 += (int)(gridDim.x * 256u)) {   // workgroup-uniform (n <= 2^24)
    const int i = i0 + (int)threadIdx.x;
    if (i >= n) continue;
    const float4 p = pts[i];
    int found = -1;
    if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(p.w))) n_bad++;
    else if (!(fabsf(p.x) < kImportReach && fabsf(p.y) < kImportReach && fabsf(p.z) < kImportReach)) n_out++;
    else {
      const int Ai = cube_abs((double)p.x), Aj = cube_abs((double)p.y), Ak = cube_abs((double)p.z);
      const int wi = Ai + cW, wj = Aj + cH, wk = Ak + cD;   // == cubeI, cubeJ, cubeK of LM:643-652
      const int lx = (int)floorf(p.x * inv) - cube_voxel_base(Ai, inv), ly = (int)floorf(p.y * inv) - cube_voxel_base(Aj, inv),
                lz = (int)floorf(p.z * inv) - cube_voxel_base(Ak, inv);
      if (wi < 0 || wi >= kCubeW || wj < 0 || wj >= kCubeH || wk < 0 || wk >= kCubeD) n_out++;   // LM:654-655
      else if ((unsigned)lx > (unsigned)kVoxMax || (unsigned)ly > (unsigned)kVoxMax || (unsigned)lz > (unsigned)kVoxMax || !cube_in_key_range(Ai, Aj, Ak)) n_out++;
      else {
        const u64 key = pack_key(Ai, Aj, Ak, lx, ly, lz);
        unsigned s = (unsigned)mix64(key) & T.mask;
        for (int probe = 0; probe < kMaxProbe; probe++, s = (s + 1) & T.mask) {
          const u64 old = atomicCAS(&T.rec[s].key, 0ull, key);
          if (old != 0ull && old != key) continue;
          if (old == 0ull) {   // first claimant: the voxel joins the list (at most one voxel per point: the list holds n entries)
            const int v = atomicAdd(&ctr->n_vox[kind], 1);
            vox_slot[v] = (int)s;
            T.rec[s].count = v;
          }
          atomicAdd(&T.rec[s].pend_cnt, 1);
          found = (int)s;
          break;
        }
        if (found < 0) atomicOr(&fr->error, kErrMapFull);   // no slot within the probe bound: the table is overloaded
      }
    }
    slot_of[i] = found;
  }
  // the two drop counters: one add per wavefront
  for (int d = 32; d > 0; d >>= 1) { n_out += __shfl_xor(n_out, d); n_bad += __shfl_xor(n_bad, d); }
  if ((threadIdx.x & 63) == 0) {
    if (n_out) atomicAdd((unsigned long long*)&res->n_outside_window[kind], (unsigned long long)n_out);
    if (n_bad) atomicAdd((unsigned long long*)&res->n_nonfinite[kind], (unsigned long long)n_bad);
  }
}

// off[v]: first place of voxel v's segment, off[n_vox]: points placed; the table's key count and the result's voxel figures
constexpr int kImportScanPer = 8;   // consecutive list entries per thread and round
__global__ __launch_bounds__(256) void k_map_import_scan(VoxelTable T, int kind, const int* __restrict__ vox_slot, const ImportCtr* __restrict__ ctr,
                                                         int* __restrict__ off, vloam_map_import_result* res) {
  __shared__ int part[256];
  const int tid = threadIdx.x, nv = ctr->n_vox[kind];
  int base = 0, most = 0;
  for (int c0 = 0; c0 < nv; c0 += 256 * kImportScanPer) {
    const int e0 = c0 + tid * kImportScanPer;
    int cnt[kImportScanPer], sum = 0;
#pragma unroll
    for (int e = 0; e < kImportScanPer; e++) {
      cnt[e] = e0 + e < nv ? T.rec[vox_slot[e0 + e]].pend_cnt : 0;
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
  if ((tid & 63) == 0 && most > 0) atomicMax(&res->max_per_voxel[kind], most);
  if (tid == 0) {
    off[nv] = base;
    T.stats[0] = nv;   // keys in the table, as map_reinsert's callers count them; the block keys are counted by map_publish_block
    res->n_voxels[kind] = (long long)nv;
  }
}

__global__ __launch_bounds__(256) void k_map_import_scatter(int n, VoxelTable T, const int* __restrict__ slot_of, const int* __restrict__ off, int* __restrict__ seg) {
  for (int i = (int)(blockIdx.x * 256u + threadIdx.x); i < n; i += (int)(gridDim.x * 256u)) {
    const int s = slot_of[i];
    if (s < 0) continue;
    const int v = T.rec[s].count;
    const int pos = atomicSub(&T.rec[s].pend_cnt, 1) - 1;
    seg[off[v] + pos] = i;
  }
}

// One lane: the voxel's points in the order of idx[0 .. cnt) -> the record of slot s (map_finalize_body's arithmetic: 0 + p0 + p1 ..., then / (float)n),
// its occupancy block and its cube's count
__device__ __forceinline__ void import_fold(const VoxelTable& T, int s, const float4* __restrict__ pts, const int* idx, int cnt, int kind, const MapState* ms,
                                            MapFrame* fr, int* __restrict__ cube_cnt) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int a = 0; a < cnt; a++) { const float4 p = pts[idx[a]]; acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w; }
  const float nn = (float)cnt;
  acc.x = acc.x / nn; acc.y = acc.y / nn; acc.z = acc.z / nn; acc.w = acc.w / nn;
  rec_store_value(&T.rec[s], acc, 1, 0);
  const u64 key = T.rec[s].key;
  int Ai, Aj, Ak;
  unpack_cube(key, &Ai, &Aj, &Ak);
  if (!map_publish_block(T, Ai, Aj, Ak, key_lx(key), key_ly(key), key_lz(key))) atomicOr(&fr->error, kErrMapFull);
  const int wi = Ai + ms->cenW, wj = Aj + ms->cenH, wk = Ak + ms->cenD;   // inside the window: k_map_import_key keyed nothing else
  atomicAdd(&cube_cnt[kind * kCubeNum + wi + kCubeW * wj + kCubeW * kCubeH * wk], 1);
}

__global__ __launch_bounds__(256) void k_map_import_reduce(VoxelTable T, int kind, const float4* __restrict__ pts, const int* __restrict__ vox_slot,
                                                           ImportCtr* ctr, const int* __restrict__ off, int* seg, int* __restrict__ big, int big_cap,
                                                           const MapState* __restrict__ ms, MapFrame* fr, int* __restrict__ cube_cnt) {
  const int nv = ctr->n_vox[kind];
  for (int v = (int)(blockIdx.x * 256u + threadIdx.x); v < nv; v += (int)(gridDim.x * 256u)) {
    const int lo = off[v], cnt = off[v + 1] - lo;
    if (cnt > kImportLaneSort) {
      const int b = atomicAdd(&ctr->n_big[kind], 1);
      if (b < big_cap) big[b] = v;   // (always: at most n / 33 voxels hold more than 32 of n points)
      continue;
    }
    int* idx = seg + lo;   // the segment is this lane's alone: ordered in place
    for (int a = 1; a < cnt; a++) {
      const int x = idx[a];
      int c = a - 1;
      while (c >= 0 && idx[c] > x) { idx[c + 1] = idx[c]; c--; }
      idx[c + 1] = x;
    }
    import_fold(T, vox_slot[v], pts, idx, cnt, kind, ms, fr, cube_cnt);
  }
}

__global__ __launch_bounds__(256) void k_map_import_big(VoxelTable T, int kind, const float4* __restrict__ pts, const int* __restrict__ vox_slot,
                                                        const ImportCtr* __restrict__ ctr, const int* __restrict__ off, int* seg, int* seg2, const int* __restrict__ big,
                                                        int big_cap, const MapState* __restrict__ ms, MapFrame* fr, int* __restrict__ cube_cnt) {
  __shared__ u64 a[kImportLdsSort];
  const int tid = threadIdx.x, nb = min(ctr->n_big[kind], big_cap);
  for (int b = (int)blockIdx.x; b < nb; b += (int)gridDim.x) {
    const int v = big[b], lo = off[v], cnt = off[v + 1] - lo;
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
    if (tid == 0) import_fold(T, vox_slot[v], pts, ordered, cnt, kind, ms, fr, cube_cnt);
    __syncthreads();   // a[] is free for the next voxel
  }
}

// k_map_finalize's table health rule on what the import created: more than 60 % of the slots (or block slots) in use -> map full
__global__ __launch_bounds__(64) void k_map_import_finish(VoxelTable T0, VoxelTable T1, MapFrame* fr) {
  const int kind = threadIdx.x;
  if (kind >= 2) return;
  const VoxelTable& T = kind ? T1 : T0;
  const long long slots = (long long)T.mask + 1, bslots = (long long)T.bslots_mask + 1;
  if ((long long)T.stats[0] * 10 > slots * 6 || (long long)T.stats[2] * 10 > bslots * 6) atomicOr(&fr->error, kErrMapFull);
}

// ---------------------------------------------------------------------------------------------- host side
struct ImportTmp {   // one allocation, laid out by the arena helper (dry pass to measure)
  ImportCtr* ctr = nullptr;
  vloam_map_import_result* res = nullptr;
  float4* pts[2] = {nullptr, nullptr};   // the host form's uploaded clouds
  int* slot_of[2] = {nullptr, nullptr};  // [n] table slot of every point, -1: dropped
  int* vox_slot[2] = {nullptr, nullptr}; // [n] the voxel list: slots in claim order
  int* off[2] = {nullptr, nullptr};      // [n + 1] segment offsets
  int* seg[2] = {nullptr, nullptr};      // [n] point indices by voxel
  int* seg2[2] = {nullptr, nullptr};     // [n] the rank path's output
  int* big[2] = {nullptr, nullptr};      // [n / 33 + 1] voxels of more than kImportLaneSort points
};
static bool import_layout(ImportTmp* I, Arena& A, const int n[2], bool upload) {
  bool ok = A.take(&I->ctr, 1) && A.take(&I->res, 1);
  for (int k = 0; k < 2 && ok; k++) {
    if (n[k] == 0) continue;
    const size_t nk = (size_t)n[k];
    ok = (!upload || A.take(&I->pts[k], nk)) && A.take(&I->slot_of[k], nk) && A.take(&I->vox_slot[k], nk) && A.take(&I->off[k], nk + 1) && A.take(&I->seg[k], nk) &&
         A.take(&I->seg2[k], nk) && A.take(&I->big[k], nk / (kImportLaneSort + 1) + 1);
  }
  return ok;
}

vloam_status map_import_run(MapContext* m, hipStream_t st, const double pose7[7], const void* const cloud[2], const int n[2], bool host_clouds,
                            vloam_map_import_result* h_result) {
  ImportTmp I;
  Arena dry;
  import_layout(&I, dry, n, host_clouds);
  Arena A;
  A.cap = dry.off; A.dry = false;
  if (hipMalloc((void**)&A.base, A.cap) != hipSuccess) return VLOAM_ERR_HIP;
  vloam_status rc = import_layout(&I, A, n, host_clouds) ? VLOAM_OK : VLOAM_ERR_HIP;
  const float4* pts[2] = {nullptr, nullptr};
  for (int k = 0; k < 2 && rc == VLOAM_OK; k++) {
    if (n[k] == 0) continue;
    if (host_clouds) {
      if (hipMemcpyAsync(I.pts[k], cloud[k], (size_t)n[k] * sizeof(float4), hipMemcpyHostToDevice, st) != hipSuccess) rc = VLOAM_ERR_HIP;
      pts[k] = I.pts[k];
    } else pts[k] = (const float4*)cloud[k];
  }
  if (rc == VLOAM_OK) {
    ImportPose pose;
    for (int k = 0; k < 4; k++) pose.q[k] = pose7[k];
    for (int k = 0; k < 3; k++) pose.t[k] = pose7[4 + k];
    VL_RAW_LAUNCH(k_map_import_prepare, dim3(1), dim3(64), 0, st, m->state, m->frame, m->tab[0].stats, m->tab[1].stats, pose, (long long)n[0], (long long)n[1], I.ctr, I.res);
    for (int k = 0; k < 2; k++) {
      if (n[k] == 0) continue;
      const VoxelTable& T = m->tab[k];
      const unsigned blocks = ((unsigned)n[k] + 255u) / 256u, grid = blocks < (unsigned)kImportMaxGrid ? blocks : (unsigned)kImportMaxGrid;
      const int big_cap = n[k] / (kImportLaneSort + 1) + 1;
      VL_RAW_LAUNCH(k_map_import_key, dim3(grid), dim3(256), 0, st, pts[k], n[k], k, T, m->inv_leaf[k], m->state, m->frame, I.slot_of[k], I.vox_slot[k], I.ctr, I.res);
      VL_RAW_LAUNCH(k_map_import_scan, dim3(1), dim3(256), 0, st, T, k, I.vox_slot[k], I.ctr, I.off[k], I.res);
      VL_RAW_LAUNCH(k_map_import_scatter, dim3(grid), dim3(256), 0, st, n[k], T, I.slot_of[k], I.off[k], I.seg[k]);
      VL_RAW_LAUNCH(k_map_import_reduce, dim3(grid), dim3(256), 0, st, T, k, pts[k], I.vox_slot[k], I.ctr, I.off[k], I.seg[k], I.big[k], big_cap, m->state, m->frame,
                    m->cube_cnt);
      VL_RAW_LAUNCH(k_map_import_big, dim3((unsigned)(big_cap < 1024 ? big_cap : 1024)), dim3(256), 0, st, T, k, pts[k], I.vox_slot[k], I.ctr, I.off[k], I.seg[k],
                    I.seg2[k], I.big[k], big_cap, m->state, m->frame, m->cube_cnt);
    }
    VL_RAW_LAUNCH(k_map_import_finish, dim3(1), dim3(64), 0, st, m->tab[0], m->tab[1], m->frame);
    if (hipGetLastError() != hipSuccess) rc = VLOAM_ERR_HIP;
    if (rc == VLOAM_OK && hipMemcpyAsync(h_result, I.res, sizeof(vloam_map_import_result), hipMemcpyDeviceToHost, st) != hipSuccess) rc = VLOAM_ERR_HIP;
  }
  if (hipStreamSynchronize(st) != hipSuccess) rc = VLOAM_ERR_HIP;   // (also on a failure: the chain may still read the allocation)
  (void)hipFree(A.base);
  return rc;
}

}  // namespace vloam
