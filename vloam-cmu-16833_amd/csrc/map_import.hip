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
#include "map_cloud_dev.h"   // what this chain shares with map_merge.hip: keying, scan, the three ordering paths, the input-order fold

namespace vloam {

struct ImportPose { double q[4], t[3]; };   // by value: the host's transform needs no upload
struct ImportCtr { int n_vox[2]; int n_big[2]; };

__global__ __launch_bounds__(64) void k_map_import_prepare(MapState* ms, MapFrame* fr, int* stats0, int* stats1, ImportPose pose, long long n0, long long n1,
                                                           ImportCtr* ctr, vloam_map_import_result* res) {
  if (threadIdx.x != 0) return;
  MapState s = *ms;
  cloud_place_start(s, pose.q, pose.t);
  const int cen[3] = {s.cenW, s.cenH, s.cenD};
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

// keying: cloud_key (map_cloud_dev.h); find-or-insert with the table's CAS and probe bound
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
    u64 key;
    if (!cloud_finite(p)) n_bad++;
    else if (!cloud_key(p, inv, cW, cH, cD, &key)) n_out++;
    else {
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
    slot_of[i] = found;
  }
  cloud_count_drops(n_out, n_bad, &res->n_outside_window[kind], &res->n_nonfinite[kind]);
}

// off[v]: first place of voxel v's segment, off[n_vox]: points placed; the table's key count and the result's voxel figures
__global__ __launch_bounds__(256) void k_map_import_scan(VoxelTable T, int kind, const int* __restrict__ vox_slot, const ImportCtr* __restrict__ ctr,
                                                         int* __restrict__ off, vloam_map_import_result* res) {
  __shared__ int part[256];
  const int tid = threadIdx.x, nv = ctr->n_vox[kind];
  int most = 0;
  const int base = cloud_scan(nv, [&](int e) { return T.rec[vox_slot[e]].pend_cnt; }, off, part, &most);
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

// One lane: the voxel's points in the order of idx[0 .. cnt) -> the record of slot s (cloud_fold from zero), its occupancy block and its cube's count
__device__ __forceinline__ void import_fold(const VoxelTable& T, int s, const float4* __restrict__ pts, const int* idx, int cnt, int kind, const MapState* ms,
                                            MapFrame* fr, int* __restrict__ cube_cnt) {
  rec_store_value(&T.rec[s], cloud_fold(make_float4(0.f, 0.f, 0.f, 0.f), pts, idx, cnt, cnt), 1, 0);
  cloud_new_voxel(T, T.rec[s].key, kind, ms, fr, cube_cnt);
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
    cloud_order_lane(idx, cnt);
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
    const int* ordered = cloud_order_block(seg, seg2, lo, cnt, a);
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
