// Map merge on gfx950 (vloam_map_merge / vloam_map_merge_device): two point clouds of another map, and the transform between the maps, are folded
// into the voxel tables of a LIVE handle.  A code object of its own, like map_import.hip and map_carve.hip: a handle that never merges launches and
// allocates nothing of this, and no kernel of a sweep changes.  The chain has map_import.hip's shape (the text the two share: map_cloud_dev.h) and
// runs once per call on the mapping stream, with nothing of the handle in flight, on temporary allocations:
//   k_map_merge_prepare  1 thread  the counters and the result record start over; a handle whose window was never placed (the host says so) gets
//                                  the window and pose of a start at the identity (apply only)
//   k_map_merge_key      grid      per point: finite? the transform (f64, rounded to f32) into xp[]; cube and voxel as k_map_insert keys a
//                                  map-frame point; find-or-insert of the KEY in a temporary hash of the call's own voxels, integer atomicAdd of
//                                  the entry's point counter; the first claimant appends the entry to the voxel list
//   k_map_merge_scan     1 WG      exclusive scan of the voxel list's counters: one segment of point indices per voxel
//   k_map_merge_scatter  grid      point index -> its voxel's segment
//   k_map_merge_reduce   grid      per voxel of up to kImportLaneSort points: one lane orders the segment ascending and folds; fuller voxels go
//                                  onto the big list
//   k_map_merge_big      1 WG/voxel  the LDS network or the ranking, then one lane folds
//   k_map_merge_dry      grid      (dry run, instead of the four above) per voxel of the list: the lookup and the point counters
//   k_map_merge_finish   1 thread  60 % rule of k_map_finalize on the live records and block keys -> the sticky map-full error
// A live record carries a value, so nothing of the chain's scratch lives in the table (the import keeps it in count / pend_cnt of the records it
// claims): the voxel list, the counters and the segments hang on the temporary hash, and the table is touched by the FOLD alone, every voxel by
// exactly one lane — one find-or-insert with k_map_insert's CAS and probe bound, then
//   no live record (none, or a tombstone of the key, which is reused):  0 + p0 + p1 + ... in input order, / (float)n, count 1
//   a live merged record (seq 0, not raw):                              centroid + p0 + p1 + ..., / (float)(1 + n), count 1
//   a raw voxel (kRecRaw):                                              untouched; its points are dropped and counted
// == what the reference holds after appending the points to the cube's cloud and re-filtering that cube (LM:654-659, LM:689-702), and what
// map_finalize_body does for a valid cube.  No floating-point atomics anywhere: the result is a function of table state, arrays and options alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "map_kernels.h"
#include "map_cloud_dev.h"

namespace vloam {

struct MergeCtr { int n_vox[2]; int n_big[2]; };
struct __attribute__((aligned(16))) MergeEnt { u64 key; int cnt; int v; };   // temporary hash: voxel key (0 = empty) | its points | its place in the voxel list
static_assert(sizeof(MergeEnt) == 16, "one entry, one 16-byte line");
// what one lane has counted over its voxels; summed per wavefront before it reaches the result record
struct MergeTally { long long n_new = 0, n_hit = 0, n_raw = 0; int n_newvox = 0, n_newkey = 0, most = 0; };

__global__ __launch_bounds__(64) void k_map_merge_prepare(MapState* ms, int place_start, long long n0, long long n1, MergeCtr* ctr, vloam_map_merge_result* res) {
  if (threadIdx.x != 0) return;
  // place_start (the host's map_window_never_placed, applied calls only): the handle gets what an import at the identity gives it, the default
  // window and the identity pose
  if (place_start) {
    MapState s = *ms;
    const double q[4] = {0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
    cloud_place_start(s, q, t);
    *ms = s;
  }
  MergeCtr c;
  memset(&c, 0, sizeof(c));
  *ctr = c;
  vloam_map_merge_result r;
  memset(&r, 0, sizeof(r));
  r.n_in[0] = n0; r.n_in[1] = n1;
  *res = r;
}

// f64 from the f32 components, every operation rounded on its own (the file is built with -ffp-contract=off), then rounded to f32
__device__ __forceinline__ float4 merge_transform(const MergeXf& X, const float4 p) {
  if (X.identity) return p;   // taken as it is: an exported map goes in bit for bit (the sign of a zero included)
  const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
  float4 o;
  o.x = (float)(((X.R[0] * x + X.R[1] * y) + X.R[2] * z) + X.t[0]);
  o.y = (float)(((X.R[3] * x + X.R[4] * y) + X.R[5] * z) + X.t[1]);
  o.z = (float)(((X.R[6] * x + X.R[7] * y) + X.R[8] * z) + X.t[2]);
  o.w = p.w;
  return o;
}

// hmask + 1 >= 2 n entries, zeroed: at most n keys ever enter, so a probe always ends at the key or at an empty entry
__global__ __launch_bounds__(256) void k_map_merge_key(const float4* __restrict__ pts, int n, int kind, MergeXf X, float inv, const MapState* __restrict__ ms,
                                                       float4* __restrict__ xp, MergeEnt* H, unsigned hmask, int* __restrict__ ent_of, int* __restrict__ vox_ent,
                                                       MergeCtr* ctr, vloam_map_merge_result* res) {
  const int cW = ms->cenW, cH = ms->cenH, cD = ms->cenD;
  int n_out = 0, n_bad = 0;
  for (int i0 = (int)(blockIdx.x * 256u); i0 < n; i0 += (int)(gridDim.x * 256u)) {   // workgroup-uniform (n <= 2^24)
    const int i = i0 + (int)threadIdx.x;
    if (i >= n) continue;
    const float4 p = pts[i];
    int found = -1;
    u64 key;
    if (!cloud_finite(p)) n_bad++;
    else {
      const float4 q = merge_transform(X, p);
      xp[i] = q;
      if (!cloud_key(q, inv, cW, cH, cD, &key)) n_out++;   // (a coordinate that left f32's range is beyond the reach, like any far point)
      else {
        unsigned e = (unsigned)mix64(key) & hmask;
        for (unsigned probe = 0; probe <= hmask; probe++, e = (e + 1) & hmask) {
          const u64 old = atomicCAS(&H[e].key, 0ull, key);
          if (old != 0ull && old != key) continue;
          if (old == 0ull) {   // first claimant: the voxel joins the list (at most one voxel per point: the list holds n entries)
            const int v = atomicAdd(&ctr->n_vox[kind], 1);
            vox_ent[v] = (int)e;
            H[e].v = v;
          }
          atomicAdd(&H[e].cnt, 1);
          found = (int)e;
          break;
        }
      }
    }
    ent_of[i] = found;
  }
  cloud_count_drops(n_out, n_bad, &res->n_outside_window[kind], &res->n_nonfinite[kind]);
}

__global__ __launch_bounds__(256) void k_map_merge_scan(int kind, const MergeEnt* __restrict__ H, const int* __restrict__ vox_ent, const MergeCtr* __restrict__ ctr,
                                                        int* __restrict__ off) {
  __shared__ int part[256];
  const int nv = ctr->n_vox[kind];
  int most = 0;
  const int base = cloud_scan(nv, [&](int e) { return H[vox_ent[e]].cnt; }, off, part, &most);
  if (threadIdx.x == 0) off[nv] = base;
}

__global__ __launch_bounds__(256) void k_map_merge_scatter(int n, MergeEnt* H, const int* __restrict__ ent_of, const int* __restrict__ off, int* __restrict__ seg) {
  for (int i = (int)(blockIdx.x * 256u + threadIdx.x); i < n; i += (int)(gridDim.x * 256u)) {
    const int e = ent_of[i];
    if (e < 0) continue;
    const int pos = atomicSub(&H[e].cnt, 1) - 1;
    seg[off[H[e].v] + pos] = i;
  }
}

// One lane, one voxel: cnt points of the call share `key`; idx[0 .. cnt): their indices ascending (apply only).  The header says what happens.
__device__ __forceinline__ void merge_fold(const VoxelTable& T, u64 key, const float4* __restrict__ xp, const int* idx, int cnt, int kind, bool apply,
                                           const MapState* ms, MapFrame* fr, int* __restrict__ cube_cnt, MergeTally& L) {
  RecVal v;
  bool found = false, claimed = false;
  unsigned s = 0;
  if (apply) {
    s = (unsigned)mix64(key) & T.mask;
    for (int probe = 0; probe < kMaxProbe && !found; probe++) {
      const u64 old = atomicCAS(&T.rec[s].key, 0ull, key);
      if (old == 0ull || old == key) { found = true; claimed = old == 0ull; }
      else s = (s + 1) & T.mask;
    }
    if (!found) { atomicOr(&fr->error, kErrMapFull); return; }   // no slot within the probe bound: the table is overloaded
    if (!claimed) v = rec_load(&T.rec[s]);
  } else {
    bool too_long = false;
    found = rec_find(T, key, &v, &s, &too_long);
  }
  const bool held = found && !claimed;                // the table knew the key: a live record or a tombstone
  if (held && rec_live(v) && rec_raw(v.count)) { L.n_raw += cnt; return; }   // un-merged raw points: the voxel is left as it is
  const bool live = held && rec_live(v);
  if (live) L.n_hit += cnt; else L.n_new += cnt;
  if (!apply) return;
  const float4 acc = cloud_fold(live ? rec_point(v) : make_float4(0.f, 0.f, 0.f, 0.f), xp, idx, cnt, (live ? 1 : 0) + cnt);
  rec_store_value(&T.rec[s], acc, 1, 0);
  if (!live) {   // a record became live: what an inserting handle owes the map (a reused tombstone's key is counted already, as k_map_insert leaves it)
    cloud_new_voxel(T, key, kind, ms, fr, cube_cnt);
    L.n_newvox++;
    if (claimed) L.n_newkey++;
  }
  L.most = max(L.most, cnt);
}

// one add per wavefront and counter
__device__ __forceinline__ void merge_tally_flush(MergeTally L, const VoxelTable& T, int kind, vloam_map_merge_result* res) {
  for (int d = 32; d > 0; d >>= 1) {
    L.n_new += __shfl_xor(L.n_new, d); L.n_hit += __shfl_xor(L.n_hit, d); L.n_raw += __shfl_xor(L.n_raw, d);
    L.n_newvox += __shfl_xor(L.n_newvox, d); L.n_newkey += __shfl_xor(L.n_newkey, d); L.most = max(L.most, __shfl_xor(L.most, d));
  }
  if ((threadIdx.x & 63) != 0) return;
  if (L.n_new) atomicAdd((unsigned long long*)&res->n_new_points[kind], (unsigned long long)L.n_new);
  if (L.n_hit) atomicAdd((unsigned long long*)&res->n_hit_points[kind], (unsigned long long)L.n_hit);
  if (L.n_raw) atomicAdd((unsigned long long*)&res->n_skipped_raw[kind], (unsigned long long)L.n_raw);
  if (L.n_newvox) atomicAdd((unsigned long long*)&res->n_new_voxels[kind], (unsigned long long)L.n_newvox);
  if (L.n_newkey) atomicAdd(&T.stats[0], L.n_newkey);   // keys in the table, as k_map_insert counts them
  if (L.most) atomicMax(&res->max_per_voxel[kind], L.most);
}

__global__ __launch_bounds__(256) void k_map_merge_reduce(VoxelTable T, int kind, const float4* __restrict__ xp, const MergeEnt* __restrict__ H,
                                                          const int* __restrict__ vox_ent, MergeCtr* ctr, const int* __restrict__ off, int* seg, int* __restrict__ big,
                                                          int big_cap, const MapState* __restrict__ ms, MapFrame* fr, int* __restrict__ cube_cnt,
                                                          vloam_map_merge_result* res) {
  const int nv = ctr->n_vox[kind];
  MergeTally L;
  for (int v = (int)(blockIdx.x * 256u + threadIdx.x); v < nv; v += (int)(gridDim.x * 256u)) {
    const int lo = off[v], cnt = off[v + 1] - lo;
    if (cnt > kImportLaneSort) {
      const int b = atomicAdd(&ctr->n_big[kind], 1);
      if (b < big_cap) big[b] = v;   // (always: at most n / 33 voxels hold more than 32 of n points)
      continue;
    }
    int* idx = seg + lo;   // the segment is this lane's alone: ordered in place
    cloud_order_lane(idx, cnt);
    merge_fold(T, H[vox_ent[v]].key, xp, idx, cnt, kind, true, ms, fr, cube_cnt, L);
  }
  merge_tally_flush(L, T, kind, res);
}

__global__ __launch_bounds__(256) void k_map_merge_big(VoxelTable T, int kind, const float4* __restrict__ xp, const MergeEnt* __restrict__ H,
                                                       const int* __restrict__ vox_ent, const MergeCtr* __restrict__ ctr, const int* __restrict__ off, int* seg, int* seg2,
                                                       const int* __restrict__ big, int big_cap, const MapState* __restrict__ ms, MapFrame* fr,
                                                       int* __restrict__ cube_cnt, vloam_map_merge_result* res) {
  __shared__ u64 a[kImportLdsSort];
  const int tid = threadIdx.x, nb = min(ctr->n_big[kind], big_cap);
  MergeTally L;
  for (int b = (int)blockIdx.x; b < nb; b += (int)gridDim.x) {
    const int v = big[b], lo = off[v], cnt = off[v + 1] - lo;
    const int* ordered = cloud_order_block(seg, seg2, lo, cnt, a);
    if (tid == 0) merge_fold(T, H[vox_ent[v]].key, xp, ordered, cnt, kind, true, ms, fr, cube_cnt, L);
    __syncthreads();   // a[] is free for the next voxel
  }
  if (tid < 64) merge_tally_flush(L, T, kind, res);   // (lane 0 of the first wavefront holds everything)
}

// dry run: lookups only
__global__ __launch_bounds__(256) void k_map_merge_dry(VoxelTable T, int kind, const MergeEnt* __restrict__ H, const int* __restrict__ vox_ent,
                                                       const MergeCtr* __restrict__ ctr, vloam_map_merge_result* res) {
  const int nv = ctr->n_vox[kind];
  MergeTally L;
  for (int v = (int)(blockIdx.x * 256u + threadIdx.x); v < nv; v += (int)(gridDim.x * 256u)) {
    const MergeEnt E = H[vox_ent[v]];
    merge_fold(T, E.key, nullptr, nullptr, E.cnt, kind, false, nullptr, nullptr, nullptr, L);
  }
  L.most = 0;
  merge_tally_flush(L, T, kind, res);
}

// k_map_finalize's table health rule after the merge: more than 60 % of the slots hold live records (or of the block slots, keys) -> map full
__global__ __launch_bounds__(64) void k_map_merge_finish(VoxelTable T0, VoxelTable T1, MapFrame* fr) {
  const int kind = threadIdx.x;
  if (kind >= 2) return;
  const VoxelTable& T = kind ? T1 : T0;
  const long long slots = (long long)T.mask + 1, bslots = (long long)T.bslots_mask + 1;
  if ((long long)(T.stats[0] - T.stats[1]) * 10 > slots * 6 || (long long)T.stats[2] * 10 > bslots * 6) atomicOr(&fr->error, kErrMapFull);
}

// ---------------------------------------------------------------------------------------------- host side
struct MergeTmp {   // one allocation, laid out by the arena helper (dry pass to measure)
  MergeCtr* ctr = nullptr;
  vloam_map_merge_result* res = nullptr;
  float4* pts[2] = {nullptr, nullptr};    // the host form's uploaded clouds
  float4* xp[2] = {nullptr, nullptr};     // [n] the points in this map's frame
  MergeEnt* hash[2] = {nullptr, nullptr}; // [hslots] the call's own voxels by key
  int* ent_of[2] = {nullptr, nullptr};    // [n] hash entry of every point, -1: dropped
  int* vox_ent[2] = {nullptr, nullptr};   // [n] the voxel list: entries in claim order
  int* off[2] = {nullptr, nullptr};       // [n + 1] segment offsets
  int* seg[2] = {nullptr, nullptr};       // [n] point indices by voxel
  int* seg2[2] = {nullptr, nullptr};      // [n] the rank path's output
  int* big[2] = {nullptr, nullptr};       // [n / 33 + 1] voxels of more than kImportLaneSort points
};
static size_t merge_hash_slots(int n) {
  size_t s = 256;
  while (s < 2 * (size_t)n) s <<= 1;
  return s;
}
static bool merge_layout(MergeTmp* I, Arena& A, const int n[2], bool upload, bool apply) {
  bool ok = A.take(&I->ctr, 1) && A.take(&I->res, 1);
  for (int k = 0; k < 2 && ok; k++) {
    if (n[k] == 0) continue;
    const size_t nk = (size_t)n[k];
    ok = (!upload || A.take(&I->pts[k], nk)) && A.take(&I->xp[k], nk) && A.take(&I->hash[k], merge_hash_slots(n[k])) && A.take(&I->ent_of[k], nk) &&
         A.take(&I->vox_ent[k], nk);
    if (apply) ok = ok && A.take(&I->off[k], nk + 1) && A.take(&I->seg[k], nk) && A.take(&I->seg2[k], nk) && A.take(&I->big[k], nk / (kImportLaneSort + 1) + 1);
  }
  return ok;
}

vloam_status map_merge_run(MapContext* m, hipStream_t st, const MergeXf& X, const void* const cloud[2], const int n[2], bool host_clouds, bool apply,
                           bool place_start, vloam_map_merge_result* h_result) {
  MergeTmp I;
  Arena dry;
  merge_layout(&I, dry, n, host_clouds, apply);
  Arena A;
  A.cap = dry.off; A.dry = false;
  if (hipMalloc((void**)&A.base, A.cap) != hipSuccess) return VLOAM_ERR_HIP;
  vloam_status rc = merge_layout(&I, A, n, host_clouds, apply) ? VLOAM_OK : VLOAM_ERR_HIP;
  const float4* pts[2] = {nullptr, nullptr};
  for (int k = 0; k < 2 && rc == VLOAM_OK; k++) {
    if (n[k] == 0) continue;
    if (host_clouds) {
      if (hipMemcpyAsync(I.pts[k], cloud[k], (size_t)n[k] * sizeof(float4), hipMemcpyHostToDevice, st) != hipSuccess) rc = VLOAM_ERR_HIP;
      pts[k] = I.pts[k];
    } else pts[k] = (const float4*)cloud[k];
  }
  if (rc == VLOAM_OK) {
    VL_RAW_LAUNCH(k_map_merge_prepare, dim3(1), dim3(64), 0, st, m->state, (apply && place_start) ? 1 : 0, (long long)n[0], (long long)n[1], I.ctr, I.res);
    for (int k = 0; k < 2 && rc == VLOAM_OK; k++) {
      if (n[k] == 0) continue;
      const VoxelTable& T = m->tab[k];
      const size_t hslots = merge_hash_slots(n[k]);
      const unsigned blocks = ((unsigned)n[k] + 255u) / 256u, grid = blocks < (unsigned)kImportMaxGrid ? blocks : (unsigned)kImportMaxGrid;
      const int big_cap = n[k] / (kImportLaneSort + 1) + 1;
      if (hipMemsetAsync(I.hash[k], 0, hslots * sizeof(MergeEnt), st) != hipSuccess) { rc = VLOAM_ERR_HIP; break; }
      VL_RAW_LAUNCH(k_map_merge_key, dim3(grid), dim3(256), 0, st, pts[k], n[k], k, X, m->inv_leaf[k], m->state, I.xp[k], I.hash[k], (unsigned)(hslots - 1), I.ent_of[k],
                    I.vox_ent[k], I.ctr, I.res);
      if (!apply) {
        VL_RAW_LAUNCH(k_map_merge_dry, dim3(grid), dim3(256), 0, st, T, k, I.hash[k], I.vox_ent[k], I.ctr, I.res);
        continue;
      }
      VL_RAW_LAUNCH(k_map_merge_scan, dim3(1), dim3(256), 0, st, k, I.hash[k], I.vox_ent[k], I.ctr, I.off[k]);
      VL_RAW_LAUNCH(k_map_merge_scatter, dim3(grid), dim3(256), 0, st, n[k], I.hash[k], I.ent_of[k], I.off[k], I.seg[k]);
      VL_RAW_LAUNCH(k_map_merge_reduce, dim3(grid), dim3(256), 0, st, T, k, I.xp[k], I.hash[k], I.vox_ent[k], I.ctr, I.off[k], I.seg[k], I.big[k], big_cap, m->state,
                    m->frame, m->cube_cnt, I.res);
      VL_RAW_LAUNCH(k_map_merge_big, dim3((unsigned)(big_cap < 1024 ? big_cap : 1024)), dim3(256), 0, st, T, k, I.xp[k], I.hash[k], I.vox_ent[k], I.ctr, I.off[k], I.seg[k],
                    I.seg2[k], I.big[k], big_cap, m->state, m->frame, m->cube_cnt, I.res);
    }
    if (rc == VLOAM_OK && apply) VL_RAW_LAUNCH(k_map_merge_finish, dim3(1), dim3(64), 0, st, m->tab[0], m->tab[1], m->frame);
    if (hipGetLastError() != hipSuccess) rc = VLOAM_ERR_HIP;
    if (rc == VLOAM_OK && hipMemcpyAsync(h_result, I.res, sizeof(vloam_map_merge_result), hipMemcpyDeviceToHost, st) != hipSuccess) rc = VLOAM_ERR_HIP;
  }
  if (hipStreamSynchronize(st) != hipSuccess) rc = VLOAM_ERR_HIP;   // (also on a failure: the chain may still read the allocation)
  (void)hipFree(A.base);
  return rc;
}

}  // namespace vloam
