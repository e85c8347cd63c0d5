// laserMapping on gfx950, the scan-feature VoxelGrid (LM:432-440): a sweep's lessSharp / lessFlat clouds -> the stack set the mapping chain
// (map_kernels.hip) consumes.  Needs nothing but the scan registration output and runs on the scan-registration stream.
//   k_map_ds_bin    grid      pcl::VoxelGrid of the scan features (LM:432-440) without a global hash, pass 1: PCL's cell index from the cloud's
//                             bounding box (incl. its index-overflow guard: output = input), sample splitters, (cell << 24 | point) keys binned
//   k_map_ds_reduce 64 WGs    pass 2: bins drawn by ticket, sorted in LDS, output slots by a decoupled look-back over the bins' cell counts,
//                             per cell the input-ordered f32 centroid, output in PCL's order (cells ascending)
#include <hip/hip_runtime.h>
#include <limits.h>
#include "map_kernels.h"
#include "bitonic.h"

namespace vloam {

// pcl::VoxelGrid<PointXYZI> (PCL 1.10 filters/impl/voxel_grid.hpp applyFilter) of laserCloudCornerLast / laserCloudSurfLast, LM:432-440:
// getMinMax3D -> the overflow guard (more than INT_MAX cells in the bounding box: a warning and output = input) -> cell index
// idx = ijk0 + ijk1 * div0 + ijk2 * div0 * div1 with ijk = floor(p * inverse_leaf) - min_b -> sort by idx -> one centroid per cell, f32
// sums in the order of the sorted index vector (std::sort leaves the order inside a cell open; canonical here and in the oracle: input order).
//
// Two launches, no global hash, no whole-chip ranking (rounds 1 - 4 hashed the points into a table, ranked the occupied cells by counting
// — u^2 compares — and folded one wavefront per cell: 80 k of the 227 k wavefront-microseconds a sweep cost at B = 8, 14 MB of traffic for
// 0.6 MB of points):
//   k_map_ds_bin     cuts the key space into P = ceil(n / 512) bins at the quantiles of a sample of the cloud (every workgroup sorts the same
//                    <= 2 048 sampled keys in LDS: same splitters everywhere, no exchange), and appends every point's sort key
//                    (cell index << 24 | point index) to its bin's region — one device-scope atomic per run of equal bins in a wavefront;
//   k_map_ds_reduce  one workgroup per bin: bitonic sort of the bin's keys in LDS, cell heads, the bin's cell count published for the bins
//                    behind it (look-back over the lower bins, in ticket order: a workgroup only ever waits for workgroups that started
//                    before it), centroids in input order, written at their final place in VoxelGrid's output order.
// A bin is a contiguous range of cell indices, so bin order == output order.  Correctness never rests on the sample: a bin that outgrows
// its region (kDsBinCap keys, e.g. thousands of points in ONE cell with a coarse leaf) spills into an overflow list and takes the slow path
// (gather, rank by counting in global memory); test_scan_voxel_bins_overflow drives it.
struct DsGrid { float mnb[3]; int div0, div1; bool overflow; };

// getMinMax3D + the guard + min_b / div_b (voxel_grid.hpp), from the per-scan-line boxes k_sr_compact left; every lane gets the result
__device__ __forceinline__ DsGrid ds_grid(const FrameScalars* __restrict__ S, int kind, float inv) {
  const int lane = threadIdx.x & 63;
  float mn[3], mx[3];
#pragma unroll
  for (int a = 0; a < 3; a++) { mn[a] = S->less_bbox[kind][lane][a]; mx[a] = S->less_bbox[kind][lane][3 + a]; }
#pragma unroll
  for (int a = 0; a < 3; a++)
    for (int d = 32; d > 0; d >>= 1) { mn[a] = fminf(mn[a], __shfl_xor(mn[a], d)); mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], d)); }
  DsGrid g;
  const long long dx = (long long)((mx[0] - mn[0]) * inv) + 1, dy = (long long)((mx[1] - mn[1]) * inv) + 1, dz = (long long)((mx[2] - mn[2]) * inv) + 1;
  g.overflow = dx * dy * dz > (long long)INT_MAX;
  int minb[3], maxb[3];
#pragma unroll
  for (int a = 0; a < 3; a++) { minb[a] = (int)floorf(mn[a] * inv); maxb[a] = (int)floorf(mx[a] * inv); g.mnb[a] = (float)minb[a]; }
  g.div0 = maxb[0] - minb[0] + 1; g.div1 = maxb[1] - minb[1] + 1;
  return g;
}
__device__ __forceinline__ u64 ds_cell(float4 p, float inv, const DsGrid& g) {
  const int i0 = (int)(floorf(p.x * inv) - g.mnb[0]), i1 = (int)(floorf(p.y * inv) - g.mnb[1]), i2 = (int)(floorf(p.z * inv) - g.mnb[2]);
  return (u64)(unsigned)i0 + (u64)(unsigned)g.div0 * ((u64)(unsigned)i1 + (u64)(unsigned)g.div1 * (u64)(unsigned)i2);
}
constexpr int kDsIdxBits = 24;   // point index in the low bits of a sort key (max_points <= 2^24, vloam_create); the cell index (< 2^33) above
__device__ __forceinline__ int ds_num_bins(int n) { const int p = (n + kDsBinTarget - 1) / kDsBinTarget; return p < 1 ? 1 : (p > kDsMaxBins ? kDsMaxBins : p); }
__device__ __forceinline__ int ds_num_samples(int P) { return P <= 32 ? 256 : (P <= 64 ? 512 : (P <= 128 ? 1024 : 2048)); }
// bin of a cell: the number of splitters <= cell (upper bound; equal cells always share a bin)
__device__ __forceinline__ int ds_bin_of(const u64* split, int P, u64 cell) {
  int lo = 0, hi = P - 1;   // answer in [0, P - 1]
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (split[mid] <= cell) lo = mid + 1; else hi = mid; }
  return lo;
}

constexpr int kDsTile = 2048;   // points a workgroup of the binning pass takes per trip
constexpr int kDsReduceGrid = 64;   // workgroups of the reduce pass per cloud (each keeps drawing bins)
__global__ __launch_bounds__(256) void k_map_ds_bin(const float4* __restrict__ corner_last, const float4* __restrict__ surf_last,
                                                    const FrameScalars* __restrict__ S, DsScratch D0, DsScratch D1, float inv0, float inv1,
                                                    float4* __restrict__ stack0, float4* __restrict__ stack1, StackInfo* fr, size_t ss) {
  VL_SESSION(ss); RB(corner_last); RB(surf_last); RB(S); D0.rebase(so_); D1.rebase(so_); RB(stack0); RB(stack1); RB(fr);
  __shared__ __attribute__((aligned(16))) u64 s_key[2048];
  __shared__ __attribute__((aligned(16))) u64 s_srt[512];
  __shared__ u64 s_split[kDsMaxBins];
  __shared__ int s_cnt[kDsMaxBins], s_base[kDsMaxBins];
  const int kind = blockIdx.y, tid = threadIdx.x;
  const DsScratch D = kind ? D1 : D0;
  const float inv = kind ? inv1 : inv0;
  const float4* pts = kind ? surf_last : corner_last;
  float4* stack = kind ? stack1 : stack0;
  const int n = kind ? S->n_less_flat : S->n_less_sharp;
  if (blockIdx.x == 0 && tid == 0) D.cursor[kDsMaxBins + 1] = 0;   // the reduce pass's ticket counter (nothing of the previous sweep draws from it any more)
  if (n <= 0) { if (blockIdx.x == 0 && tid == 0) fr->n_stack[kind] = 0; return; }
  if ((int)blockIdx.x * kDsTile >= n) return;
  const DsGrid g = ds_grid(S, kind, inv);
  if (g.overflow) {   // "Leaf size is too small for the input dataset. Integer indices would overflow." — output = *input_
    for (int t0 = blockIdx.x * kDsTile; t0 < n; t0 += gridDim.x * kDsTile)   // (only the workgroups whose first tile exists are here)
      for (int i = t0 + tid; i < min(t0 + kDsTile, n); i += 256) if (i < D.stack_cap) stack[i] = pts[i];
    if (blockIdx.x == 0 && tid == 0) { fr->n_stack[kind] = min(n, D.stack_cap); if (n > D.stack_cap) atomicOr(&fr->error, kErrStackFull); }
    return;
  }
  const int P = ds_num_bins(n);
  if (P > 1) {
    // the splitters: P - 1 quantiles of Sn evenly spaced sample points; every workgroup computes the same ones
    const int Sn = ds_num_samples(P);
    for (int j = tid; j < Sn; j += 256) s_key[j] = ds_cell(pts[(int)(((long long)j * n) / Sn)], inv, g);
    __syncthreads();
    const u64* srt = s_key;
    if (Sn <= 512) {
      // few samples: rank by counting (every lane reads every key once, broadcast LDS reads, no dependent exchange stages — a bitonic
      // network over 512 keys is ~45 dependent stages; this is the prologue of EVERY workgroup of the pass)
      for (int j = tid; j < Sn; j += 256) {
        const u64 mine = s_key[j];
        int rank = 0;
#pragma unroll 8
        for (int e = 0; e < Sn; e += 2) {   // (unrolled: eight LDS reads in flight, or every iteration waits out the LDS latency)
          const ulonglong2 k2 = *(const ulonglong2*)&s_key[e];
          rank += (k2.x < mine || (k2.x == mine && e < j)) ? 1 : 0;
          rank += (k2.y < mine || (k2.y == mine && e + 1 < j)) ? 1 : 0;
        }
        s_srt[rank] = mine;
      }
      __syncthreads();
      srt = s_srt;
    } else {
      block_bitonic_sort_u64(s_key, Sn, tid, 256);
    }
    for (int j = tid; j < P - 1; j += 256) {
      const u64 sp = srt[(int)(((long long)(j + 1) * Sn) / P)];
      s_split[j] = sp;
      if (blockIdx.x == 0) D.splitters[j] = sp;   // the reduce pass's slow path tells the bins of the overflow list by them
    }
    __syncthreads();
  }
  for (int t0 = blockIdx.x * kDsTile; t0 < n; t0 += gridDim.x * kDsTile) {
    // the tile's points are counted per bin in LDS first: ONE device-scope cursor update per (workgroup, bin) and one memory round trip for
    // all of them, instead of a dependent atomic round trip per 64 points
    constexpr int kPer = kDsTile / 256;
    __syncthreads();
    for (int b = tid; b < P; b += 256) s_cnt[b] = 0;
    __syncthreads();
    float4 p[kPer];
#pragma unroll
    for (int e = 0; e < kPer; e++) { const int i = t0 + e * 256 + tid; p[e] = i < n ? pts[i] : make_float4(0.f, 0.f, 0.f, 0.f); }
    u64 cell[kPer];
    int bin[kPer], pos[kPer];
#pragma unroll
    for (int e = 0; e < kPer; e++) {
      const int i = t0 + e * 256 + tid;
      bin[e] = -1; pos[e] = 0; cell[e] = 0ull;
      if (i < n) {
        cell[e] = ds_cell(p[e], inv, g);
        bin[e] = P > 1 ? ds_bin_of(s_split, P, cell[e]) : 0;
        pos[e] = atomicAdd(&s_cnt[bin[e]], 1);
      }
    }
    __syncthreads();
    for (int b = tid; b < P; b += 256) { const int c = s_cnt[b]; s_base[b] = c > 0 ? atomicAdd(&D.cursor[b], c) : 0; }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kPer; e++) {
      const int i = t0 + e * 256 + tid;
      if (i < n) {
        const u64 key = (cell[e] << kDsIdxBits) | (u64)(unsigned)i;
        const int at = s_base[bin[e]] + pos[e];
        if (at < kDsBinCap) D.region[(size_t)bin[e] * kDsBinCap + at] = key;
        else { const int o = atomicAdd(&D.cursor[kDsMaxBins], 1); D.over[o] = key; }   // (o < n <= max_points: every point is written exactly once)
      }
    }
  }
}

__device__ __forceinline__ float rl(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }

// heads / look-back / centroids of one bin whose keys lie sorted in `key` (LDS on the fast path, global memory on the slow one)
template <bool LDS_KEYS>
__device__ __forceinline__ void ds_reduce_sorted(const u64* key, int m, int bin, int P, const float4* __restrict__ pts, float4* __restrict__ stack,
                                                 const DsScratch& D, StackInfo* fr, int kind, unsigned gen, int* s_cnt /* [256 + 8] */, int* s_big /* [3 * kDsBigCap + 1] */) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // contiguous chunks: thread t owns keys [t * per, t * per + per)
  const int per = (m + 255) / 256;
  const int c0 = min(tid * per, m), c1 = min(c0 + per, m);
  int heads = 0;
  for (int i = c0; i < c1; i++) heads += (i == 0 || (key[i] >> kDsIdxBits) != (key[i - 1] >> kDsIdxBits)) ? 1 : 0;
  // block exclusive scan of the head counts
  int inc = heads;
  for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d); if (lane >= d) inc += o; }
  if (lane == 63) s_cnt[256 + wave] = inc;
  if (tid == 0) s_big[0] = 0;
  __syncthreads();
  int wbase = 0, u = 0;
  for (int w = 0; w < 4; w++) { const int t = s_cnt[256 + w]; wbase += w < wave ? t : 0; u += t; }
  const int rank0 = wbase + inc - heads;   // output rank (inside the bin) of this thread's first head
  // publish this bin's cell count, then add up the bins in front (look-back; every one of them started before this workgroup took its ticket)
  u64* done = D.done;
  if (tid == 0) __hip_atomic_store(&done[bin], ((u64)gen << 32) | (u64)(unsigned)u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  int before = 0;
  if (wave == 0) {
    bool bad = false;
    for (int b = lane; b < bin; b += 64) {
      u64 v = 0ull;
      int spins = 0;
      for (;;) {
        v = __hip_atomic_load(&done[b], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)(v >> 32) == gen) break;
        if (++spins > (1 << 22)) { bad = true; break; }
        __builtin_amdgcn_s_sleep(2);
      }
      before += (int)(unsigned)(v & 0xffffffffull);
    }
    for (int d = 32; d > 0; d >>= 1) before += __shfl_xor(before, d);
    // (never seen: a bounded wait instead of a hang.)  The offset would come from a partial sum: this bin stores NOTHING (its centroids would
    // land on other bins' slots) and the sweep's stack is declared empty, so the mapping of this sweep associates nothing instead of
    // consuming misplaced centroids; vloam_sync reports the sticky bit
    const bool any_bad = __ballot(bad) != 0ull;
    if (any_bad && lane == 0) { atomicOr(&fr->error, kErrSolverSync); }
    if (lane == 0) s_cnt[0] = any_bad ? -1 : before;
  }
  __syncthreads();
  const bool timed_out = s_cnt[0] < 0;
  before = timed_out ? D.stack_cap : s_cnt[0];   // (every output slot then counts as beyond the stack: nothing is stored)
  // centroids: the thread that owns a head walks the cell (its points in input order: the sort key ends in the point index); cells of more
  // than kDsBigCell points are left to a whole wavefront each
  int r = rank0;
  for (int i = c0; i < c1; i++) {
    const u64 ci = key[i] >> kDsIdxBits;
    if (!(i == 0 || ci != (key[i - 1] >> kDsIdxBits))) continue;
    int e = i + 1;
    while (e < m && (key[e] >> kDsIdxBits) == ci) e++;
    const int out = before + r;
    r++;
    if (out >= D.stack_cap) continue;   // reported by the last bin
    if (e - i > kDsBigCell) {
      const int q = atomicAdd(&s_big[0], 1);
      if (q < kDsBigCap) { s_big[1 + 3 * q] = i; s_big[2 + 3 * q] = e; s_big[3 + 3 * q] = out; }
      else {   // (more big cells than the list holds: this thread folds it after all)
        float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
        for (int j = i; j < e; j++) { const float4 p = pts[(int)(key[j] & ((1ull << kDsIdxBits) - 1ull))]; sx += p.x; sy += p.y; sz += p.z; si += p.w; }
        const float nn = (float)(e - i);
        stack[out] = make_float4(sx / nn, sy / nn, sz / nn, si / nn);
      }
      continue;
    }
    float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
    for (int j = i; j < e; j += 4) {   // four loads in flight, added in order
      float4 p[4];
#pragma unroll
      for (int q = 0; q < 4; q++) if (j + q < e) p[q] = pts[(int)(key[j + q] & ((1ull << kDsIdxBits) - 1ull))];
#pragma unroll
      for (int q = 0; q < 4; q++) if (j + q < e) { sx += p[q].x; sy += p[q].y; sz += p[q].z; si += p[q].w; }
    }
    const float nn = (float)(e - i);
    stack[out] = make_float4(sx / nn, sy / nn, sz / nn, si / nn);
  }
  __syncthreads();
  const int nbig = min(s_big[0], kDsBigCap);
  for (int q = wave; q < nbig; q += 4) {   // a wavefront per big cell: 64 points fetched at once, folded one by one (f32, CentroidPoint's order)
    const int i = s_big[1 + 3 * q], e = s_big[2 + 3 * q], out = s_big[3 + 3 * q];
    float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
    for (int j0 = i; j0 < e; j0 += 64) {
      const int mm = min(64, e - j0);
      const float4 p = lane < mm ? pts[(int)(key[j0 + lane] & ((1ull << kDsIdxBits) - 1ull))] : make_float4(0.f, 0.f, 0.f, 0.f);
      for (int t = 0; t < mm; t++) { sx += rl(p.x, t); sy += rl(p.y, t); sz += rl(p.z, t); si += rl(p.w, t); }
    }
    if (lane == 0) { const float nn = (float)(e - i); stack[out] = make_float4(sx / nn, sy / nn, sz / nn, si / nn); }
  }
  if (bin == P - 1 && tid == 0) {
    // the last bin has seen every other bin's count, i.e. every workgroup of this pass is done with the region counters, the overflow list
    // and the ticket: hand them back clean for the next sweep
    const int total = timed_out ? 0 : before + u;
    fr->n_stack[kind] = min(total, D.stack_cap);
    if (total > D.stack_cap) atomicOr(&fr->error, kErrStackFull);
    D.cursor[kDsMaxBins] = 0; D.cursor[kDsMaxBins + 2] = 0;   // (the ticket counter is reset by the next sweep's binning pass: workgroups still draw from it)
  }
}

__global__ __launch_bounds__(256) void k_map_ds_reduce(const float4* __restrict__ corner_last, const float4* __restrict__ surf_last,
                                                       const FrameScalars* __restrict__ S, DsScratch D0, DsScratch D1, float inv0, float inv1,
                                                       float4* __restrict__ stack0, float4* __restrict__ stack1, StackInfo* __restrict__ fr, unsigned gen,
                                                       size_t ss) {
  VL_SESSION(ss); RB(corner_last); RB(surf_last); RB(S); D0.rebase(so_); D1.rebase(so_); RB(stack0); RB(stack1); RB(fr);
  __shared__ __attribute__((aligned(16))) u64 s_key[kDsBinCap];
  __shared__ u64 s_split[kDsMaxBins];
  __shared__ int s_cnt[256 + 8];
  __shared__ int s_big[3 * kDsBigCap + 1];
  __shared__ int s_bin;
  const int kind = blockIdx.y, tid = threadIdx.x;
  const DsScratch D = kind ? D1 : D0;
  const float inv = kind ? inv1 : inv0;
  const float4* pts = kind ? surf_last : corner_last;
  float4* stack = kind ? stack1 : stack0;
  const int n = kind ? S->n_less_flat : S->n_less_sharp;
  if (n <= 0) return;
  const int P = ds_num_bins(n);
  if ((int)blockIdx.x >= P) return;
  if (ds_grid(S, kind, inv).overflow) return;   // the binning pass copied the cloud (voxel_grid.hpp's guard)
  // Bins are taken in ticket order, not in blockIdx order: the look-back then only waits for workgroups that are already running.  The
  // grid is a fraction of kDsMaxBins (a capacity): a workgroup keeps taking tickets until the bins are gone — workgroups that only
  // find out that there is nothing for them cost a wave slot for a memory round trip each, and on a chip full of sessions that adds up
  // (8 192 such workgroups per launch at B = 16 were 85 % of this kernel's wave-microseconds).
  for (;;) {
  __syncthreads();   // (the previous bin's LDS is no longer read)
  if (tid == 0) s_bin = atomicAdd(&D.cursor[kDsMaxBins + 1], 1);
  __syncthreads();
  const int bin = s_bin;
  if (bin >= P) {
    return;   // every ticket is out (the counter is reset by the next sweep's binning pass)
  }
  const int m_raw = D.cursor[bin];
  __syncthreads();
  if (tid == 0) D.cursor[bin] = 0;   // this bin's region counter, clean for the next sweep
  if (m_raw <= kDsBinCap) {
    int P2 = 256;
    while (P2 < m_raw) P2 <<= 1;
    const u64* reg = D.region + (size_t)bin * kDsBinCap;
    for (int i = tid; i < P2; i += 256) s_key[i] = i < m_raw ? reg[i] : ~0ull;
    __syncthreads();
    block_bitonic_sort_u64(s_key, P2, tid, 256);
    ds_reduce_sorted<true>(s_key, m_raw, bin, P, pts, stack, D, fr, kind, gen, s_cnt, s_big);
    continue;
  }
  // ---- slow path: the bin outgrew its region.  Gather region + this bin's share of the overflow list, rank by counting (keys are unique:
  // they end in the point index), continue from global memory.
  const int n_over = D.cursor[kDsMaxBins];
  for (int j = tid; j < P - 1; j += 256) s_split[j] = D.splitters[j];
  __syncthreads();
  int mine = 0;
  for (int j = tid; j < n_over; j += 256) mine += (P > 1 ? ds_bin_of(s_split, P, D.over[j] >> kDsIdxBits) : 0) == bin ? 1 : 0;
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
  if ((tid & 63) == 0) s_cnt[256 + (tid >> 6)] = mine;
  __syncthreads();
  const int m = kDsBinCap + s_cnt[256] + s_cnt[257] + s_cnt[258] + s_cnt[259];
  __syncthreads();
  if (tid == 0) { s_cnt[1] = atomicAdd(&D.cursor[kDsMaxBins + 2], m); s_cnt[2] = kDsBinCap; }
  __syncthreads();
  u64* raw = D.tmp + s_cnt[1];
  u64* srt = D.sorted + s_cnt[1];
  const u64* reg = D.region + (size_t)bin * kDsBinCap;
  for (int i = tid; i < kDsBinCap; i += 256) raw[i] = reg[i];
  for (int j = tid; j < n_over; j += 256) {
    const u64 k = D.over[j];
    if ((P > 1 ? ds_bin_of(s_split, P, k >> kDsIdxBits) : 0) == bin) raw[atomicAdd(&s_cnt[2], 1)] = k;
  }
  __threadfence();
  __syncthreads();
  for (int i = tid; i < m; i += 256) {
    const u64 k = raw[i];
    int rank = 0;
    for (int j = 0; j < m; j++) rank += raw[j] < k ? 1 : 0;
    srt[rank] = k;
  }
  __threadfence();
  __syncthreads();
  ds_reduce_sorted<false>(srt, m, bin, P, pts, stack, D, fr, kind, gen, s_cnt, s_big);
  }   // next ticket
}

// pcl::VoxelGrid of this sweep's lessSharp / lessFlat clouds (LM:432-440) -> stack set `set`.  Needs nothing but the scan
// registration output, so it is enqueued on the scan-registration stream, ahead of the mapping stage that consumes it.
vloam_status map_stack_enqueue(MapContext* m, hipStream_t st, const SRBuffers& cur, int set, ProfHook* ph, hipEvent_t done) {
  StackInfo* si = m->stack_info[set];
  const unsigned Z = (unsigned)m->se.B;
  const size_t ss = m->se.ss;
  m->ds_gen++;   // tags the per-bin cell counts of this sweep's reduce pass (look-back words are never reset)
  VLOAM_LAUNCH(ph, kKMapStack, st, k_map_ds_bin, dim3(32, 2, Z), dim3(256), 0, st, cur.less_sharp, cur.less_flat, cur.S, m->ds[0], m->ds[1],
               m->inv_leaf[0], m->inv_leaf[1], m->stack_sets[set][0], m->stack_sets[set][1], si, ss);
  // `done` (the stack of this sweep is complete) is bound to the last dispatch instead of a marker packet behind it
  VLOAM_LAUNCH_EV(ph, kKMapDsReduce, st, done, k_map_ds_reduce, dim3(kDsReduceGrid, 2, Z), dim3(256), 0, st, cur.less_sharp, cur.less_flat, cur.S, m->ds[0], m->ds[1],
                  m->inv_leaf[0], m->inv_leaf[1], m->stack_sets[set][0], m->stack_sets[set][1], si, m->ds_gen, ss);
  return hipGetLastError() == hipSuccess ? VLOAM_OK : VLOAM_ERR_HIP;
}

// The same two launches for a localisation's foreign clouds (vloam_map_localize): into the scratch stack pair, with the scratch's own
// DsScratch, StackInfo and generation counter; L->S holds the clouds' counts and bounding boxes (k_sr_adopt).  One sequence, no session stride.
void map_stack_enqueue_loc(MapContext* m, hipStream_t st, const float4* corner, const float4* surf) {
  MapLocalize* L = m->loc;
  L->ds_gen++;
  VL_RAW_LAUNCH(k_map_ds_bin, dim3(32, 2, 1), dim3(256), 0, st, corner, surf, L->S, L->ds[0], L->ds[1], m->inv_leaf[0], m->inv_leaf[1], L->stack[0],
                L->stack[1], L->si, (size_t)0);
  VL_RAW_LAUNCH(k_map_ds_reduce, dim3(kDsReduceGrid, 2, 1), dim3(256), 0, st, corner, surf, L->S, L->ds[0], L->ds[1], m->inv_leaf[0], m->inv_leaf[1],
                L->stack[0], L->stack[1], L->si, L->ds_gen, (size_t)0);
}

}  // namespace vloam
