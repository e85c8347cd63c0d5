// scanRegistration on gfx950: NaN / min-range removal, ring + relTime labelling, stable per-ring
// compaction, 11-tap curvature, greedy sharp / flat pick per sector (== walking the sorted sector), per-ring VoxelGrid(0.2).
// Restates ScanRegistration::input, /root/reference/src/lidar_odometry_mapping/src/scan_registration.cpp:131-449
// (cited per step as "SR:<line>").  Integer / index results are bit-identical to the CPU oracle; f32
// arithmetic follows the reference's expression order with FMA contraction disabled at compile time.
//
// Kernels (one sweep = 6 launches, no host synchronisation):
//   k_sr_first_last  16 WGs      first / last surviving point: eight strided walkers from each end of the cloud (their records are folded by
//                                every k_sr_label workgroup)                                                                    SR:157-176
//   k_sr_label       n/1024 WGs  scanID, raw ori, halfPassed pivot (atomicMin), ring histogram SR:186-262   (1 024 lanes x 1 point for one or two
//   k_sr_scatter     n/1024 WGs  ring offsets + per-WG bases (SR:276-281), relTime / intensity, stable scatter SR:264-266   sessions, 256 x 4 for a batch)
//   k_sr_ring        1 WG/ring   LDS-resident ring: curvature, sort-free picks (wavefront arg-max rounds, six sectors
//                                at once + boundary fixed point), lessFlat + VoxelGrid(0.2) over voxel runs  SR:288-439
//                                (two capacity tiers: 2 176 points in 78.75 KB of LDS = two rings per CU; the 4 096-point tier follows on every
//                                sweep — its full grid while long rings are around, one catch-all workgroup otherwise)
//   k_sr_ring_long   1 WG/ring   opt-in third tier (vloam_config::max_ring_points > 4 096): rings of 4 097 .. max_ring_points points,
//                                working arrays in HBM, sectors walked in order; launched like the big tier, behind it
//   k_sr_compact     1 WG/ring   ring/sector-ordered feature clouds (+ per-ring bounding boxes of the less-clouds for the mapping
//                                stage's VoxelGrid)                                                 SR:338-344,388,439
// This file: first / last, label, scatter, compact, adopt and the launch.  k_sr_ring: sr_ring.hip; k_sr_ring_long: sr_ring_long.hip; the rules
// those two share: sr_ring_dev.h.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <float.h>
#include <math.h>
#include "sr_kernels.h"
#include "sr_ring.h"
#include "sr_wave.h"
#include "fdlibm_f32.h"
#include <cstdlib>

namespace vloam {

// SR:157 removeNaNFromPointCloud + SR:100-129 removeClosedPointCloud
__device__ __forceinline__ bool sr_survives_s1(float x, float y, float z, float thres) {
  if (!isfinite(x) || !isfinite(y) || !isfinite(z)) return false;
  if (x * x + y * y + z * z < thres * thres) return false;
  return true;
}

// atan2f / atanf exactly as glibc (fdlibm float) computes them on the reference's platform — fdlibm_f32.h; OCML's bodies differ from them in the
// last bit on ~10 % of the arguments, which moves returns that sit on a scan-line bin edge or on an unwrap threshold.  One out-of-line body
// each: every caller, every batch size, the same instruction sequence.
__device__ __noinline__ float sr_atan2f(float y, float x) { return fd_atan2f(y, x); }
__device__ __noinline__ float sr_atanf(float v) { return fd_atanf(v); }

// SR:192-226.  Returns the ring id or -1 when the point is dropped.
__device__ __forceinline__ int sr_scan_id(float x, float y, float z, int N_SCANS) {
  float angle = (float)((double)(sr_atanf(z / sqrtf(x * x + y * y)) * 180) / M_PI);
  // a return at the origin itself (0 / 0; it survives S1 only with minimum_range <= 0): int(NaN) is INT_MIN on the reference's x86-64
  // (cvttsd2si), i.e. "scanID < 0" in every branch below — dropped; the GPU's conversion would give 0, i.e. scan line 0 / 32
  if (angle != angle) return -1;
  int scanID = 0;
  if (N_SCANS == 16) {
    scanID = int((double)((angle + 15) / 2) + 0.5);
    if (scanID > (N_SCANS - 1) || scanID < 0) return -1;
  } else if (N_SCANS == 32) {
    scanID = int(((double)angle + 92.0 / 3.0) * 3.0 / 4.0);
    if (scanID > (N_SCANS - 1) || scanID < 0) return -1;
  } else {
    if ((double)angle >= -8.83) scanID = int((double)(2 - angle) * 3.0 + 0.5);
    else scanID = N_SCANS / 2 + int((-8.83 - (double)angle) * 2.0 + 0.5);
    if (angle > 2 || (double)angle < -24.33 || scanID > 50 || scanID < 0) return -1;
  }
  return scanID;
}

// SR:237-244, the !halfPassed branch
__device__ __forceinline__ float sr_ori_first_half(float ori, float startOri) {
  if ((double)ori < (double)startOri - M_PI / 2) ori = (float)((double)ori + 2 * M_PI);
  else if ((double)ori > (double)startOri + M_PI * 3 / 2) ori = (float)((double)ori - 2 * M_PI);
  return ori;
}
// SR:253-261, the halfPassed branch
__device__ __forceinline__ float sr_ori_second_half(float ori, float endOri) {
  ori = (float)((double)ori + 2 * M_PI);
  if ((double)ori < (double)endOri - M_PI * 3 / 2) ori = (float)((double)ori + 2 * M_PI);
  else if ((double)ori > (double)endOri + M_PI / 2) ori = (float)((double)ori - 2 * M_PI);
  return ori;
}

// ------------------------------------------------------------------------------------------------
// First / last surviving point (SR:157-176) in two steps without a single-workgroup stage on the critical path: every 256-lane
// workgroup of k_sr_first_last reports the first / last surviving point of its slice (one pass over the input at full width);
// every workgroup of k_sr_label folds the ~512 slice records itself (4 KB from L2) and derives startOri / endOri locally.
// 256-lane workgroups: small enough to slip onto CUs whose register file is mostly taken by the previous sweep's odometry
// kernels (the stages of consecutive sweeps overlap), where a 1024-lane workgroup would have to wait for them to drain.
constexpr int kFLThreads = 256;
constexpr int kFLPoints = 4096;   // points a workgroup looks at per trip (sixteen loads in flight per lane: a cloud that opens with a few thousand dropped returns is still one trip)
// 2 x kFLWalkers workgroups per session: kFLWalkers walk the cloud from the front — walker j looks at trips j, j + kFLWalkers, ... and stops at
// its first trip with a surviving point — and kFLWalkers from the back.  The first surviving point of the cloud is the smallest of the
// front walkers' answers (every k_sr_label workgroup folds the records), the last one the largest of the back walkers'.  On a real sweep that
// is one trip each, 32 KB per walker of the 2 MB cloud (rounds 1 - 4 read all of it for these two indices); a ring-major cloud that closes
// with ten rings of dropped returns (the synthetic one does: five trips, 15.6 us with ONE walker per end) still is one trip deep.
// slice[j] = (first, -1) for a front walker, (INT_MAX, last) for a back walker.
constexpr int kFLWalkers = 8;
__global__ __launch_bounds__(kFLThreads) void k_sr_first_last(BatchIn bi, float thres, int2* __restrict__ slice, size_t ss) {
  VL_SESSION(ss); RB(slice);
  const float4* __restrict__ in = bi.in[blockIdx.z];
  const int n = bi.n[blockIdx.z];
  __shared__ int s_first, s_last;
  const int tid = threadIdx.x, lane = tid & 63;
  const bool back = blockIdx.x >= kFLWalkers;
  const int walker = blockIdx.x - (back ? kFLWalkers : 0);
  if (tid == 0) { s_first = INT_MAX; s_last = -1; }
  __syncthreads();
  const int ntrip = (n + kFLPoints - 1) / kFLPoints;
  for (int trip = walker; trip < ntrip; trip += kFLWalkers) {
    const int t0 = (back ? ntrip - 1 - trip : trip) * kFLPoints;
    float4 p[kFLPoints / kFLThreads];
#pragma unroll
    for (int e = 0; e < kFLPoints / kFLThreads; e++) {
      const int i = t0 + e * kFLThreads + tid;
      p[e] = i < n ? in[i] : make_float4(NAN, NAN, NAN, 0.f);
    }
    int first = INT_MAX, last = -1;
#pragma unroll
    for (int e = 0; e < kFLPoints / kFLThreads; e++) {
      const int i = t0 + e * kFLThreads + tid;
      const bool v = i < n && sr_survives_s1(p[e].x, p[e].y, p[e].z, thres);
      const unsigned long long m = __ballot(v);
      if (m != 0ull) {
        const int base = i - lane;
        first = min(first, base + __ffsll((long long)m) - 1);
        last = max(last, base + 63 - __clzll((long long)m));
      }
    }
    if (lane == 0 && last >= 0) { atomicMin(&s_first, first); atomicMax(&s_last, last); }
    __syncthreads();
    if (s_last >= 0) break;   // (uniform: read behind the barrier)
    __syncthreads();
  }
  if (tid == 0) slice[blockIdx.x] = back ? make_int2(INT_MAX, s_last) : make_int2(s_first, -1);
}

// ------------------------------------------------------------------------------------------------
// blk: per-workgroup results for k_sr_scatter — [0, nblk): candidate pivot (SR:246-249) or INT_MAX, [nblk, 2 nblk): points
// surviving S1.  Plain stores, no counters to re-arm between sweeps.
// A label / scatter workgroup owns kLabelBlock points and comes in two shapes: kLabelThreads = 256 lanes with four points each (chunk e =
// points e * 256 .. e * 256 + 255) — a quarter of the wavefronts, what a batch of sessions wants (the chip is short of wave slots there) —
// and 1024 lanes with one point each for one or two sessions, where the 128 workgroups of a sweep leave the chip mostly empty and four
// dependent rounds per lane only add latency (B = 1: label 9.3 -> 7.4 us, scatter 12.2 -> 7.0 us).  Same blocks, same results.
template <int kLabelThreads>
__global__ __launch_bounds__(kLabelThreads) void k_sr_label(BatchIn bi, float thres, int N_SCANS,
                                                           FrameScalars* S, signed char* __restrict__ sid,
                                                           float* __restrict__ ori_raw, int* __restrict__ blockhist,
                                                           const int2* __restrict__ slice, int nslice, int* __restrict__ blk, size_t ss) {
  VL_SESSION(ss); RB(S); RB(sid); RB(ori_raw); RB(blockhist); RB(slice); RB(blk);
  constexpr int kLabelPer = kLabelBlock / kLabelThreads;
  const float4* __restrict__ in = bi.in[blockIdx.z];
  const int n = bi.n[blockIdx.z];
  __shared__ int hist[kMaxRings];
  __shared__ int s_istar, s_cnt, s_first, s_last;
  __shared__ float s_start;
  const int tid = threadIdx.x, lane = tid & 63;
  // this workgroup's points first: their loads are in flight while the slice records are folded
  float4 p[kLabelPer];
#pragma unroll
  for (int e = 0; e < kLabelPer; e++) {
    const int i = blockIdx.x * kLabelBlock + e * kLabelThreads + tid;
    p[e] = i < n ? in[i] : make_float4(NAN, NAN, NAN, 0.f);
  }
  if (tid < kMaxRings) hist[tid] = 0;
  if (tid == 0) { s_istar = INT_MAX; s_cnt = 0; s_first = INT_MAX; s_last = -1; }
  __syncthreads();
  {
    int f = INT_MAX, l = -1;
    for (int b = tid; b < nslice; b += kLabelThreads) { const int2 fl = slice[b]; f = min(f, fl.x); l = max(l, fl.y); }
    for (int d = 32; d > 0; d >>= 1) { f = min(f, __shfl_xor(f, d)); l = max(l, __shfl_xor(l, d)); }
    if (lane == 0) { atomicMin(&s_first, f); atomicMax(&s_last, l); }
  }
  __syncthreads();
  if (tid == 0) {
    float startOri = 0.f, endOri = 0.f;
    if (s_last >= 0) {
      const float4 pf = in[s_first], pl = in[s_last];
      startOri = -sr_atan2f(pf.y, pf.x);                                                // SR:166
      endOri = (float)((double)(-sr_atan2f(pl.y, pl.x)) + 2 * M_PI);                    // SR:167
      if ((double)(endOri - startOri) > 3 * M_PI) endOri = (float)((double)endOri - 2 * M_PI);        // SR:169-172
      else if ((double)(endOri - startOri) < M_PI) endOri = (float)((double)endOri + 2 * M_PI);      // SR:173-176
    }
    s_start = startOri;
    if (blockIdx.x == 0) {  // the sweep's first writer of the scalars: also clears the error word
      S->first_valid = s_first == INT_MAX ? -1 : s_first;
      S->last_valid = s_last;
      S->startOri = startOri; S->endOri = endOri;
      S->error = s_last < 0 ? kErrEmpty : 0;
    }
  }
  __syncthreads();
  const float startOri = s_start;
  int nv = 0, istar = INT_MAX;
#pragma unroll
  for (int e = 0; e < kLabelPer; e++) {
    const int i = blockIdx.x * kLabelBlock + e * kLabelThreads + tid;
    int id = -1;
    bool v1 = false;
    if (i < n) {
      v1 = sr_survives_s1(p[e].x, p[e].y, p[e].z, thres);
      if (v1) {
        id = sr_scan_id(p[e].x, p[e].y, p[e].z, N_SCANS);
        float ori = -sr_atan2f(p[e].y, p[e].x);  // SR:234
        ori_raw[i] = ori;
        if (id >= 0) {
          atomicAdd(&hist[id], 1);
          float o = sr_ori_first_half(ori, startOri);
          if ((double)(o - startOri) > M_PI) istar = min(istar, i);  // SR:246-249 candidate pivot
        }
      }
      sid[i] = (signed char)id;
    }
    nv += __popcll(__ballot(v1));
  }
  if (istar != INT_MAX) atomicMin(&s_istar, istar);
  if (lane == 0 && nv) atomicAdd(&s_cnt, nv);
  __syncthreads();
  if (tid < kMaxRings) blockhist[blockIdx.x * kMaxRings + tid] = hist[tid];
  if (tid == 0) { blk[blockIdx.x] = s_istar; blk[gridDim.x + blockIdx.x] = s_cnt; }
}

// ------------------------------------------------------------------------------------------------
// Stable scatter into the ring-major cloud.  Every workgroup first derives, from the per-WG ring histograms of k_sr_label,
// the ring offsets (SR:276-281) and its own base inside every ring — 32 KB of L2 reads per WG instead of a separate
// single-workgroup scan kernel on the critical path.
template <int kLabelThreads>
__global__ __launch_bounds__(kLabelThreads) void k_sr_scatter(BatchIn bi, FrameScalars* S,
                                                             const signed char* __restrict__ sid, const float* __restrict__ ori_raw,
                                                             const int* __restrict__ blockhist, int nblk, float4* __restrict__ cloud,
                                                             const int* __restrict__ blk, size_t ss) {
  VL_SESSION(ss); RB(S); RB(sid); RB(ori_raw); RB(blockhist); RB(cloud); RB(blk);
  const float4* __restrict__ in = bi.in[blockIdx.z];
  const int n = bi.n[blockIdx.z];
  constexpr int kLabelPer = kLabelBlock / kLabelThreads;
  constexpr int kChunks = kLabelBlock / 64, kWaves = kLabelThreads / 64;   // 64-point chunks of the workgroup's points, in input order: chunk c = e * kWaves + wave
  __shared__ int wcnt[kChunks][kMaxRings];
  __shared__ int s_istar, s_nvalid;
  __shared__ int part_before[kWaves][kMaxRings], part_all[kWaves][kMaxRings];
  __shared__ int ring_base[kMaxRings];   // ring offset + points of this ring in earlier workgroups
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // this workgroup's points, ring ids and raw azimuths first (in flight during the prologue)
  float4 p[kLabelPer];
  float oraw[kLabelPer];
  int ids[kLabelPer];
#pragma unroll
  for (int e = 0; e < kLabelPer; e++) {
    const int i = blockIdx.x * kLabelBlock + e * kLabelThreads + tid;
    ids[e] = (i < n) ? (int)sid[i] : -1;
    p[e] = i < n ? in[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    oraw[e] = i < n ? ori_raw[i] : 0.f;
  }
  for (int k = tid; k < kChunks * kMaxRings; k += kLabelThreads) (&wcnt[0][0])[k] = 0;
  if (tid == 0) { s_istar = INT_MAX; s_nvalid = 0; }
  __syncthreads();
  {
    // the pivot of the sweep = the smallest candidate of any label workgroup; the S1 survivor count is a debug scalar
    int mi = INT_MAX, cnt = 0;
    for (int b = tid; b < nblk; b += kLabelThreads) { mi = min(mi, blk[b]); cnt += blk[nblk + b]; }
    for (int d = 32; d > 0; d >>= 1) { mi = min(mi, __shfl_xor(mi, d)); cnt += __shfl_xor(cnt, d); }
    if (lane == 0) { atomicMin(&s_istar, mi); atomicAdd(&s_nvalid, cnt); }
  }
  {
    // wavefront w sums blocks w, w + kWaves, ... for ring = lane
    int before = 0, all = 0;
    for (int b = wave; b < nblk; b += kWaves) {
      const int h = blockhist[b * kMaxRings + lane];
      all += h;
      if (b < (int)blockIdx.x) before += h;
    }
    part_before[wave][lane] = before;
    part_all[wave][lane] = all;
  }
  __syncthreads();
  if (tid < kMaxRings) {
    int before = 0, all = 0;
    for (int w = 0; w < kWaves; w++) { before += part_before[w][tid]; all += part_all[w][tid]; }
    // exclusive prefix of the ring totals across the 64 rings of this wavefront
    int inc = all;
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (tid >= d) inc += t; }
    const int roff = inc - all;
    ring_base[tid] = roff + before;
    if (blockIdx.x == 0) {
      S->ring_count[tid] = all;
      S->ring_off[tid] = roff;
      S->scanStartInd[tid] = roff + 5;         // SR:278
      S->scanEndInd[tid] = roff + all - 6;     // SR:280
      if (tid == kMaxRings - 1) { S->N2 = inc; S->ring_off[kMaxRings] = inc; S->istar = s_istar; S->n_after_s1 = s_nvalid; }
    }
  }
  // stable rank of every point among the same-ring points of its 64-point chunk
  int rank[kLabelPer];
#pragma unroll
  for (int e = 0; e < kLabelPer; e++) {
    const int id = ids[e];
    rank[e] = 0;
    bool pending = id >= 0;
    while (true) {
      u64 act = __ballot(pending);
      if (act == 0) break;
      int leader = __ffsll((long long)act) - 1;
      int lid = __shfl(id, leader);
      u64 same = __ballot(pending && id == lid);
      if (pending && id == lid) {
        rank[e] = __popcll(same & ((1ull << lane) - 1ull));
        pending = false;
      }
      if (lane == leader) wcnt[e * kWaves + wave][lid] = __popcll(same);
    }
  }
  __syncthreads();
  const float startOri = S->startOri, endOri = S->endOri;
  const int istar = s_istar;
#pragma unroll
  for (int e = 0; e < kLabelPer; e++) {
    const int id = ids[e];
    if (id < 0) continue;
    const int i = blockIdx.x * kLabelBlock + e * kLabelThreads + tid;
    int base = ring_base[id];
    for (int c = 0; c < e * kWaves + wave; c++) base += wcnt[c][id];
    float ori = oraw[e];
    if (i <= istar) ori = sr_ori_first_half(ori, startOri);
    else ori = sr_ori_second_half(ori, endOri);
    float relTime = (ori - startOri) / (endOri - startOri);  // SR:264
    float4 o;
    o.x = p[e].x; o.y = p[e].y; o.z = p[e].z;
    o.w = (float)((double)id + 0.1 * (double)relTime);  // SR:265, scanPeriod = 0.1 (scan_registration.h:84)
    cloud[base + rank[e]] = o;
  }
}

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sr_compact(const float4* __restrict__ cloud, FrameScalars* S, const int* __restrict__ sharp_idx,
                                                    const int* __restrict__ less_sharp_idx, const int* __restrict__ flat_idx,
                                                    const float4* __restrict__ ring_ds, float4* __restrict__ sharp,
                                                    float4* __restrict__ less_sharp, float4* __restrict__ flat,
                                                    float4* __restrict__ less_flat, int* __restrict__ dbg_feat_idx /* [3][kMaxLessSharp] */,
                                                    int* sticky_err, const float4* __restrict__ long_ds /* [kMaxRings][long_cap] or null */,
                                                    int long_cap, size_t ss) {
  VL_SESSION(ss); RB(cloud); RB(S); RB(sharp_idx); RB(less_sharp_idx); RB(flat_idx); RB(ring_ds); RB(sharp); RB(less_sharp); RB(flat); RB(less_flat);
  RB(dbg_feat_idx); RB(sticky_err); RB(long_ds);
  __shared__ int base[4];
  __shared__ int soff[kSectors][3];
  __shared__ float s_box[4][12];
  const int r = blockIdx.x, tid = threadIdx.x;
  float bmn[2][3], bmx[2][3];   // this thread's share of the line's lessSharp [0] / lessFlat [1] bounding boxes
#pragma unroll
  for (int c = 0; c < 2; c++)
#pragma unroll
    for (int a = 0; a < 3; a++) { bmn[c][a] = FLT_MAX; bmx[c][a] = -FLT_MAX; }
  // last launch of the sweep's scan registration: its error bits (S->error is per buffer set and rewritten every sweep) go into the
  // handle's sticky word, so that a burst of vloam_process_scan calls cannot lose them
  if (r == 0 && tid == 0 && sticky_err && S->error) atomicOr(sticky_err, S->error);
  {
    // 4 wavefronts: kinds 0..2 = sharp / lessSharp / flat picks per ring, kind 3 = per-ring VoxelGrid output size
    const int kind = tid >> 6, q = tid & 63;
    int v = 0;
    if (kind < 3) { for (int s = 0; s < kSectors; s++) v += S->sect_cnt[q][s][kind]; }
    else v = S->ring_ds_cnt[q];
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) { int t = __shfl_up(inc, d); if (q >= d) inc += t; }
    if (q == r) base[kind] = inc - v;
    if (q == 63 && r == kMaxRings - 1) {
      if (kind == 0) S->n_sharp = inc; else if (kind == 1) S->n_less_sharp = inc; else if (kind == 2) S->n_flat = inc; else S->n_less_flat = inc;
    }
  }
  __syncthreads();
  if (tid < 3) {
    int run = base[tid];
    for (int s = 0; s < kSectors; s++) { soff[s][tid] = run; run += S->sect_cnt[r][s][tid]; }
  }
  __syncthreads();
  // sector lists: tiny — one thread per (sector, kind, slot)
  for (int k = tid; k < kSectors * (kMaxSharpPerSect + kMaxLessSharpPerSect + kMaxFlatPerSect); k += 256) {
    const int per = kMaxSharpPerSect + kMaxLessSharpPerSect + kMaxFlatPerSect;
    const int s = k / per, q = k % per;
    if (q < kMaxSharpPerSect) {
      if (q < S->sect_cnt[r][s][0]) {
        int src = sharp_idx[(r * kSectors + s) * kMaxSharpPerSect + q];
        sharp[soff[s][0] + q] = cloud[src];
        if (dbg_feat_idx) dbg_feat_idx[soff[s][0] + q] = src;
      }
    } else if (q < kMaxSharpPerSect + kMaxLessSharpPerSect) {
      const int qq = q - kMaxSharpPerSect;
      if (qq < S->sect_cnt[r][s][1]) {
        int src = less_sharp_idx[(r * kSectors + s) * kMaxLessSharpPerSect + qq];
        const float4 p = cloud[src];
        less_sharp[soff[s][1] + qq] = p;
        bmn[0][0] = fminf(bmn[0][0], p.x); bmn[0][1] = fminf(bmn[0][1], p.y); bmn[0][2] = fminf(bmn[0][2], p.z);
        bmx[0][0] = fmaxf(bmx[0][0], p.x); bmx[0][1] = fmaxf(bmx[0][1], p.y); bmx[0][2] = fmaxf(bmx[0][2], p.z);
        if (dbg_feat_idx) dbg_feat_idx[kMaxLessSharp + soff[s][1] + qq] = src;
      }
    } else {
      const int qq = q - kMaxSharpPerSect - kMaxLessSharpPerSect;
      if (qq < S->sect_cnt[r][s][2]) {
        int src = flat_idx[(r * kSectors + s) * kMaxFlatPerSect + qq];
        flat[soff[s][2] + qq] = cloud[src];
        if (dbg_feat_idx) dbg_feat_idx[2 * kMaxLessSharp + soff[s][2] + qq] = src;
      }
    }
  }
  const int nds = S->ring_ds_cnt[r];
  // a ring of more than kMaxRingLen points was downsampled by the long tier (long-tier handles only)
  const float4* src = long_ds && S->ring_count[r] > kMaxRingLen ? long_ds + (size_t)r * long_cap : ring_ds + (size_t)r * kMaxRingLen;
  for (int k = tid; k < nds; k += 256) {
    const float4 p = src[k];
    less_flat[base[3] + k] = p;
    bmn[1][0] = fminf(bmn[1][0], p.x); bmn[1][1] = fminf(bmn[1][1], p.y); bmn[1][2] = fminf(bmn[1][2], p.z);
    bmx[1][0] = fmaxf(bmx[1][0], p.x); bmx[1][1] = fmaxf(bmx[1][1], p.y); bmx[1][2] = fmaxf(bmx[1][2], p.z);
  }
  // the line's two boxes: wavefront reductions, then the four wavefronts' results by twelve lanes
#pragma unroll
  for (int c = 0; c < 2; c++)
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float lo = wave_fminmax<false>(bmn[c][a]), hi = wave_fminmax<true>(bmx[c][a]);
      if ((tid & 63) == 0) { s_box[tid >> 6][c * 6 + a] = lo; s_box[tid >> 6][c * 6 + 3 + a] = hi; }
    }
  __syncthreads();
  if (tid < 12) {
    const bool is_max = (tid % 6) >= 3;
    float v = s_box[0][tid];
    for (int w = 1; w < 4; w++) v = is_max ? fmaxf(v, s_box[w][tid]) : fminf(v, s_box[w][tid]);
    S->less_bbox[tid / 6][r][tid % 6] = v;
  }
}

// ---- clouds handed in by the caller instead of produced by the kernels above (LaserOdometry::input / LaserMapping::input deep-copy whatever
// they are given, laser_odometry.cpp:141-145, laser_mapping.cpp:172-181): the counts and the two VoxelGrid bounding boxes of a buffer set are
// re-derived from the uploaded clouds.  One workgroup; a count < 0 keeps what the set holds.  (The boxes are only ever min / max-reduced over
// all 64 slots, so any partition of the points over the slots will do.)
__global__ __launch_bounds__(256) void k_sr_adopt(FrameScalars* S, const float4* __restrict__ less_sharp, const float4* __restrict__ less_flat, int n_full,
                                                  int n_sharp, int n_less_sharp, int n_flat, int n_less_flat) {
  __shared__ float s_box[4][64][6];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) {
    if (n_full >= 0) S->N2 = n_full;
    if (n_sharp >= 0) S->n_sharp = n_sharp;
    if (n_flat >= 0) S->n_flat = n_flat;
    if (n_less_sharp >= 0) S->n_less_sharp = n_less_sharp;
    if (n_less_flat >= 0) S->n_less_flat = n_less_flat;
  }
  for (int kind = 0; kind < 2; kind++) {
    const int n = kind ? n_less_flat : n_less_sharp;
    if (n < 0) continue;   // (uniform)
    const float4* pts = kind ? less_flat : less_sharp;
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = tid; i < n; i += 256) {
      const float4 p = pts[i];
      mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
      mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
    }
    for (int a = 0; a < 3; a++) { s_box[w][lane][a] = mn[a]; s_box[w][lane][3 + a] = mx[a]; }
    __syncthreads();
    if (tid < 64)
      for (int a = 0; a < 6; a++) {
        float v = s_box[0][tid][a];
        for (int ww = 1; ww < 4; ww++) v = a < 3 ? fminf(v, s_box[ww][tid][a]) : fmaxf(v, s_box[ww][tid][a]);
        S->less_bbox[kind][tid][a] = v;
      }
    __syncthreads();
  }
}
void sr_adopt_launch(hipStream_t st, const SRBuffers& b, int n_full, int n_sharp, int n_less_sharp, int n_flat, int n_less_flat) {
  VL_RAW_LAUNCH(k_sr_adopt, dim3(1, 1, 1), dim3(256), 0, st, b.S, b.less_sharp, b.less_flat, n_full, n_sharp, n_less_sharp, n_flat, n_less_flat);
}

// ------------------------------------------------------------------------------------------------
hipError_t sr_init() {
  hipError_t e = hipFuncSetAttribute((const void*)k_sr_ring<kRingCapSmall, kSectCapSmall, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)SrRingLds<kRingCapSmall, kSectCapSmall>::bytes);
  if (e != hipSuccess) return e;
  return hipFuncSetAttribute((const void*)k_sr_ring<kMaxRingLen, kSectCap, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)SrRingLds<kMaxRingLen, kSectCap>::bytes);   // (k_sr_ring_long: static LDS only)
}

hipError_t sr_launch(hipStream_t st, const SRBuffers& b, const BatchIn& bi, Sess se, int N_SCANS, float min_range, int debug_level, ProfHook* ph, hipEvent_t done,
                     int* ring_watch, bool big_tier, bool long_tier) {
  const bool debug = debug_level == 1, stamps = debug_level != 0;   // debug = 2: only the ring kernel's phase stamps (no reference-order debug sort)
  int n = 0;
  for (int k = 0; k < se.B; k++) n = bi.n[k] > n ? bi.n[k] : n;   // launch geometry for the largest sweep of the batch (blocks beyond a session's n idle)
  const unsigned Z = (unsigned)se.B;
  const int nblk = (n + kLabelBlock - 1) / kLabelBlock;
  const int nslice = 2 * kFLWalkers;   // (first, last) from the two ends, kFLWalkers strided walkers each
  int2* slice = (int2*)b.blockoff;         // [nslice] records of 8 B
  int* blk = b.blockoff + 2 * nslice;      // [2][nblk], behind the slice records (blockoff holds 64 ints per label workgroup: 32 + 2 nblk <= 64 nblk)
  VLOAM_LAUNCH(ph, kKSrFirstLast, st, k_sr_first_last, dim3(nslice, 1, Z), dim3(kFLThreads), 0, st, bi, min_range, slice, se.ss);
  static const int wide_env = getenv("VLOAM_SR_WIDE") ? atoi(getenv("VLOAM_SR_WIDE")) : -1;   // A/B and tests: 1 = always 1024 lanes, 0 = always 256
  if (wide_env >= 0 ? wide_env != 0 : se.B <= 2) {   // one or two sessions: one point per lane (latency); a batch: four points per lane (wave slots)
    VLOAM_LAUNCH(ph, kKSrLabel, st, k_sr_label<1024>, dim3(nblk, 1, Z), dim3(1024), 0, st, bi, min_range, N_SCANS, b.S, b.sid, b.ori, b.blockhist,
                 slice, nslice, blk, se.ss);
    VLOAM_LAUNCH(ph, kKSrScatter, st, k_sr_scatter<1024>, dim3(nblk, 1, Z), dim3(1024), 0, st, bi, b.S, b.sid, b.ori, b.blockhist, nblk, b.cloud, blk, se.ss);
  } else {
    VLOAM_LAUNCH(ph, kKSrLabel, st, k_sr_label<256>, dim3(nblk, 1, Z), dim3(256), 0, st, bi, min_range, N_SCANS, b.S, b.sid, b.ori, b.blockhist,
                 slice, nslice, blk, se.ss);
    VLOAM_LAUNCH(ph, kKSrScatter, st, k_sr_scatter<256>, dim3(nblk, 1, Z), dim3(256), 0, st, bi, b.S, b.sid, b.ori, b.blockhist, nblk, b.cloud, blk, se.ss);
  }
  // Behind the small tier ALWAYS comes the big tier: its full grid while the host has seen long rings (watch word), otherwise ONE catch-all
  // workgroup per session that looks at the ring lengths and works on the (normally zero) rings the small tier had to leave.  Any ring of up
  // to kMaxRingLen points is therefore processed on any sweep, like the reference's 400 000-point scratch (scan_registration.h:90) takes any
  // ring; the catch-all costs 13 - 16 us of single-sweep latency (a 146 KB LDS request) and 1.4 % of the B = 8 throughput on ordinary sweeps.
  // (Rounds 2 - 3 made it optional and REPORTED a ring that outgrew the small tier without the watch word's warning: a results gap on
  // reachable input.)
  // VLOAM_SR_CATCHALL=0: a host that KNOWS its rings stay below kRingCapSmall points (any 10 Hz sensor of the reference's three scan_line
  // settings) may drop the catch-all launch: a ring that outgrows the small tier without the watch word's warning is then REPORTED
  // (kErrRingTooLong -> VLOAM_ERR_CAPACITY) instead of processed; with the warning the full big tier runs as always.
  // The long tier (handles with max_ring_points > kMaxRingLen only) follows the big tier the same way: its full grid while the big tier has
  // seen rings near kMaxRingLen (second watch word), else its one-workgroup catch-all; VLOAM_SR_CATCHALL=0 drops that catch-all as well.
  // Default handles launch neither.
  static const int catchall = getenv("VLOAM_SR_CATCHALL") ? atoi(getenv("VLOAM_SR_CATCHALL")) : 1;
  const bool has_long = b.long_cap > kMaxRingLen;
  long_tier = long_tier && has_long;
  const bool big_launch = big_tier || long_tier || catchall != 0;
  const bool long_launch = has_long && (long_tier || catchall != 0);
  VLOAM_LAUNCH(ph, kKSrRing, st, (k_sr_ring<kRingCapSmall, kSectCapSmall, false>), dim3(kMaxRings, 1, Z), dim3(kRingThreads),
               (SrRingLds<kRingCapSmall, kSectCapSmall>::bytes), st, b.cloud, b.S, b.sharp_idx, b.less_sharp_idx,
               b.flat_idx, b.ring_ds, debug ? b.dbg_curv : nullptr, debug ? b.dbg_sort : nullptr, debug ? b.dbg_picked : nullptr,
               debug ? b.dbg_label : nullptr, stamps ? b.dbg_cyc : nullptr, ring_watch, big_launch ? 1 : 0, se.ss);
  // the full big tier while rings near the small tier's capacity are around, else its one-workgroup catch-all
  if (big_launch)
    VLOAM_LAUNCH(ph, kKSrRingBig, st, (k_sr_ring<kMaxRingLen, kSectCap, true>), dim3(big_tier ? kMaxRings : 1, 1, Z), dim3(kRingThreads),
                 (SrRingLds<kMaxRingLen, kSectCap>::bytes), st, b.cloud, b.S, b.sharp_idx, b.less_sharp_idx,
                 b.flat_idx, b.ring_ds, debug ? b.dbg_curv : nullptr, debug ? b.dbg_sort : nullptr, debug ? b.dbg_picked : nullptr,
                 debug ? b.dbg_label : nullptr, stamps ? b.dbg_cyc : nullptr, ring_watch, long_launch ? 1 : 0, se.ss);
  if (long_launch)
    VLOAM_LAUNCH(ph, kKSrRingLong, st, k_sr_ring_long, dim3(long_tier ? kMaxRings : 1, 1, Z), dim3(kRingThreads), 0, st, b.cloud, b.S, b.sharp_idx,
                 b.less_sharp_idx, b.flat_idx, b.long_cap, b.long_kcap, b.long_keys, b.long_iscr, b.long_bytes, b.long_ds,
                 debug ? b.dbg_curv : nullptr, debug ? b.dbg_sort : nullptr, debug ? b.dbg_picked : nullptr, debug ? b.dbg_label : nullptr, se.ss);
  VLOAM_LAUNCH_EV(ph, kKSrCompact, st, done, k_sr_compact, dim3(kMaxRings, 1, Z), dim3(256), 0, st, b.cloud, b.S, b.sharp_idx, b.less_sharp_idx, b.flat_idx, b.ring_ds,
                     b.sharp, b.less_sharp, b.flat, b.less_flat, debug ? b.dbg_feat_idx : nullptr, b.sticky_err, has_long ? b.long_ds : nullptr,
                     b.long_cap, se.ss);
  return hipGetLastError();
}

}  // namespace vloam
