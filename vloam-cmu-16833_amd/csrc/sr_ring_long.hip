// k_sr_ring_long: the long ring tier of the scan registration (the whole stage: sr_kernels.hip) — opt-in, vloam_config::max_ring_points > kMaxRingLen: rings of kMaxRingLen + 1 .. max_ring_points points, on handles that
// asked for them.  Such a ring does not fit the LDS of a CU (~36 B per point in the tiers above, 590 KB at 16 384 points), so this tier keeps
// its per-point arrays in HBM (SRBuffers::long_*, one region per ring and session; the points themselves are read from the ring-major cloud)
// and only the reduction slots in LDS.  It is written for global memory rather than as a third instantiation of the LDS body: that body's
// sector walks keep a sector in registers (211 VGPRs at the big tier's 682-point sectors; a 16 384-point ring has 2 729-point sectors) and its
// run keys carry 12-bit point indices.  Here, as in the reference:
//  - the six sectors are walked one after the other by wavefront 0, so a pick's neighbour suppression reaches into the next sector exactly as
//    cloudNeighborPicked does (SR:353-376) and no boundary fixed point is needed.  A pick is the arg-max (sharp walk) / arg-min (flat walk)
//    of (curvature, index) over the sector's eligible points, i.e. the first eligible entry of the sector sorted by (curvature, index),
//    walked from the top or the bottom (the canonical order of the LDS tiers and of the oracle);
//  - lessFlat's VoxelGrid(0.2) sorts one key per point (voxel : index, non-candidates last), so it takes any number of voxels, and sums every
//    voxel's points in input order (CentroidPoint, f32).
// Memory ordering: everything exchanged through these arrays stays inside the workgroup, i.e. on one CU behind one L1: between wavefronts
// behind __syncthreads() (workgroup-scope release / acquire), between the lanes of wavefront 0 behind lds_fence_wave() — a workgroup-scope
// fence over every address space (it waits for the wavefront's stores) and a wave barrier.  No other workgroup reads them during the launch;
// the next launch that does (k_sr_compact: long_ds) is ordered behind this one on the stream.
// The rules it shares with the LDS tiers (sr_ring.hip): sr_ring_dev.h.
#include <hip/hip_runtime.h>
#include "sr_ring.h"
#include "bitonic.h"

namespace vloam {

constexpr int kLongSlots = ((kMaxRingLenLong - 11 + kSectors - 1) / kSectors + 63) / 64;   // register slots per lane of a sector walk (2 729 points at 16 384)

__global__ __launch_bounds__(kRingThreads) void k_sr_ring_long(const float4* __restrict__ cloud, FrameScalars* S, int* __restrict__ sharp_idx,
                                                               int* __restrict__ less_sharp_idx, int* __restrict__ flat_idx, int cap, int kcap,
                                                               u64* keys_all, int* iscr_all, unsigned char* bytes_all, float4* ds_all,
                                                               float* __restrict__ dbg_curv, int* __restrict__ dbg_sort, int* __restrict__ dbg_picked,
                                                               int* __restrict__ dbg_label, size_t ss) {
  VL_SESSION(ss); RB(cloud); RB(S); RB(sharp_idx); RB(less_sharp_idx); RB(flat_idx); RB(keys_all); RB(iscr_all); RB(bytes_all); RB(ds_all);
  RB(dbg_curv); RB(dbg_sort); RB(dbg_picked); RB(dbg_label);
  __shared__ int scan_tmp[kRingThreads];
  __shared__ float wred[kRingThreads / 64 * 8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  auto one_ring = [&](const int r) {
    const int len = S->ring_count[r], off = S->ring_off[r];
    const int start = off + 5, end = off + len - 6;  // SR:278-280
    // (the entry checks are k_sr_ring's, kept here in text: as a shared inline function they cost this kernel, at its 256 VGPRs, a spill)
    if (len <= kMaxRingLen) return;                  // an LDS tier has done this ring
    if (tid < kSectors * 3) (&S->sect_cnt[r][0][0])[tid] = 0;
    if (tid == 0) S->ring_ds_cnt[r] = 0;
    if (len > cap) { if (tid == 0) atomicOr(&S->error, kErrRingTooLong); return; }
    if (end - start < 6) return;  // SR:314
    const float4* p = cloud + off;
    const auto get = [=](int l) { return p[l]; };   // point l of the ring
    u64* keys = keys_all + (size_t)r * kcap;
    int* iscr = iscr_all + (size_t)r * kcap;
    float* curv = (float*)iscr;
    unsigned char* picked = bytes_all + (size_t)r * 4 * cap;
    signed char* label = (signed char*)(picked + cap);
    unsigned char* gap = picked + 2 * cap;
    unsigned char* reach = picked + 3 * cap;
    float4* out = ds_all + (size_t)r * cap;

    // gap[l] = 1 where the neighbour suppression stops between l and l + 1
    for (int l = tid; l < len; l += kRingThreads) {
      picked[l] = 0; label[l] = 0;  // SR:305-306
      const bool g = l + 1 < len ? sr_gap(get(l), get(l + 1)) : true;
      gap[l] = g ? 1 : 0;
    }
    __syncthreads();
    // curvature (SR:288-303) of every sector point and its suppression reach: how many of l-1 .. l-5 (low nibble) and of l+1 .. l+5 (high
    // nibble) a pick at l marks
    for (int l = 5 + tid; l <= len - 7; l += kRingThreads) {
      const float c = sr_curvature(get, l);
      curv[l] = c;
      if (dbg_curv) dbg_curv[off + l] = c;
      int f = 0, k = 0;
      while (f < 5 && !gap[l + f]) f++;
      while (k < 5 && !gap[l - 1 - k]) k++;
      reach[l] = (unsigned char)(k | (f << 4));
    }
    __syncthreads();
    auto sect_lo = [&](int s) { return sr_sector_lo(start, end, s) - off; };   // local
    auto sect_hi = [&](int s) { return sr_sector_hi(start, end, s) - off; };

    // ---- debug only: the reference's std::sort of every sector (SR:323, ties by index), one sector after the other
    if (dbg_sort) {
      for (int s = 0; s < kSectors; s++) {
        const int sp_l = sect_lo(s), seclen = sect_hi(s) - sp_l + 1;
        int P = 256;
        while (P < seclen) P <<= 1;
        for (int t = tid; t < P; t += kRingThreads)
          keys[t] = t < seclen ? ((u64)__float_as_uint(curv[sp_l + t]) << 32) | (unsigned)(sp_l + t) : ~0ull;   // c >= 0: bits order like the value
        __syncthreads();
        block_bitonic_sort_u64(keys, P, tid, kRingThreads);
        for (int t = tid; t < seclen; t += kRingThreads) dbg_sort[off + sp_l + t] = off + (int)(keys[t] & 0xffffffffu);
        __syncthreads();
      }
    }

    // ---- greedy picks (SR:325-422), wavefront 0, sector after sector
    if (wave == 0) {
      for (int s = 0; s < kSectors; s++) {
        const int sp_l = sect_lo(s), ep_l = sect_hi(s);
        int* o_sharp = sharp_idx + (r * kSectors + s) * kMaxSharpPerSect;
        int* o_less = less_sharp_idx + (r * kSectors + s) * kMaxLessSharpPerSect;
        int* o_flat = flat_idx + (r * kSectors + s) * kMaxFlatPerSect;
        unsigned v[kLongSlots];   // point sp_l + q * 64 + lane: its curvature bits while it is a candidate of the running walk, else the walk's neutral value
        // the candidates of a walk: points no earlier pick has marked — of this sector or, over the seam, of the previous one
        auto load = [&](bool sharp_walk) {
          lds_fence_wave();   // this wavefront's marks are stored before they are read back
#pragma unroll
          for (int q = 0; q < kLongSlots; q++) {
            const int i = sp_l + q * 64 + lane;
            v[q] = sharp_walk ? 0u : 0xffffffffu;
            if (i <= ep_l && !picked[i]) {
              const unsigned cb = __float_as_uint(curv[i]);
              if (sharp_walk ? sr_sharp_cand(cb) : sr_flat_cand(cb)) v[q] = cb;   // SR:330 / SR:383
            }
          }
        };
        // SR:345-376 around the winner: cloudNeighborPicked in memory (one lane per marked point), and the marked points leave the walk
        auto mark = [&](int w, unsigned neutral) {
          const unsigned rb = reach[w];
          const int lo_m = w - (int)(rb & 15u), hi_m = w + (int)(rb >> 4);
          if (lane <= hi_m - lo_m) picked[lo_m + lane] = 1;
#pragma unroll
          for (int q = 0; q < kLongSlots; q++) {
            const int i = sp_l + q * 64 + lane;
            if (i >= lo_m && i <= hi_m) v[q] = neutral;
          }
        };
        // SR:327-378, descending (curvature, index)
        load(true);
        int n_less = 0;
        while (n_less < kMaxLessSharpPerSect) {
          unsigned lb = v[0];
          int qb = 0;
#pragma unroll
          for (int q = 1; q < kLongSlots; q++) if (v[q] >= lb) { lb = v[q]; qb = q; }   // ties: the higher index
          const unsigned hi = wave_max_u32(lb);
          if (hi == 0) break;   // (candidates have c >= 0.1f: non-zero bits)
          const int w = (int)wave_max_u32(lb == hi ? (unsigned)(sp_l + qb * 64 + lane) : 0u);
          if (lane == 0) {
            label[w] = n_less < kMaxSharpPerSect ? 2 : 1;
            o_less[n_less] = off + w;
            if (n_less < kMaxSharpPerSect) o_sharp[n_less] = off + w;
          }
          n_less++;
          mark(w, 0u);
        }
        // SR:380-422, ascending (curvature, index)
        load(false);
        int n_flat = 0;
        while (n_flat < kMaxFlatPerSect) {
          unsigned lb = v[0];
          int qb = 0;
#pragma unroll
          for (int q = 1; q < kLongSlots; q++) if (v[q] < lb) { lb = v[q]; qb = q; }   // ties: the lower index
          const unsigned hi = wave_min_u32(lb);
          if (hi == 0xffffffffu) break;   // (c < 0.1f: never all ones)
          const int w = (int)wave_min_u32(lb == hi ? (unsigned)(sp_l + qb * 64 + lane) : 0xffffffffu);
          if (lane == 0) { label[w] = -1; o_flat[n_flat] = off + w; }
          n_flat++;
          if (n_flat >= kMaxFlatPerSect) break;  // the 4th flat point is emitted but not suppressed (SR:390-394)
          mark(w, 0xffffffffu);
        }
        if (lane == 0) { S->sect_cnt[r][s][0] = min(n_less, kMaxSharpPerSect); S->sect_cnt[r][s][1] = n_less; S->sect_cnt[r][s][2] = n_flat; }
      }
    }
    __syncthreads();
    sr_dump_marks(dbg_picked, dbg_label, off, len, picked, label);

    // ---- lessFlat (SR:424-430) + per-ring pcl::VoxelGrid leaf 0.2 (SR:433-437)
    const int c_lo = 5, c_hi = len - 7;  // local range covered by the six sectors: [start, end-1]
    const SrBox box = sr_lessflat_box(get, label, c_lo, c_hi, wred);
    const int ncand = box.ncand;
    if (ncand == 0) return;
    if (SrGrid::too_fine(box)) { sr_ds_passthrough(get, label, len, c_lo, c_hi, iscr, scan_tmp, out, S, r, ncand); return; }
    const SrGrid grid(box);
    // key = voxel index : point, ~0 for a point that is no candidate (sorted behind the ncand candidates)
    int P2 = 256;
    while (P2 < len) P2 <<= 1;   // <= kcap
    for (int l = tid; l < P2; l += kRingThreads) {
      u64 key = ~0ull;
      if (l >= c_lo && l <= c_hi && label[l] <= 0) {
        const float4 q = p[l];
        key = ((u64)(unsigned)grid.voxel_of(q.x, q.y, q.z) << 32) | (unsigned)l;
      }
      keys[l] = key;
    }
    __syncthreads();
    block_bitonic_sort_u64(keys, P2, tid, kRingThreads);
    // voxel heads -> output rank, then one lane per voxel sums its points in input order
    for (int t = tid; t < ncand; t += kRingThreads) iscr[t] = (t == 0 || (keys[t] >> 32) != (keys[t - 1] >> 32)) ? 1 : 0;
    __syncthreads();
    const int nvox = block_exclusive_scan(iscr, ncand, scan_tmp);
    for (int t = tid; t < ncand; t += kRingThreads) {
      const unsigned vid = (unsigned)(keys[t] >> 32);
      if (t > 0 && (unsigned)(keys[t - 1] >> 32) == vid) continue;
      float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;  // CentroidPoint<PointXYZI>: f32 sums in input order
      int npt = 0;
      for (int u = t; u < ncand; u++) {
        const u64 k = keys[u];
        if ((unsigned)(k >> 32) != vid) break;
        const float4 q = p[(int)(k & 0xffffffffu)];
        sx += q.x; sy += q.y; sz += q.z; si += q.w;
        npt++;
      }
      const float cnt = (float)npt;
      out[iscr[t]] = make_float4(sx / cnt, sy / cnt, sz / cnt, si / cnt);
    }
    if (tid == 0) S->ring_ds_cnt[r] = nvox;
  };
  sr_for_rings(S, kMaxRingLen, one_ring);   // one workgroup per ring, or the catch-all behind the big tier
}

}  // namespace vloam
