// What sr_launch / sr_init (sr_kernels.hip) need of the ring kernels: the tier capacities, the LDS carve-up of k_sr_ring and the kernels'
// declarations.  The kernels themselves: sr_ring.hip (LDS tiers), sr_ring_long.hip (long tier).
#pragma once
#include <hip/hip_runtime.h>
#include "vloam_device.h"
#include "sr_ring_dev.h"

namespace vloam {

typedef unsigned long long u64;

// Two capacity tiers of the LDS-resident ring.  CAP = kRingCapSmall covers every real HDL-64E / HDL-32 / VLP-16 ring (a revolution
// has <= ~2 100 firings) in 78.75 KB of LDS, so TWO rings share a CU (and other kernels' workgroups still find LDS next to one);
// the kMaxRingLen tier (146 KB, one workgroup per CU) is launched right behind it and only works on rings the small tier had to
// leave alone (len > kRingCapSmall).
constexpr int kRingCapSmall = 2176, kSectCapSmall = 512;

// The dynamic LDS of k_sr_ring<CAP, SECT>: byte offsets of its arrays and their total.  (All LDS lives in the dynamic region so its base
// stays 16-B aligned.)
template <int CAP, int SECT>
struct SrRingLds {
  static_assert(CAP % 4 == 0, "the byte arrays keep the words behind them aligned");
  static constexpr size_t px = 0, py = px + sizeof(float) * CAP, pz = py + sizeof(float) * CAP;   // [CAP] floats each
  static constexpr size_t pi = pz + sizeof(float) * CAP;                                          // [CAP] intensity
  static constexpr size_t keys = pi + sizeof(float) * CAP;   // debug sort: u64 [kSectors * SECT]; VoxelGrid: run keys [CAP] + voxel ids [CAP]
  static constexpr size_t keys_bytes = sizeof(u64) * kSectors * SECT > (size_t)12 * CAP ? sizeof(u64) * kSectors * SECT : (size_t)12 * CAP;
  static constexpr size_t iscratch = keys + keys_bytes;                    // [CAP] ints: heads / ranks
  static constexpr size_t scan_tmp = iscratch + sizeof(int) * CAP;         // [kRingThreads] ints
  static constexpr size_t picked = scan_tmp + sizeof(int) * kRingThreads;  // [CAP] bytes each: picked, label, gap, reach
  static constexpr size_t label = picked + CAP, gap = label + CAP, reach = gap + CAP;
  // per-sector words, eight ints a slot (slots 2 and 3 are unused)
  static constexpr size_t slot = 8 * sizeof(int);
  static constexpr size_t sp = reach + CAP, ep = sp + slot;          // [kSectors] sector bounds
  static constexpr size_t leak_lo = sp + 4 * slot, leak_hi = sp + 5 * slot;   // [kSectors] lowest / highest local index marked by sector s's picks (unclipped)
  static constexpr size_t zone = sp + 6 * slot;                      // [kSectors] incoming spill the sector was computed with
  static constexpr size_t any = sp + 7 * slot;
  static constexpr size_t bytes = sp + 8 * slot;
};
static_assert(2 * SrRingLds<kRingCapSmall, kSectCapSmall>::bytes <= 160 * 1024, "two small-tier rings must fit the 160 KB of LDS of one CU");

template <int CAP, int SECT, bool BIG_TIER>
__global__ void k_sr_ring(const float4* __restrict__ cloud, FrameScalars* S, int* __restrict__ sharp_idx, int* __restrict__ less_sharp_idx,
                          int* __restrict__ flat_idx, float4* __restrict__ ring_ds, float* __restrict__ dbg_curv, int* __restrict__ dbg_sort,
                          int* __restrict__ dbg_picked, int* __restrict__ dbg_label, long long* __restrict__ dbg_cyc /* [rings][8] */,
                          int* ring_watch /* host-mapped [2][kMaxBatch] */, int tier_follows, size_t ss);   // instantiated in sr_ring.hip: the two tiers

__global__ void k_sr_ring_long(const float4* __restrict__ cloud, FrameScalars* S, int* __restrict__ sharp_idx, int* __restrict__ less_sharp_idx,
                               int* __restrict__ flat_idx, int cap, int kcap, u64* keys_all, int* iscr_all, unsigned char* bytes_all, float4* ds_all,
                               float* __restrict__ dbg_curv, int* __restrict__ dbg_sort, int* __restrict__ dbg_picked, int* __restrict__ dbg_label,
                               size_t ss);

}  // namespace vloam
