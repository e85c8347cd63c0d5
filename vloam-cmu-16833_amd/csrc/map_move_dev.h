// Device text that the three movers of voxel records share, and nothing else includes: the tombstone rebuild of a fixed handle
// (k_map_rebuild_* in map_kernels.hip), the growth step and same-size rehash of a growable one (k_map_grow in map_grow.hip) and the restore of a
// checkpoint (k_map_ckpt_unpack in map_ckpt.hip).  Each moves every live record of a source (a staging list, the old table, a dense stream)
// into an EMPTY table Tn; what happens to a record on the way is written here once.  Every function is inlined.  k_map_grow and
// k_map_ckpt_unpack are wavefront-uniform and count the keys by ballot (map_reinsert_wave); k_map_rebuild_insert knows the count from its list
// and calls map_reinsert per lane (the ballot form of it measured 0.6 us slower per launch, profiles/r15_table_moves_one_text.txt).
#pragma once
#include <hip/hip_runtime.h>
#include "map_kernels.h"
#include "map_table.h"

namespace vloam {

// grid of a mover over n slots or records: every wave slot of the chip (256 CUs x 8 workgroups of 4 wavefronts), grid-stride beyond
constexpr int kMoveMaxGrid = 2048;
static inline unsigned map_move_grid(size_t n) { const size_t b = (n + 255) / 256; return (unsigned)(b < kMoveMaxGrid ? b : kMoveMaxGrid); }
static inline unsigned map_move_grid(const VoxelTable& T) { return map_move_grid((size_t)T.mask + 1); }   // over a table's slots

// In front of a move into Tn, by one thread: slot ids change, so the lists that hold them (deferred, newraw) are rebuilt from the raw flags,
// and the table's counters {keys, purged, block keys, -} start over
__device__ __forceinline__ void map_move_begin(const VoxelTable& Tn, MapFrame* fr, int kind) {
  fr->n_deferred[kind] = 0; fr->n_newraw[kind] = 0;
  Tn.stats[0] = 0; Tn.stats[1] = 0; Tn.stats[2] = 0; Tn.stats[3] = 0;
}

// One live record into table Tn: claim a slot (keys are unique in the source), store the value, publish the voxel's occupancy block and
// re-append a raw voxel (still owed a centroid, see k_map_finalize) to the deferred list.  pend[] of Tn is not written: between two sweeps
// every seq-0 record has pend_cnt == 0 (k_map_finalize stored it), and a raw point's pend_cnt is its arrival stamp, kept with the value.
// false: no slot within the probe bound (kErrMapFull raised).
__device__ __forceinline__ bool map_reinsert(const VoxelTable& Tn, const RecVal& v, MapFrame* fr, int kind, int* __restrict__ deferred, int deferred_cap) {
  bool done = false;
  const int seq = key_seq(v.key);
  unsigned s = (unsigned)mix64(v.key) & Tn.mask;
  for (int probe = 0; probe < kMaxProbe && !done; probe++, s = (s + 1) & Tn.mask) {
    if (atomicCAS(&Tn.rec[s].key, 0ull, v.key) != 0ull) continue;
    rec_store_value(&Tn.rec[s], v.sum, v.count, seq ? v.pend_cnt : 0);
    int Ai, Aj, Ak;
    unpack_cube(v.key, &Ai, &Aj, &Ak);
    if (seq == 0 && !map_publish_block(Tn, Ai, Aj, Ak, key_lx(v.key), key_ly(v.key), key_lz(v.key))) atomicOr(&fr->error, kErrMapFull);
    if (seq == 0 && rec_raw(v.count)) {
      const int dpos = atomicAdd(&fr->n_deferred[kind], 1);
      if (dpos < deferred_cap) deferred[dpos] = (int)s;
    }
    done = true;
  }
  if (!done) atomicOr(&fr->error, kErrMapFull);
  return done;
}

// Called by a whole wavefront: the lanes that hold a live record re-insert it, and the keys now in Tn are counted with one add per wavefront:
// stats {keys, 0, block keys} (the block keys are counted by map_publish_block)
__device__ __forceinline__ void map_reinsert_wave(const VoxelTable& Tn, bool live, const RecVal& v, MapFrame* fr, int kind, int* __restrict__ deferred, int deferred_cap) {
  const bool done = live && map_reinsert(Tn, v, fr, kind, deferred, deferred_cap);
  const u64 lm = __ballot(done);
  if ((threadIdx.x & 63) == 0 && lm != 0ull) atomicAdd(&Tn.stats[0], __popcll(lm));
}

}  // namespace vloam
