// The voxel tables of the map as device code sees them: hash, voxel key, record access, occupancy blocks.  Shared by map_kernels.hip (the
// sweep's kernels), map_output.hip (export and publication), map_import.hip, the three movers of records (through map_move_dev.h, which holds
// their text) and, through map_walk.h, map_query.hip and map_score.hip, which are separate code objects.  rec_find, rec_point and rec_order_key serve the map's readers
// only (map_output.hip, map_walk.h and its two kernels): the sweep's kernels keep their own lookups.
#pragma once
#include <hip/hip_runtime.h>
#include "map_kernels.h"

namespace vloam {

typedef unsigned long long u64;

__device__ __forceinline__ u64 mix64(u64 x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}

// Voxel key: | seq 8 (56-63) | - | cube i + 512 (10: 45-54) | cube j + 512 (10: 35-44) | cube k + 128 (8: 27-34) | voxel lx (18-26), ly (9-17),
// lz (0-8) inside the cube, 9 bits each |.  Nine bits per axis take any leaf down to 50 m / 508 (the reference's launch files use 0.2 / 0.4 and
// 0.4 / 0.8, laser_mapping.cpp:95-101 takes any value; vloam_create's bound of 0.132 m comes from the 32-bit tie rank of k_map_assoc, not
// from the key).  seq = 0: the voxel's record (centroid, or the running sum of a raw voxel); seq = 1..255: one RAW point of a voxel whose
// cube lies outside the valid 5 x 5 x 3 block (see k_map_finalize) — the reference keeps such points un-merged in their cube until the
// cube is next re-filtered, and its kd-tree sees them one by one.  Cubes are absolute (no window offset): +-25.6 km horizontally,
// +-6.4 km vertically around the start (k_map_insert reports anything beyond).
constexpr int kCubeOffXY = 512, kCubeOffZ = 128;
constexpr int kVoxBits = 9, kVoxMax = (1 << kVoxBits) - 1;
__device__ __forceinline__ u64 pack_key(int Ai, int Aj, int Ak, int lx, int ly, int lz) {
  return ((u64)(unsigned)(Ai + kCubeOffXY) << 45) | ((u64)(unsigned)(Aj + kCubeOffXY) << 35) | ((u64)(unsigned)(Ak + kCubeOffZ) << 27) |
         ((u64)(unsigned)lx << (2 * kVoxBits)) | ((u64)(unsigned)ly << kVoxBits) | (u64)(unsigned)lz;
}
__device__ __forceinline__ void unpack_cube(u64 k, int* Ai, int* Aj, int* Ak) {
  *Ai = (int)((k >> 45) & 0x3ff) - kCubeOffXY; *Aj = (int)((k >> 35) & 0x3ff) - kCubeOffXY; *Ak = (int)((k >> 27) & 0xff) - kCubeOffZ;
}
__device__ __forceinline__ int key_lx(u64 k) { return (int)((k >> (2 * kVoxBits)) & kVoxMax); }
__device__ __forceinline__ int key_ly(u64 k) { return (int)((k >> kVoxBits) & kVoxMax); }
__device__ __forceinline__ int key_lz(u64 k) { return (int)(k & kVoxMax); }
__device__ __forceinline__ bool cube_in_key_range(int Ai, int Aj, int Ak) {
  return Ai >= -kCubeOffXY && Ai < kCubeOffXY && Aj >= -kCubeOffXY && Aj < kCubeOffXY && Ak >= -kCubeOffZ && Ak < kCubeOffZ;
}
__device__ __forceinline__ int key_seq(u64 k) { return (int)(k >> 56); }
__device__ __forceinline__ u64 key_with_seq(u64 k, int seq) { return (k & 0x00ffffffffffffffull) | ((u64)(unsigned)seq << 56); }
// VoxelRec::count of a seq-0 record: points in the sum (low 16 bits) | kRecRaw when the voxel holds raw points (its cube was outside the
// valid block when they arrived): then records seq = 1..n hold the points themselves
constexpr int kRecRaw = 1 << 30;
__device__ __forceinline__ int rec_n(int count) { return count & 0xffff; }
__device__ __forceinline__ bool rec_raw(int count) { return (count & kRecRaw) != 0; }

// A voxel record as two 16-byte loads of one 32-byte line
struct RecVal { u64 key; float4 sum; int count, pend_cnt; };
__device__ __forceinline__ RecVal rec_load(const VoxelRec* r) {
  const uint4 a = reinterpret_cast<const uint4*>(r)[0], b = reinterpret_cast<const uint4*>(r)[1];
  RecVal v;
  v.key = (u64)a.x | ((u64)a.y << 32);
  v.sum = make_float4(__uint_as_float(a.z), __uint_as_float(a.w), __uint_as_float(b.x), __uint_as_float(b.y));
  v.count = (int)b.z; v.pend_cnt = (int)b.w;
  return v;
}
// live: the slot holds a key that was not purged (a purged record keeps its key so that probe chains stay intact)
__device__ __forceinline__ bool rec_live(const RecVal& v) { return v.key != 0ull && v.count != 0; }
// everything but the key (which only find-or-insert writes)
__device__ __forceinline__ void rec_store_value(VoxelRec* r, float4 sum, int count, int pend_cnt) {
  reinterpret_cast<float2*>(r)[1] = make_float2(sum.x, sum.y);
  reinterpret_cast<uint4*>(r)[1] = make_uint4(__float_as_uint(sum.z), __float_as_uint(sum.w), (unsigned)count, (unsigned)pend_cnt);
}
// a whole record into a list or stream (not a table slot: no reader races for the key).  pend_cnt leaves a table as what it is between two
// sweeps: a point record's arrival stamp, zero for a voxel's record
__device__ __forceinline__ void rec_store_all(VoxelRec* r, const RecVal& v) {
  uint4* o = reinterpret_cast<uint4*>(r);
  o[0] = make_uint4((unsigned)v.key, (unsigned)(v.key >> 32), __float_as_uint(v.sum.x), __float_as_uint(v.sum.y));
  o[1] = make_uint4(__float_as_uint(v.sum.z), __float_as_uint(v.sum.w), (unsigned)v.count, key_seq(v.key) ? (unsigned)v.pend_cnt : 0u);
}

// bounded lookup of one record; a chain of kMaxProbe slots counts as absent and is reported.  slot (may be null): where the record was found
__device__ __forceinline__ bool rec_find(const VoxelTable& T, u64 key, RecVal* out, unsigned* slot, bool* chain_too_long) {
  unsigned s = (unsigned)mix64(key) & T.mask;
  for (int probe = 0; probe < kMaxProbe; probe++, s = (s + 1) & T.mask) {
    const RecVal v = rec_load(&T.rec[s]);
    if (v.key == 0ull) return false;
    if (v.key == key) { *out = v; if (slot) *slot = s; return true; }
  }
  *chain_too_long = true;
  return false;
}

// What the map's readers (export, publication, queries, scores) make of a live record that is not a raw voxel's running sum; they are compared
// bit for bit with each other, so this is the only text of it.  The point: a centroid is sum / n in f32, a point record (seq != 0) the point itself.
__device__ __forceinline__ float4 rec_point(const RecVal& v) {
  const int n = key_seq(v.key) ? 1 : rec_n(v.count);
  const float nn = (float)n;
  return make_float4(n > 1 ? v.sum.x / nn : v.sum.x, n > 1 ? v.sum.y / nn : v.sum.y, n > 1 ? v.sum.z / nn : v.sum.z, n > 1 ? v.sum.w / nn : v.sum.w);
}
// Its place in /laser_cloud_map: | window cube index 13 | kind 1 | tail 1 | 16 zero bits | voxel (lz, ly, lx) or arrival stamp, 32 |.  tail: an
// un-merged arrival, behind the cube's voxel-ordered part by arrival stamp (a centroid that became raw point number one has stamp 0 and stays)
__device__ __forceinline__ u64 rec_order_key(const RecVal& v, int cube_index, int kind) {
  const u64 lx = (u64)key_lx(v.key), ly = (u64)key_ly(v.key), lz = (u64)key_lz(v.key);
  const bool tail = key_seq(v.key) != 0 && v.pend_cnt != 0;
  return ((u64)cube_index << 50) | ((u64)kind << 49) | ((u64)(tail ? 1 : 0) << 48) | (tail ? (u64)(unsigned)v.pend_cnt : ((lz << (2 * kVoxBits)) | (ly << kVoxBits) | lx));
}

// set the voxel's bit in its 4 x 4 x 4 block's occupancy mask (find-or-insert of the block entry)
__device__ bool map_publish_block(const VoxelTable& T, int Ai, int Aj, int Ak, int lx, int ly, int lz) {
  const u64 bkey = pack_key(Ai, Aj, Ak, lx >> 2, ly >> 2, lz >> 2) | (1ull << 63);
  unsigned bs = (unsigned)mix64(bkey) & T.bslots_mask;
  for (int bp = 0; bp < kMaxProbe; bp++, bs = (bs + 1) & T.bslots_mask) {
    const u64 bold = atomicCAS(&T.blk[bs].x, 0ull, bkey);
    if (bold == 0ull || bold == bkey) {
      if (bold == 0ull) atomicAdd(&T.stats[2], 1);
      atomicOr(&T.blk[bs].y, 1ull << (((lz & 3) << 4) | ((ly & 3) << 2) | (lx & 3)));
      return true;
    }
  }
  return false;
}

}  // namespace vloam
