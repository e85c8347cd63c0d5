// The walk through the occupancy-block index that finds every map point within a radius of a point: the one text of it, for k_map_query
// (map_query.hip) and k_map_score (map_score.hip).  Functions only — group width, LDS arrays, wave-level fences, tiling, reductions and
// outputs are each kernel's own.  (k_map_assoc of the sweep walks another box with another probe structure and keeps its text.)
//
// The searched set is k_map_export's: live records (count != 0) of cubes inside the 21 x 21 x 11 window; a raw voxel is represented by its
// point records (seq 1 .. 255).  Per point and kind:
//   walk_axis_pieces  one lane per axis: the voxel-index box of the radius, cut into (cube, 4-voxel block, 4-bit mask) pieces in an LDS row
//   walk_block        one lane per combination of three pieces: the block's occupancy word, cut to the box; then the set voxels of that
//                     word: their records, a raw voxel's point records, each handed to the caller's functor
// Why nothing the box can hold is left out.  A record's voxel index on an axis is floorf(p * inv) of the points keyed into it (k_map_insert),
// and its cube comes from the f64 test on the same points, so a voxel that straddles a 50 m cube face exists once per cube.
//   kBoxSlack        the box is floorf((q -+ r) * inv) widened by one voxel: a centroid may sit an ulp outside the voxel its points were keyed
//                    into, and the box edges are f32 products
//   kCubeTopSlack    cube A holds the voxel indices [cube_voxel_base(A), cube_voxel_base(A + 1) + kCubeTopSlack].  Its points lie between the
//                    faces 50 A -+ 25, and the f32 product p * inv may land one cell from the f64 product of a face: the base is
//                    floor(face * inv) - 1 (so that a local index is never negative), the top is floor(next face * inv) + 1, which is the
//                    next cube's base + 2; the cell that the upper face cuts belongs to both cubes
//   kCubeRangeVoxels, kCubeRangeCubes   the cubes tried for a box [lo, hi].  By the line above an index i can belong to cube A only for
//                    floor(((i - 1) * leaf + 25) / 50) - 1 <= A <= floor(((i + 2) * leaf + 25) / 50); the range tried is that of lo - 3 below
//                    and of hi + 3, plus one cube, above: two cells, or a cell and a cube, of room for the roundings of leaf = 1 / inv and
//                    of these f64 products.  A cube tried in vain costs one empty intersection
//   kVoxMax          a local index has kVoxBits bits; k_map_insert stores nothing beyond (it reports such a point)
// Enumerating too much is harmless: a candidate counts by its distance, not by its index.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "map_table.h"
#include "map_device.h"

namespace vloam {

constexpr int kWalkPieces = 32;   // pieces per axis: 16 leaves of radius are <= 36 voxels = 10 blocks (+ 2 per cube face crossed)
constexpr int kBoxSlack = 1, kCubeTopSlack = 2, kCubeRangeVoxels = 3, kCubeRangeCubes = 1;

// a piece: | cube + 8192 | block of the cube (kVoxBits - 2 bits) | which of the block's four voxels are in the box |
__device__ __forceinline__ int piece_pack(int A, int blk, int m4) { return ((A + 8192) << 11) | (blk << 4) | m4; }
__device__ __forceinline__ int piece_cube(int w) { return (w >> 11) - 8192; }
__device__ __forceinline__ int piece_blk(int w) { return (w >> 4) & 127; }
__device__ __forceinline__ int piece_m4(int w) { return w & 15; }

// One axis of the box around coordinate qa as pieces in row[kWalkPieces].  Only cubes that can hold a map point are listed: those of the
// window (cen / wdim: its centre and size on that axis; k_map_export publishes no others) that the voxel key can name (koff: kCubeOffXY or
// kCubeOffZ, the axis' share of cube_in_key_range; nothing was ever stored under another cube), so walk_block tests neither.
// Returns the number of pieces, or the overflow flag -1: the row cannot hold them and is not to be used.
__device__ __forceinline__ int walk_axis_pieces(float qa, float radius, float inv, int cen, int wdim, int koff, int* row) {
  const int lo = (int)floorf((qa - radius) * inv) - kBoxSlack, hi = (int)floorf((qa + radius) * inv) + kBoxSlack;
  const double leaf = 1.0 / (double)inv;
  const int Amin = max(max(-koff, -cen), (int)floor(((double)(lo - kCubeRangeVoxels) * leaf + 25.0) * 0.02) - kCubeRangeCubes);
  const int Amax = min(min(koff - 1, wdim - 1 - cen), (int)floor(((double)(hi + kCubeRangeVoxels) * leaf + 25.0) * 0.02) + kCubeRangeCubes);
  int np = 0;
  bool ovf = false;
  for (int A = Amin; A <= Amax && !ovf; A++) {
    const int base = cube_voxel_base(A, inv);
    const int ia = max(lo, base), ib = min(min(hi, cube_voxel_base(A + 1, inv) + kCubeTopSlack), base + kVoxMax);
    if (ia > ib) continue;
    for (int blk = (ia - base) >> 2; blk <= ((ib - base) >> 2); blk++) {
      if (np >= kWalkPieces) { ovf = true; break; }
      int m4 = 0;
#pragma unroll
      for (int t = 0; t < 4; t++) { const int iv = base + (blk << 2) + t; if (iv >= ia && iv <= ib) m4 |= 1 << t; }
      row[np] = piece_pack(A, blk, m4);
      np++;
    }
  }
  return ovf ? -1 : np;
}

// The block that the pieces w0, w1, w2 of the x, y and z rows name, and visit(const RecVal&, unsigned slot) for every live record it leads
// to, one after the other.  Block lookup: the pieces name cubes the key holds (walk_axis_pieces); the occupancy word
// (bit = z * 16 + y * 4 + x) is cut to the box by the pieces' masks.  Voxel visit: the set bits' records; a record that was never finalized
// or was purged (count == 0) is skipped, a raw voxel stands for its point records.  A chain of kMaxProbe entries, of blocks or of records,
// counts as absent and is reported.  One function, and no test of the cube per block: with the lookup and the visit apart, or with
// cube_in_key_range in front of every probe, the score and the k = 1 query measured slower than the two copies this replaces
// (profiles/r13_map_walk.txt, section 3).
template <class Visit>
__device__ __forceinline__ void walk_block(const VoxelTable& T, int w0, int w1, int w2, bool* chain_too_long, Visit&& visit) {
  const int A0 = piece_cube(w0), A1 = piece_cube(w1), A2 = piece_cube(w2);
  const int b0 = piece_blk(w0), b1 = piece_blk(w1), b2 = piece_blk(w2);
  const int mx = piece_m4(w0), my = piece_m4(w1), mz = piece_m4(w2);
  const u64 bkey = pack_key(A0, A1, A2, b0, b1, b2) | (1ull << 63);
  u64 occ = 0ull;
  {
    unsigned bs = (unsigned)mix64(bkey) & T.bslots_mask;
    int probe = 0;
    for (; probe < kMaxProbe; probe++, bs = (bs + 1) & T.bslots_mask) {
      const ulonglong2 e = T.blk[bs];
      if (e.x == 0ull) break;
      if (e.x == bkey) { occ = e.y; break; }
    }
    if (probe == kMaxProbe) *chain_too_long = true;
  }
  const u64 ex4 = (u64)mx * 0x1111111111111111ull;
  const u64 ey4 = ((u64)((my & 1) * 0xF) | ((u64)(((my >> 1) & 1) * 0xF) << 4) | ((u64)(((my >> 2) & 1) * 0xF) << 8) | ((u64)(((my >> 3) & 1) * 0xF) << 12)) * 0x0001000100010001ull;
  const u64 ez4 = ((mz & 1) ? 0xFFFFull : 0ull) | ((mz & 2) ? 0xFFFFull << 16 : 0ull) | ((mz & 4) ? 0xFFFFull << 32 : 0ull) | ((mz & 8) ? 0xFFFFull << 48 : 0ull);
  occ &= ex4 & ey4 & ez4;
  while (occ) {
    const int bit = __ffsll((long long)occ) - 1;
    occ &= occ - 1;
    const u64 key = pack_key(A0, A1, A2, (b0 << 2) | (bit & 3), (b1 << 2) | ((bit >> 2) & 3), (b2 << 2) | (bit >> 4));
    RecVal v;
    unsigned slot = 0;
    if (!rec_find(T, key, &v, &slot, chain_too_long) || v.count == 0) continue;
    if (!rec_raw(v.count)) { visit(v, slot); continue; }
    const int nr = min(rec_n(v.count), 255);
    for (int seq = 1; seq <= nr; seq++) {
      RecVal pv;
      unsigned ps = 0;
      if (rec_find(T, key_with_seq(key, seq), &pv, &ps, chain_too_long) && pv.count != 0) visit(pv, ps);
    }
  }
}

}  // namespace vloam

