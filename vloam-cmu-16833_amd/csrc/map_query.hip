// Map queries on gfx950: the k nearest map points of caller-supplied points (vloam_map_query / vloam_map_query_device).
// A code object of its own (map_table.h and map_device.h are all it shares with the sweep's kernels): a handle that never queries launches
// nothing of this, and no kernel of a sweep changes.
//
// The searched set is k_map_export's.  The walk through the occupancy-block index — the box of the radius as per-axis pieces, the blocks, the
// voxel records, and why nothing the box can hold is left out — is map_walk.h's, shared with map_score.hip.  Here: 32 lanes per query take
// the box's blocks in turn and keep a sorted top-k of (d2, export order key) in registers; the group's lists are merged by k arg-min rounds
// over shuffles.
//   d2 = (dx*dx + dy*dy) + dz*dz, every product and sum rounded on its own (__fmul_rn / __fadd_rn: no FMA); a neighbour qualifies when
//   d2 <= r*r (f32 product); equal d2 resolve to the smaller export order key.
#include <hip/hip_runtime.h>
#include <math.h>
#include "map_walk.h"

namespace vloam {

namespace {

constexpr int kQG = 32;              // lanes per query: two queries per wavefront, eight per workgroup
constexpr int kQPerWg = 256 / kQG;
constexpr unsigned kQNone = 0xffffffffu;

// a lane's best K so far, ascending by (d2 bits, order key); ref = kind << 31 | table slot (the point is read again when it wins)
template <int K>
struct QTop { unsigned d[K]; u64 ok[K]; unsigned ref[K]; };

template <int K>
__device__ __forceinline__ void q_insert(QTop<K>& t, unsigned d, u64 ok, unsigned ref) {
  if (!(d < t.d[K - 1] || (d == t.d[K - 1] && ok < t.ok[K - 1]))) return;
#pragma unroll
  for (int j = 0; j < K; j++) {
    const bool lt = d < t.d[j] || (d == t.d[j] && ok < t.ok[j]);
    const unsigned td = t.d[j], tr = t.ref[j];
    const u64 to = t.ok[j];
    t.d[j] = lt ? d : td; t.ok[j] = lt ? ok : to; t.ref[j] = lt ? ref : tr;
    d = lt ? td : d; ok = lt ? to : ok; ref = lt ? tr : ref;
  }
}

}  // namespace

// kinds: bit 0 corner map, bit 1 surf map.  out / d2: [n][k], count: [n].  Any n on a bounded grid (grid-stride over groups of kQPerWg queries).
template <int K>
__global__ __launch_bounds__(256) void k_map_query(VoxelTable T0, VoxelTable T1, float inv0, float inv1, const MapState* __restrict__ ms, MapFrame* fr,
                                                   int kinds, int k, float radius, float r2, const float4* __restrict__ qpts, int n,
                                                   float4* __restrict__ out, float* __restrict__ out_d2, int* __restrict__ out_count) {
  __shared__ int s_piece[kQPerWg][3][kWalkPieces];
  __shared__ int s_np[kQPerWg][4];   // pieces per axis | more pieces than the table holds
  const int lane = threadIdx.x & 63, gl = lane & (kQG - 1), qi = threadIdx.x / kQG;
  const int cen0 = ms->cenW, cen1 = ms->cenH, cen2 = ms->cenD;
  bool chain_too_long = false, piece_overflow = false;
  for (int q0 = (int)blockIdx.x * kQPerWg; q0 < n; q0 += (int)gridDim.x * kQPerWg) {   // workgroup-uniform
    const int q = q0 + qi;
    const bool live = q < n;
    const float4 qp = live ? qpts[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    // a non-finite query, or one far outside the +-25.6 km the voxel key spans (and outside what an int voxel index holds), has no neighbours
    const bool search = live && fabsf(qp.x) <= 1.0e6f && fabsf(qp.y) <= 1.0e6f && fabsf(qp.z) <= 1.0e6f;
    QTop<K> top;
#pragma unroll
    for (int j = 0; j < K; j++) { top.d[j] = kQNone; top.ok[j] = ~0ull; top.ref[j] = 0u; }
    for (int kind = 0; kind < 2; kind++) {
      if (!((kinds >> kind) & 1)) continue;
      const VoxelTable T = kind ? T1 : T0;
      const float inv = kind ? inv1 : inv0;
      // ---- the box, per axis, as pieces (lane a of the group lists axis a)
      if (gl < 4) s_np[qi][gl] = 0;
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (search && gl < 3) {
        const float qa = gl == 0 ? qp.x : (gl == 1 ? qp.y : qp.z);
        const int cen = gl == 0 ? cen0 : (gl == 1 ? cen1 : cen2), wdim = gl == 0 ? kCubeW : (gl == 1 ? kCubeH : kCubeD);
        const int np = walk_axis_pieces(qa, radius, inv, cen, wdim, gl == 2 ? kCubeOffZ : kCubeOffXY, s_piece[qi][gl]);
        s_np[qi][gl] = np;
        if (np < 0) s_np[qi][3] = 1;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const int np0 = s_np[qi][0], np1 = s_np[qi][1], np2 = s_np[qi][2];
      const bool ovf = s_np[qi][3] != 0;
      piece_overflow = piece_overflow || ovf;
      const int nblocks = (search && !ovf) ? np0 * np1 * np2 : 0;
      // ---- blocks over the lanes, voxels of a block one after the other
      for (int bb = gl; bb < nblocks; bb += kQG) {
        const int n01 = np0 * np1;
        const int ez = bb / n01, rem = bb - ez * n01, ey = rem / np0, ex = rem - ey * np0;
        const int w0 = s_piece[qi][0][ex], w1 = s_piece[qi][1][ey], w2 = s_piece[qi][2][ez];
        const int cube = (piece_cube(w0) + cen0) + kCubeW * (piece_cube(w1) + cen1) + kCubeW * kCubeH * (piece_cube(w2) + cen2);   // of the window
        walk_block(T, w0, w1, w2, &chain_too_long, [&](const RecVal& v, unsigned slot) {
          const float4 c = rec_point(v);
          const u64 okey = rec_order_key(v, cube, kind);
          const float dx = qp.x - c.x, dy = qp.y - c.y, dz = qp.z - c.z;
          const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
          if (d2 <= r2) q_insert<K>(top, __float_as_uint(d2), okey, ((unsigned)kind << 31) | slot);
        });
      }
    }
    // ---- merge: k rounds of the group's arg-min over the lanes' heads (keys are unique: one order key per record); the winner writes its point
    int found = 0;
    for (int r = 0; r < k; r++) {
      unsigned md = top.d[0];
      u64 mo = top.ok[0];
#pragma unroll
      for (int sh = kQG / 2; sh >= 1; sh >>= 1) {
        const unsigned od = (unsigned)__shfl_xor((int)md, sh);
        const u64 oo = (u64)__shfl_xor((unsigned long long)mo, sh);
        const bool lt = od < md || (od == md && oo < mo);
        md = lt ? od : md; mo = lt ? oo : mo;
      }
      if (md == kQNone) continue;
      found++;
      if (live && top.d[0] == md && top.ok[0] == mo) {
        const unsigned ref = top.ref[0];
        const int kind = (int)(ref >> 31);
        const VoxelTable T = kind ? T1 : T0;
        out[(size_t)q * k + r] = rec_point(rec_load(&T.rec[ref & 0x7fffffffu]));
        out_d2[(size_t)q * k + r] = __uint_as_float(md);
#pragma unroll
        for (int j = 0; j + 1 < K; j++) { top.d[j] = top.d[j + 1]; top.ok[j] = top.ok[j + 1]; top.ref[j] = top.ref[j + 1]; }
        top.d[K - 1] = kQNone; top.ok[K - 1] = ~0ull; top.ref[K - 1] = 0u;
      }
    }
    if (live && gl >= found && gl < k) { out[(size_t)q * k + gl] = make_float4(0.f, 0.f, 0.f, 0.f); out_d2[(size_t)q * k + gl] = 0.f; }
    if (live && gl == 0) out_count[q] = found;
  }
  if (__ballot(chain_too_long || piece_overflow) != 0ull && lane == 0) atomicOr(&fr->error, kErrMapFull);
}

// Enqueue only: the selected session's tables as they are on `st` at this point (behind the last mapping and any growth step enqueued so far).
vloam_status map_query_enqueue(MapContext* m0, hipStream_t st, int kind, int k, float radius, const void* d_xyz_pad4, int n, void* d_xyzi4, void* d_d2,
                               void* d_count) {
  const MapContext msel = m0->for_session(m0->sel);
  const MapContext* m = &msel;
  const int kinds = kind == 2 ? 3 : (1 << kind);
  const float r2 = radius * radius;
  const int groups = (n + kQPerWg - 1) / kQPerWg;
  const dim3 grid((unsigned)(groups < 4096 ? groups : 4096));
#define VL_QUERY(KK)                                                                                                                              \
  VL_RAW_LAUNCH(k_map_query<KK>, grid, dim3(256), 0, st, m->tab[0], m->tab[1], m->inv_leaf[0], m->inv_leaf[1], m->state, m->frame, kinds, k, radius, r2, \
                (const float4*)d_xyz_pad4, n, (float4*)d_xyzi4, (float*)d_d2, (int*)d_count)
  if (k == 1) VL_QUERY(1);
  else if (k <= 5) VL_QUERY(5);
  else VL_QUERY(8);
#undef VL_QUERY
  return hipGetLastError() == hipSuccess ? VLOAM_OK : VLOAM_ERR_HIP;
}

}  // namespace vloam
