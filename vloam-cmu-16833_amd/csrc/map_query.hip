// Map queries on gfx950: the k nearest map points of caller-supplied points (vloam_map_query / vloam_map_query_device).
// A code object of its own, with its own text of the walk through the occupancy-block index (map_table.h is all it shares with the sweep's
// kernels): a handle that never queries launches nothing of this, and no kernel of a sweep changes.
//
// The searched set is k_map_export's: live records (count != 0) of cubes inside the 21 x 21 x 11 window; a centroid is sum / n in f32, a raw
// voxel is represented by its point records (seq 1 .. 255).  Per query and kind the voxel-index box of the radius (one voxel of slack on
// every side: a centroid may sit an ulp outside the voxel its points were keyed into, and the box edges are f32 products) is cut per axis
// into (cube, 4-voxel block, 4-bit mask) pieces — a voxel that straddles a 50 m cube face exists once per cube —, the lanes of the query's
// group probe VoxelTable::blk for the blocks, visit the voxels whose bit is set, and keep a sorted top-k of (d2, export order key) in
// registers.  The group's lists are merged by k arg-min rounds over shuffles.  Enumerating too much is harmless (a candidate counts by
// its distance, not by its index); nothing the box can hold is left out.
//   d2 = (dx*dx + dy*dy) + dz*dz, every product and sum rounded on its own (__fmul_rn / __fadd_rn: no FMA); a neighbour qualifies when
//   d2 <= r*r (f32 product); equal d2 resolve to the smaller export order key.
#include <hip/hip_runtime.h>
#include <math.h>
#include "map_table.h"

namespace vloam {

namespace {

constexpr int kQG = 32;              // lanes per query: two queries per wavefront, eight per workgroup
constexpr int kQPerWg = 256 / kQG;
constexpr int kQPieces = 32;         // (cube, block) pieces per axis: 16 leaves of radius are <= 36 voxels = 10 blocks (+ 2 per cube face crossed)
constexpr unsigned kQNone = 0xffffffffu;

struct QPoint { float4 p; u64 okey; };

// the point a live record stands for and its place in vloam_get_map's order: k_map_export's arithmetic (map_output.hip)
__device__ __forceinline__ QPoint q_point(const RecVal& v, int wi, int wj, int wk, int kind) {
  const int seq = key_seq(v.key);
  const u64 cube = (u64)(wi + kCubeW * wj + kCubeW * kCubeH * wk);
  const u64 lx = (u64)key_lx(v.key), ly = (u64)key_ly(v.key), lz = (u64)key_lz(v.key);
  const bool tail = seq != 0 && v.pend_cnt != 0;
  QPoint r;
  r.okey = (cube << 50) | ((u64)kind << 49) | ((u64)(tail ? 1 : 0) << 48) | (tail ? (u64)(unsigned)v.pend_cnt : ((lz << (2 * kVoxBits)) | (ly << kVoxBits) | lx));
  const int n = seq ? 1 : rec_n(v.count);
  const float nn = (float)n;
  r.p.x = n > 1 ? v.sum.x / nn : v.sum.x; r.p.y = n > 1 ? v.sum.y / nn : v.sum.y; r.p.z = n > 1 ? v.sum.z / nn : v.sum.z;
  r.p.w = n > 1 ? v.sum.w / nn : v.sum.w;
  return r;
}

// bounded lookup of one record; a chain of kMaxProbe slots counts as absent and is reported
__device__ __forceinline__ bool q_find(const VoxelTable& T, u64 key, RecVal* out, unsigned* slot, bool* chain_too_long) {
  unsigned s = (unsigned)mix64(key) & T.mask;
  for (int probe = 0; probe < kMaxProbe; probe++, s = (s + 1) & T.mask) {
    const RecVal v = rec_load(&T.rec[s]);
    if (v.key == 0ull) return false;
    if (v.key == key) { *out = v; *slot = s; return true; }
  }
  *chain_too_long = true;
  return false;
}

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
  __shared__ int s_piece[kQPerWg][3][kQPieces];
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
        const int lo = (int)floorf((qa - radius) * inv) - 1, hi = (int)floorf((qa + radius) * inv) + 1;
        const double leaf = 1.0 / (double)inv;
        // cube A holds the voxel indices [base(A), base(A + 1) + 2] (k_map_insert: index = floorf(p * inv), cube by the f64 test)
        const int Amin = (int)floor(((double)(lo - 3) * leaf + 25.0) * 0.02) - 1, Amax = (int)floor(((double)(hi + 3) * leaf + 25.0) * 0.02) + 1;
        int np = 0;
        bool ovf = false;
        for (int A = Amin; A <= Amax && !ovf; A++) {
          const int wv = A + cen;
          if (wv < 0 || wv >= wdim) continue;   // outside the window: not part of the map (k_map_export)
          const int base = (int)floor((50.0 * (double)A - 25.0) * (double)inv) - 1;
          const int top_i = (int)floor((50.0 * (double)(A + 1) - 25.0) * (double)inv) - 1 + 2;
          const int ia = max(lo, base), ib = min(min(hi, top_i), base + kVoxMax);
          if (ia > ib) continue;
          for (int blk = (ia - base) >> 2; blk <= ((ib - base) >> 2); blk++) {
            if (np >= kQPieces) { ovf = true; break; }
            int m4 = 0;
#pragma unroll
            for (int t = 0; t < 4; t++) { const int iv = base + (blk << 2) + t; if (iv >= ia && iv <= ib) m4 |= 1 << t; }
            s_piece[qi][gl][np] = ((A + 8192) << 11) | (blk << 4) | m4;
            np++;
          }
        }
        s_np[qi][gl] = np;
        if (ovf) s_np[qi][3] = 1;
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
        const int A0 = (w0 >> 11) - 8192, A1 = (w1 >> 11) - 8192, A2 = (w2 >> 11) - 8192;
        const int b0 = (w0 >> 4) & 127, b1 = (w1 >> 4) & 127, b2 = (w2 >> 4) & 127;
        const int mx = w0 & 15, my = w1 & 15, mz = w2 & 15;
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
          if (probe == kMaxProbe) chain_too_long = true;
        }
        // voxels of the block inside the box: bit = z * 16 + y * 4 + x
        const u64 ex4 = (u64)mx * 0x1111111111111111ull;
        const u64 ey4 = ((u64)((my & 1) * 0xF) | ((u64)(((my >> 1) & 1) * 0xF) << 4) | ((u64)(((my >> 2) & 1) * 0xF) << 8) | ((u64)(((my >> 3) & 1) * 0xF) << 12)) * 0x0001000100010001ull;
        const u64 ez4 = ((mz & 1) ? 0xFFFFull : 0ull) | ((mz & 2) ? 0xFFFFull << 16 : 0ull) | ((mz & 4) ? 0xFFFFull << 32 : 0ull) | ((mz & 8) ? 0xFFFFull << 48 : 0ull);
        occ &= ex4 & ey4 & ez4;
        const int wi = A0 + cen0, wj = A1 + cen1, wk = A2 + cen2;
        auto consider = [&](const RecVal& v, unsigned slot) {
          const QPoint c = q_point(v, wi, wj, wk, kind);
          const float dx = qp.x - c.p.x, dy = qp.y - c.p.y, dz = qp.z - c.p.z;
          const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
          if (d2 <= r2) q_insert<K>(top, __float_as_uint(d2), c.okey, ((unsigned)kind << 31) | slot);
        };
        while (occ) {
          const int bit = __ffsll((long long)occ) - 1;
          occ &= occ - 1;
          const u64 key = pack_key(A0, A1, A2, (b0 << 2) | (bit & 3), (b1 << 2) | ((bit >> 2) & 3), (b2 << 2) | (bit >> 4));
          RecVal v;
          unsigned slot = 0;
          if (!q_find(T, key, &v, &slot, &chain_too_long) || v.count == 0) continue;   // never finalized, or purged
          if (!rec_raw(v.count)) { consider(v, slot); continue; }
          const int nr = min(rec_n(v.count), 255);   // a raw voxel: its points, one record each
          for (int seq = 1; seq <= nr; seq++) {
            RecVal pv;
            unsigned ps = 0;
            if (q_find(T, key_with_seq(key, seq), &pv, &ps, &chain_too_long) && pv.count != 0) consider(pv, ps);
          }
        }
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
        const RecVal v = rec_load(&T.rec[ref & 0x7fffffffu]);
        int Ai, Aj, Ak;
        unpack_cube(v.key, &Ai, &Aj, &Ak);
        const QPoint c = q_point(v, Ai + cen0, Aj + cen1, Ak + cen2, kind);
        out[(size_t)q * k + r] = c.p;
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
