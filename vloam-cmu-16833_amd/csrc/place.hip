// Place recognition on gfx950: the descriptor of a sweep, and one descriptor against every row of a database at every yaw shift
// (vloam_place_*; c_api.h holds the specification).  A code object of its own: a handle that never calls vloam_place_enable launches nothing
// of this, and no kernel of a sweep changes.  Floating point ends where a point has its cell; everything behind that is integers, so a
// descriptor, a distance and a ranking are functions of the inputs alone, whatever the launch geometry.
//
// k_place_describe: grid-stride over the points; a workgroup keeps the cell maxima in LDS (integer atomicMax) and merges its non-empty cells
//   into the global scratch with integer atomicMax.  k_place_pack: one workgroup turns the scratch into sector-major bytes and counts.
// k_place_match (the hot path): rows x shifts x cells.  One wavefront per row, lanes are shifts.  The query sits DOUBLED in LDS (2 S sectors),
//   so lane s reads sector j + s and no modulo is taken.  The row is read once per pass of lanes, 64 words at a time with one coalesced load,
//   and each word then reaches all lanes through v_readlane (a scalar operand, no LDS traffic); a lane adds four cells per v_sad_u8.
//   LDS layout: lane s and row word (j, i) read dword (j + s) * Wp + i.  ds_read_b32 banks are dword % 32 within each 32-lane half, so the
//   lane stride must be odd: Wp = W | 1 (W = 5, the default, stays 5; W = 8 becomes 9 — with 8, lanes l and l + 4 would share a bank, eight
//   lanes per bank).  With an odd stride the 32 lanes of a half hit 32 different banks for every (j, i).
//   S > 64: a second pass of lanes over the same row (then hot in L2).  The wave's minimum of (dist << 7 | shift) is one u64 per row.
// k_place_topk: one workgroup; a thread keeps the eight best (dist << 32 | row) of its rows in registers, then k rounds of a workgroup-wide
//   minimum over the lists' heads.
#include <hip/hip_runtime.h>
#include <math.h>
#include "fdlibm_f32.h"
#include "place.h"

namespace vloam {

namespace {

constexpr int kPlaceMaxWp = (kPlaceMaxRing / 4) | 1;   // 9
constexpr int kPlaceDescGrid = 1024, kPlaceMatchGrid = 2048, kPlaceTopkThreads = 1024;
constexpr float kPiF = 3.14159274101257324f;   // 0x40490fdb

}  // namespace

// cells: [kPlaceMaxCells] maxima at [sector * R + ring], then n_used; zeroed before the launch
__global__ __launch_bounds__(256) void k_place_describe(PlaceGeom g, const float4* __restrict__ pts, int n, int* __restrict__ cells) {
  __shared__ int s_cell[kPlaceMaxCells];
  __shared__ int s_used;
  const int nc = g.R * g.S;
  for (int c = (int)threadIdx.x; c < nc; c += 256) s_cell[c] = 0;
  if (threadIdx.x == 0) s_used = 0;
  __syncthreads();
  int used = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float4 p = pts[i];
    if (!(fabsf(p.x) <= 3.402823466e+38f) || !(fabsf(p.y) <= 3.402823466e+38f) || !(fabsf(p.z) <= 3.402823466e+38f)) continue;
    const float r2 = __fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y));
    if (!(r2 >= g.min2 && r2 < g.max2)) continue;
    int ring = 0;
    for (int e = 1; e < g.R; e++) ring += r2 >= g.edge2[e] ? 1 : 0;
    const float a = fd_atan2f(p.y, p.x);
    const float fs = floorf(__fmul_rn(__fadd_rn(a, kPiF), g.k_sector));
    const int sector = fs >= (float)(g.S - 1) ? g.S - 1 : (fs <= 0.f ? 0 : (int)fs);
    // the clamps taken in f32, before the conversion: where (int)floorf(...) is defined this is min(254, max(0, .))
    const float fz = floorf(__fdiv_rn(__fsub_rn(p.z, g.z_min), g.z_step));
    const int q = (fz >= 254.f ? 254 : (fz <= 0.f ? 0 : (int)fz)) + 1;
    atomicMax(&s_cell[sector * g.R + ring], q);
    used++;
  }
  if (used) atomicAdd(&s_used, used);
  __syncthreads();
  for (int c = (int)threadIdx.x; c < nc; c += 256) {
    const int v = s_cell[c];
    if (v) atomicMax(&cells[c], v);
  }
  if (threadIdx.x == 0 && s_used) atomicAdd(&cells[kPlaceMaxCells], s_used);
}

// one workgroup: desc[sector * W + ring / 4], byte ring % 4; info2 = n_used, n_occupied; the row's tag when it is an append
__global__ __launch_bounds__(256) void k_place_pack(int R, int S, int W, const int* __restrict__ cells, unsigned* __restrict__ desc, int* __restrict__ info2,
                                                    int* __restrict__ tag_out, int tag) {
  __shared__ int s_occ;
  if (threadIdx.x == 0) s_occ = 0;
  __syncthreads();
  int occ = 0;
  for (int t = (int)threadIdx.x; t < S * W; t += 256) {
    const int j = t / W, wi = t - j * W;
    unsigned word = 0u;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int ring = wi * 4 + b;
      const int v = ring < R ? cells[j * R + ring] : 0;
      word |= (unsigned)v << (8 * b);
      occ += v != 0 ? 1 : 0;
    }
    desc[t] = word;
  }
  if (occ) atomicAdd(&s_occ, occ);
  __syncthreads();
  if (threadIdx.x == 0) {
    info2[0] = cells[kPlaceMaxCells]; info2[1] = s_occ;
    if (tag_out) *tag_out = tag;
  }
}

// best[row] = (dist << 32) | shift of the smallest (dist, shift) of row `row`, rows 0 .. rows - 1
__global__ __launch_bounds__(256) void k_place_match(int S, int W, int Wp, const unsigned* __restrict__ q, const unsigned* __restrict__ db, int rows,
                                                     unsigned long long* __restrict__ best) {
  __shared__ unsigned s_q[2 * kPlaceMaxSector * kPlaceMaxWp];
  for (int t = (int)threadIdx.x; t < 2 * S * W; t += 256) {
    const int j2 = t / W, i = t - j2 * W;
    s_q[j2 * Wp + i] = q[(j2 >= S ? j2 - S : j2) * W + i];
  }
  __syncthreads();
  const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int SW = S * W;
  for (int row = (int)blockIdx.x * 4 + wave; row < rows; row += (int)gridDim.x * 4) {   // wave-uniform
    const unsigned* rp = db + (size_t)row * (size_t)SW;
    unsigned key = 0xffffffffu;
    for (int s0 = 0; s0 < S; s0 += 64) {
      const int s = s0 + lane;
      const bool live = s < S;
      const unsigned* ql = s_q + (live ? s : 0) * Wp;   // (an idle lane reads shift 0's words: in bounds, its sum is dropped)
      unsigned acc = 0u;
      int j = 0, i = 0;
      for (int base = 0; base < SW; base += 64) {
        const unsigned mine = base + lane < SW ? rp[base + lane] : 0u;
        const int cnt = SW - base < 64 ? SW - base : 64;
        for (int k = 0; k < cnt; k++) {
          const unsigned d = (unsigned)__builtin_amdgcn_readlane((int)mine, k);
          acc = __builtin_amdgcn_sad_u8(ql[j * Wp + i], d, acc);
          if (++i == W) { i = 0; j++; }
        }
      }
      const unsigned cand = live ? ((acc << 7) | (unsigned)s) : 0xffffffffu;   // dist <= 255 * 3840 < 2^20, shift < 2^7
      key = cand < key ? cand : key;
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
      const unsigned o = (unsigned)__shfl_xor((int)key, sh);
      key = o < key ? o : key;
    }
    if (lane == 0) best[row] = ((unsigned long long)(key >> 7) << 32) | (unsigned long long)(key & 127u);
  }
}

// the k first rows of 0 .. limit - 1 by (dist, row); out[r] for r < k, unused places row == -1 and the rest zero
__global__ __launch_bounds__(kPlaceTopkThreads) void k_place_topk(const unsigned long long* __restrict__ best, const int* __restrict__ tags,
                                                                  const int* __restrict__ info, const int* __restrict__ qinfo, int limit, int k,
                                                                  vloam_place_match* __restrict__ out) {
  constexpr unsigned long long kNone = ~0ull;
  __shared__ unsigned long long s_min[kPlaceTopkThreads / 64];
  __shared__ unsigned long long s_win;
  unsigned long long L[kPlaceMaxK];
#pragma unroll
  for (int t = 0; t < kPlaceMaxK; t++) L[t] = kNone;
  for (int row = (int)threadIdx.x; row < limit; row += kPlaceTopkThreads) {
    unsigned long long x = (best[row] & 0xffffffff00000000ull) | (unsigned long long)(unsigned)row;
    if (x < L[kPlaceMaxK - 1]) {
#pragma unroll
      for (int t = 0; t < kPlaceMaxK; t++)
        if (x < L[t]) { const unsigned long long y = L[t]; L[t] = x; x = y; }
    }
  }
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int r = 0; r < k; r++) {
    unsigned long long c = L[0];
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
      const unsigned long long o = __shfl_xor(c, sh);
      c = o < c ? o : c;
    }
    if (lane == 0) s_min[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long m = s_min[0];
      for (int w = 1; w < kPlaceTopkThreads / 64; w++) m = s_min[w] < m ? s_min[w] : m;
      s_win = m;
      vloam_place_match rec;
      rec.row = -1; rec.tag = 0; rec.shift = 0; rec.dist = 0; rec.n_occupied_query = 0; rec.n_occupied_row = 0; rec.pad[0] = 0; rec.pad[1] = 0;
      if (m != kNone) {
        const int row = (int)(unsigned)(m & 0xffffffffull);
        rec.row = row; rec.tag = tags[row]; rec.shift = (int)(unsigned)(best[row] & 0xffffffffull); rec.dist = (int)(unsigned)(m >> 32);
        rec.n_occupied_query = qinfo[1]; rec.n_occupied_row = info[2 * row + 1];
      }
      out[r] = rec;
    }
    __syncthreads();
    const unsigned long long w = s_win;
    if (w != kNone && L[0] == w) {   // keys are unique (the row is part of them): one thread advances
#pragma unroll
      for (int t = 0; t + 1 < kPlaceMaxK; t++) L[t] = L[t + 1];
      L[kPlaceMaxK - 1] = kNone;
    }
  }
}

vloam_status place_describe_enqueue(PlaceContext* p, hipStream_t st, const void* d_pts, int n, void* d_desc, void* d_info, int* d_tag, int tag) {
  if (hipMemsetAsync(p->cells, 0, (kPlaceMaxCells + 1) * sizeof(int), st) != hipSuccess) return VLOAM_ERR_HIP;
  if (n > 0) {
    const int blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_place_describe, dim3((unsigned)(blocks < kPlaceDescGrid ? blocks : kPlaceDescGrid)), dim3(256), 0, st, p->g, (const float4*)d_pts, n, p->cells);
  }
  hipLaunchKernelGGL(k_place_pack, dim3(1), dim3(256), 0, st, p->g.R, p->g.S, p->g.W, (const int*)p->cells, (unsigned*)d_desc, (int*)d_info, d_tag, tag);
  return hipGetLastError() == hipSuccess ? VLOAM_OK : VLOAM_ERR_HIP;
}

vloam_status place_match_enqueue(PlaceContext* p, hipStream_t st, const void* d_qdesc, const void* d_qinfo, int limit, int k, void* d_out) {
  if (limit > 0) {
    const int blocks = (limit + 3) / 4;
    hipLaunchKernelGGL(k_place_match, dim3((unsigned)(blocks < kPlaceMatchGrid ? blocks : kPlaceMatchGrid)), dim3(256), 0, st, p->g.S, p->g.W, p->g.W | 1,
                       (const unsigned*)d_qdesc, (const unsigned*)p->db, limit, p->best);
  }
  hipLaunchKernelGGL(k_place_topk, dim3(1), dim3(kPlaceTopkThreads), 0, st, (const unsigned long long*)p->best, (const int*)p->tags, (const int*)p->info,
                     (const int*)d_qinfo, limit > 0 ? limit : 0, k, (vloam_place_match*)d_out);
  return hipGetLastError() == hipSuccess ? VLOAM_OK : VLOAM_ERR_HIP;
}

}  // namespace vloam
