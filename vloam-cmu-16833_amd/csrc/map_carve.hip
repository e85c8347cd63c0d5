// Map clean-up (vloam_map_carve): voxels that later sweeps see through leave the map.  A translation unit (and code object) of its own: the
// kernels every handle launches are not touched by it, and a handle that never carves allocates and launches nothing of this.
//   k_carve_image  grid  one launch per sweep: every point that projects leaves the minimum of its quantised range in its pixel (atomicMin)
//   k_carve_map    grid  one launch per selected table, the slot walk of map_purge: a live seq-0 record that is not a raw voxel is projected
//                        into every sweep's image and collects its votes in registers; the removed points and their slots go to a list
//   k_carve_apply  grid  (apply only) the listed records become tombstones, stats[1] and cube_cnt follow; the host then enqueues the table's
//                        same-size reclamation (map_reclaim_enqueue), which leaves no trace of them in the table or the occupancy blocks
// The projection is stated once (carve_project) for both the sweeps' points and the map's; c_api.h and DESIGN.md §8 give it in words,
// tests/carve_model.py in NumPy.  Everything behind it is integer: counters and the removed set are a function of the inputs alone.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <algorithm>
#include "map_kernels.h"
#include "map_table.h"
#include "map_move_dev.h"   // (map_move_grid only)
#include "fdlibm_f32.h"

namespace vloam {

constexpr unsigned kCarveEmpty = 0xffffffffu;

struct CarvePix { int row, col; unsigned q; };
__device__ __forceinline__ bool carve_finite(float v) { return fabsf(v) <= FLT_MAX; }
// f32, every operation rounded on its own (the file is built with -ffp-contract=off)
__device__ __forceinline__ bool carve_project(const CarveGeom& G, float x, float y, float z, CarvePix* o) {
  if (!(carve_finite(x) && carve_finite(y) && carve_finite(z))) return false;
  const float h2 = x * x + y * y;
  const float r = sqrtf(h2 + z * z);
  if (!(r >= G.min_range && r <= G.max_range)) return false;
  const float el = fd_atanf(z / sqrtf(h2));
  const float rf = (el - G.elev_min) * G.row_scale;
  if (!(rf >= 0.0f && rf < (float)G.rows)) return false;
  const float az = fd_atan2f(y, x);
  const float cf = (az + fd_from_bits(0x40490fdbu)) * G.col_scale;
  int col = (int)floorf(cf);
  if (col >= G.cols) col -= G.cols;   // azimuth +pi
  o->row = (int)floorf(rf);
  o->col = min(max(col, 0), G.cols - 1);
  o->q = (unsigned)floorf(r / G.range_res);
  return true;
}

__global__ __launch_bounds__(256) void k_carve_image(const float4* __restrict__ pts, int n, unsigned* __restrict__ img, CarveGeom G) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float4 p = pts[i];
    CarvePix px;
    if (carve_project(G, p.x, p.y, p.z, &px)) atomicMin(&img[(size_t)px.row * G.cols + px.col], px.q);
  }
}

__global__ __launch_bounds__(256) void k_carve_map(VoxelTable T, const MapState* __restrict__ ms, int kind, CarveGeom G, const CarvePose* __restrict__ poses,
                                                   const unsigned* __restrict__ imgs, CarveCounters* C, float4* __restrict__ removed,
                                                   unsigned* __restrict__ slots, unsigned long long cap) {
  __shared__ unsigned s_cnt[kCarveCounters];
  if (threadIdx.x < kCarveCounters) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  const int cW = ms->cenW, cH = ms->cenH, cD = ms->cenD;
  const size_t pixels = (size_t)G.rows * G.cols;
  unsigned c[kCarveCounters] = {0u, 0u, 0u, 0u, 0u, 0u};
  for (unsigned s = blockIdx.x * 256 + threadIdx.x; s <= T.mask; s += gridDim.x * 256) {
    const RecVal v = rec_load(&T.rec[s]);
    if (!rec_live(v) || key_seq(v.key) != 0) continue;
    int Ai, Aj, Ak;
    unpack_cube(v.key, &Ai, &Aj, &Ak);
    const int i = Ai + cW, j = Aj + cH, kk = Ak + cD;
    if (i < 0 || i >= kCubeW || j < 0 || j >= kCubeH || kk < 0 || kk >= kCubeD) continue;
    if (rec_raw(v.count)) { c[5]++; continue; }
    c[0]++;
    const float4 p = rec_point(v);
    int n_view = 0, n_through = 0, n_confirm = 0;
    for (int sw = 0; sw < G.n_sweeps; sw++) {
      const CarvePose& P = poses[sw];
      const double d0 = (double)p.x - P.t[0], d1 = (double)p.y - P.t[1], d2 = (double)p.z - P.t[2];
      const float x = (float)((P.R[0] * d0 + P.R[3] * d1) + P.R[6] * d2);
      const float y = (float)((P.R[1] * d0 + P.R[4] * d1) + P.R[7] * d2);
      const float z = (float)((P.R[2] * d0 + P.R[5] * d1) + P.R[8] * d2);
      CarvePix px;
      if (!carve_project(G, x, y, z, &px)) continue;
      n_view++;
      const unsigned* img = imgs + (size_t)sw * pixels;
      const unsigned cen = img[(size_t)px.row * G.cols + px.col];
      if (cen == kCarveEmpty) continue;
      unsigned m = cen;
#pragma unroll
      for (int dr = -1; dr <= 1; dr++) {
        const int rr = min(max(px.row + dr, 0), G.rows - 1);
#pragma unroll
        for (int dc = -1; dc <= 1; dc++) {
          int cc = px.col + dc;
          cc = cc < 0 ? cc + G.cols : (cc >= G.cols ? cc - G.cols : cc);
          m = min(m, img[(size_t)rr * G.cols + cc]);
        }
      }
      if (px.q + G.margin_q < m) n_through++;
      if ((px.q > cen ? px.q - cen : cen - px.q) <= G.margin_q) n_confirm++;
    }
    if (n_view) c[1]++;
    if (n_through) c[2]++;
    if (n_confirm) c[3]++;
    if (n_through >= G.min_votes && n_confirm == 0) {
      c[4]++;
      const unsigned long long pos = atomicAdd(&C->n_removed, 1ull);
      if (pos < cap) { removed[pos] = p; slots[pos] = s | ((unsigned)kind << 31); }
    }
  }
#pragma unroll
  for (int k = 0; k < kCarveCounters; k++) if (c[k]) atomicAdd(&s_cnt[k], c[k]);
  __syncthreads();
  if (threadIdx.x < kCarveCounters && s_cnt[threadIdx.x]) atomicAdd(&C->cnt[kind][threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// the listed records (slot | kind << 31) become tombstones, as map_purge leaves them; a list that overflowed is not applied at all
__global__ __launch_bounds__(256) void k_carve_apply(VoxelTable T0, VoxelTable T1, const MapState* __restrict__ ms, int* __restrict__ cube_cnt,
                                                     const unsigned* __restrict__ slots, const CarveCounters* __restrict__ C, unsigned long long cap) {
  const unsigned long long n = C->n_removed;
  if (n > cap) return;
  for (unsigned long long e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
    const unsigned w = slots[e];
    const int kind = (int)(w >> 31);
    const VoxelTable& T = kind ? T1 : T0;
    const unsigned s = w & 0x7fffffffu;
    if (s > T.mask) continue;
    const RecVal v = rec_load(&T.rec[s]);
    int Ai, Aj, Ak;
    unpack_cube(v.key, &Ai, &Aj, &Ak);
    const int wi = Ai + ms->cenW, wj = Aj + ms->cenH, wk = Ak + ms->cenD;
    rec_store_value(&T.rec[s], make_float4(0.f, 0.f, 0.f, 0.f), 0, 0);
    atomicAdd(&T.stats[1], 1);
    if (wi >= 0 && wi < kCubeW && wj >= 0 && wj < kCubeH && wk >= 0 && wk < kCubeD)
      atomicSub(&cube_cnt[kind * kCubeNum + wi + kCubeW * wj + kCubeW * kCubeH * wk], 1);   // a merged voxel is one point of its cube's cloud
  }
}

// ---------------------------------------------------------------------------------------------- host side
static inline size_t carve_pad(size_t b) { return (b + 255) & ~(size_t)255; }

void map_carve_free(MapContext* m) {
  if (!m->carve) return;
  if (m->carve->base) (void)hipFree(m->carve->base);
  delete m->carve;
  m->carve = nullptr;
}

vloam_status map_carve_run(MapContext* m0, int session, hipStream_t st, const CarveGeom& G, int kind_mask, const void* const* clouds, const int* n,
                           const CarvePose* poses, bool host_io, void* removed, long long cap, bool apply, CarveCounters* h_out) {
  MapContext ms_ = m0->for_session(session);
  MapContext* m = &ms_;
  // no more records can leave than the selected tables hold keys: the lists are sized by that, not by the caller's cap
  long long keys = 0;
  for (int k = 0; k < 2; k++) {
    if (!(kind_mask & (1 << k))) continue;
    int stats[4];
    if (hipMemcpy(stats, m->tab[k].stats, sizeof(stats), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
    keys += std::max(0, stats[0]);
  }
  const unsigned long long cap_eff = (unsigned long long)std::min(cap, keys);
  const size_t pixels = (size_t)G.rows * G.cols;
  size_t pts = 0;
  for (int s = 0; s < G.n_sweeps; s++) pts += (size_t)n[s];
  const size_t off_cnt = carve_pad(sizeof(CarvePose) * kCarveMaxSweeps), off_img = off_cnt + carve_pad(sizeof(CarveCounters)),
               off_slots = off_img + carve_pad(pixels * G.n_sweeps * sizeof(unsigned)), off_pts = off_slots + carve_pad((size_t)(cap_eff + 1) * sizeof(unsigned)),
               off_out = off_pts + carve_pad(host_io ? pts * sizeof(float4) : 0), total = off_out + carve_pad(host_io ? (size_t)(cap_eff + 1) * sizeof(float4) : 0);
  if (!m0->carve) m0->carve = new MapCarve;
  MapCarve& S = *m0->carve;
  if (S.bytes < total) {
    if (S.base) (void)hipFree(S.base);
    S.base = nullptr; S.bytes = 0;
    if (hipMalloc((void**)&S.base, total) != hipSuccess) { S.base = nullptr; return VLOAM_ERR_HIP; }
    S.bytes = total;
  }
  CarvePose* d_poses = (CarvePose*)S.base;
  CarveCounters* d_cnt = (CarveCounters*)(S.base + off_cnt);
  unsigned* d_img = (unsigned*)(S.base + off_img);
  unsigned* d_slots = (unsigned*)(S.base + off_slots);
  float4* d_pts = (float4*)(S.base + off_pts);
  float4* d_out = host_io ? (float4*)(S.base + off_out) : (float4*)removed;
  bool ok = hipMemcpyAsync(d_poses, poses, sizeof(CarvePose) * G.n_sweeps, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemsetAsync(d_cnt, 0, sizeof(CarveCounters), st) == hipSuccess &&
            hipMemsetAsync(d_img, 0xff, pixels * G.n_sweeps * sizeof(unsigned), st) == hipSuccess;
  size_t at = 0;
  for (int s = 0; s < G.n_sweeps && ok; s++) {
    if (n[s] == 0) continue;
    const float4* src = (const float4*)clouds[s];
    if (host_io) {
      ok = hipMemcpyAsync(d_pts + at, clouds[s], (size_t)n[s] * sizeof(float4), hipMemcpyHostToDevice, st) == hipSuccess;
      src = d_pts + at;
      at += (size_t)n[s];
    }
    if (ok) VL_RAW_LAUNCH(k_carve_image, dim3(map_move_grid((size_t)n[s])), dim3(256), 0, st, src, n[s], d_img + (size_t)s * pixels, G);
  }
  for (int k = 0; k < 2 && ok; k++)
    if (kind_mask & (1 << k))
      VL_RAW_LAUNCH(k_carve_map, dim3(map_move_grid(m->tab[k])), dim3(256), 0, st, m->tab[k], m->state, k, G, d_poses, d_img, d_cnt, d_out, d_slots, cap_eff);
  if (ok && apply && cap_eff > 0)
    VL_RAW_LAUNCH(k_carve_apply, dim3(map_move_grid((size_t)cap_eff)), dim3(256), 0, st, m->tab[0], m->tab[1], m->state, m->cube_cnt, d_slots, d_cnt, cap_eff);
  ok = ok && hipGetLastError() == hipSuccess && hipMemcpyAsync(h_out, d_cnt, sizeof(CarveCounters), hipMemcpyDeviceToHost, st) == hipSuccess;
  ok = hipStreamSynchronize(st) == hipSuccess && ok;
  if (!ok) return VLOAM_ERR_HIP;
  if (h_out->n_removed > (unsigned long long)cap) return VLOAM_OK;   // the caller reports the overflow; nothing was applied (cap_eff <= cap < n_removed)
  if (host_io && h_out->n_removed > 0 &&
      hipMemcpy(removed, d_out, (size_t)h_out->n_removed * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
  if (apply)
    for (int k = 0; k < 2; k++)
      if (h_out->cnt[k][4] > 0 && map_reclaim_enqueue(m0, st, k) != VLOAM_OK) return VLOAM_ERR_HIP;
  return VLOAM_OK;
}

}  // namespace vloam
