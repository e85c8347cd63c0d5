// laserMapping on gfx950, the output paths: what a caller reads of the map and of a sweep's clouds.  Nothing here is on the mapping chain
// (map_kernels.hip) that sets the sweep period.
//   k_map_register  grid      the sweep's full-resolution cloud in the map frame (LM:795-799): vloam_get_features(h, 11) and the published cloud
//   k_map_export    grid      /laser_cloud_map (LM:778-793) for vloam_get_map / vloam_get_map_kind
//   k_map_pub_*     grid      the same cloud ordered on the device, published behind a sweep's mapping (vloam_limits::map_pub_number)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include "map_kernels.h"
#include "map_table.h"
#include "map_device.h"
#include "bitonic.h"

namespace vloam {

__global__ void k_map_register(const float4* __restrict__ cloud, const FrameScalars* __restrict__ S, const MapState* __restrict__ ms,
                               float4* __restrict__ out) {
  const int n = S->N2;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = associate_to_map(cloud[i], ms->parameters, ms->parameters + 4);  // LM:795-799
}

// ---------------------------------------------------------------------------------------------- map export
// /laser_cloud_map (LM:778-793): for cube index 0..4850 the corner cloud then the surf cloud of the cube.  A cube cloud that has been
// through its VoxelGrid re-filter (every cube that was ever valid) is ordered by voxel (iz, iy, ix); points that arrived while the cube
// was outside the valid block follow un-merged, in arrival order (sweep, then stack order) — the raw point records of k_map_finalize; a
// centroid that became raw point number one (stamp 0) keeps its place in the voxel-ordered part.  The device compacts the live records
// with their order key; the final ordering of this OUTPUT path is a host sort of the compacted list.

// Is the record at a table slot a point of /laser_cloud_map (the window's centre cube at cW, cH, cD), and then its order key and the point:
// the export's and the publication's one rule
__device__ __forceinline__ bool pub_row(const RecVal& v, int cW, int cH, int cD, int kind, u64* okey, float4* p) {
  if (!rec_live(v)) return false;
  if (key_seq(v.key) == 0 && rec_raw(v.count)) return false;   // a raw voxel is published through its point records
  int Ai, Aj, Ak;
  unpack_cube(v.key, &Ai, &Aj, &Ak);
  const int i = Ai + cW, j = Aj + cH, k = Ak + cD;
  if (i < 0 || i >= kCubeW || j < 0 || j >= kCubeH || k < 0 || k >= kCubeD) return false;
  *okey = rec_order_key(v, i + kCubeW * j + kCubeW * kCubeH * k, kind);
  *p = rec_point(v);
  return true;
}

struct ExportRow { u64 okey; float x, y, z, w; };
__global__ __launch_bounds__(256) void k_map_export(VoxelTable T, const MapState* __restrict__ ms, int kind, ExportRow* __restrict__ out, long long cap,
                                                    unsigned long long* n_out) {
  const int cW = ms->cenW, cH = ms->cenH, cD = ms->cenD;
  for (unsigned s = blockIdx.x * 256 + threadIdx.x; s <= T.mask; s += gridDim.x * 256) {
    u64 okey; float4 p;
    if (!pub_row(rec_load(&T.rec[s]), cW, cH, cD, kind, &okey, &p)) continue;
    const unsigned long long o = atomicAdd(n_out, 1ull);
    if ((long long)o < cap) out[o] = ExportRow{okey, p.x, p.y, p.z, p.w};
  }
}

// kinds: bit 0 the corner clouds, bit 1 the surf clouds
static vloam_status map_export_kinds(MapContext* m0, hipStream_t st, int kinds, float* xyzi4, long long cap, long long* n) {
  const MapContext msel = m0->for_session(m0->sel);
  const MapContext* m = &msel;
  if (hipStreamSynchronize(st) != hipSuccess) return VLOAM_ERR_HIP;
  int stats[2][4];
  for (int k = 0; k < 2; k++) if (hipMemcpy(stats[k], m->tab[k].stats, sizeof(stats[k]), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
  const long long bound = (long long)stats[0][0] + stats[1][0] + 1;  // keys ever inserted >= live voxels
  ExportRow* d_rows = nullptr;
  unsigned long long* d_n = nullptr;
  if (hipMalloc((void**)&d_rows, (size_t)bound * sizeof(ExportRow)) != hipSuccess || hipMalloc((void**)&d_n, sizeof(*d_n)) != hipSuccess) return VLOAM_ERR_HIP;
  vloam_status rc = VLOAM_OK;
  unsigned long long cnt = 0;
  if (hipMemsetAsync(d_n, 0, sizeof(*d_n), st) != hipSuccess) rc = VLOAM_ERR_HIP;
  for (int k = 0; k < 2 && rc == VLOAM_OK; k++) if ((kinds >> k) & 1) VL_RAW_LAUNCH(k_map_export, dim3(1024), dim3(256), 0, st, m->tab[k], m->state, k, d_rows, bound, d_n);
  if (rc == VLOAM_OK && (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(&cnt, d_n, sizeof(cnt), hipMemcpyDeviceToHost) != hipSuccess)) rc = VLOAM_ERR_HIP;
  std::vector<ExportRow> rows((size_t)((long long)cnt < bound ? (long long)cnt : bound));
  if (rc == VLOAM_OK && !rows.empty() && hipMemcpy(rows.data(), d_rows, rows.size() * sizeof(ExportRow), hipMemcpyDeviceToHost) != hipSuccess) rc = VLOAM_ERR_HIP;
  (void)hipFree(d_rows); (void)hipFree(d_n);
  if (rc != VLOAM_OK) return rc;
  std::sort(rows.begin(), rows.end(), [](const ExportRow& a, const ExportRow& b) { return a.okey < b.okey; });
  if (n) *n = (long long)rows.size();
  const long long c = (long long)rows.size() < cap ? (long long)rows.size() : cap;
  for (long long i = 0; xyzi4 && i < c; i++) { xyzi4[4 * i] = rows[(size_t)i].x; xyzi4[4 * i + 1] = rows[(size_t)i].y; xyzi4[4 * i + 2] = rows[(size_t)i].z; xyzi4[4 * i + 3] = rows[(size_t)i].w; }
  return VLOAM_OK;
}

vloam_status map_export(MapContext* m, hipStream_t st, float* xyzi4, long long cap, long long* n) { return map_export_kinds(m, st, 3, xyzi4, cap, n); }
vloam_status map_export_kind(MapContext* m, hipStream_t st, int kind, float* xyzi4, long long cap, long long* n) { return map_export_kinds(m, st, 1 << kind, xyzi4, cap, n); }

vloam_status map_get_cloud(MapContext* m0, hipStream_t st, int which, const SRBuffers& cur, float* xyzi4, int cap, int* n) {
  // `cur` is already the selected session's buffer set (the caller rebased it)
  const MapContext msel = m0->for_session(m0->sel);
  const MapContext* m = &msel;
  if (hipStreamSynchronize(st) != hipSuccess) return VLOAM_ERR_HIP;
  MapState ms;
  if (hipMemcpy(&ms, m->state, sizeof(ms), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
  const float4* src = nullptr;
  int cnt = 0;
  if (which == 7) { src = m->stack[0]; cnt = ms.n_corner_stack; }
  else if (which == 8) { src = m->stack[1]; cnt = ms.n_surf_stack; }
  else if (which == 11) {
    FrameScalars S;
    if (hipMemcpy(&S, cur.S, sizeof(S), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
    VL_RAW_LAUNCH(k_map_register, dim3(256), dim3(256), 0, st, cur.cloud, cur.S, m->state, m->registered);
    if (hipStreamSynchronize(st) != hipSuccess) return VLOAM_ERR_HIP;
    src = m->registered; cnt = S.N2;
  } else return VLOAM_ERR_INVALID;
  *n = cnt;
  const int c = cnt < cap ? cnt : cap;
  if (xyzi4 && c > 0 && hipMemcpy(xyzi4, src, (size_t)c * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
  return VLOAM_OK;
}

// ---------------------------------------------------------------------------------------------- published clouds (MapPub, map_kernels.h)
// /laser_cloud_map ordered on the device, on the mapping stream, behind k_map_finalize of the publishing sweep.  The order key is
// k_map_export's (pub_row; rec_order_key of map_table.h); its top 14 bits, cube and kind, name the bucket.
//   k_map_pub_count    both tables: live records per bucket
//   k_map_pub_scan     exclusive scan of the 9 702 counts, the publication's header (count, overflow), cursors cleared
//   k_map_pub_scatter  both tables again: every record into its bucket's segment (place inside the segment: arrival, fixed up next)
//   k_map_pub_sort     one workgroup per bucket: segments of up to kPubLdsKeys records ordered in LDS (bitonic.h), points written out
//   k_map_pub_rank     the longer segments: a record's place is the number of smaller keys in its segment
// Keys are unique (one record per cube, kind and voxel, one per arrival stamp), so the result is the host sort's of map_export, byte for byte.
// A publication that does not fit the capacity writes the header only.
__device__ __forceinline__ int pub_bucket(u64 okey) { return (int)(okey >> 49); }   // cube * 2 + kind < kPubBuckets

__global__ __launch_bounds__(256) void k_map_pub_count(VoxelTable T0, VoxelTable T1, const MapState* __restrict__ ms, int* __restrict__ cnt, size_t ss) {
  VL_SESSION(ss); T0.rebase(so_); T1.rebase(so_); RB(ms); RB(cnt);
  const int kind = blockIdx.y;
  const VoxelTable& T = kind ? T1 : T0;
  const int cW = ms->cenW, cH = ms->cenH, cD = ms->cenD;
  for (unsigned s = blockIdx.x * 256 + threadIdx.x; s <= T.mask; s += gridDim.x * 256) {
    const RecVal v = rec_load(&T.rec[s]);
    u64 okey; float4 p;
    if (pub_row(v, cW, cH, cD, kind, &okey, &p)) atomicAdd(&cnt[pub_bucket(okey)], 1);
  }
}

constexpr int kPubScanPer = (kPubBuckets + 255) / 256;   // buckets per thread of the one-workgroup scan
__global__ __launch_bounds__(256) void k_map_pub_scan(const int* __restrict__ cnt, int* __restrict__ off, int* __restrict__ cur, PubHeader* __restrict__ hdr,
                                                      long long cap, size_t ss) {
  VL_SESSION(ss); RB(cnt); RB(off); RB(cur); RB(hdr);
  __shared__ int part[256];
  const int tid = threadIdx.x, b0 = tid * kPubScanPer;
  int sum = 0;
  for (int e = 0; e < kPubScanPer; e++) if (b0 + e < kPubBuckets) sum += cnt[b0 + e];
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {   // inclusive scan of the 256 partial sums
    const int add = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  int run = part[tid] - sum;
  for (int e = 0; e < kPubScanPer; e++)
    if (b0 + e < kPubBuckets) { off[b0 + e] = run; cur[b0 + e] = 0; run += cnt[b0 + e]; }
  if (tid == 255) {
    const int total = part[255];
    off[kPubBuckets] = total;
    hdr->n = (long long)total;
    hdr->overflow = (long long)total > cap ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void k_map_pub_scatter(VoxelTable T0, VoxelTable T1, const MapState* __restrict__ ms, const int* __restrict__ off,
                                                         int* __restrict__ cur, const PubHeader* __restrict__ hdr, u64* __restrict__ keys,
                                                         float4* __restrict__ vals, long long cap, size_t ss) {
  VL_SESSION(ss); T0.rebase(so_); T1.rebase(so_); RB(ms); RB(off); RB(cur); RB(hdr); RB(keys); RB(vals);
  if (hdr->overflow) return;
  const int kind = blockIdx.y;
  const VoxelTable& T = kind ? T1 : T0;
  const int cW = ms->cenW, cH = ms->cenH, cD = ms->cenD;
  for (unsigned s = blockIdx.x * 256 + threadIdx.x; s <= T.mask; s += gridDim.x * 256) {
    const RecVal v = rec_load(&T.rec[s]);
    u64 okey; float4 p;
    if (!pub_row(v, cW, cH, cD, kind, &okey, &p)) continue;
    const int b = pub_bucket(okey);
    const long long pos = (long long)off[b] + atomicAdd(&cur[b], 1);
    if (pos < cap) { keys[pos] = okey; vals[pos] = p; }   // (always: the tables have not changed since the count)
  }
}

constexpr int kPubIdxBits = 13;   // a record's index inside its segment rides in the low bits of the LDS sort key
static_assert(kPubLdsKeys <= (1 << kPubIdxBits) && 49 + kPubIdxBits <= 63, "key below the bucket bits + index must fit 64 bits under the padding value");
__global__ __launch_bounds__(256) void k_map_pub_sort(int* __restrict__ cnt, const int* __restrict__ off, const PubHeader* __restrict__ hdr,
                                                      const u64* __restrict__ keys, const float4* __restrict__ vals, float4* __restrict__ out, long long cap,
                                                      size_t ss) {
  VL_SESSION(ss); RB(cnt); RB(off); RB(hdr); RB(keys); RB(vals); RB(out);
  __shared__ u64 a[kPubLdsKeys];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = cnt[b], base = off[b];
  const bool skip = hdr->overflow != 0;
  __syncthreads();
  if (tid == 0) cnt[b] = 0;   // ready for the next publication
  if (skip || n == 0 || n > kPubLdsKeys || (long long)base + n > cap) return;   // longer segments: k_map_pub_rank
  if (n == 1) { if (tid == 0) out[base] = vals[base]; return; }
  int P2 = 256;
  while (P2 < n) P2 <<= 1;
  for (int e = tid; e < P2; e += 256)
    a[e] = e < n ? (((keys[base + e] & ((1ull << 49) - 1)) << kPubIdxBits) | (u64)e) : ~0ull;
  __syncthreads();
  block_bitonic_sort_u64(a, P2, tid, 256);
  for (int e = tid; e < n; e += 256) out[base + e] = vals[base + (int)(a[e] & ((1u << kPubIdxBits) - 1))];
}

__global__ __launch_bounds__(256) void k_map_pub_rank(const int* __restrict__ off, const PubHeader* __restrict__ hdr, const u64* __restrict__ keys,
                                                      const float4* __restrict__ vals, float4* __restrict__ out, long long cap, size_t ss) {
  VL_SESSION(ss); RB(off); RB(hdr); RB(keys); RB(vals); RB(out);
  if (hdr->overflow) return;
  const long long total = hdr->n < cap ? hdr->n : cap;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const u64 key = keys[i];
    const int b = pub_bucket(key);
    const int lo = off[b], hi = off[b + 1];
    if (hi - lo <= kPubLdsKeys) continue;   // k_map_pub_sort wrote it
    int r = 0;
    for (int j = lo; j < hi; j++) r += keys[j] < key ? 1 : 0;
    out[lo + r] = vals[i];
  }
}

bool map_publishes(const MapContext* m, bool skip_frame) {
  const MapPub& P = m->pub;
  if (P.cloud_on) return true;
  // LM:778 with frameCount == MapState::sweep_no after this sweep's increment; a skipped sweep leaves the last publication current
  return P.pub_number > 0 && !skip_frame && P.due(P.mapped + 1);
}

vloam_status map_publish_enqueue(MapContext* m, hipStream_t st, const float4* cloud, const FrameScalars* S, int frame, bool skip_frame, ProfHook* ph,
                                 hipEvent_t done) {
  MapPub& P = m->pub;
  const unsigned Z = (unsigned)m->se.B;
  const size_t ss = m->se.ss;
  if (P.cloud_on) {
    const int slot = P.cloud_seq & 1;
    for (int b = 0; b < m->se.B; b++) {   // k_map_register as vloam_get_features(h, 11) launches it, once per session
      const size_t o = (size_t)b * ss;
      const float4* c = cloud; const FrameScalars* Sb = S; const MapState* msb = m->state; float4* dst = P.cloud[slot]; int* nb = P.cloud_n[slot];
      rbp(c, o); rbp(Sb, o); rbp(msb, o); rbp(dst, o); rbp(nb, o);
      VLOAM_LAUNCH(ph, kKMapRegister, st, k_map_register, dim3(256), dim3(256), 0, st, c, Sb, msb, dst);
      if (hipMemcpyAsync(nb, &Sb->N2, sizeof(int), hipMemcpyDeviceToDevice, st) != hipSuccess) return VLOAM_ERR_HIP;
    }
    if (hipEventRecord(P.ev_cloud[slot], st) != hipSuccess) return VLOAM_ERR_HIP;
    P.cloud_frame[slot] = frame;
    P.cloud_seq++;
  }
  if (done && hipEventRecord(done, st) != hipSuccess) return VLOAM_ERR_HIP;   // the sweep's buffer set is free once k_map_register has read it
  if (P.pub_number > 0 && !skip_frame && P.due(P.mapped)) {   // (map_enqueue has counted the sweep)
    const int slot = P.map_seq & 1;
    VLOAM_LAUNCH(ph, kKMapPubCount, st, k_map_pub_count, dim3(1024, 2, Z), dim3(256), 0, st, m->tab[0], m->tab[1], m->state, P.cnt, ss);
    VLOAM_LAUNCH(ph, kKMapPubScan, st, k_map_pub_scan, dim3(1, 1, Z), dim3(256), 0, st, P.cnt, P.off, P.cur, P.hdr[slot], P.cap, ss);
    VLOAM_LAUNCH(ph, kKMapPubScatter, st, k_map_pub_scatter, dim3(1024, 2, Z), dim3(256), 0, st, m->tab[0], m->tab[1], m->state, P.off, P.cur, P.hdr[slot],
                 P.keys, P.vals, P.cap, ss);
    VLOAM_LAUNCH(ph, kKMapPubSort, st, k_map_pub_sort, dim3(kPubBuckets, 1, Z), dim3(256), 0, st, P.cnt, P.off, P.hdr[slot], P.keys, P.vals, P.out[slot], P.cap, ss);
    VLOAM_LAUNCH(ph, kKMapPubRank, st, k_map_pub_rank, dim3(1024, 1, Z), dim3(256), 0, st, P.off, P.hdr[slot], P.keys, P.vals, P.out[slot], P.cap, ss);
    if (hipEventRecord(P.ev_map[slot], st) != hipSuccess) return VLOAM_ERR_HIP;
    P.map_frame[slot] = frame;
    P.map_seq++;
  }
  return hipGetLastError() == hipSuccess ? VLOAM_OK : VLOAM_ERR_HIP;
}

vloam_status map_published_get(MapContext* m0, int which, float* xyzi4, long long cap, long long* n, int* frame, void** d_ptr) {
  const MapContext msel = m0->for_session(m0->sel);
  const MapPub& P = msel.pub;
  const int seq = which == 0 ? P.map_seq : P.cloud_seq;
  *n = 0; *frame = -1;
  if (d_ptr) *d_ptr = nullptr;
  if (seq == 0) return VLOAM_OK;   // nothing published yet
  const int slot = (seq - 1) & 1;
  if (hipEventSynchronize(which == 0 ? P.ev_map[slot] : P.ev_cloud[slot]) != hipSuccess) return VLOAM_ERR_HIP;
  *frame = which == 0 ? P.map_frame[slot] : P.cloud_frame[slot];
  const float4* src = nullptr;
  if (which == 0) {
    PubHeader hd;
    if (hipMemcpy(&hd, P.hdr[slot], sizeof(hd), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
    *n = hd.n;
    if (hd.overflow) return VLOAM_ERR_CAPACITY;
    src = P.out[slot];
  } else {
    int cnt = 0;
    if (hipMemcpy(&cnt, P.cloud_n[slot], sizeof(cnt), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
    *n = cnt;
    src = P.cloud[slot];
  }
  if (d_ptr) *d_ptr = (void*)src;
  const long long c = *n < cap ? *n : cap;
  if (xyzi4 && c > 0 && hipMemcpy(xyzi4, src, (size_t)c * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
  return VLOAM_OK;
}

}  // namespace vloam
