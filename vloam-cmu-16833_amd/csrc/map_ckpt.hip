// Checkpoint of the voxel map (vloam_checkpoint_save / _load): the live records of a table as a dense stream, and back into a table of any size.
// A translation unit (and code object) of its own, like map_grow.hip: nothing here is launched or allocated by a handle that is not saved or
// loaded.  Both directions run with nothing of the handle in flight, on one stream.
//   k_map_ckpt_count   grid      live records per workgroup (a workgroup owns a contiguous range of slots)
//   k_map_ckpt_scan    1 WG      exclusive scan of the workgroup counts of both tables: one offset per workgroup, the surf stream behind the corner stream
//   k_map_ckpt_pack    grid      table -> stream: a ballot prefix per wavefront on top of the workgroup's offset.  No atomics: the same-address
//                                atomic per record is what k_map_pub_count / _scatter and k_map_grow cost.  Stream order = slot order.
//   k_map_ckpt_begin   1 thread  the table's counters and the raw-voxel list start over
//   k_map_ckpt_unpack  grid      stream -> table: what k_map_grow does with a record of the old table (the movers' one text: map_move_dev.h)
#include <hip/hip_runtime.h>
#include "map_kernels.h"
#include "map_move_dev.h"

namespace vloam {

__global__ __launch_bounds__(256) void k_map_ckpt_count(VoxelTable T, int* __restrict__ cnt) {
  __shared__ int s_w[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned span = (T.mask + 1) / gridDim.x, begin = blockIdx.x * span;   // slots and grid are powers of two, span >= 256
  int c = 0;
  for (unsigned s0 = begin; s0 < begin + span; s0 += 256) c += __popcll(__ballot(rec_live(rec_load(&T.rec[s0 + threadIdx.x]))));
  if (lane == 0) s_w[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// off[k][b]: first stream position of workgroup b of table k; total[k]: records of table k
__global__ __launch_bounds__(256) void k_map_ckpt_scan(const int* __restrict__ cnt, int n0, int n1, long long* __restrict__ off, long long* __restrict__ total) {
  __shared__ long long s_sum[256];
  long long base = 0;
  for (int k = 0; k < 2; k++) {
    const int n = k ? n1 : n0;
    const int* c = cnt + k * kMoveMaxGrid;
    long long* o = off + k * kMoveMaxGrid;
    const int per = (n + 255) / 256, b0 = threadIdx.x * per;
    long long mine = 0;
    for (int i = b0; i < b0 + per && i < n; i++) mine += c[i];
    s_sum[threadIdx.x] = mine;
    __syncthreads();
    long long before = base, all = 0;
    for (int t = 0; t < 256; t++) { const long long v = s_sum[t]; if (t < (int)threadIdx.x) before += v; all += v; }
    for (int i = b0; i < b0 + per && i < n; i++) { o[i] = before; before += c[i]; }
    if (threadIdx.x == 0) total[k] = all;
    base += all;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_map_ckpt_pack(VoxelTable T, const long long* __restrict__ off, VoxelRec* __restrict__ out, long long cap) {
  __shared__ int s_w[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned span = (T.mask + 1) / gridDim.x, begin = blockIdx.x * span;
  long long base = off[blockIdx.x];
  for (unsigned s0 = begin; s0 < begin + span; s0 += 256) {
    const RecVal v = rec_load(&T.rec[s0 + threadIdx.x]);
    const bool live = rec_live(v);
    const u64 m = __ballot(live);
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 4; w++) { const int c = s_w[w]; if (w < wave) before += c; all += c; }
    const long long pos = base + before + __popcll(m & ((1ull << lane) - 1ull));
    if (live && pos < cap) rec_store_all(&out[pos], v);   // (pos < cap whenever the table is what k_map_ckpt_count saw: nothing of the handle is in flight)
    base += all;
    __syncthreads();
  }
}

__global__ void k_map_ckpt_begin(VoxelTable Tn, MapFrame* fr, int kind) {
  if (threadIdx.x == 0) map_move_begin(Tn, fr, kind);
}
__global__ __launch_bounds__(256) void k_map_ckpt_unpack(const VoxelRec* __restrict__ in, long long n, VoxelTable Tn, MapFrame* fr, int kind,
                                                         int* __restrict__ deferred, int deferred_cap) {
  for (long long i0 = (long long)blockIdx.x * 256 + (threadIdx.x & ~63u); i0 < n; i0 += (long long)gridDim.x * 256) {   // wavefront-uniform
    const long long i = i0 + (threadIdx.x & 63);
    RecVal v = {};
    if (i < n) v = rec_load(&in[i]);
    map_reinsert_wave(Tn, rec_live(v), v, fr, kind, deferred, deferred_cap);
  }
}

// ---------------------------------------------------------------------------------------------- host side

// Live records of both tables -> n_rec; with d_out != nullptr also the stream itself, in a device buffer of the caller's to hipFree
// (corner records, then surf records).  Temporary allocations only; the handle is not changed.  ms: kernel times of count + scan / pack (may be null).
vloam_status map_ckpt_pack(MapContext* m, hipStream_t st, long long n_rec[2], VoxelRec** d_out, float ms[2]) {
  int* d_cnt = nullptr;
  long long* d_off = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  if (d_out) *d_out = nullptr;
  vloam_status rc = VLOAM_OK;
  if (hipMalloc((void**)&d_cnt, sizeof(int) * 2 * kMoveMaxGrid) != hipSuccess || hipMalloc((void**)&d_off, sizeof(long long) * (2 * kMoveMaxGrid + 2)) != hipSuccess) rc = VLOAM_ERR_HIP;
  if (rc == VLOAM_OK && ms) for (hipEvent_t& e : ev) if (hipEventCreate(&e) != hipSuccess) rc = VLOAM_ERR_HIP;
  long long* d_total = d_off ? d_off + 2 * kMoveMaxGrid : nullptr;
  if (rc == VLOAM_OK) {
    if (ms) (void)hipEventRecord(ev[0], st);
    for (int k = 0; k < 2; k++) VL_RAW_LAUNCH(k_map_ckpt_count, dim3(map_move_grid(m->tab[k])), dim3(256), 0, st, m->tab[k], d_cnt + k * kMoveMaxGrid);
    VL_RAW_LAUNCH(k_map_ckpt_scan, dim3(1), dim3(256), 0, st, d_cnt, (int)map_move_grid(m->tab[0]), (int)map_move_grid(m->tab[1]), d_off, d_total);
    if (ms) (void)hipEventRecord(ev[1], st);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess ||
        hipMemcpy(n_rec, d_total, 2 * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) rc = VLOAM_ERR_HIP;
  }
  if (rc == VLOAM_OK && d_out) {
    const long long n = n_rec[0] + n_rec[1];
    if (hipMalloc((void**)d_out, (size_t)(n + 1) * sizeof(VoxelRec)) != hipSuccess) { *d_out = nullptr; rc = VLOAM_ERR_HIP; }
    if (rc == VLOAM_OK) {
      for (int k = 0; k < 2; k++) VL_RAW_LAUNCH(k_map_ckpt_pack, dim3(map_move_grid(m->tab[k])), dim3(256), 0, st, m->tab[k], d_off + k * kMoveMaxGrid, *d_out, n);
      if (ms) (void)hipEventRecord(ev[2], st);
      if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = VLOAM_ERR_HIP;
    }
    if (rc != VLOAM_OK && *d_out) { (void)hipFree(*d_out); *d_out = nullptr; }
  }
  if (ms) {
    ms[0] = ms[1] = 0.f;
    if (rc == VLOAM_OK) { (void)hipEventElapsedTime(&ms[0], ev[0], ev[1]); if (d_out) (void)hipEventElapsedTime(&ms[1], ev[1], ev[2]); }
  }
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  if (d_cnt) (void)hipFree(d_cnt);
  if (d_off) (void)hipFree(d_off);
  return rc;
}

// The stream (host memory: n_rec[0] corner records, then n_rec[1] surf records) into the handle's two tables, which are empty (a fresh handle).
// Occupancy blocks are published, raw voxels re-appended to the deferred lists and stats written, exactly as by a growth step.  Synchronises.
vloam_status map_ckpt_unpack(MapContext* m, hipStream_t st, const void* recs, const long long n_rec[2], float* ms) {
  const long long n = n_rec[0] + n_rec[1];
  VoxelRec* d_in = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (hipMalloc((void**)&d_in, (size_t)(n + 1) * sizeof(VoxelRec)) != hipSuccess) return VLOAM_ERR_HIP;
  vloam_status rc = VLOAM_OK;
  if (n > 0 && hipMemcpy(d_in, recs, (size_t)n * sizeof(VoxelRec), hipMemcpyHostToDevice) != hipSuccess) rc = VLOAM_ERR_HIP;
  if (rc == VLOAM_OK && ms) for (hipEvent_t& e : ev) if (hipEventCreate(&e) != hipSuccess) rc = VLOAM_ERR_HIP;
  if (rc == VLOAM_OK) {
    if (ms) (void)hipEventRecord(ev[0], st);
    for (int k = 0; k < 2; k++) {
      VL_RAW_LAUNCH(k_map_ckpt_begin, dim3(1), dim3(64), 0, st, m->tab[k], m->frame, k);
      if (n_rec[k] == 0) continue;
      VL_RAW_LAUNCH(k_map_ckpt_unpack, dim3(map_move_grid((size_t)n_rec[k])), dim3(256), 0, st, d_in + (k ? n_rec[0] : 0), n_rec[k], m->tab[k],
                    m->frame, k, m->deferred[k], k ? m->surf_cap : kStackCapCorner);
    }
    if (ms) (void)hipEventRecord(ev[1], st);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = VLOAM_ERR_HIP;
    if (ms) { *ms = 0.f; if (rc == VLOAM_OK) (void)hipEventElapsedTime(ms, ev[0], ev[1]); }
  }
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  (void)hipFree(d_in);
  return rc;
}

}  // namespace vloam
