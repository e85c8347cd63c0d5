// laserMapping on gfx950, host inspection of the mapping state: the sticky error words (vloam_sync), the parity hooks of the tests
// (vloam_debug_get, stage 2) and the counts of vloam_get_counts.  Synchronous copies; nothing here is enqueued by a sweep.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>
#include "map_kernels.h"

namespace vloam {

__global__ void k_map_error_fetch(MapFrame* fr, int clear_mask, int* out) { out[0] = atomicAnd(&fr->error, ~clear_mask); out[1] = fr->fallback_solves; }

// the sticky error words of all sessions OR-ed; the bits of clear_mask are reported once and cleared (transient per-sweep conditions)
vloam_status map_error(MapContext* m, int* e, int clear_mask, long long* fallback_solves) {
  *e = 0;
  if (fallback_solves) *fallback_solves = 0;
  for (int b = 0; b < m->se.B; b++) {
    const MapContext mb = m->for_session(b);
    int* d_out = mb.rebuild_n;  // scratch ints (no rebuild can be in flight: the caller has synchronised the streams)
    VL_RAW_LAUNCH(k_map_error_fetch, dim3(1), dim3(1), 0, 0, mb.frame, clear_mask, d_out);
    int v[2] = {0, 0};
    if (hipMemcpy(v, d_out, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
    *e |= v[0];
    if (fallback_solves) *fallback_solves += v[1];
  }
  return VLOAM_OK;
}

// item = outer * 16 + k:  k = 0 factor types i32[cap = 8 192 + the surf capacity], 1 A f64[3][cap], 2 B f64[3][cap], 3 LM record, 4 residuals f64[3][cap],
//                         5 p f64[3][cap].  item 64: MapState.  item 65: MapFrame.  item 66: cube_cnt i32[2][4851].
//                         item 67/68: dump of the corner / surf table as rows {key lo, key hi, count, x, y, z, w} (7 x 4 bytes) for live slots.
vloam_status map_debug_get(MapContext* m0, int item, void* buf, long long cap, long long* n) {
  const MapContext msel = m0->for_session(m0->sel);
  const MapContext* m = &msel;
  if (item == 64) return copy_dev(m->state, sizeof(MapState), buf, cap, n);
  if (item == 65) return copy_dev(m->frame, sizeof(MapFrame), buf, cap, n);
  if (item == 66) return copy_dev(m->cube_cnt, sizeof(int) * 2 * kCubeNum, buf, cap, n);
  if (item == 67 || item == 68) {
    const VoxelTable& T = m->tab[item - 67];
    const size_t slots = (size_t)T.mask + 1;
    std::vector<VoxelRec> recs(slots);
    if (hipMemcpy(recs.data(), T.rec, slots * sizeof(VoxelRec), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
    std::vector<unsigned> rows;
    for (size_t s = 0; s < slots; s++) {
      if (recs[s].key == 0 || recs[s].count == 0) continue;
      if ((recs[s].key >> 56) == 0 && (recs[s].count & (1 << 30))) continue;   // a raw voxel shows up as its point records (seq != 0)
      unsigned r[7];
      r[0] = (unsigned)(recs[s].key & 0xffffffffu); r[1] = (unsigned)(recs[s].key >> 32); r[2] = (unsigned)recs[s].count;
      memcpy(r + 3, &recs[s].sx, 16);
      rows.insert(rows.end(), r, r + 7);
    }
    if (n) *n = (long long)(rows.size() * 4);
    const size_t c = rows.size() * 4 < (size_t)cap ? rows.size() * 4 : (size_t)cap;
    if (buf && c) memcpy(buf, rows.data(), c);
    return VLOAM_OK;
  }
  if (item == 72) return copy_dev(m->ts_log, sizeof(long long) * 2048, buf, cap, n);   // VLOAM_TS_LOG=1: [sweep % 1024][prepare start, finalize start], 100 MHz ticks
  if (item == 73) return copy_dev(m->cbox, sizeof(int4) * 2 * (size_t)m->factor_cap(), buf, cap, n);   // per stack slot: the first round's search box + its candidate count (-1: not cached)
  if (item == 71) return copy_dev(m->assoc_cyc, sizeof(long long) * 16, buf, cap, n);   // k_map_assoc phase cycles (debug handles): [outer][6 phases, spare, wavefronts]
  if (item == 69) {  // table health: {keys, purged, block keys, spare} x {corner, surf}, rebuilds, largest candidate list
    int out[12] = {0};
    for (int k = 0; k < 2; k++) if (hipMemcpy(out + 4 * k, m->tab[k].stats, 4 * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
    MapFrame fr;
    if (hipMemcpy(&fr, m->frame, sizeof(fr), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
    out[8] = (int)m0->rebuilds; out[9] = fr.max_candidates; out[10] = fr.n_deferred[0] + fr.n_newraw[0]; out[11] = fr.n_deferred[1] + fr.n_newraw[1];
    if (n) *n = sizeof(out);
    if (buf) memcpy(buf, out, (size_t)cap < sizeof(out) ? (size_t)cap : sizeof(out));
    return VLOAM_OK;
  }
  const int outer = item / 16, k = item % 16;
  if (outer < 0 || outer > 1) return VLOAM_ERR_INVALID;
  const FactorTable& F = m->F[outer];
  switch (k) {
    case 0: return copy_dev(F.type, sizeof(int) * F.cap, buf, cap, n);
    case 1: return copy_dev(F.A, sizeof(double) * 3 * F.cap, buf, cap, n);
    case 2: return copy_dev(F.B, sizeof(double) * 3 * F.cap, buf, cap, n);
    case 3: return copy_dev(m->rec + outer, sizeof(LMRecord), buf, cap, n);
    case 4: return copy_dev(F.resid, sizeof(double) * 3 * F.cap, buf, cap, n);
    case 5: return copy_dev(F.p, sizeof(double) * 3 * F.cap, buf, cap, n);
  }
  return VLOAM_ERR_INVALID;
}

vloam_status map_counts(MapContext* m0, long long c[16]) {
  const MapContext msel = m0->for_session(m0->sel);
  const MapContext* m = &msel;
  MapState ms;
  MapFrame fr;
  LMRecord rec[2];
  if (hipMemcpy(&ms, m->state, sizeof(ms), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
  if (hipMemcpy(&fr, m->frame, sizeof(fr), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
  if (hipMemcpy(rec, m->rec, sizeof(rec), hipMemcpyDeviceToHost) != hipSuccess) return VLOAM_ERR_HIP;
  c[11] = ms.n_corner_stack; c[12] = ms.n_surf_stack;
  c[13] = fr.n_factors[1][0] + fr.n_factors[1][1];
  c[14] = ms.do_optimize ? (long long)(rec[0].n_evals + rec[1].n_evals) : 0;
  c[15] = ms.n_map_corner + ms.n_map_surf;
  return VLOAM_OK;
}

}  // namespace vloam
