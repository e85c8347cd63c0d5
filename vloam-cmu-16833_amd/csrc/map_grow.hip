// Growable voxel map (vloam_map_options::grow, single-sequence handles): the rehash of a table into a larger one between two sweeps, the
// per-sweep report the host's growth decision starts from, and that decision.  A translation unit (and code object) of its own: the kernels
// every handle launches (map_kernels.hip, map_stack.hip, map_output.hip) are not touched by it.
//   k_map_grow_begin  1 thread  the lists that hold slot ids and the table's counters start over
//   k_map_grow        grid      every live record of the old table -> the new one (the movers' one text: map_move_dev.h)
//   k_map_progress    1 WG      behind k_map_finalize of every mapped sweep: live keys, block keys, keys incl. tombstones -> host-mapped words
#include <hip/hip_runtime.h>
#include <algorithm>
#include "map_kernels.h"
#include "map_move_dev.h"

namespace vloam {

// One step: k_map_grow_begin, memsets of the new rec / blk, k_map_grow — between two sweeps on the mapping stream, in front of k_map_prepare.
// k_map_grow walks the OLD table in place (no staging list: the new table is another buffer) and moves every live record into the new one
// (map_move_dev.h) — slot ids change, exactly as in a rebuild.  Tombstones (count 0) are not carried over, so a step into a table of the SAME
// size is the tombstone reclamation of such a handle.  stats / deferred / the frame counters stay where they are (session arena);
// To.stats == Tn.stats.
__global__ void k_map_grow_begin(VoxelTable Tn, MapFrame* fr, int kind) {
  if (threadIdx.x == 0) map_move_begin(Tn, fr, kind);
}
__global__ __launch_bounds__(256) void k_map_grow(VoxelTable To, VoxelTable Tn, MapFrame* fr, int kind, int* __restrict__ deferred, int deferred_cap,
                                                  int* host_flags) {
  for (unsigned s0 = blockIdx.x * 256 + (threadIdx.x & ~63u); s0 <= To.mask; s0 += gridDim.x * 256) {   // wavefront-uniform (slots are a multiple of 64)
    const RecVal v = rec_load(&To.rec[s0 + (threadIdx.x & 63)]);
    map_reinsert_wave(Tn, rec_live(v), v, fr, kind, deferred, deferred_cap);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && host_flags) __hip_atomic_store(&host_flags[kind], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// Each word carries the sweep number it belongs to, so the host needs no ordering between the words (map_grow_report).
__global__ void k_map_progress(const MapState* __restrict__ ms, const int* __restrict__ stats0, const int* __restrict__ stats1, u64* progress) {
  const int kind = threadIdx.x;
  if (kind >= 2) return;
  const int* st = kind ? stats1 : stats0;
  const u64 sweep = (u64)(unsigned)ms->sweep_no << 32;
  __hip_atomic_store(&progress[3 * kind], sweep | (u64)(unsigned)(st[0] - st[1]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&progress[3 * kind + 1], sweep | (u64)(unsigned)st[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&progress[3 * kind + 2], sweep | (u64)(unsigned)st[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---------------------------------------------------------------------------------------------- host side
// rec / pend / blk of a table of 2^lg slots in allocations of their own (+ the arena's 256 B of slack); rec and blk zeroed on st.  A failure
// frees nothing (hipFree synchronises the device): what it had got goes to `leftover`.
static vloam_status map_grow_alloc(MapGrow& G, int lg, hipStream_t st, void* p[3]) {
  const size_t slots = (size_t)1 << lg, bytes[3] = {slots * sizeof(VoxelRec) + 256, slots * kPendCap * sizeof(int) + 256, slots / 2 * sizeof(ulonglong2) + 256};
  p[0] = p[1] = p[2] = nullptr;
  bool ok = true;
  for (int k = 0; k < 3 && ok; k++) ok = hipMalloc(&p[k], bytes[k]) == hipSuccess;
  ok = ok && hipMemsetAsync(p[0], 0, bytes[0], st) == hipSuccess && hipMemsetAsync(p[2], 0, bytes[2], st) == hipSuccess;
  if (ok) return VLOAM_OK;
  (void)hipGetLastError();
  for (int k = 0; k < 3; k++) if (p[k]) { G.leftover.push_back(p[k]); p[k] = nullptr; }
  G.failed_log2 = lg;
  return VLOAM_ERR_HIP;
}
static void map_grow_adopt(VoxelTable& T, int lg, void* const p[3]) {
  T.rec = (VoxelRec*)p[0]; T.pend = (int*)p[1]; T.blk = (ulonglong2*)p[2];
  T.mask = (unsigned)(((size_t)1 << lg) - 1); T.bslots_mask = (unsigned)(((size_t)1 << lg) / 2 - 1);
}

vloam_status map_grow_init(MapContext* m, hipStream_t st) {
  MapGrow& G = *m->grow;
  if (hipHostMalloc((void**)&G.progress, sizeof(u64) * 6, hipHostMallocMapped) != hipSuccess) { G.progress = nullptr; return VLOAM_ERR_HIP; }
  for (int k = 0; k < 6; k++) G.progress[k] = 0ull;
  for (hipEvent_t& e : G.ev_prog) if (hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventBlockingSync) != hipSuccess) { e = nullptr; return VLOAM_ERR_HIP; }
  for (int k = 0; k < 2; k++) {
    void* p[3];
    if (map_grow_alloc(G, G.lg[k], st, p) != VLOAM_OK) return VLOAM_ERR_HIP;
    map_grow_adopt(m->tab[k], G.lg[k], p);
  }
  return VLOAM_OK;
}

void map_grow_release(MapContext* m) {
  if (!m->grow) return;
  MapGrow& G = *m->grow;
  size_t keep = 0;
  for (size_t i = 0; i < G.retired.size(); i++) {
    if (hipEventQuery(G.retired[i].ev) != hipSuccess) { (void)hipGetLastError(); G.retired[keep++] = G.retired[i]; continue; }
    for (void* p : G.retired[i].p) (void)hipFree(p);
    (void)hipEventDestroy(G.retired[i].ev);
  }
  G.retired.resize(keep);
  for (void* p : G.leftover) (void)hipFree(p);
  G.leftover.clear();
}

void map_grow_destroy(MapContext* m) {   // (vloam_destroy has drained the handle's streams)
  map_grow_release(m);
  MapGrow& G = *m->grow;
  for (MapGrow::Retired& r : G.retired) { for (void* p : r.p) (void)hipFree(p); (void)hipEventDestroy(r.ev); }   // (an event that did not fire: a failed stream)
  for (int k = 0; k < 2; k++) { (void)hipFree(m->tab[k].rec); (void)hipFree(m->tab[k].pend); (void)hipFree(m->tab[k].blk); m->tab[k].rec = nullptr; }
  for (hipEvent_t e : G.ev_prog) if (e) (void)hipEventDestroy(e);
  if (G.progress) (void)hipHostFree(G.progress);
  delete m->grow;
  m->grow = nullptr;
}

// Rehash table `kind` into a fresh one of 2^new_lg slots (new_lg == the current log2: tombstone reclamation).  Enqueued between two sweeps,
// in front of k_map_prepare: no sweep is in flight BEHIND this point of the stream, so pend_cnt of every seq-0 record is zero when k_map_grow
// runs and the new pend[] needs no copy.  hipMalloc from the enqueueing thread; a failure leaves the old table in use and nothing enqueued.
// The old buffers are retired with an event behind the chain (map_grow_release).  The rebuild flag of this kind may still be up from a sweep
// that ran before the step: the cool-down of map_enqueue's flag poll covers it, as after a rebuild.
static vloam_status map_grow_step(MapContext* m, hipStream_t st, int kind, int new_lg) {
  MapGrow& G = *m->grow;
  const VoxelTable To = m->tab[kind];
  void* p[3];
  MapGrow::Retired old = {{To.rec, To.pend, To.blk}, nullptr};
  if (hipEventCreateWithFlags(&old.ev, hipEventDisableTiming) != hipSuccess) return VLOAM_ERR_HIP;
  if (map_grow_alloc(G, new_lg, st, p) != VLOAM_OK) { (void)hipEventDestroy(old.ev); return VLOAM_ERR_HIP; }
  VL_RAW_LAUNCH(k_map_grow_begin, dim3(1), dim3(64), 0, st, To, m->frame, kind);
  VoxelTable Tn = To;
  map_grow_adopt(Tn, new_lg, p);
  VL_RAW_LAUNCH(k_map_grow, dim3(map_move_grid(To)), dim3(256), 0, st, To, Tn, m->frame, kind, m->deferred[kind], kind ? m->surf_cap : kStackCapCorner, m->host_flags);
  const bool ok = hipGetLastError() == hipSuccess && hipEventRecord(old.ev, st) == hipSuccess;
  m->tab[kind] = Tn;   // (whatever was enqueued reads the new table from here on)
  G.retired.push_back(old);
  if (new_lg > G.lg[kind]) G.steps++; else m->rebuilds++;
  G.lg[kind] = new_lg;
  G.step_at[kind] = m->pub.mapped;
  m->rebuild_cooldown[0][kind] = 8;
  return ok ? VLOAM_OK : VLOAM_ERR_HIP;
}

vloam_status map_grow_rehash(MapContext* m, hipStream_t st, int kind) { return map_grow_step(m, st, kind, m->grow->lg[kind]); }

// the latest report of table `kind`, and the mapped sweep it is no older than
struct GrowReport { long long sweep, live, blk, keys; };
static GrowReport map_grow_report(const MapGrow& G, int kind) {
  u64 w[3];
  for (int i = 0; i < 3; i++) w[i] = __atomic_load_n(&G.progress[3 * kind + i], __ATOMIC_RELAXED);
  // the words may belong to different sweeps: the OLDEST number with all three values is still an upper bound (a value of a later sweep plus
  // the allowance of the sweeps since the earlier one)
  GrowReport r;
  r.sweep = (long long)std::min(w[0] >> 32, std::min(w[1] >> 32, w[2] >> 32));
  r.live = (long long)(w[0] & 0xffffffffull); r.blk = (long long)(w[1] & 0xffffffffull); r.keys = (long long)(w[2] & 0xffffffffull);
  if (r.sweep <= G.step_at[kind]) r.keys = r.live;   // the table was rehashed since: its tombstones are gone
  return r;
}

// In front of every mapped sweep, per kind:
//   bound = last reported keys + (mapped sweeps enqueued since that report + this one) x (what a sweep can add)
// for the live records, for the block keys, and for the slots in use (live records + tombstones: probe chains run through both).  If the live
// records or the block keys could cross k_map_finalize's 60 % during this sweep, the table is doubled first and the bound re-evaluated; if only
// the slots in use could, the table is rehashed at its size.  The host runs up to kBufferSets sweeps ahead of the mapping, so the
// un-confirmed part of the bound can be most of it.  Rule: if the reported keys plus TWO sweeps' allowance (this sweep and the newest
// enqueued one, which the host never waits for) fit, i.e. only the staler part asks for the doubling, the host first waits for the report
// event of the mapped sweep before the newest one — whose report then covers everything but the newest — and re-evaluates; once per kind
// and sweep.  A table that close to its threshold costs the host one sweep of run-ahead, not memory.
vloam_status map_grow_before_sweep(MapContext* m, hipStream_t st) {
  MapGrow& G = *m->grow;
  const long long mapped = m->pub.mapped;   // mapped sweeps enqueued so far; this one will be number mapped + 1
  for (int k = 0; k < 2; k++) {
    bool refreshed = false, rehashed = false;
    for (;;) {
      const GrowReport r = map_grow_report(G, k);
      const long long u = mapped - r.sweep, slots = (long long)m->tab[k].mask + 1, bslots = (long long)m->tab[k].bslots_mask + 1;
      auto over = [&](long long keys, long long sweeps) { return (keys + sweeps * G.inc_rec[k]) * 10 > slots * 6; };
      auto over_live = [&](long long sweeps) { return over(r.live, sweeps) || (r.blk + sweeps * G.inc_blk[k]) * 10 > bslots * 6; };
      if (!over_live(u + 1)) {
        if (over(r.keys, u + 1) && !rehashed) {   // tombstones: a fresh table of the same size
          if (map_grow_step(m, st, k, G.lg[k]) != VLOAM_OK) return VLOAM_ERR_HIP;
          rehashed = true;
          continue;
        }
        break;
      }
      if (G.lg[k] >= G.max_log2) break;   // at the ceiling: from there on k_map_finalize decides, as on a fixed handle
      if (u > 1 && !over_live(2) && !refreshed && mapped >= 2) {
        if (hipEventSynchronize(G.ev_prog[(mapped - 2) % MapGrow::kEvRing]) != hipSuccess) return VLOAM_ERR_HIP;   // report of mapped sweep number mapped - 1
        refreshed = true;
        continue;
      }
      if (map_grow_step(m, st, k, G.lg[k] + 1) != VLOAM_OK) return VLOAM_ERR_HIP;
    }
  }
  return VLOAM_OK;
}

// behind k_map_finalize of the mapped sweep map_enqueue has just counted (pub.mapped); the event is bound to the dispatch
void map_grow_progress_enqueue(MapContext* m, hipStream_t st) {
  hipEvent_t ev = m->grow->ev_prog[(m->pub.mapped - 1) % MapGrow::kEvRing];
  VLOAM_LAUNCH_EV((ProfHook*)nullptr, kKNone, st, ev, k_map_progress, dim3(1), dim3(64), 0, st, m->state, m->tab[0].stats, m->tab[1].stats, m->grow->progress);
}

// vloam_checkpoint_load on a growable handle, whose tables are still empty.  map_grow_restore_log2: the smallest size from the current one up to
// the ceiling under which the growth bound holds for a table of `live` records and `blk` block keys with one sweep to come.
// map_grow_restore: the tables step to lg[] (a step of an empty table) and the report words say what the tables hold once the checkpoint's records
// are in, as of mapped sweep `mapped`, so that the next sweep's decision starts from them.
int map_grow_restore_log2(const MapContext* m, int kind, long long live, long long blk) {
  const MapGrow& G = *m->grow;
  int lg = G.lg[kind];
  while (lg < G.max_log2 && ((live + G.inc_rec[kind]) * 10 > ((long long)1 << lg) * 6 || (blk + G.inc_blk[kind]) * 10 > ((long long)1 << (lg - 1)) * 6)) lg++;
  return lg;
}
vloam_status map_grow_restore(MapContext* m, hipStream_t st, const int lg[2], const long long live[2], const long long blk[2], long long mapped) {
  MapGrow& G = *m->grow;
  for (int k = 0; k < 2; k++) {
    const int old_lg = G.lg[k];
    if (lg[k] != old_lg) {
      if (map_grow_step(m, st, k, lg[k]) != VLOAM_OK) return VLOAM_ERR_HIP;
      G.steps += lg[k] - old_lg - 1;   // (health counts doublings)
    }
    const u64 sweep = (u64)(unsigned)mapped << 32;
    G.progress[3 * k] = sweep | (u64)(unsigned)live[k]; G.progress[3 * k + 1] = sweep | (u64)(unsigned)blk[k]; G.progress[3 * k + 2] = sweep | (u64)(unsigned)live[k];
    G.step_at[k] = mapped;
  }
  return VLOAM_OK;
}

vloam_status map_force_grow(MapContext* m, hipStream_t st) {
  if (!m->grow) return VLOAM_ERR_INVALID;
  for (int k = 0; k < 2; k++)
    if (m->grow->lg[k] < m->grow->max_log2 && map_grow_step(m, st, k, m->grow->lg[k] + 1) != VLOAM_OK) return VLOAM_ERR_HIP;
  return VLOAM_OK;
}

}  // namespace vloam
