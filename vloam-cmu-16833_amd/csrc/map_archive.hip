// Map archive (vloam_map_archive_enable): the points of cubes that roll out of the 21 x 21 x 11 window are copied into a list just before
// k_map_finalize's purge turns their records into tombstones.  A translation unit (and code object) of its own: no kernel of the sweep chain is
// touched by it, and a handle that never enables the archive allocates and launches nothing of this.
//   k_map_archive  grid (x, kind)  one launch per mapped sweep, between k_map_prepare (which decides the roll and writes the NEW cenW / cenH / cenD
//                                  and MapFrame::rolled) and k_map_finalize (which purges).  No roll: every wavefront reads MapFrame::rolled and
//                                  returns, no slot is loaded.  Roll: the slot walk of map_purge; a record that is a point of /laser_cloud_map
//                                  (rec_is_point below: the export's rule) and whose cube lies outside the new window becomes one 32-byte row.
// Rows are appended per wavefront (ballot, popcount, one integer atomicAdd by the leading lane), each with two 16-byte stores.  The cursor never
// stays above the capacity: a wavefront that finds it there takes its share back and adds it to the dropped counter instead, so the
// cursor is the number of rows held.  Everything is integer and read-only against the map.
// Skipped sweeps (mapping_skip_frame): map_enqueue returns behind k_map_prepare, so nothing is launched; k_map_prepare writes rolled = 0 on such a
// sweep, so the word is never stale.  Were it stale, the second walk would find tombstones only (count == 0 fails rec_is_point): harmless.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "map_kernels.h"
#include "map_table.h"

namespace vloam {

static_assert(sizeof(vloam_map_archive_row) == 32, "one row, two 16-byte stores");
// a point of /laser_cloud_map wherever the window is: pub_row's rule (map_output.hip) without its window test — live, and not a raw voxel's
// running sum, which is read through its point records
__device__ __forceinline__ bool rec_is_point(const RecVal& v) { return rec_live(v) && !(key_seq(v.key) == 0 && rec_raw(v.count)); }

constexpr unsigned kArchiveGrid = 512;  // workgroups per table at most: most launches find no roll and only have to start and end

__global__ __launch_bounds__(256) void k_map_archive(VoxelTable T0, VoxelTable T1, const MapState* __restrict__ ms, const MapFrame* __restrict__ fr,
                                                     vloam_map_archive_row* __restrict__ rows, int* __restrict__ cnt, int cap, int sweep) {
  if (!fr->rolled) return;
  const int kind = blockIdx.y;
  const VoxelTable& T = kind ? T1 : T0;
  const int cW = ms->cenW, cH = ms->cenH, cD = ms->cenD;
  const unsigned lane = threadIdx.x & 63u;
  if (kind == 0 && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&cnt[2], 1);   // rolls seen
  // wavefront-uniform trips: a table has a power of two of at least 1 024 slots, so a workgroup's 256 slots are inside it or none is
  for (unsigned base = blockIdx.x * 256; base <= T.mask; base += gridDim.x * 256) {
    const unsigned s = base + threadIdx.x;
    bool take = false;
    RecVal v;
    int Ai = 0, Aj = 0, Ak = 0;
    if (s <= T.mask) {
      v = rec_load(&T.rec[s]);
      if (rec_is_point(v)) {
        unpack_cube(v.key, &Ai, &Aj, &Ak);
        const int i = Ai + cW, j = Aj + cH, kk = Ak + cD;   // map_purge's test, against the window k_map_prepare has just placed
        take = i < 0 || i >= kCubeW || j < 0 || j >= kCubeH || kk < 0 || kk >= kCubeD;
      }
    }
    const unsigned long long m = __ballot(take);
    if (m == 0ull) continue;
    const int n = __popcll(m);
    int first = 0;
    if (lane == (unsigned)(__ffsll((long long)m) - 1)) {
      first = atomicAdd(&cnt[0], n);
      const int over = first >= cap ? n : (first + n > cap ? first + n - cap : 0);
      if (over) { atomicSub(&cnt[0], over); atomicAdd(&cnt[1], over); }
    }
    first = __shfl(first, __ffsll((long long)m) - 1);
    const int pos = first + __popcll(m & ((1ull << lane) - 1ull));
    if (take && pos < cap) {
      const float4 p = rec_point(v);
      const u64 okey = rec_order_key(v, 0, kind);   // low 32 bits: voxel (lz, ly, lx) or arrival stamp; bit 48: tail
      const unsigned flags = (unsigned)kind | ((unsigned)((okey >> 48) & 1ull) << 1);
      uint4* o = reinterpret_cast<uint4*>(rows + pos);
      o[0] = make_uint4(__float_as_uint(p.x), __float_as_uint(p.y), __float_as_uint(p.z), __float_as_uint(p.w));
      o[1] = make_uint4((unsigned)okey, ((unsigned)Ai & 0xffffu) | ((unsigned)Aj << 16), ((unsigned)Ak & 0xffffu) | (flags << 16), (unsigned)sweep);
    }
  }
}

// ---------------------------------------------------------------------------------------------- host side
constexpr size_t kArchiveHead = 256;   // the counters' line in front of the rows: rows held | rows dropped | rolls seen | -

vloam_status map_archive_alloc(MapContext* m, hipStream_t st, long long capacity_rows) {
  MapArchive* A = new MapArchive;
  if (hipMalloc((void**)&A->base, kArchiveHead + (size_t)capacity_rows * sizeof(vloam_map_archive_row)) != hipSuccess) { delete A; return VLOAM_ERR_HIP; }
  A->cnt = (int*)A->base;
  A->rows = (vloam_map_archive_row*)(A->base + kArchiveHead);
  A->cap = capacity_rows;
  if (hipMemsetAsync(A->base, 0, kArchiveHead, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { (void)hipFree(A->base); delete A; return VLOAM_ERR_HIP; }
  m->archive = A;
  return VLOAM_OK;
}

void map_archive_free(MapContext* m) {
  if (!m->archive) return;
  if (m->archive->base) (void)hipFree(m->archive->base);
  delete m->archive;
  m->archive = nullptr;
}

// m->tab[] as it is at enqueue time: behind a growth step or a same-size reclamation the launch walks the new tables
void map_archive_enqueue(const MapContext* m, hipStream_t st) {
  const MapArchive& A = *m->archive;
  const unsigned slots = std::max(m->tab[0].mask, m->tab[1].mask) + 1u;
  VL_RAW_LAUNCH(k_map_archive, dim3(std::min(slots / 256u, kArchiveGrid), 2, 1), dim3(256), 0, st, m->tab[0], m->tab[1], m->state, m->frame, A.rows, A.cnt, (int)A.cap,
                A.frame);
}

}  // namespace vloam
