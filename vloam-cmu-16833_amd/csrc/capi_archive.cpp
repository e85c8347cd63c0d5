// Map archive of libvloam_hip.so: vloam_map_archive_enable / _info / _get / _device_ptr — the points of cubes that roll out of the window are
// kept in a list on the device (kernel and launch: map_archive.hip).
#include "handle.h"

static_assert(sizeof(vloam_map_archive_options) == 16 && offsetof(vloam_map_archive_options, capacity_rows) == 8, "vloam_map_archive_options: int, long long");
static_assert(sizeof(vloam_map_archive_row) == 32 && offsetof(vloam_map_archive_row, order) == 16 && offsetof(vloam_map_archive_row, cube_i) == 20 &&
              offsetof(vloam_map_archive_row, flags) == 26 && offsetof(vloam_map_archive_row, sweep) == 28, "vloam_map_archive_row: 4 floats, order, 3 shorts, flags, sweep");

constexpr long long kArchiveCapDefault = 1ll << 20, kArchiveCapMax = 1ll << 26;

// the handle of info / get / device_ptr: enabled, and nothing of it in flight
static vloam_status archive_ready(const char* call, vloam_handle* h) {
  if (!h) { set_err("%s: null handle", call); return VLOAM_ERR_INVALID; }
  if (!h->map.archive) { set_err("%s: the handle keeps no archive (vloam_map_archive_enable was not called)", call); return VLOAM_ERR_INVALID; }
  HIPCHK(hipSetDevice(h->device));
  return sync_all(h);
}

// (sweep, kind, cube_k, cube_j, cube_i, tail, order): unique per row
static inline bool archive_less(const vloam_map_archive_row& a, const vloam_map_archive_row& b) {
  if (a.sweep != b.sweep) return a.sweep < b.sweep;
  if ((a.flags & 1) != (b.flags & 1)) return (a.flags & 1) < (b.flags & 1);
  if (a.cube_k != b.cube_k) return a.cube_k < b.cube_k;
  if (a.cube_j != b.cube_j) return a.cube_j < b.cube_j;
  if (a.cube_i != b.cube_i) return a.cube_i < b.cube_i;
  if ((a.flags & 2) != (b.flags & 2)) return (a.flags & 2) < (b.flags & 2);
  return a.order < b.order;
}

extern "C" {

void vloam_default_map_archive_options(vloam_map_archive_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->struct_size = (int)sizeof(*o);
  o->capacity_rows = kArchiveCapDefault;
}

vloam_status vloam_map_archive_enable(vloam_handle* h, const vloam_map_archive_options* o) {
  const char* call = "vloam_map_archive_enable";
  if (!o) { set_err("%s: null options", call); return VLOAM_ERR_INVALID; }
  if (o->struct_size != (int)sizeof(vloam_map_archive_options)) { set_err("%s: vloam_map_archive_options: struct_size must be %d", call, (int)sizeof(vloam_map_archive_options)); return VLOAM_ERR_INVALID; }
  if (o->capacity_rows < 1 || o->capacity_rows > kArchiveCapMax) { set_err("%s: capacity_rows must be 1 .. %lld rows, not %lld", call, kArchiveCapMax, o->capacity_rows); return VLOAM_ERR_INVALID; }
  if (!h) { set_err("%s: null handle", call); return VLOAM_ERR_INVALID; }
  if (h->se.B != 1) { set_err("%s: the archive follows one sequence: the handle has %d sessions (their tables lie at an arena stride)", call, h->se.B); return VLOAM_ERR_INVALID; }
  if (!h->cfg.with_mapping) { set_err("%s: the handle was created with with_mapping == 0: it keeps no map", call); return VLOAM_ERR_INVALID; }
  if (h->map.archive) { set_err("%s: the handle already keeps an archive of %lld rows", call, h->map.archive->cap); return VLOAM_ERR_INVALID; }
  HIPCHK(hipSetDevice(h->device));
  TRY(sync_all(h));
  if (map_archive_alloc(&h->map, h->s_map, o->capacity_rows) != VLOAM_OK) {
    set_err("%s: could not allocate %lld rows of 32 bytes: %s", call, o->capacity_rows, hipGetErrorString(hipGetLastError())); return VLOAM_ERR_HIP;
  }
  return VLOAM_OK;
}

vloam_status vloam_map_archive_info(vloam_handle* h, long long out4[4]) {
  const char* call = "vloam_map_archive_info";
  if (!out4) { set_err("%s: null output", call); return VLOAM_ERR_INVALID; }
  TRY(archive_ready(call, h));
  int cnt[4];
  HIPCHK(hipMemcpy(cnt, h->map.archive->cnt, sizeof(cnt), hipMemcpyDeviceToHost));
  out4[0] = cnt[0]; out4[1] = cnt[1]; out4[2] = h->map.archive->cap; out4[3] = cnt[2];
  return VLOAM_OK;
}

vloam_status vloam_map_archive_get(vloam_handle* h, vloam_map_archive_row* rows, long long cap, long long* n, int clear) {
  const char* call = "vloam_map_archive_get";
  if (!n) { set_err("%s: null count", call); return VLOAM_ERR_INVALID; }
  if (cap < 0 || (cap > 0 && !rows)) { set_err("%s: a buffer of %lld rows at a %s address", call, cap, rows ? "non-null" : "null"); return VLOAM_ERR_INVALID; }
  if (clear < 0 || clear > 1) { set_err("%s: clear must be 0 or 1, not %d", call, clear); return VLOAM_ERR_INVALID; }
  TRY(archive_ready(call, h));
  const MapArchive& A = *h->map.archive;
  int cnt[2];
  HIPCHK(hipMemcpy(cnt, A.cnt, sizeof(cnt), hipMemcpyDeviceToHost));
  *n = cnt[0];
  if (*n > cap) { set_err("%s: the archive holds %lld rows, the buffer %lld: nothing was copied or cleared", call, *n, cap); return VLOAM_ERR_CAPACITY; }
  if (*n > 0) {
    HIPCHK(hipMemcpy(rows, A.rows, (size_t)*n * sizeof(vloam_map_archive_row), hipMemcpyDeviceToHost));
    std::sort(rows, rows + *n, archive_less);
  }
  if (clear) HIPCHK(hipMemset(A.cnt, 0, 2 * sizeof(int)));
  return VLOAM_OK;
}

vloam_status vloam_map_archive_device_ptr(vloam_handle* h, void** d_rows, int** d_n_rows) {
  const char* call = "vloam_map_archive_device_ptr";
  if (!d_rows || !d_n_rows) { set_err("%s: null output", call); return VLOAM_ERR_INVALID; }
  if (!h) { set_err("%s: null handle", call); return VLOAM_ERR_INVALID; }
  if (!h->map.archive) { set_err("%s: the handle keeps no archive (vloam_map_archive_enable was not called)", call); return VLOAM_ERR_INVALID; }
  *d_rows = h->map.archive->rows;
  *d_n_rows = h->map.archive->cnt;
  return VLOAM_OK;
}

}  // extern "C"
