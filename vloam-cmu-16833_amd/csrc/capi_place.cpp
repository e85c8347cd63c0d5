// Place recognition of libvloam_hip.so: vloam_place_enable, _describe, _add, _count, _get, _load and _query* (sweep descriptors, a database of
// them on the device, one descriptor against every row at every yaw shift; kernels: place.hip).  Everything runs on the scan-registration
// stream, which every handle owns; nothing of a sequence is read or written.
#include "handle.h"

static_assert(sizeof(vloam_place_options) == 36 && offsetof(vloam_place_options, min_range) == 16 && offsetof(vloam_place_options, reserved) == 32,
              "vloam_place_options: 4 ints, 4 floats, 1 int");
static_assert(sizeof(vloam_place_query_options) == 16 && sizeof(vloam_place_match) == 32, "vloam_place_query_options: 4 ints; vloam_place_match: 8 ints");

static bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }

// ------------------------------------------------------------------ the refusals that need no handle, in the order c_api.h lists them
static vloam_status place_check_options(const char* call, const vloam_place_options* o) {
  if (!o) { set_err("%s: null options", call); return VLOAM_ERR_INVALID; }
  if (o->struct_size != (int)sizeof(vloam_place_options)) { set_err("%s: vloam_place_options: struct_size must be %d", call, (int)sizeof(vloam_place_options)); return VLOAM_ERR_INVALID; }
  if (o->reserved != 0) { set_err("%s: reserved must be 0", call); return VLOAM_ERR_INVALID; }
  if (o->n_ring < 1 || o->n_ring > kPlaceMaxRing) { set_err("%s: n_ring must be 1 .. %d, not %d", call, kPlaceMaxRing, o->n_ring); return VLOAM_ERR_INVALID; }
  if (o->n_sector < 1 || o->n_sector > kPlaceMaxSector) { set_err("%s: n_sector must be 1 .. %d, not %d", call, kPlaceMaxSector, o->n_sector); return VLOAM_ERR_INVALID; }
  if (o->capacity < 1 || o->capacity > kPlaceMaxRows) { set_err("%s: capacity must be 1 .. %d rows, not %d", call, kPlaceMaxRows, o->capacity); return VLOAM_ERR_INVALID; }
  if (!(o->max_range > 0.f) || !finite_f(o->max_range)) { set_err("%s: max_range must be positive and finite", call); return VLOAM_ERR_INVALID; }
  if (!(o->z_step > 0.f) || !finite_f(o->z_step)) { set_err("%s: z_step must be positive and finite", call); return VLOAM_ERR_INVALID; }
  if (!finite_f(o->z_min)) { set_err("%s: z_min must be finite", call); return VLOAM_ERR_INVALID; }
  if (!(o->min_range >= 0.f) || !finite_f(o->min_range)) { set_err("%s: min_range must be finite and not negative", call); return VLOAM_ERR_INVALID; }
  if (o->min_range >= o->max_range) { set_err("%s: min_range %.9g m must be below max_range %.9g m", call, (double)o->min_range, (double)o->max_range); return VLOAM_ERR_INVALID; }
  return VLOAM_OK;
}

static vloam_status place_check_query_options(const char* call, const vloam_place_query_options* o) {
  if (!o) { set_err("%s: null options", call); return VLOAM_ERR_INVALID; }
  if (o->struct_size != (int)sizeof(vloam_place_query_options)) { set_err("%s: vloam_place_query_options: struct_size must be %d", call, (int)sizeof(vloam_place_query_options)); return VLOAM_ERR_INVALID; }
  if (o->reserved != 0) { set_err("%s: reserved must be 0", call); return VLOAM_ERR_INVALID; }
  if (o->k < 1 || o->k > kPlaceMaxK) { set_err("%s: k must be 1 .. %d matches, not %d", call, kPlaceMaxK, o->k); return VLOAM_ERR_INVALID; }
  if (o->exclude_last < 0) { set_err("%s: exclude_last must not be negative (%d)", call, o->exclude_last); return VLOAM_ERR_INVALID; }
  return VLOAM_OK;
}

static vloam_status place_check_cloud(const char* call, const void* xyzi4, int n) {
  if (n < 0) { set_err("%s: negative cloud size (%d points)", call, n); return VLOAM_ERR_INVALID; }
  if (n > kPlaceMaxPoints) { set_err("%s: %d points: at most %d", call, n, kPlaceMaxPoints); return VLOAM_ERR_INVALID; }
  if (n > 0 && !xyzi4) { set_err("%s: null cloud with %d points", call, n); return VLOAM_ERR_INVALID; }
  return VLOAM_OK;
}

// ------------------------------------------------------------------ ... and the ones that do
static vloam_status place_admit(const char* call, vloam_handle* h) {
  if (!h) { set_err("%s: null handle", call); return VLOAM_ERR_INVALID; }
  if (!h->place.enabled) { set_err("%s: vloam_place_enable has not been called on this handle", call); return VLOAM_ERR_ORDER; }
  HIPCHK(hipSetDevice(h->device));
  return VLOAM_OK;
}

// the host forms' copy of a cloud: on the stream, into a buffer that only grows
static vloam_status place_stage(const char* call, vloam_handle* h, const float* xyzi4, int n, const void** d_out) {
  PlaceContext& P = h->place;
  *d_out = nullptr;
  if (n == 0) return VLOAM_OK;
  if (n > P.cloud_cap) {
    HIPCHK(hipStreamSynchronize(h->stream));   // an earlier device form may still read the old buffer
    if (P.cloud) (void)hipFree(P.cloud);
    P.cloud = nullptr; P.cloud_cap = 0;
    if (hipMalloc((void**)&P.cloud, (size_t)n * sizeof(float4)) != hipSuccess) { set_err("%s: hipMalloc of %zu bytes failed", call, (size_t)n * sizeof(float4)); return VLOAM_ERR_HIP; }
    P.cloud_cap = n;
  }
  HIPCHK(hipMemcpyAsync(P.cloud, xyzi4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
  *d_out = P.cloud;
  return VLOAM_OK;
}

static vloam_status place_launch_failed(const char* call) {
  set_err("%s: the launch failed: %s", call, hipGetErrorString(hipGetLastError()));
  return VLOAM_ERR_HIP;
}

// describe into row `count` and count it
static vloam_status place_append(const char* call, vloam_handle* h, const void* d_pts, int n, int tag, int* row_out) {
  PlaceContext& P = h->place;
  if (P.count >= P.capacity) { set_err("%s: the database is full (%d rows)", call, P.capacity); return VLOAM_ERR_CAPACITY; }
  const int row = P.count;
  if (place_describe_enqueue(&P, h->stream, d_pts, n, P.db + (size_t)row * P.words(), P.info + 2 * (size_t)row, P.tags + row, tag) != VLOAM_OK) return place_launch_failed(call);
  P.count = row + 1;
  if (row_out) *row_out = row;
  return VLOAM_OK;
}

static int place_limit(const PlaceContext& P, const vloam_place_query_options* o) { return o->exclude_last >= P.count ? 0 : P.count - o->exclude_last; }

// pad bytes (rings R .. 4 W - 1 of every sector) of `rows` packed descriptors; returns the first offending row, -1: none
static int place_bad_pad(const PlaceGeom& g, const unsigned* words, int rows) {
  const int pad = 4 * g.W - g.R;
  if (pad == 0) return -1;
  const unsigned mask = ~0u << (8 * (4 - pad));   // the upper `pad` bytes of a sector's last word
  for (int r = 0; r < rows; r++)
    for (int j = 0; j < g.S; j++)
      if (words[((size_t)r * g.S + j) * g.W + g.W - 1] & mask) return r;
  return -1;
}

static int place_occupied(const PlaceGeom& g, const unsigned* words) {
  int occ = 0;
  for (int t = 0; t < g.S * g.W; t++)
    for (int b = 0; b < 4; b++) occ += ((words[t] >> (8 * b)) & 255u) ? 1 : 0;
  return occ;
}

extern "C" {

void vloam_default_place_options(vloam_place_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->struct_size = (int)sizeof(*o);
  o->n_ring = 20; o->n_sector = 60; o->capacity = 16384;
  o->min_range = 0.f; o->max_range = 80.f; o->z_min = -3.f; o->z_step = 0.05f;
}

void vloam_default_place_query_options(vloam_place_query_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->struct_size = (int)sizeof(*o);
  o->k = 1;
}

vloam_status vloam_place_enable(vloam_handle* h, const vloam_place_options* o) {
  static const char* const call = "vloam_place_enable";
  TRY(place_check_options(call, o));
  if (!h) { set_err("%s: null handle", call); return VLOAM_ERR_INVALID; }
  if (h->se.B != 1) { set_err("%s: not offered on a batched handle (%d sessions)", call, h->se.B); return VLOAM_ERR_INVALID; }
  if (h->place.enabled) { set_err("%s: already enabled on this handle", call); return VLOAM_ERR_ORDER; }
  const float min_range = o->min_range != 0.f ? o->min_range : (float)h->cfg.minimum_range;
  if (!(min_range >= 0.f) || !(min_range < o->max_range)) {
    set_err("%s: the handle's minimum_range %.9g m must be below max_range %.9g m", call, (double)min_range, (double)o->max_range); return VLOAM_ERR_INVALID;
  }
  HIPCHK(hipSetDevice(h->device));
  PlaceContext P;
  PlaceGeom& g = P.g;
  g.R = o->n_ring; g.S = o->n_sector; g.W = (o->n_ring + 3) / 4;
  g.min2 = min_range * min_range; g.max2 = o->max_range * o->max_range;
  g.z_min = o->z_min; g.z_step = o->z_step;
  const float pi_f = 3.14159274101257324f;
  g.k_sector = (float)g.S / (2.f * pi_f);
  const float w = o->max_range / (float)g.R;
  for (int i = 0; i < kPlaceMaxRing; i++) { const float e = (float)i * w; g.edge2[i] = e * e; }
  P.capacity = o->capacity;
  const size_t words = (size_t)P.words();
  bool ok = hipMalloc((void**)&P.db, (size_t)P.capacity * words * sizeof(unsigned)) == hipSuccess;
  ok = ok && hipMalloc((void**)&P.tags, (size_t)P.capacity * sizeof(int)) == hipSuccess;
  ok = ok && hipMalloc((void**)&P.info, (size_t)P.capacity * 2 * sizeof(int)) == hipSuccess;
  ok = ok && hipMalloc((void**)&P.best, (size_t)P.capacity * sizeof(unsigned long long)) == hipSuccess;
  ok = ok && hipMalloc((void**)&P.cells, (kPlaceMaxCells + 1) * sizeof(int)) == hipSuccess;
  ok = ok && hipMalloc((void**)&P.qdesc, words * sizeof(unsigned)) == hipSuccess;
  ok = ok && hipMalloc((void**)&P.qinfo, 2 * sizeof(int)) == hipSuccess;
  ok = ok && hipMalloc((void**)&P.qmatch, kPlaceMaxK * sizeof(vloam_place_match)) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    for (void* p : {(void*)P.db, (void*)P.tags, (void*)P.info, (void*)P.best, (void*)P.cells, (void*)P.qdesc, (void*)P.qinfo, (void*)P.qmatch}) if (p) (void)hipFree(p);
    set_err("%s: hipMalloc failed for %d rows of %zu bytes", call, P.capacity, words * sizeof(unsigned) + 20);
    return VLOAM_ERR_HIP;
  }
  P.enabled = true;
  h->place = P;   // (vloam_destroy frees them)
  return VLOAM_OK;
}

vloam_status vloam_place_describe_device(vloam_handle* h, const void* d_xyzi4, int n, void* d_desc_words, void* d_info2) {
  static const char* const call = "vloam_place_describe_device";
  TRY(place_check_cloud(call, d_xyzi4, n));
  if (!d_desc_words) { set_err("%s: null descriptor buffer", call); return VLOAM_ERR_INVALID; }
  TRY(place_admit(call, h));
  if (place_describe_enqueue(&h->place, h->stream, d_xyzi4, n, d_desc_words, d_info2 ? d_info2 : (void*)h->place.qinfo, nullptr, 0) != VLOAM_OK) return place_launch_failed(call);
  return VLOAM_OK;
}

vloam_status vloam_place_describe(vloam_handle* h, const float* xyzi4, int n, unsigned int* desc_words, int* info2) {
  static const char* const call = "vloam_place_describe";
  TRY(place_check_cloud(call, xyzi4, n));
  if (!desc_words) { set_err("%s: null descriptor buffer", call); return VLOAM_ERR_INVALID; }
  TRY(place_admit(call, h));
  PlaceContext& P = h->place;
  const void* d = nullptr;
  TRY(place_stage(call, h, xyzi4, n, &d));
  if (place_describe_enqueue(&P, h->stream, d, n, P.qdesc, P.qinfo, nullptr, 0) != VLOAM_OK) return place_launch_failed(call);
  HIPCHK(hipMemcpyAsync(desc_words, P.qdesc, (size_t)P.words() * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
  if (info2) HIPCHK(hipMemcpyAsync(info2, P.qinfo, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VLOAM_OK;
}

vloam_status vloam_place_add_device(vloam_handle* h, const void* d_xyzi4, int n, int tag, int* row_out) {
  static const char* const call = "vloam_place_add_device";
  TRY(place_check_cloud(call, d_xyzi4, n));
  TRY(place_admit(call, h));
  return place_append(call, h, d_xyzi4, n, tag, row_out);
}

vloam_status vloam_place_add(vloam_handle* h, const float* xyzi4, int n, int tag, int* row_out) {
  static const char* const call = "vloam_place_add";
  TRY(place_check_cloud(call, xyzi4, n));
  TRY(place_admit(call, h));
  if (h->place.count >= h->place.capacity) { set_err("%s: the database is full (%d rows)", call, h->place.capacity); return VLOAM_ERR_CAPACITY; }
  const void* d = nullptr;
  TRY(place_stage(call, h, xyzi4, n, &d));
  TRY(place_append(call, h, d, n, tag, row_out));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VLOAM_OK;
}

vloam_status vloam_place_count(vloam_handle* h, int* count) {
  static const char* const call = "vloam_place_count";
  if (!count) { set_err("%s: null count", call); return VLOAM_ERR_INVALID; }
  TRY(place_admit(call, h));
  *count = h->place.count;
  return VLOAM_OK;
}

vloam_status vloam_place_get(vloam_handle* h, int first, int count, unsigned int* desc_words, int* tags, int* info2) {
  static const char* const call = "vloam_place_get";
  if (first < 0 || count < 0) { set_err("%s: negative range (first %d, count %d)", call, first, count); return VLOAM_ERR_INVALID; }
  if (count > 0 && !desc_words) { set_err("%s: null descriptor buffer with %d rows", call, count); return VLOAM_ERR_INVALID; }
  TRY(place_admit(call, h));
  PlaceContext& P = h->place;
  if ((long long)first + count > P.count) { set_err("%s: rows %d .. %lld of a database of %d rows", call, first, (long long)first + count - 1, P.count); return VLOAM_ERR_INVALID; }
  if (count == 0) return VLOAM_OK;
  const size_t words = (size_t)P.words();
  HIPCHK(hipMemcpyAsync(desc_words, P.db + (size_t)first * words, (size_t)count * words * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
  if (tags) HIPCHK(hipMemcpyAsync(tags, P.tags + first, (size_t)count * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (info2) HIPCHK(hipMemcpyAsync(info2, P.info + 2 * (size_t)first, (size_t)count * 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VLOAM_OK;
}

vloam_status vloam_place_load(vloam_handle* h, const unsigned int* desc_words, const int* tags, int count) {
  static const char* const call = "vloam_place_load";
  if (count < 0) { set_err("%s: negative row count (%d)", call, count); return VLOAM_ERR_INVALID; }
  if (count > 0 && (!desc_words || !tags)) { set_err("%s: null buffer with %d rows", call, count); return VLOAM_ERR_INVALID; }
  TRY(place_admit(call, h));
  PlaceContext& P = h->place;
  if (count == 0) return VLOAM_OK;
  const int bad = place_bad_pad(P.g, desc_words, count);
  if (bad >= 0) { set_err("%s: row %d: a pad byte (ring >= %d) is not zero", call, bad, P.g.R); return VLOAM_ERR_INVALID; }
  if ((long long)P.count + count > P.capacity) { set_err("%s: %d rows do not fit: %d of %d are taken", call, count, P.count, P.capacity); return VLOAM_ERR_CAPACITY; }
  const size_t words = (size_t)P.words();
  std::vector<int> info((size_t)count * 2);
  for (int r = 0; r < count; r++) { info[2 * (size_t)r] = -1; info[2 * (size_t)r + 1] = place_occupied(P.g, desc_words + (size_t)r * words); }
  HIPCHK(hipMemcpyAsync(P.db + (size_t)P.count * words, desc_words, (size_t)count * words * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(P.tags + P.count, tags, (size_t)count * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(P.info + 2 * (size_t)P.count, info.data(), (size_t)count * 2 * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  P.count += count;
  return VLOAM_OK;
}

vloam_status vloam_place_query_device(vloam_handle* h, const vloam_place_query_options* o, const void* d_xyzi4, int n, void* d_matches) {
  static const char* const call = "vloam_place_query_device";
  TRY(place_check_query_options(call, o));
  TRY(place_check_cloud(call, d_xyzi4, n));
  if (!d_matches) { set_err("%s: null result", call); return VLOAM_ERR_INVALID; }
  TRY(place_admit(call, h));
  PlaceContext& P = h->place;
  if (place_describe_enqueue(&P, h->stream, d_xyzi4, n, P.qdesc, P.qinfo, nullptr, 0) != VLOAM_OK ||
      place_match_enqueue(&P, h->stream, P.qdesc, P.qinfo, place_limit(P, o), o->k, d_matches) != VLOAM_OK) return place_launch_failed(call);
  return VLOAM_OK;
}

// the host forms behind their checks: the descriptor is in qdesc / qinfo (or enqueued to get there)
static vloam_status place_query_host(const char* call, vloam_handle* h, const vloam_place_query_options* o, vloam_place_match* matches) {
  PlaceContext& P = h->place;
  if (place_match_enqueue(&P, h->stream, P.qdesc, P.qinfo, place_limit(P, o), o->k, P.qmatch) != VLOAM_OK) {
    (void)hipStreamSynchronize(h->stream);   // the copies in front of it have left the caller's memory
    return place_launch_failed(call);
  }
  HIPCHK(hipMemcpyAsync(matches, P.qmatch, (size_t)o->k * sizeof(vloam_place_match), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return VLOAM_OK;
}

vloam_status vloam_place_query(vloam_handle* h, const vloam_place_query_options* o, const float* xyzi4, int n, vloam_place_match* matches) {
  static const char* const call = "vloam_place_query";
  TRY(place_check_query_options(call, o));
  TRY(place_check_cloud(call, xyzi4, n));
  if (!matches) { set_err("%s: null result", call); return VLOAM_ERR_INVALID; }
  TRY(place_admit(call, h));
  const void* d = nullptr;
  TRY(place_stage(call, h, xyzi4, n, &d));
  if (place_describe_enqueue(&h->place, h->stream, d, n, h->place.qdesc, h->place.qinfo, nullptr, 0) != VLOAM_OK) return place_launch_failed(call);
  return place_query_host(call, h, o, matches);
}

vloam_status vloam_place_query_descriptor(vloam_handle* h, const vloam_place_query_options* o, const unsigned int* desc_words, vloam_place_match* matches) {
  static const char* const call = "vloam_place_query_descriptor";
  TRY(place_check_query_options(call, o));
  if (!desc_words) { set_err("%s: null descriptor", call); return VLOAM_ERR_INVALID; }
  if (!matches) { set_err("%s: null result", call); return VLOAM_ERR_INVALID; }
  TRY(place_admit(call, h));
  PlaceContext& P = h->place;
  if (place_bad_pad(P.g, desc_words, 1) >= 0) { set_err("%s: a pad byte (ring >= %d) is not zero", call, P.g.R); return VLOAM_ERR_INVALID; }
  const int info[2] = {-1, place_occupied(P.g, desc_words)};
  HIPCHK(hipMemcpyAsync(P.qdesc, desc_words, (size_t)P.words() * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(P.qinfo, info, sizeof(info), hipMemcpyHostToDevice, h->stream));
  return place_query_host(call, h, o, matches);
}

// measurement hook (tools/place_probe.py): `repeats` queries back to back, each bracketed by HIP events on the stream
vloam_status vloam_place_time_query(vloam_handle* h, const vloam_place_query_options* o, const unsigned int* desc_words, int repeats, float* ms) {
  static const char* const call = "vloam_place_time_query";
  TRY(place_check_query_options(call, o));
  if (!desc_words || !ms) { set_err("%s: null buffer", call); return VLOAM_ERR_INVALID; }
  if (repeats < 1 || repeats > 1024) { set_err("%s: repeats must be 1 .. 1024, not %d", call, repeats); return VLOAM_ERR_INVALID; }
  TRY(place_admit(call, h));
  PlaceContext& P = h->place;
  if (place_bad_pad(P.g, desc_words, 1) >= 0) { set_err("%s: a pad byte (ring >= %d) is not zero", call, P.g.R); return VLOAM_ERR_INVALID; }
  const int info[2] = {-1, place_occupied(P.g, desc_words)};
  HIPCHK(hipMemcpyAsync(P.qdesc, desc_words, (size_t)P.words() * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(P.qinfo, info, sizeof(info), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  std::vector<hipEvent_t> ev(2 * (size_t)repeats, nullptr);
  bool ok = true;
  for (hipEvent_t& e : ev) ok = ok && hipEventCreate(&e) == hipSuccess;
  for (int r = 0; ok && r < repeats; r++) {
    ok = hipEventRecord(ev[2 * r], h->stream) == hipSuccess && place_match_enqueue(&P, h->stream, P.qdesc, P.qinfo, place_limit(P, o), o->k, P.qmatch) == VLOAM_OK &&
         hipEventRecord(ev[2 * r + 1], h->stream) == hipSuccess;
  }
  ok = hipStreamSynchronize(h->stream) == hipSuccess && ok;
  for (int r = 0; ok && r < repeats; r++) ok = hipEventElapsedTime(&ms[r], ev[2 * r], ev[2 * r + 1]) == hipSuccess;
  if (!ok) set_err("%s: %s", call, hipGetErrorString(hipGetLastError()));
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  return ok ? VLOAM_OK : VLOAM_ERR_HIP;
}

}  // extern "C"
