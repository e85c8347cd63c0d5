// Place recognition (place.hip: the kernels and their launch code; capi_place.cpp: the ABI side): what a handle holds once vloam_place_enable
// has been called, and nothing before.  Every buffer is an allocation of its own, outside the session arenas.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/vloam_hip/c_api.h"

namespace vloam {

constexpr int kPlaceMaxRing = 32, kPlaceMaxSector = 120, kPlaceMaxCells = kPlaceMaxRing * kPlaceMaxSector, kPlaceMaxK = 8;
constexpr int kPlaceMaxRows = 1 << 20, kPlaceMaxPoints = 1 << 24;

// the descriptor's geometry as the kernels take it: every derived f32 value is computed once on the host (c_api.h: the specification)
struct PlaceGeom {
  int R, S, W;                  // rings, sectors, words per sector = ceil(R / 4)
  float min2, max2;             // f32 squares of the two ranges
  float z_min, z_step;
  float k_sector;               // (float)S / (2 * PI_F)
  float edge2[kPlaceMaxRing];   // [i]: the f32 square of (float)((float)i * (max_range / (float)R)); [0] unused
};

struct PlaceContext {
  bool enabled = false;
  PlaceGeom g{};
  int capacity = 0, count = 0;           // rows; count is the host's: a row exists once its append has been enqueued
  unsigned* db = nullptr;                // [capacity][S * W]
  int* tags = nullptr;                   // [capacity]
  int* info = nullptr;                   // [capacity][2]: n_used, n_occupied
  unsigned long long* best = nullptr;    // [capacity]: (dist << 32) | shift of the last query, per row
  int* cells = nullptr;                  // [kPlaceMaxCells + 1]: the cell maxima of the cloud being described, then n_used
  unsigned* qdesc = nullptr;             // [S * W] the query's descriptor
  int* qinfo = nullptr;                  // [2]
  vloam_place_match* qmatch = nullptr;   // [kPlaceMaxK] the host forms' records
  float4* cloud = nullptr;               // the host forms' copy of the cloud, grown on demand
  int cloud_cap = 0;
  int words() const { return g.S * g.W; }
};

// Enqueue only, on `st`.  d_pts: n packed float4 (sensor frame); d_desc: S * W words; d_info: 2 ints; d_tag: null, or where `tag` is written.
vloam_status place_describe_enqueue(PlaceContext* p, hipStream_t st, const void* d_pts, int n, void* d_desc, void* d_info, int* d_tag, int tag);
// rows 0 .. limit - 1 against the descriptor at d_qdesc (its info at d_qinfo); d_out: k records
vloam_status place_match_enqueue(PlaceContext* p, hipStream_t st, const void* d_qdesc, const void* d_qinfo, int limit, int k, void* d_out);

}  // namespace vloam
