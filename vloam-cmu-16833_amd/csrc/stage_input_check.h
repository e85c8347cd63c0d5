// Admission rule of the clouds a caller hands to vloam_set_odometry_input / vloam_set_mapping_input (host only, no HIP: tests compile it
// on its own with g++, tests/cpp/stage_input_check.cpp).
//
// The odometry kernels do not walk the less-clouds the way the reference does.  The reference walks outwards from the closest point's own
// index and breaks at the first point whose line lies outside r +- NEARBY_SCAN (laser_odometry.cpp:294-324,371-428; r = int(intensity) of
// the closest point, NEARBY_SCAN = 2.5).  The device bounds the walk by two stops per line that do not depend on the index: the FIRST index
// of the cloud whose line is >= r + 3 and the LAST whose line is <= r - 3 (k_lo_grid_scan in lo_kernels.hip).  The two agree for every
// index exactly when no point comes before a point whose line is 3 or more below its own: max_{i<j} L[i] - L[j] <= 2.  Scan registration's
// clouds keep this (their lines ascend up to the r / r - 1 jitter of int(intensity)); a substituted cloud that breaks it is refused.
//   rule 1 (every cloud): all four floats of every point are finite (int(NaN) is undefined in the reference)
//   rule 2 (walked clouds): L = int(intensity) lies in [0, kStageLines) (the stop tables are indexed by line)
//   rule 3 (walked clouds): L[j] >= max_{i<j} L[i] - 2 (one pass, running maximum)
// The rule is conservative: some orders that break rule 3 still walk the same way in the reference (no walk that reaches the inversion
// breaks differently because of it), and they are refused all the same.
#pragma once
#include <math.h>

namespace vloam_stage_check {

constexpr int kStageLines = 64;   // == kMaxRings: lines the walk-stop tables hold
constexpr int kMaxInversion = 2;  // NEARBY_SCAN = 2.5 on integer lines

enum Rule { kOk = 0, kNonFinite = 1, kLineRange = 2, kLineOrder = 3 };

struct Fault {
  int rule = kOk;      // Rule
  int point = -1;      // index of the first point that breaks it
  float value = 0.f;   // its intensity
  int max_line = -1;   // the largest line before it (rule 3)
};

// xyzi: n packed (x, y, z, intensity) floats.  walked: the cloud is one of the two less-clouds, which the next sweep's odometry walks by
// scan line (rules 2 and 3 apply).  Returns the first fault in index order; at one point rule 1 is checked before 2, and 2 before 3.
inline Fault check_cloud(const float* xyzi, int n, bool walked) {
  Fault f;
  int max_line = -1;
  for (int i = 0; i < n; i++) {
    const float* p = xyzi + 4 * (long long)i;
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(p[3]))) { f.rule = kNonFinite; f.point = i; f.value = p[3]; return f; }
    if (!walked) continue;
    // int() truncates towards zero: int(x) is in [0, kStageLines) exactly for x in (-1, kStageLines).  Compared as a float first: the
    // conversion is only defined for values that fit an int.
    if (!(p[3] > -1.0f && p[3] < (float)kStageLines)) { f.rule = kLineRange; f.point = i; f.value = p[3]; return f; }
    const int line = (int)p[3];
    if (max_line - line > kMaxInversion) { f.rule = kLineOrder; f.point = i; f.value = p[3]; f.max_line = max_line; return f; }
    if (line > max_line) max_line = line;
  }
  return f;
}

inline const char* rule_text(int rule) {
  switch (rule) {
    case kNonFinite: return "a coordinate or the intensity is not finite";
    case kLineRange: return "int(intensity) lies outside [0, 64)";
    case kLineOrder: return "int(intensity) lies more than 2 lines below the largest line before it (the rule is max_{i<j} L[i] - L[j] <= 2)";
    default: return "ok";
  }
}

}  // namespace vloam_stage_check
