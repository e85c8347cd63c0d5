// Test program: the admission rule of vloam_set_odometry_input / vloam_set_mapping_input (csrc/stage_input_check.h), compiled on its own
// (no HIP).  Reads cases from a file and prints one line per case: "<rule> <point> <max_line>".
//   file: int32 n_cases, then per case int32 n, int32 walked, float32[n][4]
#include <cstdio>
#include <vector>
#include "stage_input_check.h"

int main(int argc, char** argv) {
  if (argc < 2) return 64;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 65;
  int n_cases = 0;
  if (std::fread(&n_cases, sizeof(int), 1, f) != 1) return 2;
  std::vector<float> pts;
  for (int c = 0; c < n_cases; c++) {
    int hdr[2];
    if (std::fread(hdr, sizeof(int), 2, f) != 2 || hdr[0] < 0) return 2;
    pts.resize(4 * (size_t)hdr[0] + 1);
    if (std::fread(pts.data(), sizeof(float), 4 * (size_t)hdr[0], f) != 4 * (size_t)hdr[0]) return 2;
    const vloam_stage_check::Fault r = vloam_stage_check::check_cloud(pts.data(), hdr[0], hdr[1] != 0);
    std::printf("%d %d %d\n", r.rule, r.point, r.max_line);
  }
  std::fclose(f);
  return 0;
}
