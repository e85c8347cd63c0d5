// The host statement of the device probes (csrc/dev_probe.hip, vloam_debug_probe): the same headers — fdlibm_f32.h, tf_dev.h — compiled by the
// host compiler with -ffp-contract=off, run over a binary argument file in the probe's element layout (include/vloam_hip/c_api.h).
// tests/test_dev_probe_host.py ties this program to tests/fdlibm_np.py, kitti_io's tf2 model and an np.longdouble evaluation;
// tests/test_gpu_dev_probe.py compares the device with it bit for bit.
//   dev_probe_host <atanf|atan2f|elev|tf_roundtrip|tf_getrot|tf_chain> <in.bin> <out.bin>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "fdlibm_f32.h"
#include "tf_dev.h"

using namespace vloam;

template <class T>
static bool read_all(const char* path, std::vector<T>* v) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  v->resize((size_t)bytes / sizeof(T));
  const bool ok = bytes % (long)sizeof(T) == 0 && fread(v->data(), 1, (size_t)bytes, f) == (size_t)bytes;
  fclose(f);
  return ok;
}
template <class T>
static bool write_all(const char* path, const std::vector<T>& v) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
  return fclose(f) == 0 && ok;
}

template <class T, class F>
static int run(const char* in_path, const char* out_path, size_t n_in, size_t n_out, F body) {
  std::vector<T> in, out;
  if (!read_all(in_path, &in) || in.size() % n_in != 0) { fprintf(stderr, "dev_probe_host: cannot read whole elements from %s\n", in_path); return 2; }
  const size_t n = in.size() / n_in;
  out.resize(n * n_out);
  for (size_t i = 0; i < n; i++) body(&in[i * n_in], &out[i * n_out]);
  if (!write_all(out_path, out)) { fprintf(stderr, "dev_probe_host: cannot write %s\n", out_path); return 2; }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: dev_probe_host <probe> <in.bin> <out.bin>\n"); return 2; }
  const char* w = argv[1];
  if (!strcmp(w, "atanf")) return run<float>(argv[2], argv[3], 1, 1, [](const float* a, float* o) { o[0] = fd_atanf(a[0]); });
  if (!strcmp(w, "atan2f")) return run<float>(argv[2], argv[3], 2, 1, [](const float* a, float* o) { o[0] = fd_atan2f(a[0], a[1]); });
  if (!strcmp(w, "elev"))
    return run<float>(argv[2], argv[3], 3, 1, [](const float* a, float* o) {
      const float x = a[0], y = a[1], z = a[2];
      o[0] = fd_atanf(z / sqrtf(x * x + y * y));
    });
  if (!strcmp(w, "tf_roundtrip"))
    return run<double>(argv[2], argv[3], 4, 13, [](const double* a, double* o) {
      TfDev t;
      tf_set_rotation(&t, a);
      tf_get_rotation(t, o + 9);
      for (int k = 0; k < 9; k++) o[k] = t.m[k];
    });
  if (!strcmp(w, "tf_getrot"))
    return run<double>(argv[2], argv[3], 9, 4, [](const double* a, double* o) {
      TfDev t;
      for (int k = 0; k < 9; k++) t.m[k] = a[k];
      tf_get_rotation(t, o);
    });
  if (!strcmp(w, "tf_chain"))
    return run<double>(argv[2], argv[3], 24, 12, [](const double* a, double* o) {
      TfDev ta, tb, bi, r;
      for (int k = 0; k < 9; k++) { ta.m[k] = a[k]; tb.m[k] = a[12 + k]; }
      for (int k = 0; k < 3; k++) { ta.o[k] = a[9 + k]; tb.o[k] = a[21 + k]; }
      tf_inverse(tb, &bi);
      tf_mul(ta, bi, &r);
      for (int k = 0; k < 9; k++) o[k] = r.m[k];
      for (int k = 0; k < 3; k++) o[9 + k] = r.o[k];
    });
  fprintf(stderr, "dev_probe_host: unknown probe %s\n", w);
  return 2;
}
