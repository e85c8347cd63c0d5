// Test hook (vloam_debug_probe, c_api.h): the device primitives every stage rests on, called on caller-supplied arguments, one element per
// thread, so that tests/test_gpu_dev_probe.py can hold the DEVICE build of fdlibm_f32.h, tf_dev.h, map_device.h and bitonic.h to the host
// statement of the same text (tests/cpp/dev_probe_host.cpp, NumPy for the __device__-only ones) bit for bit, on arguments no drive produces.
// Built with the default flags of the Makefile (-ffp-contract=off), like sr_kernels.hip.  The kernels call the headers' functions and hold no
// copy of their text; they use plain loads and stores, no atomics, and no LDS outside the sort probe.  A process that never calls the entry
// point launches and allocates nothing here.
#include "vloam_device.h"   // launch geometry (blockIdx / gridDim are the logical coordinates, VL_RAW_LAUNCH), tf_dev.h
#include "fdlibm_f32.h"
#include "map_device.h"
#include "bitonic.h"

namespace vloam {

void set_err(const char* fmt, ...);   // c_api.cpp

constexpr int kProbeThreads = 256;
constexpr int kProbeMaxGrid = 2048;
#define PROBE_LOOP(i, n) for (long long i = (long long)blockIdx.x * kProbeThreads + threadIdx.x; i < (n); i += (long long)gridDim.x * kProbeThreads)

__global__ __launch_bounds__(kProbeThreads) void k_probe_atanf(const float* __restrict__ in, float* __restrict__ out, long long n) {
  PROBE_LOOP(i, n) out[i] = fd_atanf(in[i]);
}
__global__ __launch_bounds__(kProbeThreads) void k_probe_atan2f(const float* __restrict__ in, float* __restrict__ out, long long n) {
  PROBE_LOOP(i, n) out[i] = fd_atan2f(in[2 * i], in[2 * i + 1]);
}
// the elevation of a return as sr_kernels.hip (sr_scan_id) and map_carve.hip (the projection) compute it: the f32 divide and sqrtf are the point
__global__ __launch_bounds__(kProbeThreads) void k_probe_elev(const float* __restrict__ in, float* __restrict__ out, long long n) {
  PROBE_LOOP(i, n) {
    const float x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
    out[i] = fd_atanf(z / sqrtf(x * x + y * y));
  }
}
__global__ __launch_bounds__(kProbeThreads) void k_probe_tf_roundtrip(const double* __restrict__ in, double* __restrict__ out, long long n) {
  PROBE_LOOP(i, n) {
    double q[4], r[4];
    for (int k = 0; k < 4; k++) q[k] = in[4 * i + k];
    TfDev t;
    tf_set_rotation(&t, q);
    tf_get_rotation(t, r);
    for (int k = 0; k < 9; k++) out[13 * i + k] = t.m[k];
    for (int k = 0; k < 4; k++) out[13 * i + 9 + k] = r[k];
  }
}
__global__ __launch_bounds__(kProbeThreads) void k_probe_tf_getrot(const double* __restrict__ in, double* __restrict__ out, long long n) {
  PROBE_LOOP(i, n) {
    TfDev t;
    double r[4];
    for (int k = 0; k < 9; k++) t.m[k] = in[9 * i + k];
    tf_get_rotation(t, r);
    for (int k = 0; k < 4; k++) out[4 * i + k] = r[k];
  }
}
__global__ __launch_bounds__(kProbeThreads) void k_probe_tf_chain(const double* __restrict__ in, double* __restrict__ out, long long n) {
  PROBE_LOOP(i, n) {
    TfDev a, b, bi, r;
    for (int k = 0; k < 9; k++) { a.m[k] = in[24 * i + k]; b.m[k] = in[24 * i + 12 + k]; }
    for (int k = 0; k < 3; k++) { a.o[k] = in[24 * i + 9 + k]; b.o[k] = in[24 * i + 21 + k]; }
    tf_inverse(b, &bi);
    tf_mul(a, bi, &r);
    for (int k = 0; k < 9; k++) out[12 * i + k] = r.m[k];
    for (int k = 0; k < 3; k++) out[12 * i + 9 + k] = r.o[k];
  }
}
constexpr int kProbeAssocIn = 16 + 7 * 8;   // float4 + q[4], t[3] in f64: 72 bytes, so only every other float4 is 16-byte aligned — component loads
__global__ __launch_bounds__(kProbeThreads) void k_probe_assoc(const unsigned char* __restrict__ in, float* __restrict__ out, long long n) {
  PROBE_LOOP(i, n) {
    const float* pf = (const float*)(in + (size_t)i * kProbeAssocIn);
    const double* pd = (const double*)(in + (size_t)i * kProbeAssocIn + 16);
    float4 p;
    p.x = pf[0]; p.y = pf[1]; p.z = pf[2]; p.w = pf[3];
    double q[4], t[3];
    for (int k = 0; k < 4; k++) q[k] = pd[k];
    for (int k = 0; k < 3; k++) t[k] = pd[4 + k];
    const float4 o = associate_to_map(p, q, t);
    out[4 * i] = o.x; out[4 * i + 1] = o.y; out[4 * i + 2] = o.z; out[4 * i + 3] = o.w;
  }
}
__global__ __launch_bounds__(kProbeThreads) void k_probe_quat(const double* __restrict__ in, double* __restrict__ out, long long n) {
  PROBE_LOOP(i, n) {
    double a[4], b[4], v[3], r[4], o[3];
    for (int k = 0; k < 4; k++) { a[k] = in[11 * i + k]; b[k] = in[11 * i + 4 + k]; }
    for (int k = 0; k < 3; k++) v[k] = in[11 * i + 8 + k];
    dquat_mul(a, b, r);
    dquat_rot(a, v, o);
    for (int k = 0; k < 4; k++) out[7 * i + k] = r[k];
    for (int k = 0; k < 3; k++) out[7 * i + 4 + k] = o[k];
  }
}

// The (P2, workgroup size) pairs block_bitonic_sort_u64 is called with today, read off its call sites.  Up to kProbeSortLds keys the callers
// sort in LDS and so does the probe; the long scan-registration tier sorts a ring's keys where they lie in HBM, and so does the probe.
//   T = 256, P2 = 256 .. 4096 (a power of two >= the key count, which is capped at 4096):
//       map_stack.hip k_map_ds_reduce (a bin's keys, kDsBinCap), map_output.hip k_map_pub_sort (a segment's records, kPubLdsKeys),
//       map_cloud_dev.h cloud_order_block (a voxel's point indices, kImportLdsSort: map import and merge);
//       map_stack.hip k_map_ds_bin sorts its 1024 or 2048 samples (ds_num_samples; 256 and 512 samples are ranked by counting)
//   T = 512 (kRingThreads), P2 = 256 .. 4096: sr_ring_long.hip k_sr_ring_long's debug sort of a sector (at most 2729 points of a 16384-point ring)
//   T = 512, P2 = 8192, 16384: sr_ring_long.hip k_sr_ring_long's voxel keys of a ring of 4097 .. 16384 points, in HBM
constexpr int kProbeSortLds = 4096;
struct ProbeSortPair { int P2, T; };
static const ProbeSortPair kProbeSortPairs[] = {
  {256, 256}, {512, 256}, {1024, 256}, {2048, 256}, {4096, 256},
  {256, 512}, {512, 512}, {1024, 512}, {2048, 512}, {4096, 512},
  {8192, 512}, {16384, 512}};

template <int T>
__global__ __launch_bounds__(T) void k_probe_sort(const u64* __restrict__ in, u64* __restrict__ out, int P2, long long nprob) {
  __shared__ u64 a[kProbeSortLds];
  const int tid = threadIdx.x;
  for (long long prob = blockIdx.x; prob < nprob; prob += gridDim.x) {
    const u64* src = in + prob * P2;
    u64* dst = out + prob * P2;
    if (P2 <= kProbeSortLds) {
      for (int e = tid; e < P2; e += T) a[e] = src[e];
      __syncthreads();
      block_bitonic_sort_u64(a, P2, tid, T);
      for (int e = tid; e < P2; e += T) dst[e] = a[e];
      __syncthreads();   // (a[] is no longer read)
    } else {
      for (int e = tid; e < P2; e += T) dst[e] = src[e];
      __syncthreads();
      block_bitonic_sort_u64(dst, P2, tid, T);
    }
  }
}

namespace {
struct ProbeBuffers {   // what a call allocates, released on every way out
  void* d_in = nullptr;
  void* d_out = nullptr;
  hipStream_t st = nullptr;
  ~ProbeBuffers() {
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (st) (void)hipStreamDestroy(st);
  }
};
}  // namespace

}  // namespace vloam

using namespace vloam;

#define PROBE_HIPCHK(expr)                                                                    \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);     \
      return VLOAM_ERR_HIP;                                                                   \
    }                                                                                         \
  } while (0)

vloam_status vloam_debug_probe(int device, int which, const void* in, long long n, void* out, long long out_bytes) {
  long long in_elem = 0, out_elem = 0;
  int sort_p2 = 0, sort_t = 0;
  switch (which) {
    case VLOAM_PROBE_ATANF: in_elem = 4; out_elem = 4; break;
    case VLOAM_PROBE_ATAN2F: in_elem = 8; out_elem = 4; break;
    case VLOAM_PROBE_ELEV: in_elem = 12; out_elem = 4; break;
    case VLOAM_PROBE_TF_ROUNDTRIP: in_elem = 4 * 8; out_elem = 13 * 8; break;
    case VLOAM_PROBE_TF_GETROT: in_elem = 9 * 8; out_elem = 4 * 8; break;
    case VLOAM_PROBE_TF_CHAIN: in_elem = 24 * 8; out_elem = 12 * 8; break;
    case VLOAM_PROBE_ASSOC: in_elem = kProbeAssocIn; out_elem = 16; break;
    case VLOAM_PROBE_QUAT: in_elem = 11 * 8; out_elem = 7 * 8; break;
    default:
      for (const ProbeSortPair& p : kProbeSortPairs)
        if (which == VLOAM_PROBE_SORT(p.P2, p.T)) { sort_p2 = p.P2; sort_t = p.T; in_elem = out_elem = 8; }
      if (!sort_p2) { set_err("vloam_debug_probe: unknown probe %d", which); return VLOAM_ERR_INVALID; }
  }
  if (n < 0 || n > (1ll << 28)) { set_err("vloam_debug_probe: n = %lld (0 .. 2^28 elements)", n); return VLOAM_ERR_INVALID; }
  if (out_bytes != n * out_elem) { set_err("vloam_debug_probe: out_bytes = %lld, the probe writes %lld bytes for %lld elements", out_bytes, n * out_elem, n); return VLOAM_ERR_INVALID; }
  if (sort_p2 && n % sort_p2 != 0) { set_err("vloam_debug_probe: %lld keys are no whole number of problems of %d keys", n, sort_p2); return VLOAM_ERR_INVALID; }
  if (n > 0 && (!in || !out)) { set_err("vloam_debug_probe: null buffer"); return VLOAM_ERR_INVALID; }
  if (n == 0) return VLOAM_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_err("no HIP device visible: libvloam_hip has no CPU fallback"); return VLOAM_ERR_NO_DEVICE; }
  if (device < 0 || device >= ndev) { set_err("device %d out of range (%d visible)", device, ndev); return VLOAM_ERR_NO_DEVICE; }
  PROBE_HIPCHK(hipSetDevice(device));
  ProbeBuffers B;
  PROBE_HIPCHK(hipStreamCreate(&B.st));
  PROBE_HIPCHK(hipMalloc(&B.d_in, (size_t)(n * in_elem)));
  PROBE_HIPCHK(hipMalloc(&B.d_out, (size_t)(n * out_elem)));
  PROBE_HIPCHK(hipMemcpyAsync(B.d_in, in, (size_t)(n * in_elem), hipMemcpyHostToDevice, B.st));
  const long long blocks = (n + kProbeThreads - 1) / kProbeThreads;
  const dim3 grid((unsigned)(blocks < kProbeMaxGrid ? blocks : kProbeMaxGrid), 1, 1), block(kProbeThreads);
  switch (which) {
    case VLOAM_PROBE_ATANF: VL_RAW_LAUNCH(k_probe_atanf, grid, block, 0, B.st, (const float*)B.d_in, (float*)B.d_out, n); break;
    case VLOAM_PROBE_ATAN2F: VL_RAW_LAUNCH(k_probe_atan2f, grid, block, 0, B.st, (const float*)B.d_in, (float*)B.d_out, n); break;
    case VLOAM_PROBE_ELEV: VL_RAW_LAUNCH(k_probe_elev, grid, block, 0, B.st, (const float*)B.d_in, (float*)B.d_out, n); break;
    case VLOAM_PROBE_TF_ROUNDTRIP: VL_RAW_LAUNCH(k_probe_tf_roundtrip, grid, block, 0, B.st, (const double*)B.d_in, (double*)B.d_out, n); break;
    case VLOAM_PROBE_TF_GETROT: VL_RAW_LAUNCH(k_probe_tf_getrot, grid, block, 0, B.st, (const double*)B.d_in, (double*)B.d_out, n); break;
    case VLOAM_PROBE_TF_CHAIN: VL_RAW_LAUNCH(k_probe_tf_chain, grid, block, 0, B.st, (const double*)B.d_in, (double*)B.d_out, n); break;
    case VLOAM_PROBE_ASSOC: VL_RAW_LAUNCH(k_probe_assoc, grid, block, 0, B.st, (const unsigned char*)B.d_in, (float*)B.d_out, n); break;
    case VLOAM_PROBE_QUAT: VL_RAW_LAUNCH(k_probe_quat, grid, block, 0, B.st, (const double*)B.d_in, (double*)B.d_out, n); break;
    default: {
      const long long nprob = n / sort_p2;
      const dim3 sgrid((unsigned)(nprob < kProbeMaxGrid ? nprob : kProbeMaxGrid), 1, 1);
      if (sort_t == 256) VL_RAW_LAUNCH(k_probe_sort<256>, sgrid, dim3(256), 0, B.st, (const u64*)B.d_in, (u64*)B.d_out, sort_p2, nprob);
      else VL_RAW_LAUNCH(k_probe_sort<512>, sgrid, dim3(512), 0, B.st, (const u64*)B.d_in, (u64*)B.d_out, sort_p2, nprob);
    }
  }
  PROBE_HIPCHK(hipGetLastError());
  PROBE_HIPCHK(hipMemcpyAsync(out, B.d_out, (size_t)(n * out_elem), hipMemcpyDeviceToHost, B.st));
  PROBE_HIPCHK(hipStreamSynchronize(B.st));
  return VLOAM_OK;
}
