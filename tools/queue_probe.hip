// Which hardware queue does each HIP stream get?  Every launch is tagged by its kernel name; run it under the kernel tracer and read the
// stream -> queue map with tools/queue_map.py (profiles/r07_hw_queue_map.txt):
//   hipcc --offload-arch=gfx950 -O2 -o queue_probe tools/queue_probe.hip
//   rocprofv3 --kernel-trace --output-format csv -d OUT -- ./queue_probe [plain | created_only] && python tools/queue_map.py OUT
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
template <int ID> __global__ void k_tag(int* p) { if (threadIdx.x == 0) p[ID] = ID; }
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "plain";
  int* d = nullptr;
  CK(hipMalloc(&d, 64 * sizeof(int)));
  int h[64] = {};
  CK(hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice));            // null stream / sync copy first (as torch's .to(cuda) does)
  int lo = 0, hi = 0;
  CK(hipDeviceGetStreamPriorityRange(&lo, &hi));
  printf("priority range: least %d greatest %d\n", lo, hi);
  hipStream_t s[12] = {};
  if (!strcmp(mode, "plain")) {
    // six normal streams created in order 0..5, first used in REVERSE order: creation or first use decides?
    for (int i = 0; i < 6; i++) CK(hipStreamCreateWithFlags(&s[i], hipStreamNonBlocking));
    hipLaunchKernelGGL(k_tag<5>, dim3(1), dim3(64), 0, s[5], d);
    hipLaunchKernelGGL(k_tag<4>, dim3(1), dim3(64), 0, s[4], d);
    hipLaunchKernelGGL(k_tag<3>, dim3(1), dim3(64), 0, s[3], d);
    hipLaunchKernelGGL(k_tag<2>, dim3(1), dim3(64), 0, s[2], d);
    hipLaunchKernelGGL(k_tag<1>, dim3(1), dim3(64), 0, s[1], d);
    hipLaunchKernelGGL(k_tag<0>, dim3(1), dim3(64), 0, s[0], d);
    hipLaunchKernelGGL(k_tag<20>, dim3(1), dim3(64), 0, nullptr, d);   // null stream
    // priorities: separate pools?
    CK(hipStreamCreateWithPriority(&s[6], hipStreamNonBlocking, hi));
    CK(hipStreamCreateWithPriority(&s[7], hipStreamNonBlocking, hi));
    CK(hipStreamCreateWithPriority(&s[8], hipStreamNonBlocking, lo));
    hipLaunchKernelGGL(k_tag<6>, dim3(1), dim3(64), 0, s[6], d);
    hipLaunchKernelGGL(k_tag<7>, dim3(1), dim3(64), 0, s[7], d);
    hipLaunchKernelGGL(k_tag<8>, dim3(1), dim3(64), 0, s[8], d);
    // a full CU mask
    uint32_t mask[8];
    for (int w = 0; w < 8; w++) mask[w] = 0xffffffffu;
    CK(hipExtStreamCreateWithCUMask(&s[9], 8, mask));
    hipLaunchKernelGGL(k_tag<9>, dim3(1), dim3(64), 0, s[9], d);
    // destroy stream 5, create a new one: does it reuse the freed slot?
    CK(hipStreamSynchronize(s[5]));
    CK(hipStreamDestroy(s[5]));
    CK(hipStreamCreateWithFlags(&s[10], hipStreamNonBlocking));
    hipLaunchKernelGGL(k_tag<10>, dim3(1), dim3(64), 0, s[10], d);
    s[5] = nullptr;
  } else {
    // "created_only": create three streams and never use the first two; then one more that is used
    for (int i = 0; i < 3; i++) CK(hipStreamCreateWithFlags(&s[i], hipStreamNonBlocking));
    hipLaunchKernelGGL(k_tag<2>, dim3(1), dim3(64), 0, s[2], d);
    hipLaunchKernelGGL(k_tag<20>, dim3(1), dim3(64), 0, nullptr, d);
    for (int i = 3; i < 7; i++) { CK(hipStreamCreateWithFlags(&s[i], hipStreamNonBlocking)); }
    hipLaunchKernelGGL(k_tag<3>, dim3(1), dim3(64), 0, s[3], d);
    hipLaunchKernelGGL(k_tag<4>, dim3(1), dim3(64), 0, s[4], d);
    hipLaunchKernelGGL(k_tag<5>, dim3(1), dim3(64), 0, s[5], d);
    hipLaunchKernelGGL(k_tag<6>, dim3(1), dim3(64), 0, s[6], d);
    hipLaunchKernelGGL(k_tag<0>, dim3(1), dim3(64), 0, s[0], d);
  }
  CK(hipDeviceSynchronize());
  for (int i = 0; i < 12; i++) if (s[i]) CK(hipStreamDestroy(s[i]));
  CK(hipFree(d));
  printf("probe %s done\n", mode);
  return 0;
}
