// Wavefront-wide reductions through DPP row operations and the wavefront's LDS fence, for the scan-registration kernels
// (sr_kernels.hip, sr_ring.hip, sr_ring_long.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace vloam {

__device__ __forceinline__ void lds_fence_wave() {
  // LDS ops of one wavefront retire in order; this only has to stop the compiler from caching or
  // reordering LDS accesses across the point where lanes exchange data.
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// Wavefront-wide unsigned max / min through DPP row operations (no LDS crossbar, a handful of cycles per step): quad swaps,
// row rotations, then the row_bcast15 / row_bcast31 carries of gfx9; the result lands in lane 63 and is broadcast.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_max_step(unsigned v) {
  const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);  // lanes without a source keep 0
  return o > v ? o : v;
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
  v = dpp_max_step<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
  v = dpp_max_step<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
  v = dpp_max_step<0x124, 0xf>(v);  // row_ror:4
  v = dpp_max_step<0x128, 0xf>(v);  // row_ror:8   -> every lane holds the max of its row of 16
  v = dpp_max_step<0x142, 0xa>(v);  // row_bcast15 -> rows 1 and 3 fold in the row below
  v = dpp_max_step<0x143, 0xc>(v);  // row_bcast31 -> rows 2 and 3 fold in lane 31
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) { return ~wave_max_u32(~v); }
// The same steps for f32 min / max (finite values) and an integer sum; lanes without a source combine with themselves (min / max) or 0 (sum).
template <int CTRL, int ROW_MASK, bool MAX>
__device__ __forceinline__ float dpp_fminmax_step(float v) {
  const float o = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
  return MAX ? fmaxf(o, v) : fminf(o, v);
}
template <bool MAX>
__device__ __forceinline__ float wave_fminmax(float v) {
  v = dpp_fminmax_step<0xB1, 0xf, MAX>(v);
  v = dpp_fminmax_step<0x4E, 0xf, MAX>(v);
  v = dpp_fminmax_step<0x124, 0xf, MAX>(v);
  v = dpp_fminmax_step<0x128, 0xf, MAX>(v);
  v = dpp_fminmax_step<0x142, 0xa, MAX>(v);
  v = dpp_fminmax_step<0x143, 0xc, MAX>(v);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_add_step(int v) { return v + __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false); }
__device__ __forceinline__ int wave_sum_i32(int v) {
  v = dpp_add_step<0xB1, 0xf>(v);
  v = dpp_add_step<0x4E, 0xf>(v);
  v = dpp_add_step<0x124, 0xf>(v);
  v = dpp_add_step<0x128, 0xf>(v);
  v = dpp_add_step<0x142, 0xa>(v);
  v = dpp_add_step<0x143, 0xc>(v);
  return __builtin_amdgcn_readlane(v, 63);
}

}  // namespace vloam
