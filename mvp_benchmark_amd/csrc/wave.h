// Wave64 reductions and the workgroup scan shared by the geometry and pointwise kernels (gfx950).
// (The EMD kernels keep their own copies of these idioms: their register allocation is tuned per kernel.)
#pragma once
#include <hip/hip_runtime.h>

namespace mvp {

// max(v, v as permuted by the DPP control CTRL): ONE DPP-fused v_max per step.  Lanes a row mask leaves unwritten
// combine with the identity -- 0 for unsigned, the lane's own value for float.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_max(unsigned v) {
  const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, false);
  return o > v ? o : v;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_max(float v) {
  const float o = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
  return __builtin_fmaxf(v, o);
}
__device__ __forceinline__ unsigned read_lane(unsigned v, int l) { return (unsigned)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ float read_lane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// The six steps of a wave64 maximum with DPP row operations only, in three stages.
// row16_max: a butterfly inside the rows of 16 -- every lane of a row gets the row's maximum.
template <typename T>
__device__ __forceinline__ T row16_max(T v) {
  v = dpp_max<0xB1, 0xF>(v);   // quad_perm [1,0,3,2]
  v = dpp_max<0x4E, 0xF>(v);   // quad_perm [2,3,0,1]
  v = dpp_max<0x141, 0xF>(v);  // row_half_mirror
  v = dpp_max<0x140, 0xF>(v);  // row_mirror
  return v;
}
// half32_max: lanes 31 and 63 hold the maximum of lanes 0..31 / 32..63.
template <typename T>
__device__ __forceinline__ T half32_max(T v) {
  return dpp_max<0x142, 0xA>(row16_max(v));  // row_bcast15 -> rows 1, 3
}
// wave_max: the maximum of all 64 lanes, wave-uniform (taken from lane 63).
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
  return read_lane(dpp_max<0x143, 0xC>(half32_max(v)), 63);  // row_bcast31 -> rows 2, 3
}

// v + (v as permuted by the DPP control CTRL): ONE DPP-fused v_add per step (a double's two halves travel separately); a
// lane a row mask leaves unwritten adds 0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
__device__ __forceinline__ double double_of(unsigned lo, unsigned hi) {
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add(double v) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, ROW_MASK, 0xF, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xF, false);
  return v + double_of(lo, hi);
}
__device__ __forceinline__ double read_lane(double v, int l) {
  const long long b = __double_as_longlong(v);
  return double_of(read_lane((unsigned)b, l), read_lane((unsigned)(b >> 32), l));
}
// wave_sum: the sum of all 64 lanes (float or double), wave-uniform (taken from lane 63), in the six steps of wave_max: a
// butterfly inside the rows of 16 (both operands of every step are the same pair of partial sums, so the lanes of a row
// agree bit for bit), then row 0 into row 1 and row 2 into row 3, then the lower half into the upper.  A fixed tree: the
// same bits on every run; a NaN or an Inf in any lane reaches the result.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  v = dpp_add<0xB1, 0xF>(v);   // quad_perm [1,0,3,2]
  v = dpp_add<0x4E, 0xF>(v);   // quad_perm [2,3,0,1]
  v = dpp_add<0x141, 0xF>(v);  // row_half_mirror
  v = dpp_add<0x140, 0xF>(v);  // row_mirror
  v = dpp_add<0x142, 0xA>(v);  // row_bcast15 -> rows 1, 3
  v = dpp_add<0x143, 0xC>(v);  // row_bcast31 -> rows 2, 3
  return read_lane(v, 63);
}

// Axis-aligned box of the wave's 64 per-lane boxes, in every lane.
__device__ __forceinline__ void wave_box(float (&lo)[3], float (&hi)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      lo[a] = __builtin_fminf(lo[a], __shfl_xor(lo[a], off, 64));
      hi[a] = __builtin_fmaxf(hi[a], __shfl_xor(hi[a], off, 64));
    }
  }
}

// Exclusive prefix sum over the workgroup's threads of one int each.  s_wsum: one int of LDS per wave; holds one
// workgroup barrier, so every thread calls it.
__device__ __forceinline__ int block_exclusive_sum(int v, int *s_wsum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  if (lane == 63) s_wsum[wave] = incl;
  __syncthreads();
  int base = incl - v;
  for (int w = 0; w < wave; ++w) base += s_wsum[w];
  return base;
}

}  // namespace mvp
