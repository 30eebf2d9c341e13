// Group-wise 4-/8-bit codec of the low-bit optimizers (groups of 128
// consecutive elements, one fp32 scale each), shared by optim_lowbit.hip
// (per-tensor Q_AdamW) and optim_qflat.hip (flat FusedQAdamW).  The maps are
// described in the header of optim_lowbit.hip; optimizers/low_bit.py holds
// the same codec in PyTorch.
#pragma once
#include "dw_common.h"

static __constant__ float kM4[16] = {0.f, 0.015625f, 0.0625f, 0.125f, 0.25f, 0.5f, 0.75f, 1.f,
                                     0.f, -0.015625f, -0.0625f, -0.125f, -0.25f, -0.5f, -0.75f, -1.f};

__device__ __forceinline__ int quant_m4(float x) {  // x in [-1, 1] -> nearest code
  const float a = fabsf(x);
  // k = how many of the midpoints of {0, 1/64, 1/16, 1/8, 1/4, 1/2, 3/4, 1} lie below a:
  // {1/128, 5/128, 3/32, 3/16, 3/8, 5/8, 7/8}, found by bisection (3 compares instead of 7)
  const bool b2 = a > 0.1875f;
  const bool b1 = a > (b2 ? 0.625f : 0.0390625f);
  const bool b0 = a > (b2 ? (b1 ? 0.875f : 0.375f) : (b1 ? 0.09375f : 0.0078125f));
  const int k = (b2 ? 4 : 0) + (b1 ? 2 : 0) + (b0 ? 1 : 0);
  return (x < 0.f && k > 0) ? (k | 8) : k;
}

template <int BITS>
__device__ __forceinline__ float deq_m(int code, float scale) {
  if constexpr (BITS == 4) return kM4[code] * scale;
  else return (float)((signed char)code) * (scale / 127.f);
}
template <int BITS>
__device__ __forceinline__ int q_m(float x, float inv_scale) {
  if constexpr (BITS == 4) return quant_m4(x * inv_scale);
  else {
    int q = __float2int_rn(x * inv_scale * 127.f);
    return (q < -127 ? -127 : (q > 127 ? 127 : q)) & 0xff;
  }
}
template <int BITS>
__device__ __forceinline__ float deq_v(int code, float scale) {
  constexpr float L = (BITS == 4) ? 16.f : 256.f;
  const float r = (float)(code + 1) / L;
  return r * r * scale;
}
template <int BITS>
__device__ __forceinline__ int q_v(float v, float scale) {  // smallest level >= (v rounded in sqrt space)
  constexpr int L = (BITS == 4) ? 16 : 256;
  if (scale <= 0.f) return 0;
  int k = __float2int_rn(sqrtf(v / scale) * (float)L) - 1;
  return k < 0 ? 0 : (k > L - 1 ? L - 1 : k);
}

// q_v from sqrt(v): k = rn(sqrt(v) * (L / sqrt(scale))) - 1 is the q_v map with
// one division and one square root per GROUP (v_levels_per_sqrt) instead of
// per element, for a kernel that has sqrt(v) at hand.  sqrt(v) / sqrt(scale)
// and sqrt(v / scale) differ in the last bit, so a code right at a rounding
// boundary can come out one level off q_v's (a few per million).
template <int BITS>
__device__ __forceinline__ float v_levels_per_sqrt(float scale) {
  constexpr float L = (BITS == 4) ? 16.f : 256.f;
  return scale > 0.f ? L / sqrtf(scale) : 0.f;
}
template <int BITS>
__device__ __forceinline__ int q_v_sqrt(float sqrt_v, float levels_per_sqrt) {
  constexpr int L = (BITS == 4) ? 16 : 256;
  int k = __float2int_rn(sqrt_v * levels_per_sqrt) - 1;  // scale 0: levels_per_sqrt 0 -> code 0
  return k < 0 ? 0 : (k > L - 1 ? L - 1 : k);
}
