// The per-element AdamW / Adam-L2 update and the element loads / stores of the
// flat optimizer kernels: shared by optim.hip (fp32 moments: flat update and
// deferred-state replay) and optim_qflat.hip (block-quantized moments), so the
// three kernels cannot drift apart.
#pragma once
#include "dw_common.h"

template <typename T> __device__ __forceinline__ float ld(const T* p, int64_t i);
template <> __device__ __forceinline__ float ld<float>(const float* p, int64_t i) { return p[i]; }
template <> __device__ __forceinline__ float ld<bf16_t>(const bf16_t* p, int64_t i) { return bf2f(p[i]); }
template <typename T> __device__ __forceinline__ void st(T* p, int64_t i, float v);
template <> __device__ __forceinline__ void st<float>(float* p, int64_t i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void st<bf16_t>(bf16_t* p, int64_t i, float v) { p[i] = f2bf(v); }

// load 8 consecutive elements (i multiple of 8) as floats
template <typename T> __device__ __forceinline__ void ld8(const T* p, int64_t i, float* f);
template <> __device__ __forceinline__ void ld8<bf16_t>(const bf16_t* p, int64_t i, float* f) {
  u32x4 v = *(const u32x4*)(p + i);
  unpack8(v, f);
}
template <> __device__ __forceinline__ void ld8<float>(const float* p, int64_t i, float* f) {
  f32x4 a = *(const f32x4*)(p + i), b = *(const f32x4*)(p + i + 4);
  f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3];
  f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
}
template <typename T> __device__ __forceinline__ void st8(T* p, int64_t i, const float* f);
template <> __device__ __forceinline__ void st8<bf16_t>(bf16_t* p, int64_t i, const float* f) {
  *(u32x4*)(p + i) = pack8(f);
}
template <> __device__ __forceinline__ void st8<float>(float* p, int64_t i, const float* f) {
  f32x4 a = {f[0], f[1], f[2], f[3]}, b = {f[4], f[5], f[6], f[7]};
  *(f32x4*)(p + i) = a;
  *(f32x4*)(p + i + 4) = b;
}

// Weight-decay selection: decay_mask (one byte per 64-element block; flat
// buffers align every parameter to 64 elements) when non-null, else the
// prefix [0, n_decay).
struct AdamArgs {
  float lr, beta1, beta2, eps, wd, bc1, bc2;  // bc = 1 - beta^t
  int64_t n, n_decay;
  int adamw;  // 1: decoupled weight decay, 0: L2 added to the gradient
  const unsigned char* decay_mask;
};

__device__ __forceinline__ bool decays(const unsigned char* mask, int64_t n_decay, int64_t i) {
  return mask ? (mask[i >> 6] != 0) : (i < n_decay);
}

// One AdamW / Adam-L2 update of one element -- shared by the flat update, the
// deferred-state replay and the quantized-moment flat update, so all of them
// produce bit-identical results from the same fp32 inputs.
__device__ __forceinline__ void adam_elem(float g, float gs, bool decay, const AdamArgs& a, float step_size,
                                          float rbc2, float& w, float& mm, float& vv) {
  // Every multiply-add is an explicit fma and no product feeds an add: the
  // library builds with -ffp-contract=fast, and the backend contracts the
  // packed-fp32 code of the vectorised flat update differently from the
  // scalar replay loop (1-ulp master differences on GPU).  With nothing left
  // to contract both kernels round identically.
  float gk = g * gs;
  if (!a.adamw && decay) gk = __builtin_fmaf(a.wd, w, gk);
  mm = __builtin_fmaf(a.beta1, mm, (1.f - a.beta1) * gk);
  vv = __builtin_fmaf(a.beta2, vv, (1.f - a.beta2) * gk * gk);
  const float denom = __builtin_fmaf(sqrtf(vv), rbc2, a.eps);
  if (a.adamw && decay) w = __builtin_fmaf(-(a.lr * a.wd), w, w);
  w = w - (step_size * mm) / denom;
}
