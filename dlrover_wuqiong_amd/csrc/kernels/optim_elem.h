// What the optimizer kernels share, so that no two of them can drift apart:
// the element loads / stores, the per-element AdamW / Adam-L2 update
// (adam_elem) and AGD update (agd_elem), and the one dispatcher from
// (param_dtype, grad_dtype) codes to element types.  Used by
//   optim.hip        adam_flat_kernel, adam_replay_kernel, agd_flat_kernel
//                    (+ the loads / stores of sumsq_kernel and scale_kernel),
//   optim_multi.hip  mt_step_kernel (Adam and AGD), mt_sumsq_kernel,
//   optim_qflat.hip  qadam_flat_kernel (block-quantized moments),
//   optim_lowbit.hip qadamw_kernel (loads / stores and dispatch only: its
//                    update is the reference's Q_AdamW formula).
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

// The only place that maps dtype codes (0 fp32, 1 bf16: ops/_hip.py
// dtype_code) to element types: launch(P{}, G{}) is called with values of the
// parameter and gradient element types and returns the launch's error.  An
// unknown code is an error, and so is a bf16 parameter without an fp32 master
// (launchers whose kernel takes no master pass has_master = true).
template <typename F>
static inline int dispatch_dtypes(int param_dtype, int grad_dtype, bool has_master, F&& launch) {
  if ((param_dtype | grad_dtype) & ~1) return (int)hipErrorInvalidValue;
  if (param_dtype == 1 && !has_master) return (int)hipErrorInvalidValue;
  if (param_dtype == 1) return grad_dtype == 1 ? launch(bf16_t{}, bf16_t{}) : launch(bf16_t{}, float{});
  return grad_dtype == 1 ? launch(float{}, bf16_t{}) : launch(float{}, float{});
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

// AGD (Auto-switchable optimizer with stepwise Gradient Difference, NeurIPS'23):
// the update of reference atorch/atorch/optimizers/agd.py:84-150 (decoupled,
// non-fixed decay; no amsgrad/win - those run the python path):
//   w   *= 1 - lr*wd                                   (decay params only)
//   m_t  = b1 m + (1-b1) g
//   s    = m_t/bc1_t - m_{t-1}/bc1_{t-1}   (s = m_t/bc1_t at t == 1)
//   v_t  = b2 v + (1-b2) s^2
//   upd  = m_t / max(sqrt(v_t), delta*sqrt(bc2_t)) ; clip to [-clip, clip]
//   w   -= lr*sqrt(bc2_t)/bc1_t * upd
struct AgdArgs {
  float lr, beta1, beta2, delta, wd, bc1, bc1_prev, bc2, clip;
  int64_t n, n_decay;
  const unsigned char* decay_mask;
};

// One AGD update of one element -- shared by the flat update (a scalar loop)
// and the multi-tensor update (8-wide), written like adam_elem so that both
// round alike.  delta_adj = delta * sqrt(bc2), lr_adj = lr * sqrt(bc2) / bc1.
__device__ __forceinline__ void agd_elem(float g, float gs, bool decay, const AgdArgs& a, float delta_adj,
                                         float lr_adj, float& w, float& mm, float& vv) {
  if (decay) w *= __builtin_fmaf(-a.lr, a.wd, 1.f);
  const float mprev = mm;
  mm = __builtin_fmaf(a.beta1, mprev, (1.f - a.beta1) * (g * gs));
  const float s = (a.bc1_prev > 0.f) ? (mm / a.bc1 - mprev / a.bc1_prev) : mm / a.bc1;
  vv = __builtin_fmaf(a.beta2, vv, (1.f - a.beta2) * s * s);
  float upd = mm / fmaxf(sqrtf(vv), delta_adj);
  if (a.clip > 0.f) upd = fminf(fmaxf(upd, -a.clip), a.clip);
  w = __builtin_fmaf(-lr_adj, upd, w);
}
