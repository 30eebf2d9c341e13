// LayerNorm / RMSNorm forward, bf16 I/O, fp32 math (the backward is
// dw_norm_bwd in colred.hip).
//
// One wave64 owns one row; the row lives in registers (VPL 16-byte vectors
// per lane), so x is read once.  Row statistics use wave shuffles only (no
// LDS, no __syncthreads in the row path).
//
// Parity: reference atorch/atorch/normalization/layernorm.py (Triton/apex
// fused LayerNorm) and the RMSNorm used by its Llama modules.
#include "dw_common.h"

// ADD: fused residual add -- h = x + res is formed in registers, rounded to
// bf16 (exactly what a separate bf16 add would store), written to h_out and
// normalized; the residual stream is read once instead of three times.
template <int VPL, bool RMS, bool ADD = false>
__global__ void __launch_bounds__(256) norm_fwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ gamma,
                                                       const bf16_t* __restrict__ beta, bf16_t* __restrict__ y,
                                                       float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                       int64_t rows, int H, float eps,
                                                       const bf16_t* __restrict__ res = nullptr,
                                                       bf16_t* __restrict__ h_out = nullptr) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nv = H >> 3;
  const bf16_t* xr = x + row * H;
  float v[VPL][8];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int c = lane + 64 * j;
    if (c < nv) {
      unpack8(*(const u32x4*)(xr + c * 8), v[j]);
      if constexpr (ADD) {
        float r[8];
        unpack8(*(const u32x4*)(res + row * H + c * 8), r);
        u32x4 hv;
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] += v[j][k];
        hv = pack8(r);
        *(u32x4*)(h_out + row * H + c * 8) = hv;
        unpack8(hv, v[j]);  // normalize the bf16-rounded sum
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) s += v[j][k];
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[j][k] = 0.f;
    }
  }
  float mu = 0.f;
  if (!RMS) mu = wave_sum(s) / (float)H;
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int c = lane + 64 * j;
    if (c < nv) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float d = v[j][k] - mu;
        ss += d * d;
      }
    }
  }
  const float var = wave_sum(ss) / (float)H;
  const float rstd = rsqrtf(var + eps);
  if (lane == 0) {
    if (!RMS) mean_out[row] = mu;
    rstd_out[row] = rstd;
  }
  bf16_t* yr = y + row * H;
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int c = lane + 64 * j;
    if (c < nv) {
      float g[8], b[8], o[8];
      unpack8(*(const u32x4*)(gamma + c * 8), g);
      if (!RMS) unpack8(*(const u32x4*)(beta + c * 8), b);
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = (v[j][k] - mu) * rstd * g[k] + (RMS ? 0.f : b[k]);
      *(u32x4*)(yr + c * 8) = pack8(o);
    }
  }
}

// (A grid-stride form that prefetches the next row and loads gamma / beta
// once per wave measured the same: 25.1 vs 24.9 us for the GPT2-1.5B add+norm,
// 8192 x 1600 -- profiles/r4/norm_fwd_gelu_ab.jsonl; one row per wave stays.)

#define DISPATCH_VPL(H, ...)                          \
  do {                                                \
    int nv_ = (H) / 8;                                \
    if (nv_ <= 64) { constexpr int VPL = 1; __VA_ARGS__; } \
    else if (nv_ <= 128) { constexpr int VPL = 2; __VA_ARGS__; } \
    else if (nv_ <= 256) { constexpr int VPL = 4; __VA_ARGS__; } \
    else if (nv_ <= 512) { constexpr int VPL = 8; __VA_ARGS__; } \
    else { constexpr int VPL = 16; __VA_ARGS__; }    \
  } while (0)

extern "C" int dw_norm_fwd(const void* x, const void* gamma, const void* beta, void* y, void* mean,
                           void* rstd, int64_t rows, int H, float eps, int rms, void* stream) {
  if (H % 8 != 0 || H > 8 * 64 * 16) return (int)hipErrorInvalidValue;
  dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  hipStream_t s = (hipStream_t)stream;
  DISPATCH_VPL(H, {
    if (rms)
      hipLaunchKernelGGL((norm_fwd_kernel<VPL, true>), grid, block, 0, s, (const bf16_t*)x,
                         (const bf16_t*)gamma, nullptr, (bf16_t*)y, nullptr, (float*)rstd, rows, H, eps);
    else
      hipLaunchKernelGGL((norm_fwd_kernel<VPL, false>), grid, block, 0, s, (const bf16_t*)x,
                         (const bf16_t*)gamma, (const bf16_t*)beta, (bf16_t*)y, (float*)mean,
                         (float*)rstd, rows, H, eps);
  });
  DW_LAUNCH_RET;
}

// y = norm(x + res), h_out = x + res (bf16).  Fused pre-norm residual add.
extern "C" int dw_add_norm_fwd(const void* x, const void* res, const void* gamma, const void* beta, void* y,
                               void* h_out, void* mean, void* rstd, int64_t rows, int H, float eps, int rms,
                               void* stream) {
  if (H % 8 != 0 || H > 8 * 64 * 16) return (int)hipErrorInvalidValue;
  dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  hipStream_t s = (hipStream_t)stream;
  DISPATCH_VPL(H, {
    if (rms)
      hipLaunchKernelGGL((norm_fwd_kernel<VPL, true, true>), grid, block, 0, s, (const bf16_t*)x,
                         (const bf16_t*)gamma, nullptr, (bf16_t*)y, nullptr, (float*)rstd, rows, H, eps,
                         (const bf16_t*)res, (bf16_t*)h_out);
    else
      hipLaunchKernelGGL((norm_fwd_kernel<VPL, false, true>), grid, block, 0, s, (const bf16_t*)x,
                         (const bf16_t*)gamma, (const bf16_t*)beta, (bf16_t*)y, (float*)mean, (float*)rstd, rows,
                         H, eps, (const bf16_t*)res, (bf16_t*)h_out);
  });
  DW_LAUNCH_RET;
}

DW_PRELOAD((norm_fwd_kernel<1, false>));
