// Top-k MoE router (ops/moe.py topk_route; parallel/moe.py TopKGate).
//
// fwd: one wave per token row over the logits [T, E] (bf16 or fp32, E <= 256:
//      lane l holds experts l, l + 64, l + 128, l + 192).  One pass gives the
//      row max, lse and the fp32 softmax; k rounds of a wave arg-max over the
//      LOGITS pick the experts -- on equal values the LOWEST expert index
//      wins (torch.topk leaves the order of ties unspecified).  Writes
//      w[T, k] (fp32, renormalised over the selected set when norm_topk),
//      idx[T, k] (int64), lse[T].  The load-balance statistics are reduced
//      without atomics and in a fixed order: every wave accumulates
//      psum[e] = sum_t p[t, e] and zsum = sum_t lse^2 over its rows in
//      registers, every block adds its 4 waves in wave order and stores one
//      partial row (psum, zsum, integer counts) to the workspace;
//      moe_route_finish_kernel (one block) adds the partial rows in block
//      order and assembles
//        loss = a * E * sum_e (counts_e / (T k)) * psum_e / T + c * zsum / T.
// bwd: one launch, one wave per row, p recomputed from logits and lse:
//        dsel_j = norm ? (gw_j - sum_m gw_m w_m) / s : gw_j      (s = sum_j p[i_j])
//        dp_e   = gL a E f_e / T + sum_j [e == i_j] dsel_j       (f_e = counts_e / (T k))
//        dl_e   = p_e (dp_e - sum_e' p_e' dp_e') + gL c 2 lse / T p_e
//      written in the logits' dtype.  gw and gL may be null.
//
// Parity: reference atorch/modules/moe/topk_gating.py (softmax -> topk ->
// renormalise, load-balance + z loss), there a chain of torch ops.
#include "dw_common.h"

constexpr int RT_MAXE = 256;          // experts (4 per lane)
constexpr int RT_MAXK = 8;
constexpr int RT_WAVES = 4;           // rows in flight per block
constexpr int RT_MAXGRID = 256;       // partial rows of the statistics
constexpr int RT_PART = 2 * RT_MAXE + 1;  // floats per partial row: psum[256], zsum, counts[256] (int)

static inline int route_grid(int64_t T) { return dw_grid_for(T, RT_WAVES, RT_MAXGRID); }

__device__ __forceinline__ float route_load(const void* logits, int dt, int64_t off) {
  return dt == 1 ? bf2f(((const bf16_t*)logits)[off]) : ((const float*)logits)[off];
}

// wave arg-max of (v, e): largest v, lowest e among equals; result in every lane
__device__ __forceinline__ void wave_argmax(float& v, int& e) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oe = __shfl_xor(e, o, 64);
    if (ov > v || (ov == v && oe < e)) { v = ov; e = oe; }
  }
}

__global__ void __launch_bounds__(256) moe_route_fwd_kernel(const void* __restrict__ logits, int dt,
                                                           float* __restrict__ w_out, int64_t* __restrict__ idx_out,
                                                           float* __restrict__ lse_out, float* __restrict__ part,
                                                           int64_t T, int E, int k, int norm) {
  __shared__ int hist[RT_MAXE];
  __shared__ float wsum[RT_WAVES][RT_MAXE + 1];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  hist[threadIdx.x] = 0;
  __syncthreads();
  const float LOG2E = 1.4426950408889634f;
  float pacc[4] = {0.f, 0.f, 0.f, 0.f};
  float zacc = 0.f;
  const int64_t nwaves = (int64_t)gridDim.x * RT_WAVES;
  for (int64_t row = (int64_t)blockIdx.x * RT_WAVES + wid; row < T; row += nwaves) {
    float v[4], p[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = lane + 64 * i;
      v[i] = e < E ? route_load(logits, dt, row * E + e) : -INFINITY;
    }
    const float m = wave_max(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      p[i] = __builtin_amdgcn_exp2f((v[i] - m) * LOG2E);  // exp2(-inf) = 0 for e >= E
      s += p[i];
    }
    s = wave_sum(s);
    const float rs = 1.f / s;
    const float lse = m + logf(s);
#pragma unroll
    for (int i = 0; i < 4; ++i) pacc[i] += p[i] * rs;
    zacc += lse * lse;
    // k rounds of arg-max; lane j keeps the j-th winner
    float myw = 0.f, ssel = 0.f;
    int myi = 0;
    for (int j = 0; j < k; ++j) {
      float bv = v[0];
      int be = lane;
#pragma unroll
      for (int i = 1; i < 4; ++i)
        if (v[i] > bv) { bv = v[i]; be = lane + 64 * i; }  // strict: the lower index stays on ties
      // a lane whose experts are all taken / out of range offers (-inf, its
      // lowest slot); with k <= E some lane always holds a finite value
      wave_argmax(bv, be);
      const float pw = __builtin_amdgcn_exp2f((bv - m) * LOG2E) * rs;
      ssel += pw;
      if (lane == j) { myw = pw; myi = be; }
      if ((be & 63) == lane) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if ((be >> 6) == i) v[i] = -INFINITY;
      }
    }
    if (lane < k) {
      w_out[row * k + lane] = norm ? myw / ssel : myw;
      idx_out[row * k + lane] = myi;
      atomicAdd(&hist[myi], 1);  // LDS, integer
    }
    if (lane == 0) lse_out[row] = lse;
  }
  // block partial: the 4 waves in wave order
#pragma unroll
  for (int i = 0; i < 4; ++i) wsum[wid][lane + 64 * i] = pacc[i];
  if (lane == 0) wsum[wid][RT_MAXE] = zacc;
  __syncthreads();
  float* prow = part + (int64_t)blockIdx.x * RT_PART;
  {
    float a = 0.f;
#pragma unroll
    for (int wv = 0; wv < RT_WAVES; ++wv) a += wsum[wv][threadIdx.x];
    prow[threadIdx.x] = a;
    ((int*)(prow + RT_MAXE + 1))[threadIdx.x] = hist[threadIdx.x];
    if (threadIdx.x == 0) {
      float z = 0.f;
#pragma unroll
      for (int wv = 0; wv < RT_WAVES; ++wv) z += wsum[wv][RT_MAXE];
      prow[RT_MAXE] = z;
    }
  }
}

// One block: partial rows added in block order; counts (int64), psum, zsum
// and the loss scalar.
__global__ void __launch_bounds__(256) moe_route_finish_kernel(const float* __restrict__ part, int nparts,
                                                              int64_t* __restrict__ counts, float* __restrict__ psum,
                                                              float* __restrict__ stats, int64_t T, int E, int k,
                                                              float aux_coef, float z_coef) {
  __shared__ float red[4];
  const int e = threadIdx.x;
  float ps = 0.f;
  int cnt = 0;
  for (int b = 0; b < nparts; ++b) {
    const float* prow = part + (int64_t)b * RT_PART;
    ps += prow[e];
    cnt += ((const int*)(prow + RT_MAXE + 1))[e];
  }
  if (e < E) {
    counts[e] = cnt;
    psum[e] = ps;
  }
  const float fT = (float)T;
  const float term = e < E ? ((float)cnt / (fT * (float)k)) * (ps / fT) : 0.f;
  const float bal = block_sum<256>(term, red);
  if (threadIdx.x == 0) {
    float z = 0.f;
    for (int b = 0; b < nparts; ++b) z += part[(int64_t)b * RT_PART + RT_MAXE];
    stats[0] = aux_coef * (float)E * bal + z_coef * z / fT;  // loss
    stats[1] = z;                                            // zsum
  }
}

__global__ void __launch_bounds__(256) moe_route_bwd_kernel(const void* __restrict__ logits, int dt,
                                                           const float* __restrict__ lse_in,
                                                           const int64_t* __restrict__ idx,
                                                           const float* __restrict__ w, const float* __restrict__ gw,
                                                           const float* __restrict__ gL,
                                                           const int64_t* __restrict__ counts,
                                                           void* __restrict__ dlogits, int64_t T, int E, int k,
                                                           int norm, float aux_coef, float z_coef) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float LOG2E = 1.4426950408889634f;
  const float fT = (float)T;
  const float g = gL ? gL[0] : 0.f;
  // gL a E f_e / T, the same for every row
  float base[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = lane + 64 * i;
    base[i] = (e < E && gL) ? g * aux_coef * (float)E * ((float)counts[e] / (fT * (float)k)) / fT : 0.f;
  }
  const int64_t nwaves = (int64_t)gridDim.x * RT_WAVES;
  for (int64_t row = (int64_t)blockIdx.x * RT_WAVES + wid; row < T; row += nwaves) {
    const float lse = lse_in[row];
    float p[4], dp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = lane + 64 * i;
      p[i] = e < E ? __builtin_amdgcn_exp2f((route_load(logits, dt, row * E + e) - lse) * LOG2E) : 0.f;
      dp[i] = base[i];
    }
    // lane j < k: the j-th selected expert
    int myi = -1;
    float mydsel = 0.f;
    if (gw) {
      float gwj = 0.f, wj = 0.f, pj = 0.f;
      if (lane < k) {
        myi = (int)idx[row * k + lane];
        myi = myi < 0 ? 0 : (myi >= E ? E - 1 : myi);  // stays inside the row whatever idx holds
        gwj = gw[row * k + lane];
        wj = w[row * k + lane];
        pj = __builtin_amdgcn_exp2f((route_load(logits, dt, row * E + myi) - lse) * LOG2E);
      }
      if (norm) {
        const float dot = wave_sum(gwj * wj);
        const float s = wave_sum(pj);
        mydsel = (gwj - dot) / s;
      } else {
        mydsel = gwj;
      }
      for (int j = 0; j < k; ++j) {
        const int ej = __shfl(myi, j, 64);
        const float dj = __shfl(mydsel, j, 64);
        if ((ej & 63) == lane) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if ((ej >> 6) == i) dp[i] += dj;
        }
      }
    }
    float inner = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) inner += p[i] * dp[i];
    inner = wave_sum(inner);
    const float zt = g * z_coef * 2.f * lse / fT;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = lane + 64 * i;
      if (e < E) {
        const float dl = p[i] * (dp[i] - inner) + zt * p[i];
        if (dt == 1) ((bf16_t*)dlogits)[row * E + e] = f2bf(dl);
        else ((float*)dlogits)[row * E + e] = dl;
      }
    }
  }
}

// fp32 words of the statistics workspace (any content on entry)
extern "C" int64_t dw_moe_route_ws_floats(int64_t T) { return (int64_t)route_grid(T) * RT_PART; }

// logits [T, E] (dtype_code 0 fp32 / 1 bf16); w [T, k] fp32; idx [T, k] int64;
// lse [T] fp32; counts [E] int64; psum [E] fp32; stats [2] fp32 (loss, zsum);
// ws: dw_moe_route_ws_floats(T) floats.
extern "C" int dw_moe_route_fwd(const void* logits, int dtype_code, void* w, void* idx, void* lse, void* counts,
                                void* psum, void* stats, void* ws, int64_t T, int E, int k, int norm,
                                float aux_coef, float z_coef, void* stream) {
  if (T <= 0 || E < 1 || E > RT_MAXE || k < 1 || k > RT_MAXK || k > E || (dtype_code != 0 && dtype_code != 1))
    return (int)hipErrorInvalidValue;
  const int grid = route_grid(T);
  hipLaunchKernelGGL(moe_route_fwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, logits, dtype_code,
                     (float*)w, (int64_t*)idx, (float*)lse, (float*)ws, T, E, k, norm);
  hipLaunchKernelGGL(moe_route_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, grid,
                     (int64_t*)counts, (float*)psum, (float*)stats, T, E, k, aux_coef, z_coef);
  DW_LAUNCH_RET;
}

// gw [T, k] fp32 or null; gL device scalar fp32 or null; dlogits in the logits' dtype
extern "C" int dw_moe_route_bwd(const void* logits, int dtype_code, const void* lse, const void* idx, const void* w,
                                const void* gw, const void* gL, const void* counts, void* dlogits, int64_t T, int E,
                                int k, int norm, float aux_coef, float z_coef, void* stream) {
  if (T <= 0 || E < 1 || E > RT_MAXE || k < 1 || k > RT_MAXK || k > E || (dtype_code != 0 && dtype_code != 1))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(moe_route_bwd_kernel, dim3(dw_grid_for(T, RT_WAVES, 2048)), dim3(256), 0, (hipStream_t)stream,
                     logits, dtype_code, (const float*)lse, (const int64_t*)idx, (const float*)w, (const float*)gw,
                     (const float*)gL, (const int64_t*)counts, dlogits, T, E, k, norm, aux_coef, z_coef);
  DW_LAUNCH_RET;
}

DW_PRELOAD(moe_route_fwd_kernel);
DW_PRELOAD(moe_route_finish_kernel);
DW_PRELOAD(moe_route_bwd_kernel);
