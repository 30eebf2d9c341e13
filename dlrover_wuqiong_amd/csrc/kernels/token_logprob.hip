// Log-prob of a label and entropy of softmax(logits), per row of a [*, V]
// bf16 / fp32 tensor (PPO: log-probs of the sampled response tokens and the
// entropy bonus), forward and backward.
//
// Rows are addressed as base + (row / R) * batch_stride + (row % R) *
// row_stride (element strides), so logits[:, P-1:-1, :] of a [B, S, V] tensor
// is read in place.
//
// fwd: one block (4 waves) per row, one pass, online state per lane
//        m = max x,  s = sum e^(x-m),  t = sum e^(x-m) * x
//      combined over the block in a fixed order:
//        lse = m + log s,  logp = x[label] - lse,  H = lse - t / s.
//      x = -inf contributes 0 to t; a label outside [0, V) gives logp = 0.
//      lse and H are saved per row (fp32); the probabilities are never written.
// bwd: one pass, with p_j = e^(x_j - lse):
//        dx_j = g_logp * ([j == label] - p_j) - g_H * p_j * ((x_j - lse) + H)
//      dense [rows, V] in the logits' dtype; p_j = 0 gives 0; a row whose
//      label is outside [0, V) has logp = 0, a constant, so its g_logp is 0.
//
// Parity: reference atorch/rl/model_utils/model_util.py (logprobs_of_labels)
// and the entropy term of atorch/rl/ppo_utils/ppo_util.py.
#include "row_iter.h"

template <typename T>
__device__ __forceinline__ const T* stats_row(const T* base, int64_t row, int64_t R, int64_t bs, int64_t rs) {
  return base + (row / R) * bs + (row % R) * rs;
}

template <typename T>
__global__ void __launch_bounds__(256) token_logprob_fwd_kernel(const T* __restrict__ logits,
                                                                const int64_t* __restrict__ labels,
                                                                float* __restrict__ logp, float* __restrict__ lse_out,
                                                                float* __restrict__ ent_out, int64_t R, int64_t bs,
                                                                int64_t rs, int V) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x;
  const T* x = stats_row(logits, row, R, bs, rs);
  float m = -INFINITY, s = 0.f, t = 0.f;
  row_foreach<T, 256>(x, V, [&](int, const auto& v) {
    constexpr int N = sizeof(v) / sizeof(float);
    float vm = v[0];
#pragma unroll
    for (int k = 1; k < N; ++k) vm = fmaxf(vm, v[k]);
    if (vm == -INFINITY) return;  // nothing to add, and m may still be -inf
    const float mn = fmaxf(m, vm);
    const float r = __expf(m - mn);  // m = -inf: 0
    s *= r;
    t *= r;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const float e = __expf(v[k] - mn);
      s += e;
      t += (v[k] == -INFINITY) ? 0.f : e * v[k];
    }
    m = mn;
  });
  const float M = block_max<256>(m, red);
  const float r = (m == -INFINITY) ? 0.f : __expf(m - M);
  const float S = block_sum<256>(s * r, red);
  const float TT = block_sum<256>(t * r, red);
  if (threadIdx.x == 0) {
    const float lse = M + logf(S);
    const int64_t lab = labels ? labels[row] : -1;
    logp[row] = (lab >= 0 && lab < V) ? RowVec<T>::load1(x + lab) - lse : 0.f;
    lse_out[row] = lse;
    ent_out[row] = lse - TT / S;
  }
}

__device__ __forceinline__ float stats_dx(float x, bool is_label, float L, float H, float g1, float g2) {
  const float d = x - L;
  const float p = __expf(d);
  const float term = (p > 0.f) ? p * (g1 + g2 * (d + H)) : 0.f;
  return (is_label ? g1 : 0.f) - term;
}

template <typename T>
__global__ void __launch_bounds__(256) token_logprob_bwd_kernel(const T* __restrict__ logits,
                                                                const int64_t* __restrict__ labels,
                                                                const float* __restrict__ lse,
                                                                const float* __restrict__ ent,
                                                                const float* __restrict__ g_logp,
                                                                const float* __restrict__ g_ent, T* __restrict__ dlogits,
                                                                int64_t R, int64_t bs, int64_t rs, int V) {
  constexpr int W = RowVec<T>::W;
  const int64_t row = blockIdx.x;
  const T* x = stats_row(logits, row, R, bs, rs);
  T* dx = dlogits + row * (int64_t)V;
  int64_t lab = labels ? labels[row] : -1;
  float g1 = g_logp ? g_logp[row] : 0.f;
  if (lab < 0 || lab >= V) {
    lab = -1;
    g1 = 0.f;
  }
  const float g2 = g_ent ? g_ent[row] : 0.f;
  const float L = lse[row], H = ent[row];
  const int nv = (row_aligned16(x) && row_aligned16(dx)) ? V / W : 0;
  for (int c = threadIdx.x; c < nv; c += 256) {
    float f[W];
    RowVec<T>::load(x + (int64_t)c * W, f);
#pragma unroll
    for (int k = 0; k < W; ++k) f[k] = stats_dx(f[k], c * W + k == lab, L, H, g1, g2);
    RowVec<T>::store(dx + (int64_t)c * W, f);
  }
  for (int j = nv * W + threadIdx.x; j < V; j += 256)
    RowVec<T>::store1(dx + j, stats_dx(RowVec<T>::load1(x + j), j == lab, L, H, g1, g2));
}

// dtype: 0 fp32, 1 bf16 (ops/_hip.py dtype_code)
extern "C" int dw_token_logprob_fwd(const void* logits, int dtype, const void* labels, void* logp, void* lse,
                                    void* ent, int64_t rows, int64_t R, int64_t bs, int64_t rs, int V,
                                    void* stream) {
  if (rows <= 0) return 0;
  if (V <= 0 || R <= 0) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)rows), block(256);
  if (dtype == 1)
    hipLaunchKernelGGL(token_logprob_fwd_kernel<bf16_t>, grid, block, 0, (hipStream_t)stream, (const bf16_t*)logits,
                       (const int64_t*)labels, (float*)logp, (float*)lse, (float*)ent, R, bs, rs, V);
  else
    hipLaunchKernelGGL(token_logprob_fwd_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)logits,
                       (const int64_t*)labels, (float*)logp, (float*)lse, (float*)ent, R, bs, rs, V);
  DW_LAUNCH_RET;
}

extern "C" int dw_token_logprob_bwd(const void* logits, int dtype, const void* labels, const void* lse,
                                    const void* ent, const void* g_logp, const void* g_ent, void* dlogits,
                                    int64_t rows, int64_t R, int64_t bs, int64_t rs, int V, void* stream) {
  if (rows <= 0) return 0;
  if (V <= 0 || R <= 0) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)rows), block(256);
  if (dtype == 1)
    hipLaunchKernelGGL(token_logprob_bwd_kernel<bf16_t>, grid, block, 0, (hipStream_t)stream, (const bf16_t*)logits,
                       (const int64_t*)labels, (const float*)lse, (const float*)ent, (const float*)g_logp,
                       (const float*)g_ent, (bf16_t*)dlogits, R, bs, rs, V);
  else
    hipLaunchKernelGGL(token_logprob_bwd_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)logits,
                       (const int64_t*)labels, (const float*)lse, (const float*)ent, (const float*)g_logp,
                       (const float*)g_ent, (float*)dlogits, R, bs, rs, V);
  DW_LAUNCH_RET;
}

DW_PRELOAD(token_logprob_fwd_kernel<bf16_t>);
