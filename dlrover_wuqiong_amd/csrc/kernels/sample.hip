// Fused temperature / top-k / top-p sampler over [B, V] bf16 / fp32 logits:
// one launch, no host read of device data, capturable in a HIP graph.
//
// Kept set (ops/sampling.py keep_mask is the definition), with z = x / T:
//   top-k: z >= the k-th largest value (ties at the threshold all kept);
//   top-p, over what top-k kept: token j is kept iff the kept mass strictly
//          above it is below p * (kept mass).
// Both are "keep j iff (weight strictly above j) < target", with weight 1 per
// token for top-k and e^(z - zmax) for top-p, so the kept set is {key >= tau}
// for one threshold tau.  T > 0, so the order of z is the order of the raw
// logit and tau is found on its bit pattern (16-bit key for bf16, 32-bit for
// fp32) by a most-significant-digit-first radix select, 8 bits per pass: a
// 256-bin LDS histogram of the weights of the keys under the current prefix,
// then a walk from the top bin down.  Weights are integers (counts, or masses
// in 2^-40 fixed point) added with integer LDS atomics, so every sum is
// order-free and the threshold is the same on every run.
//
// Draw: Gumbel-max over the kept set, argmax_j (z_j - log(-log u_j)), lowest
// index on ties.  u_j = (2 * (h >> 9) + 1) * 2^-24 (a 24-bit odd numerator:
// 0 < u < 1) with h the splitmix64 finalizer (the one the attention dropout
// hash uses) of (seed, (offset * B + row) * V + j).  `offset` is read from
// device memory; the caller advances it after the launch.
//
// One block (16 waves) per row: passes after the first hit L2.
#include "row_iter.h"

constexpr int SAMPLE_NT = 1024;
constexpr int SAMPLE_COPIES = 8;  // histogram copies (lane & 7): spreads same-bin LDS atomics
constexpr float SAMPLE_FIX = 1099511627776.f;  // 2^40

// splitmix64 finalizer over (seed, element index); same mixing as attn_hash
// (attn_common.h), kept separate so attention's results cannot change
__device__ __forceinline__ unsigned int sample_hash(unsigned long long seed, unsigned long long idx) {
  unsigned long long z = seed + (idx + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (unsigned int)((z ^ (z >> 31)) >> 32);
}

// order-preserving key of a float: a < b  <=>  key(a) < key(b)
template <int KEYBITS>
__device__ __forceinline__ unsigned int sample_key(float v) {
  const unsigned int b = __float_as_uint(v);
  const unsigned int k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return k >> (32 - KEYBITS);
}

struct SampleShared {
  unsigned long long hist[SAMPLE_COPIES * 256];
  unsigned long long carry;  // weight strictly above the current prefix's key range
  double target;
  unsigned int digit;
  float redf[SAMPLE_NT / 64];
  int redi[SAMPLE_NT / 64];
};

// Smallest key tau with (weight of keys > tau') < target for every present
// tau' >= tau; weight(v, key) is an integer.  frac >= 0: target = frac * total
// weight (known after the first pass); else target = fixed.  A key with no
// weight above it is always kept.
template <typename T, int KEYBITS, typename WF>
__device__ __forceinline__ unsigned int sample_select(const T* __restrict__ x, int V, SampleShared& sh, double fixed,
                                                      double frac, WF&& weight) {
  const int tid = threadIdx.x;
  const int copy = (tid & (SAMPLE_COPIES - 1)) * 256;
  unsigned int prefix = 0;
  if (tid == 0) {
    sh.carry = 0;
    sh.target = fixed;
  }
  for (int shift = KEYBITS - 8; shift >= 0; shift -= 8) {
    for (int i = tid; i < SAMPLE_COPIES * 256; i += SAMPLE_NT) sh.hist[i] = 0;
    __syncthreads();
    row_foreach<T, SAMPLE_NT>(x, V, [&](int, const auto& v) {
      constexpr int N = sizeof(v) / sizeof(float);
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const unsigned int key = sample_key<KEYBITS>(v[k]);
        if ((unsigned int)((unsigned long long)key >> (shift + 8)) != prefix) continue;
        const unsigned long long w = weight(v[k], key);
        if (w) atomicAdd(&sh.hist[copy + ((key >> shift) & 255u)], w);
      }
    });
    __syncthreads();
    if (tid < 256) {
      unsigned long long a = 0;
#pragma unroll
      for (int c = 0; c < SAMPLE_COPIES; ++c) a += sh.hist[c * 256 + tid];
      sh.hist[tid] = a;
    }
    __syncthreads();
    if (tid < 64) {
      // Walk from the top bin down, by wave 0 with bins 4 * lane .. 4 * lane + 3
      // per lane: `above` of a bin = carry + the weight of the bins over it.
      // It grows as the bin falls, so the kept bins are a top range and the
      // digit is the lowest kept bin.  (A serial walk by one lane took longer
      // than the pass over a 32000-token row: docs/rl_token_ops.md.)
      unsigned long long h[4], s = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) s += h[i] = sh.hist[4 * tid + i];
      unsigned long long incl = s;  // this lane's bins and every higher lane's
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_down(incl, o, 64);
        if (tid + o < 64) incl += up;
      }
      double target = sh.target;
      if (shift == KEYBITS - 8 && frac >= 0.) target = frac * (double)__shfl(incl, 0, 64);
      unsigned long long above = sh.carry + (incl - s);
      int mine = 256;
      unsigned long long mine_above = 0;
#pragma unroll
      for (int i = 3; i >= 0; --i) {
        if (above == 0 || (double)above < target) {
          mine = 4 * tid + i;
          mine_above = above;
        }
        above += h[i];
      }
      int lowest = mine;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) lowest = min(lowest, __shfl_xor(lowest, o, 64));
      if (mine == lowest && lowest < 256) {  // one lane: bins are distinct
        sh.digit = lowest;
        sh.carry = mine_above;
        sh.target = target;
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | sh.digit;
  }
  return prefix;
}

template <typename T, int KEYBITS>
__global__ void __launch_bounds__(SAMPLE_NT) sample_tokens_kernel(const T* __restrict__ logits, int64_t* __restrict__ out,
                                                                  const int64_t* __restrict__ offset, int B, int V,
                                                                  int64_t row_stride, float inv_temp, int top_k,
                                                                  float top_p, unsigned long long seed) {
  __shared__ SampleShared sh;
  const int row = blockIdx.x, tid = threadIdx.x;
  const T* x = logits + (int64_t)row * row_stride;
  unsigned int tau = 0;
  if (top_k > 0 && top_k < V)
    tau = sample_select<T, KEYBITS>(x, V, sh, (double)top_k, -1., [](float, unsigned int) { return 1ull; });
  if (top_p < 1.f) {
    float m = -INFINITY;
    row_foreach<T, SAMPLE_NT>(x, V, [&](int, const auto& v) {
      constexpr int N = sizeof(v) / sizeof(float);
#pragma unroll
      for (int k = 0; k < N; ++k) m = fmaxf(m, v[k]);
    });
    const float xmax = block_max<SAMPLE_NT>(m, sh.redf);
    const unsigned int tau_k = tau;
    const unsigned int tau_p = sample_select<T, KEYBITS>(x, V, sh, 0., (double)top_p, [=](float v, unsigned int key) {
      return key >= tau_k ? (unsigned long long)(__expf((v - xmax) * inv_temp) * SAMPLE_FIX) : 0ull;
    });
    tau = tau_p > tau_k ? tau_p : tau_k;
  }
  // Gumbel-max over {key >= tau}
  const unsigned long long base = ((unsigned long long)offset[0] * (unsigned long long)B + row) * (unsigned long long)V;
  float best = -INFINITY;
  int besti = V;
  row_foreach<T, SAMPLE_NT>(x, V, [&](int j0, const auto& v) {
    constexpr int N = sizeof(v) / sizeof(float);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (sample_key<KEYBITS>(v[k]) < tau) continue;
      // the noise is at most -log(-log(1 - 2^-24)) = 16.64: this token cannot beat the lane's best
      if (v[k] * inv_temp + 16.7f <= best) continue;
      const unsigned int h = sample_hash(seed, base + (unsigned long long)(j0 + k));
      const float u = (float)(2u * (h >> 9) + 1u) * 5.9604644775390625e-08f;  // 2^-24
      const float sc = v[k] * inv_temp - logf(-logf(u));
      if (sc > best || (sc == best && j0 + k < besti)) {
        best = sc;
        besti = j0 + k;
      }
    }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float b2 = __shfl_xor(best, o, 64);
    const int i2 = __shfl_xor(besti, o, 64);
    if (b2 > best || (b2 == best && i2 < besti)) {
      best = b2;
      besti = i2;
    }
  }
  if ((tid & 63) == 0) {
    sh.redf[tid >> 6] = best;
    sh.redi[tid >> 6] = besti;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < SAMPLE_NT / 64; ++w)
      if (sh.redf[w] > best || (sh.redf[w] == best && sh.redi[w] < besti)) {
        best = sh.redf[w];
        besti = sh.redi[w];
      }
    out[row] = besti < V ? besti : 0;
  }
}

// dtype: 0 fp32, 1 bf16 (ops/_hip.py dtype_code); row_stride in elements
extern "C" int dw_sample_tokens(const void* logits, int dtype, void* out, const void* offset, int B, int V,
                                int64_t row_stride, float inv_temp, int top_k, float top_p,
                                unsigned long long seed, void* stream) {
  if (B <= 0) return 0;
  if (V <= 0 || !offset || !(inv_temp > 0.f)) return (int)hipErrorInvalidValue;
  const dim3 grid((unsigned)B), block(SAMPLE_NT);
  if (dtype == 1)
    hipLaunchKernelGGL((sample_tokens_kernel<bf16_t, 16>), grid, block, 0, (hipStream_t)stream,
                       (const bf16_t*)logits, (int64_t*)out, (const int64_t*)offset, B, V, row_stride, inv_temp,
                       top_k, top_p, seed);
  else
    hipLaunchKernelGGL((sample_tokens_kernel<float, 32>), grid, block, 0, (hipStream_t)stream, (const float*)logits,
                       (int64_t*)out, (const int64_t*)offset, B, V, row_stride, inv_temp, top_k, top_p, seed);
  DW_LAUNCH_RET;
}

DW_PRELOAD((sample_tokens_kernel<bf16_t, 16>));
