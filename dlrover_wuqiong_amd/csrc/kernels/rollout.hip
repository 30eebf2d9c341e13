// RL rollout decode step: the K/V bookkeeping of one token, two launches.
//
//  * dw_kv_append_rope: QKV split + RoPE + K/V append into the static cache.
//    The decode step of the hybrid engine (atorch/rl/hybrid_engine.py) did
//    this with split views, two .contiguous() copies, two rope launches, an
//    index computation and two index_copy_ calls per layer.
//  * dw_rollout_step: what follows the sampler for ragged rollouts with an
//    EOS token: place the token in each row's own column, count response
//    lengths, latch `finished`, count the rows still running.
//
// Forward only: rollouts run without autograd.
#include "dw_common.h"

// qkv [B, S, NH + 2 NKV, D] bf16 contiguous -> q [B, S, NH, D] contiguous
// (rotated); rotated k and plain v written to k_cache / v_cache, logical
// [B, Smax, NKV, D] with element strides (cache_bs, cache_rs), heads x D dense.
// Token (b, s) sits at position lens[b] + s (lens null: s).  The cos / sin row
// is clamped to the table as in qkv_rope_kernel (elementwise.hip); a token at
// a position outside [0, Smax) writes no K/V, its q is still produced.  Work
// split and arithmetic are qkv_rope_kernel's -- one thread per (token, head,
// 8-wide vector of the first half), the same fp32 expression on the same fp32
// table, one bf16 rounding -- so q and k equal dw_qkv_rope's bit for bit.
__global__ void __launch_bounds__(256) kv_append_rope_kernel(
    const bf16_t* __restrict__ qkv, bf16_t* __restrict__ q, bf16_t* __restrict__ k_cache,
    bf16_t* __restrict__ v_cache, const float* __restrict__ cosb, const float* __restrict__ sinb,
    const int* __restrict__ lens, int64_t BS, int S, int NH, int NKV, int D, int Smax, int64_t cache_bs,
    int64_t cache_rs, int rows) {
  const int half = D >> 1;
  const int hv = half >> 3;
  const int NT = NH + 2 * NKV;
  const int64_t total = BS * NT * hv;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int vi = (int)(t % hv);
    const int64_t rh = t / hv;  // (b*S + s) * NT + head
    const int head = (int)(rh % NT);
    const int64_t bs = rh / NT;
    const int64_t b = bs / S;
    const int pos = (lens ? lens[b] : 0) + (int)(bs % S);
    const bool in_cache = pos >= 0 && pos < Smax;
    const bf16_t* src = qkv + rh * D;
    bf16_t* dst;
    if (head < NH) {
      dst = q + (bs * NH + head) * D;
    } else {
      if (!in_cache) continue;
      const bool is_k = head < NH + NKV;
      dst = (is_k ? k_cache : v_cache) + b * cache_bs + pos * cache_rs + (int64_t)(head - NH - (is_k ? 0 : NKV)) * D;
    }
    const u32x4 a4 = *(const u32x4*)(src + vi * 8), b4 = *(const u32x4*)(src + half + vi * 8);
    if (head >= NH + NKV) {  // value head: a plain copy
      *(u32x4*)(dst + vi * 8) = a4;
      *(u32x4*)(dst + half + vi * 8) = b4;
      continue;
    }
    const int sp = min(max(pos, 0), rows - 1);
    const float* cr = cosb + (int64_t)sp * half + vi * 8;
    const float* sr = sinb + (int64_t)sp * half + vi * 8;
    const f32x4 c0 = *(const f32x4*)cr, c1 = *(const f32x4*)(cr + 4);
    const f32x4 s0 = *(const f32x4*)sr, s1 = *(const f32x4*)(sr + 4);
    float a[8], bb[8], o1[8], o2[8];
    unpack8(a4, a);
    unpack8(b4, bb);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float c = j < 4 ? c0[j] : c1[j - 4];
      const float sn = j < 4 ? s0[j] : s1[j - 4];
      o1[j] = a[j] * c - bb[j] * sn;
      o2[j] = bb[j] * c + a[j] * sn;
    }
    *(u32x4*)(dst + vi * 8) = pack8(o1);
    *(u32x4*)(dst + half + vi * 8) = pack8(o2);
  }
}

// cos / sin: fp32 [rows, D/2]; lens (nullable) int32 [B]; cache strides in
// elements, multiples of 8 (16-byte stores).
extern "C" int dw_kv_append_rope(const void* qkv, void* q, void* k_cache, void* v_cache, const void* cosb,
                                 const void* sinb, const void* lens, int64_t B, int S, int NH, int NKV, int D,
                                 int Smax, int64_t cache_bs, int64_t cache_rs, int rows, void* stream) {
  if (D % 16 || rows < 1 || B < 1 || S < 1 || NH < 1 || NKV < 1 || Smax < 1) return (int)hipErrorInvalidValue;
  if (cache_rs < (int64_t)NKV * D || cache_bs < cache_rs * Smax || cache_rs % 8 || cache_bs % 8)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)qkv | (uintptr_t)q | (uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)cosb |
       (uintptr_t)sinb) & 15)
    return (int)hipErrorInvalidValue;
  const int64_t total = B * S * (NH + 2 * NKV) * (D / 16);
  hipLaunchKernelGGL(kv_append_rope_kernel, dim3(dw_grid_for(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)qkv, (bf16_t*)q, (bf16_t*)k_cache, (bf16_t*)v_cache, (const float*)cosb,
                     (const float*)sinb, (const int*)lens, B * S, S, NH, NKV, D, Smax, cache_bs, cache_rs, rows);
  DW_LAUNCH_RET;
}

// One block; the threads stride over the B rows.  Per row b:
//   tok = finished[b] ? pad : sampled[b]
//   seq[b, lens[b]] = tok                       (when 0 <= lens[b] < L)
//   resp_len[b] += 1                            (rows not finished before)
//   finished[b] |= tok == eos                   (eos = -1: never)
//   tok_out[b] = tok                            (what the next forward reads)
// n_active[0] = rows not finished after the update: an integer block
// reduction (wave shuffles, then LDS), written by one thread.
constexpr int STEP_THREADS = 256;
__global__ void __launch_bounds__(STEP_THREADS) rollout_step_kernel(
    const int64_t* __restrict__ sampled, const int* __restrict__ lens, int* __restrict__ finished,
    int* __restrict__ resp_len, int64_t* __restrict__ seq, int64_t* __restrict__ tok_out,
    int* __restrict__ n_active, int B, int64_t L, int64_t eos, int64_t pad) {
  __shared__ int red[STEP_THREADS / 64];
  int active = 0;
  for (int b = threadIdx.x; b < B; b += STEP_THREADS) {
    const int fin = finished[b];
    const int64_t tok = fin ? pad : sampled[b];
    const int col = lens[b];
    if (col >= 0 && col < L) seq[(int64_t)b * L + col] = tok;
    if (!fin) resp_len[b] += 1;
    const int now = (fin || tok == eos) ? 1 : 0;
    finished[b] = now;
    tok_out[b] = tok;
    active += 1 - now;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) active += __shfl_xor(active, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = active;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int i = 0; i < STEP_THREADS / 64; ++i) t += red[i];
    n_active[0] = t;
  }
}

extern "C" int dw_rollout_step(const void* sampled, const void* lens, void* finished, void* resp_len, void* seq,
                               void* tok_out, void* n_active, int B, int64_t L, int64_t eos, int64_t pad,
                               void* stream) {
  if (B < 1 || L < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(rollout_step_kernel, dim3(1), dim3(STEP_THREADS), 0, (hipStream_t)stream,
                     (const int64_t*)sampled, (const int*)lens, (int*)finished, (int*)resp_len, (int64_t*)seq,
                     (int64_t*)tok_out, (int*)n_active, B, L, eos, pad);
  DW_LAUNCH_RET;
}

DW_PRELOAD(kv_append_rope_kernel);
