// Column reductions (bias / norm-weight gradients) and the row-wise norm dx.
//
// Bias grads db = sum_rows dy and norm weight grads dgamma = sum_rows dy*xhat,
// dbeta = sum_rows dy are column sums over [rows, C] -- tall and skinny
// (rows = tokens = 8K..64K, C = hidden).  One kernel per reduction:
//   * block = 4 waves; a wave covers 512 consecutive columns (64 lanes x one
//     16-byte vector of 8 bf16) of its rows, a block a [rows/RS] x 512 tile;
//   * per-lane fp32 accumulation in registers over the block's rows, one LDS
//     combine of the 4 waves, then ONE fp32 atomicAdd per column per block
//     into a workspace -> grid = (C/512) x RS blocks fills the chip without
//     any partial-row buffer or second pass over the data;
//   * the last block to finish in each 512-column strip (per-strip
//     completion counters after the sums) converts the strip's fp32 sums
//     into the gradient (bf16 or fp32), optionally
//     ACCUMULATING into it (grad += sum), so the result lands directly in the
//     flat gradient buffer with no second launch.  The workspace (sums +
//     counter) is SELF-CLEANING: the finishing block zeroes what it consumed,
//     so it is all-zero between calls and needs no per-call memset.
//
// The LayerNorm / RMSNorm backward (dw_norm_bwd) lives here because its
// weight gradients are such column sums.  One path per hidden size H
// (norm_bwd_plan, docs/norm_backward.md):
//   * H <= 1024: norm_bwd_part_kernel, one wave per row, dx plus one fp32
//     partial row of dgamma / dbeta (/ dx column sums) per workgroup;
//   * 1024 < H < 2048: norm_bwd_pair_kernel<G = 2>, a row split over a wave pair;
//   * 2048 <= H <= 4096: norm_bwd_pair_kernel<G = 4>, a row split over a wave quad;
//     all three followed by colsum_f32_kernel over the workgroups' partial rows;
//   * 4096 < H <= 8192: norm_dx_kernel (row pass, dx only), then
//     colred_kernel<1 or 2> reads dy and x a second time for the weight gradients.
#include "dw_common.h"

#include <algorithm>

__device__ __forceinline__ void colred_store(void* out, int c, float v, int is_fp32, int accumulate) {
  if (!out) return;
  if (is_fp32) {
    float* o = (float*)out;
    o[c] = accumulate ? o[c] + v : v;
  } else {
    bf16_t* o = (bf16_t*)out;
    o[c] = f2bf(accumulate ? bf2f(o[c]) + v : v);
  }
}

// Deterministic mode (``part`` != nullptr; DWAMD_DETERMINISTIC=1 or
// torch.use_deterministic_algorithms(True) on the Python side): every block
// stores its partial column sums instead of adding them atomically, and the
// finishing block adds the partials in block order -- bit-identical results
// from run to run at the cost of the partial buffer and the finishing
// block's serial sum.  Loads are issued 8 at a time, the adds stay in order.
__device__ __forceinline__ float ordered_sum(const float* p, int64_t stride, int n) {
  float a = 0.f;
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      v[u] = __hip_atomic_load(p + (int64_t)(i + u) * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int u = 0; u < 8; ++u) a += v[u];
  }
  for (; i < n; ++i) a += __hip_atomic_load(p + (int64_t)i * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return a;
}

// MODE 0: acc0 += dy ;  MODE 1: acc0 += dy * xhat, acc1 += dy (LayerNorm) ;
// MODE 2: acc0 += dy * xhat (RMSNorm) ;
// MODE 3: dxo = dy * gelu'(x), acc0 += dxo (GELU backward fused with the
//         gradient of the bias added before it: one pass instead of two)
template <int MODE>
__global__ void __launch_bounds__(256) colred_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     float* __restrict__ ws, int64_t rows, int C, int rows_per_blk,
                                                     void* __restrict__ out0, void* __restrict__ out1, int is_fp32,
                                                     int accumulate, bf16_t* __restrict__ dxo = nullptr,
                                                     float* __restrict__ part = nullptr) {
  __shared__ float red[2][4][512 + 4];
  constexpr int NS = MODE == 1 ? 2 : 1;  // sums per column
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c0 = blockIdx.x * 512 + lane * 8;
  const int64_t r_beg = (int64_t)blockIdx.y * rows_per_blk;
  const int64_t r_end = min(rows, r_beg + rows_per_blk);
  float a0[8], a1[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) a0[k] = a1[k] = 0.f;
  if (c0 < C) {
    // U rows per wave per iteration, every load issued before any math
    constexpr int U = 4;
    for (int64_t r0 = r_beg + wid; r0 < r_end; r0 += 4 * U) {
      u32x4 dv[U], xw[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t r = r0 + 4 * u;
        if (r < r_end) {
          dv[u] = *(const u32x4*)(dy + r * C + c0);
          if constexpr (MODE != 0) xw[u] = *(const u32x4*)(x + r * C + c0);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t r = r0 + 4 * u;
        if (r >= r_end) break;
        float d[8];
        unpack8(dv[u], d);
        if constexpr (MODE == 0) {
#pragma unroll
          for (int k = 0; k < 8; ++k) a0[k] += d[k];
        } else if constexpr (MODE == 3) {
          float xv[8];
          unpack8(xw[u], xv);
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            d[k] *= gelu_tanh_grad(xv[k]);
            a0[k] += d[k];
          }
          *(u32x4*)(dxo + r * C + c0) = pack8(d);
        } else {
          float xv[8];
          unpack8(xw[u], xv);
          const float mu = (MODE == 1) ? mean[r] : 0.f, rs = rstd[r];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            a0[k] += d[k] * (xv[k] - mu) * rs;
            if constexpr (MODE == 1) a1[k] += d[k];
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    red[0][wid][lane * 8 + k] = a0[k];
    if constexpr (MODE == 1) red[1][wid][lane * 8 + k] = a1[k];
  }
  __syncthreads();
  // 256 threads combine 512 columns (2 each) x 4 waves, one atomic per column
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int cl = threadIdx.x + 256 * j;
    const int c = blockIdx.x * 512 + cl;
    if (c >= C) continue;
    const float s0 = red[0][0][cl] + red[0][1][cl] + red[0][2][cl] + red[0][3][cl];
    if (part) {
      // deterministic mode: this block's partial sums, combined in a fixed
      // order by the finishing block (agent-scope stores: performed at the
      // coherent level, like the atomics of the default mode)
      __hip_atomic_store(part + (int64_t)blockIdx.y * NS * C + c, s0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      atomicAdd(ws + c, s0);
    }
    if constexpr (MODE == 1) {
      const float s1 = red[1][0][cl] + red[1][1][cl] + red[1][2][cl] + red[1][3][cl];
      if (part)
        __hip_atomic_store(part + ((int64_t)blockIdx.y * NS + 1) * C + c, s1, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      else
        atomicAdd(ws + C + c, s1);
    }
  }
  // The last block of each 512-column strip converts the strip's fp32 sums
  // into the output(s) -- no second launch (a ~5 us kernel per reduction,
  // ~450 per GPT2-1.5B step), and the finish is spread over the strips.
  //
  // Ordering without a device-scope fence: a __threadfence() here is an L2
  // write-back + invalidate on gfx950 (per-XCD L2s), in every block -- it
  // made this kernel 5x slower.  All the data the finishing block reads was
  // produced by agent-scope atomics, so it is enough that this block's
  // atomics have COMPLETED (vmcnt drained: performed at the coherent level)
  // before its counter increment is issued, and that the finishing block
  // reads the sums with atomics too.
  __shared__ int is_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  unsigned* cnt = (unsigned*)(ws + (MODE == 1 ? 2 * C : C)) + blockIdx.x;
  if (threadIdx.x == 0)
    is_last = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.y - 1;
  __syncthreads();
  if (!is_last) return;
  float v0[2], v1[2];
  if (part) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = blockIdx.x * 512 + threadIdx.x + 256 * j;
      if (c < C) {
        v0[j] = ordered_sum(part + c, (int64_t)NS * C, gridDim.y);
        if constexpr (MODE == 1) v1[j] = ordered_sum(part + C + c, (int64_t)NS * C, gridDim.y);
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      // read + clear (self-cleaning) with the same atomics that built the sums:
      // single-location atomicity, no cache maintenance; all in flight at once
      const int c = blockIdx.x * 512 + threadIdx.x + 256 * j;
      if (c < C) {
        v0[j] = __hip_atomic_exchange(ws + c, 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (MODE == 1)
          v1[j] = __hip_atomic_exchange(ws + C + c, 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = blockIdx.x * 512 + threadIdx.x + 256 * j;
    if (c < C) {
      colred_store(out0, c, v0[j], is_fp32, accumulate);
      if constexpr (MODE == 1) colred_store(out1, c, v1[j], is_fp32, accumulate);
    }
  }
  if (threadIdx.x == 0) __hip_atomic_exchange(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// dx = rstd * (dy*g - mean(dy*g) - xhat * mean(dy*g*xhat)) [+ dres]; one wave
// per row, for 4096 < H <= 8192 (VPL = 16 vectors per lane): xhat and dy*g
// do not fit in registers there, so the second loop reads the row again
template <int VPL, bool RMS>
__global__ void __launch_bounds__(256) norm_dx_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                      const bf16_t* __restrict__ gamma,
                                                      const float* __restrict__ mean_in,
                                                      const float* __restrict__ rstd_in,
                                                      const bf16_t* __restrict__ dres, bf16_t* __restrict__ dx,
                                                      int64_t rows, int H) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nv = H >> 3;
  const float mu = RMS ? 0.f : mean_in[row];
  const float rstd = rstd_in[row];
  const bf16_t* xr = x + row * H;
  const bf16_t* dr = dy + row * H;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int c = lane + 64 * j;
    if (c < nv) {
      float xv[8], dv[8], gm[8];
      unpack8(*(const u32x4*)(xr + c * 8), xv);
      unpack8(*(const u32x4*)(dr + c * 8), dv);
      unpack8(*(const u32x4*)(gamma + c * 8), gm);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float a = (xv[k] - mu) * rstd, b = dv[k] * gm[k];
        s1 += b;
        s2 += b * a;
      }
    }
  }
  const float m1 = RMS ? 0.f : wave_sum(s1) / (float)H;
  const float m2 = wave_sum(s2) / (float)H;
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int c = lane + 64 * j;
    if (c < nv) {
      float xv[8], dv[8], gm[8], o[8];
      unpack8(*(const u32x4*)(xr + c * 8), xv);
      unpack8(*(const u32x4*)(dr + c * 8), dv);
      unpack8(*(const u32x4*)(gamma + c * 8), gm);
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = rstd * (dv[k] * gm[k] - m1 - (xv[k] - mu) * rstd * m2);
      if (dres) {  // fused residual-branch gradient (uniform branch)
        float r[8];
        unpack8(*(const u32x4*)(dres + row * H + c * 8), r);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] += r[k];
      }
      *(u32x4*)(dx + row * H + c * 8) = pack8(o);
    }
  }
}

// Norm backward for H <= 1024 (VPL <= 2), one pass over dy / x (/ dres):
// every wave strides over rows (grid = the resident workgroups), loading the
// next row before computing the current one, writes dx like norm_dx_kernel
// and keeps per-lane dgamma / dbeta sums; at the end the block's 4 waves
// combine them in LDS and store ONE fp32 partial row per block -- plain
// stores, no atomics.  The [blocks, 2H] partials are summed by
// colsum_f32_kernel.
// DS: also the column sums of dx itself (the bias gradient of the Linear
// whose output is this add-norm's residual input): partial rows [3H].
// Two row register sets per wave; 3-4 sets: kernel -2 %, step time within
// noise (profiles/r5/norm_bwd_pf_ab.jsonl).  The block's sums in LDS
// (ds_add_f32) instead of registers: GPT2-1.5B step 108.4 -> 124.7 ms
// (profiles/r5/norm_bwd_ldsacc_ab.jsonl).
template <int VPL, bool RMS, bool DS = false>
__global__ void __launch_bounds__(256, 1)
norm_bwd_part_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const bf16_t* __restrict__ gamma,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in, const bf16_t* __restrict__ dres,
    bf16_t* __restrict__ dx, float* __restrict__ part, int64_t rows, int H) {
  static_assert(VPL <= 2, "one wave per row: H <= 1024");
  __shared__ float red[2][4][512 + 4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nv = H >> 3;
  float ag[VPL][8], ab[VPL][8], ad[VPL][8];
#pragma unroll
  for (int j = 0; j < VPL; ++j)
#pragma unroll
    for (int k = 0; k < 8; ++k) ag[j][k] = ab[j][k] = ad[j][k] = 0.f;
  u32x4 gv[VPL];
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int c = lane + 64 * j;
    if (c < nv) gv[j] = *(const u32x4*)(gamma + c * 8);
  }
  // grid-stride over rows, one row per wave per step, the next row's x / dy
  // / dres (and mean / rstd) loaded before the current one is computed: two
  // named register sets, the loop unrolled by two so nothing is copied
  const int64_t stride = (int64_t)gridDim.x * 4;
  struct Row {
    u32x4 x[VPL], d[VPL], r[VPL];
    float mu, rs;
  };
  auto load = [&](Row& b, int64_t row) {
    if (row >= rows) return;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      const int c = lane + 64 * j;
      if (c < nv) {
        b.x[j] = *(const u32x4*)(x + row * H + c * 8);
        b.d[j] = *(const u32x4*)(dy + row * H + c * 8);
        if (dres) b.r[j] = *(const u32x4*)(dres + row * H + c * 8);
      }
    }
    b.mu = RMS ? 0.f : mean_in[row];
    b.rs = rstd_in[row];
  };
  auto process = [&](const Row& b, int64_t row) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      const int c = lane + 64 * j;
      if (c < nv) {
        float xf[8], df[8], gm[8];
        unpack8(b.x[j], xf);
        unpack8(b.d[j], df);
        unpack8(gv[j], gm);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float a = (xf[k] - b.mu) * b.rs, g = df[k] * gm[k];
          ag[j][k] += df[k] * a;
          if constexpr (!RMS) ab[j][k] += df[k];
          s1 += g;
          s2 += g * a;
        }
      }
    }
    const float m1 = RMS ? 0.f : wave_sum(s1) / (float)H;
    const float m2 = wave_sum(s2) / (float)H;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      const int c = lane + 64 * j;
      if (c < nv) {
        float xf[8], df[8], gm[8], o[8];
        unpack8(b.x[j], xf);  // recomputed: cheaper than 64 more live registers
        unpack8(b.d[j], df);
        unpack8(gv[j], gm);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = b.rs * (df[k] * gm[k] - m1 - (xf[k] - b.mu) * b.rs * m2);
        if (dres) {
          float r[8];
          unpack8(b.r[j], r);
#pragma unroll
          for (int k = 0; k < 8; ++k) o[k] += r[k];
        }
        if constexpr (DS) {
#pragma unroll
          for (int k = 0; k < 8; ++k) ad[j][k] += o[k];
        }
        *(u32x4*)(dx + row * H + c * 8) = pack8(o);
      }
    }
  };
  int64_t row = (int64_t)blockIdx.x * 4 + wid;
  Row A, B;
  load(A, row);
  while (row < rows) {
    load(B, row + stride);
    process(A, row);
    row += stride;
    if (row >= rows) break;
    load(A, row + stride);
    process(B, row);
    row += stride;
  }
  float* prow = part + (int64_t)blockIdx.x * (DS ? 3 : 2) * H;
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      red[0][wid][lane * 8 + k] = ag[j][k];
      if constexpr (!RMS) red[1][wid][lane * 8 + k] = ab[j][k];
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int cl = threadIdx.x + 256 * h;
      const int c = 512 * j + cl;
      if (c < H) {
        prow[c] = red[0][0][cl] + red[0][1][cl] + red[0][2][cl] + red[0][3][cl];
        prow[H + c] = RMS ? 0.f : red[1][0][cl] + red[1][1][cl] + red[1][2][cl] + red[1][3][cl];
      }
    }
    __syncthreads();
    if constexpr (DS) {
#pragma unroll
      for (int k = 0; k < 8; ++k) red[0][wid][lane * 8 + k] = ad[j][k];
      __syncthreads();
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int cl = threadIdx.x + 256 * h;
        const int c = 512 * j + cl;
        if (c < H) prow[2 * H + c] = red[0][0][cl] + red[0][1][cl] + red[0][2][cl] + red[0][3][cl];
      }
      __syncthreads();
    }
  }
}

// Norm backward for 1024 < H < 2048 with TWO waves per row.  One wave per
// row would hold 4 vectors x 3 arrays of a row per lane plus 96 per-lane
// column accumulators: ~310 VGPRs, one wave per SIMD, latency-bound at
// ~3 TB/s.  Here a row is split between a wave pair (each wave 2 vectors per
// lane = half the columns): 48 accumulators, 180-242 VGPRs, two waves per
// SIMD; the row reductions (sum g, sum g a) combine through LDS with one
// barrier per row step (parity double-buffered).  One 8-wave workgroup per CU
// (4 rows in flight, the next row of each pair prefetched) keeps ONE partial
// row per workgroup.  GPT2-1.5B's call (H = 1600, 8192 rows): 38.9 -> 33.2 us
// against one wave per row (profiles/r6/norm_bwd_pair_ab.jsonl).  Two waves
// per SIMD by 512 one-wave workgroups with one row register set instead:
// call 39.0 -> 36.9 us, but the column sums over twice the partial rows 7.6
// -> 10.4 us in the step (profiles/r6/norm_bwd_w2_ab.jsonl).
// Deterministic: a fixed row order per pair and a fixed half-0 + half-1
// order for the row sums.
//
// G = 4 (2048 <= H <= 4096, Llama's 4096): the same with a row split over a
// wave QUAD -- each wave still 2 vectors per lane (1024 columns), two rows
// in flight per workgroup.  Llama-3-8B's call (RMSNorm, 4096 x 4096, residual
// gradient fused) 43.1 -> 32.5 us, 8192 rows 66.7 -> 56.6 us against a
// one-pass kernel with float atomics per block (profiles/r6/norm_bwd_quad_ab.jsonl).
// The dx column sums (DS) exist for G = 2 only: no fold at H >= 2048.
constexpr int NORM_BWD_PAIR_WAVES = 8;  // waves per workgroup: 4 pairs or 2 quads, one workgroup per CU
template <bool RMS, bool DS, int G = 2>
__global__ void __launch_bounds__(64 * NORM_BWD_PAIR_WAVES, 1)
norm_bwd_pair_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const bf16_t* __restrict__ gamma,
                     const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                     const bf16_t* __restrict__ dres, bf16_t* __restrict__ dx, float* __restrict__ part,
                     int64_t rows, int H) {
  static_assert(G == 2 || (G == 4 && !DS), "wave pair, or wave quad without the dx column sums");
  constexpr int NW = NORM_BWD_PAIR_WAVES, NP = NW / G;
  __shared__ float xch[2][NP][G][2];  // [parity][row group][part][sum g, sum g a]
  __shared__ float red[NW][1024];     // per-wave column partials of one array (final reduction)
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int pair = wid / G, half = wid % G;  // row group, column part
  const int nv = H >> 3;
  float ag[2][8], ab[2][8], ad[2][8];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int k = 0; k < 8; ++k) ag[j][k] = ab[j][k] = ad[j][k] = 0.f;
  // this lane's vectors: half * 128 + lane + 64 j (j < 2) cover 0 .. 255
  int vc[2];
  bool vok[2];
  u32x4 gv[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    vc[j] = 128 * half + lane + 64 * j;
    vok[j] = vc[j] < nv;
    gv[j] = vok[j] ? *(const u32x4*)(gamma + vc[j] * 8) : (u32x4){0, 0, 0, 0};
  }
  struct Row {
    u32x4 x[2], d[2], r[2];
    float mu, rs;
  };
  auto load = [&](Row& b, int64_t row) {
    if (row >= rows) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (vok[j]) {
        b.x[j] = *(const u32x4*)(x + row * H + vc[j] * 8);
        b.d[j] = *(const u32x4*)(dy + row * H + vc[j] * 8);
        if (dres) b.r[j] = *(const u32x4*)(dres + row * H + vc[j] * 8);
      }
    }
    b.mu = RMS ? 0.f : mean_in[row];
    b.rs = rstd_in[row];
  };
  auto process = [&](const Row& b, int64_t row, int it) {
    const bool ok = row < rows;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (ok && vok[j]) {
        float xf[8], df[8], gm[8];
        unpack8(b.x[j], xf);
        unpack8(b.d[j], df);
        unpack8(gv[j], gm);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float a = (xf[k] - b.mu) * b.rs, g = df[k] * gm[k];
          ag[j][k] += df[k] * a;
          if constexpr (!RMS) ab[j][k] += df[k];
          s1 += g;
          s2 += g * a;
        }
      }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    float(*xc)[G][2] = xch[it & 1];
    if (lane == 0) {
      xc[pair][half][0] = s1;
      xc[pair][half][1] = s2;
    }
    __syncthreads();  // the only barrier of the row step (the slot of step it-1 stays untouched)
    float t1 = 0.f, t2 = 0.f;  // fixed part order
#pragma unroll
    for (int q = 0; q < G; ++q) {
      t1 += xc[pair][q][0];
      t2 += xc[pair][q][1];
    }
    const float m1 = RMS ? 0.f : t1 / (float)H;
    const float m2 = t2 / (float)H;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (ok && vok[j]) {
        float xf[8], df[8], gm[8], o[8];
        unpack8(b.x[j], xf);
        unpack8(b.d[j], df);
        unpack8(gv[j], gm);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = b.rs * (df[k] * gm[k] - m1 - (xf[k] - b.mu) * b.rs * m2);
        if (dres) {
          float r[8];
          unpack8(b.r[j], r);
#pragma unroll
          for (int k = 0; k < 8; ++k) o[k] += r[k];
        }
        if constexpr (DS) {
#pragma unroll
          for (int k = 0; k < 8; ++k) ad[j][k] += o[k];
        }
        *(u32x4*)(dx + row * H + vc[j] * 8) = pack8(o);
      }
    }
  };
  // every wave of the workgroup runs the same number of row steps (barriers)
  const int64_t stride = (int64_t)gridDim.x * NP;
  const int64_t first = (int64_t)blockIdx.x * NP;
  const int n_it = first < rows ? (int)((rows - first + stride - 1) / stride) : 0;
  int64_t row = first + pair;
  Row A, B;
  load(A, row);
  for (int it = 0; it < n_it; ++it) {
    if (it & 1) {
      load(A, row + stride);
      process(B, row, it);
    } else {
      load(B, row + stride);
      process(A, row, it);
    }
    row += stride;
  }
  // column partials of the workgroup: the 6 waves of each half summed in a fixed order
  float* prow = part + (int64_t)blockIdx.x * (DS ? 3 : 2) * H;
  auto reduce = [&](const float (*acc)[8], int off) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < 8; ++k) red[wid][8 * (lane + 64 * j) + k] = acc[j][k];
    __syncthreads();
    for (int c = threadIdx.x; c < H; c += 64 * NW) {
      const int h = c >> 10, lc = c & 1023;
      float sum = 0.f;
#pragma unroll
      for (int p2 = 0; p2 < NP; ++p2) sum += red[G * p2 + h][lc];
      prow[off + c] = sum;
    }
    __syncthreads();
  };
  reduce(ag, 0);
  if constexpr (!RMS) reduce(ab, H);
  else
    for (int c = threadIdx.x; c < H; c += 64 * NW) prow[H + c] = 0.f;
  if constexpr (DS) reduce(ad, 2 * H);
}

// Column sums of fp32 partials [R, H2 = 2H or 3H] into out0 (columns 0..H-1),
// out1 (H..2H-1, may be null) and out2 (2H..3H-1): thread = column, grid.y
// splits the rows; one atomic per (column, row-split) into ws, the last
// row-split block of each 256-column strip converts (+ accumulates) and
// clears -- colred_kernel's completion protocol.
// ws: fp32 [H2 + ceil(H2/256)], zero on entry and exit.
__global__ void __launch_bounds__(256) colsum_f32_kernel(const float* __restrict__ part, int R, int H2,
                                                         int rows_per_blk, float* __restrict__ ws,
                                                         void* __restrict__ out0, void* __restrict__ out1,
                                                         int is_fp32, int accumulate, int H,
                                                         void* __restrict__ out2, int accumulate2,
                                                         float* __restrict__ detp) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int r0 = blockIdx.y * rows_per_blk, r1 = min(R, r0 + rows_per_blk);
  if (c < H2) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int r = r0;
    for (; r + 4 <= r1; r += 4) {
      a0 += part[(int64_t)r * H2 + c];
      a1 += part[(int64_t)(r + 1) * H2 + c];
      a2 += part[(int64_t)(r + 2) * H2 + c];
      a3 += part[(int64_t)(r + 3) * H2 + c];
    }
    for (; r < r1; ++r) a0 += part[(int64_t)r * H2 + c];
    if (detp)
      __hip_atomic_store(detp + (int64_t)blockIdx.y * H2 + c, (a0 + a1) + (a2 + a3), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    else
      atomicAdd(ws + c, (a0 + a1) + (a2 + a3));
  }
  __shared__ int is_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  unsigned* cnt = (unsigned*)(ws + H2) + blockIdx.x;
  if (threadIdx.x == 0)
    is_last = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.y - 1;
  __syncthreads();
  if (!is_last) return;
  if (c < H2) {
    const float v = detp ? ordered_sum(detp + c, H2, gridDim.y)
                         : __hip_atomic_exchange(ws + c, 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c < H)
      colred_store(out0, c, v, is_fp32, accumulate);
    else if (c < 2 * H)
      colred_store(out1, c - H, v, is_fp32, accumulate);
    else
      colred_store(out2, c - 2 * H, v, is_fp32, accumulate2);  // the folded bias gradient
  }
  if (threadIdx.x == 0) __hip_atomic_exchange(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Grid-size targets (row blocks x 512-column strips) per kernel flavour.
// Fewer row blocks = fewer same-address atomics per column; the plain column
// sum is atomic-bound and wants ~1 block per CU, the fused GELU backward (3
// streams of HBM traffic) wants more memory parallelism.  Measured on
// GPT2-1.5B shapes (scripts/bench_colred.py, profiles/r2/bench_colred.jsonl):
// colsum 8192x1600 16.5 -> 10.9 us at 256 blocks, gelu_bwd_dbias 8192x6400
// 60.9 -> 56.9 us at 2048.
constexpr int COLSUM_BLOCKS = 256, GELU_DBIAS_BLOCKS = 2048, NORM_COLRED_BLOCKS = 1024;

static int colred_rows_per_blk(int64_t rows, int C, int target) {
  const int64_t col_blks = (C + 511) / 512;
  const int64_t rs = (target + col_blks - 1) / col_blks;
  int64_t per = (rows + rs - 1) / rs;
  per = (per + 3) / 4 * 4;
  return (int)(per < 4 ? 4 : per);
}

// ws: fp32 [C + ceil(C/512)] (sums + per-strip completion counters), all-zero on entry, left all-zero.  out (+)= column sums of dy [rows, C].
// det: nullptr (atomic combine) or fp32 scratch of dw_colred_det_floats(rows, C, 0) floats (any content).
extern "C" int dw_colsum_acc(const void* dy, int64_t rows, int C, void* ws, void* out, int out_fp32, int accumulate,
                             void* stream, void* det) {
  if (C % 8 != 0) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int per = colred_rows_per_blk(rows, C, COLSUM_BLOCKS);
  dim3 grid((C + 511) / 512, (unsigned)((rows + per - 1) / per));
  hipLaunchKernelGGL(colred_kernel<0>, grid, dim3(256), 0, s, (const bf16_t*)dy, nullptr, nullptr, nullptr,
                     (float*)ws, rows, C, per, out, nullptr, out_fp32, accumulate, nullptr, (float*)det);
  DW_LAUNCH_RET;
}

// dx = dy * gelu'(pre) [rows, C]; dbias (+)= column sums of dx.  ws as above.
// det: as dw_colsum_acc (dw_colred_det_floats(rows, C, 1) floats).
extern "C" int dw_gelu_bwd_dbias(const void* dy, const void* pre, void* dx, int64_t rows, int C, void* ws,
                                 void* dbias, int out_fp32, int accumulate, void* stream, void* det) {
  if (C % 8 != 0) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int per = colred_rows_per_blk(rows, C, GELU_DBIAS_BLOCKS);
  dim3 grid((C + 511) / 512, (unsigned)((rows + per - 1) / per));
  hipLaunchKernelGGL(colred_kernel<3>, grid, dim3(256), 0, s, (const bf16_t*)dy, (const bf16_t*)pre, nullptr,
                     nullptr, (float*)ws, rows, C, per, dbias, nullptr, out_fp32, accumulate, (bf16_t*)dx,
                     (float*)det);
  DW_LAUNCH_RET;
}

// The norm backward's launch geometry, in one place: the entry launches from
// it, and the callers size ``part`` and the deterministic scratch from it.
// Which kernels run depends on (H, rms, dsum given) only.
enum NormBwdPath {
  NORM_BWD_WAVE,     // H <= 1024: norm_bwd_part_kernel + colsum_f32_kernel
  NORM_BWD_PAIR,     // 1024 < H < 2048: norm_bwd_pair_kernel<G = 2> + colsum_f32_kernel
  NORM_BWD_QUAD,     // 2048 <= H <= 4096: norm_bwd_pair_kernel<G = 4> + colsum_f32_kernel
  NORM_BWD_TWO_PASS  // 4096 < H <= 8192: norm_dx_kernel + colred_kernel<1 or 2>
};
struct NormBwdPlan {
  NormBwdPath path;
  int64_t blocks;       // workgroups of the row kernel
  int threads;          // per workgroup
  int64_t part_floats;  // one partial row [2H, or 3H with dsum] per workgroup; 0 on the two-pass path
  int red_per;          // second kernel: partial rows (two-pass: rows of dy) per block ...
  int64_t red_splits;   // ... and its grid.y
  int64_t det_floats;   // deterministic mode: one partial row per grid.y of the second kernel
};

static NormBwdPlan norm_bwd_plan(int64_t rows, int H, bool with_dsum) {
  NormBwdPlan p;
  p.path = H <= 1024 ? NORM_BWD_WAVE : H < 2048 ? NORM_BWD_PAIR : H <= 4096 ? NORM_BWD_QUAD : NORM_BWD_TWO_PASS;
  if (p.path == NORM_BWD_TWO_PASS) {
    p.blocks = (rows + 3) / 4;  // one wave per row
    p.threads = 256;
    p.part_floats = 0;
    p.red_per = colred_rows_per_blk(rows, H, NORM_COLRED_BLOCKS);
    p.red_splits = (rows + p.red_per - 1) / p.red_per;
    p.det_floats = p.red_splits * 2 * H;
    return p;
  }
  // every workgroup resident at once, its waves striding over the rows: two
  // 4-wave workgroups per CU (a row per wave), or one 8-wave workgroup per CU
  // (4 wave pairs or 2 wave quads, a row each)
  const int rows_per_step = p.path == NORM_BWD_QUAD ? NORM_BWD_PAIR_WAVES / 4 : 4;
  p.blocks = std::min<int64_t>((rows + rows_per_step - 1) / rows_per_step, p.path == NORM_BWD_WAVE ? 512 : 256);
  p.threads = p.path == NORM_BWD_WAVE ? 256 : 64 * NORM_BWD_PAIR_WAVES;
  const int64_t pw = with_dsum ? 3 : 2;
  p.part_floats = p.blocks * pw * H;
  const int64_t splits = std::max<int64_t>(1, std::min<int64_t>(64, p.blocks / 16));
  p.red_per = (int)((p.blocks + splits - 1) / splits);
  p.red_splits = (p.blocks + p.red_per - 1) / p.red_per;
  p.det_floats = p.red_splits * pw * H;
  return p;
}

// fp32 scratch the deterministic mode needs (kind 0: dw_colsum_acc, 1:
// dw_gelu_bwd_dbias, 2: dw_norm_bwd with or without dsum): one partial row
// per row-block.
extern "C" int64_t dw_colred_det_floats(int64_t rows, int C, int kind) {
  if (kind == 2) return norm_bwd_plan(rows, C, C < 2048).det_floats;
  const int per = colred_rows_per_blk(rows, C, kind == 0 ? COLSUM_BLOCKS : GELU_DBIAS_BLOCKS);
  return (rows + per - 1) / per * C;
}

// Floats of dw_norm_bwd's ``part`` scratch; 0 for H > 4096 (no partial rows).
extern "C" int64_t dw_norm_bwd_part_floats(int64_t rows, int H, int with_dsum) {
  return norm_bwd_plan(rows, H, with_dsum != 0).part_floats;
}

using NormRowKernel = void (*)(const bf16_t*, const bf16_t*, const bf16_t*, const float*, const float*, const bf16_t*,
                               bf16_t*, float*, int64_t, int);
template <bool RMS, bool DS>
static NormRowKernel norm_row_kernel(NormBwdPath path, int H) {
  if (path == NORM_BWD_WAVE) return H <= 512 ? norm_bwd_part_kernel<1, RMS, DS> : norm_bwd_part_kernel<2, RMS, DS>;
  if (path == NORM_BWD_PAIR) return norm_bwd_pair_kernel<RMS, DS, 2>;
  if constexpr (!DS) return norm_bwd_pair_kernel<RMS, false, 4>;
  return nullptr;  // dsum at H >= 2048: rejected by the entry
}

// LayerNorm / RMSNorm backward: dx = norm_bwd(dy) [+ dres], dgamma / dbeta (+)= their column sums.
// H % 8 == 0, H <= 8192; dbeta may be null (RMSNorm, LayerNorm without bias), dgamma not.
// dres (nullable): gradient of the residual sum that this norm's input also
// feeds (fused add+norm) -> dx += dres.
// dsum (nullable, H < 2048 only): column sums of dx (same dtype as dgamma)
// -- the bias gradient of the Linear that produced the residual input.
// accumulate: bit 0 -- dgamma / dbeta accumulate; bit 1 -- dsum is
// OVERWRITTEN (its parameter's first gradient contribution of the step),
// else accumulated.
// ws: fp32 [3H + max(ceil(H/512), ceil(3H/256))] -- the sums and strip
// counters of colsum_f32_kernel over <= 3H columns, or of colred_kernel over
// 2H -- all-zero on entry, left all-zero.
// part: fp32 scratch of part_floats >= dw_norm_bwd_part_floats(rows, H, dsum != null) floats (any content).
// det: nullptr, or fp32 scratch of dw_colred_det_floats(rows, H, 2) floats
// (any content): deterministic weight gradients, the same kernels with
// ordered partials instead of float atomics.
// Returns hipErrorInvalidValue, with nothing launched, for arguments outside this contract.
extern "C" int dw_norm_bwd(const void* dy, const void* x, const void* gamma, const void* mean, const void* rstd,
                           const void* dres, void* dx, void* dgamma, void* dbeta, void* ws, void* part,
                           int64_t part_floats, int64_t rows, int H, int rms, int out_fp32, int accumulate,
                           void* dsum, void* stream, void* det) {
  if (rows < 1 || H < 8 || H % 8 != 0 || H > 8192 || !dgamma || (dsum && H >= 2048)) return (int)hipErrorInvalidValue;
  const NormBwdPlan p = norm_bwd_plan(rows, H, dsum != nullptr);
  if (p.part_floats && (!part || part_floats < p.part_floats)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  const int acc = accumulate & 1, acc_dsum = (accumulate & 2) ? 0 : 1;
  if (p.path == NORM_BWD_TWO_PASS) {
    hipLaunchKernelGGL((rms ? norm_dx_kernel<16, true> : norm_dx_kernel<16, false>), dim3((unsigned)p.blocks),
                       dim3(p.threads), 0, s, (const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)gamma,
                       (const float*)mean, (const float*)rstd, (const bf16_t*)dres, (bf16_t*)dx, rows, H);
    // both halves of ws are consumed (and cleared) even if dbeta is absent
    hipLaunchKernelGGL(rms ? colred_kernel<2> : colred_kernel<1>, dim3((H + 511) / 512, (unsigned)p.red_splits),
                       dim3(256), 0, s, (const bf16_t*)dy, (const bf16_t*)x, (const float*)mean, (const float*)rstd,
                       (float*)ws, rows, H, p.red_per, dgamma, rms ? nullptr : dbeta, out_fp32, acc, (bf16_t*)nullptr,
                       (float*)det);
    DW_LAUNCH_RET;
  }
  const NormRowKernel row_kernel =
      rms ? (dsum ? norm_row_kernel<true, true> : norm_row_kernel<true, false>)(p.path, H)
          : (dsum ? norm_row_kernel<false, true> : norm_row_kernel<false, false>)(p.path, H);
  hipLaunchKernelGGL(row_kernel, dim3((unsigned)p.blocks), dim3(p.threads), 0, s, (const bf16_t*)dy, (const bf16_t*)x,
                     (const bf16_t*)gamma, (const float*)mean, (const float*)rstd, (const bf16_t*)dres, (bf16_t*)dx,
                     (float*)part, rows, H);
  const int H2 = (dsum ? 3 : 2) * H;
  hipLaunchKernelGGL(colsum_f32_kernel, dim3((H2 + 255) / 256, (unsigned)p.red_splits), dim3(256), 0, s,
                     (const float*)part, (int)p.blocks, H2, p.red_per, (float*)ws, dgamma, rms ? nullptr : dbeta,
                     out_fp32, acc, H, dsum, acc_dsum, (float*)det);
  DW_LAUNCH_RET;
}

DW_PRELOAD(colred_kernel<0>);
