// MoE token movement around the experts (ops/moe.py; parallel/moe.py MoELayer):
// expert sort, row gather (dispatch) and k-way row sum (combine).
//
// sort:   the flat top-k assignment idx[n] (n = T k, int64 in [0, nb),
//         nb <= 1025: the experts plus the capacity path's sentinel bucket)
//         -> counts[nb], order[n] (grouped row -> flat assignment, exactly
//         argsort(stable)) and pos[n] (its inverse).  A stable counting sort
//         in three launches: (1) every wave histograms its contiguous
//         512-assignment slice (a block of 4 waves covers a 2048 chunk) in
//         LDS; (2) one block turns the [slice, bucket] histogram into
//         exclusive offsets, bucket-major then slice-minor; (3) every wave
//         walks its slice 64 assignments at a time in order and ranks equal
//         buckets with ballot / popcount against its LDS cursors.
// gather: out[r] = r < n_valid ? scale[order[r]] * src[order[r] / k] : 0, one
//         wave per row.  Dispatch forward (no scale); with scale = w and
//         src = dout the combine's dy, and in the same pass
//         dw[order[r]] = sum_h y[r, h] dout[order[r] / k, h] (0 past n_valid).
// ksum:   out[t] = sum_{j < k, pos[t k + j] < n_valid} s_j src[pos[t k + j]],
//         fp32 in the fixed order j = 0..k-1, one rounding to bf16.  Combine
//         forward (s = w) and dispatch backward (s = 1): the per-destination
//         sum through the inverted index instead of float atomics -- every
//         token has exactly k contributions, so the waves are evenly loaded
//         and the result is bitwise reproducible.
// n_valid = n - counts[sentinel] is read on the device; rows at or past it
// (dropped assignments, sorted last) are never read: they may hold anything.
//
// Parity: reference atorch/modules/moe/grouped_gemm_moe.py (megablocks
// ops.sort / histogram / gather / scatter).
#include "dw_common.h"

constexpr int ST_MAXNB = 1025;
constexpr int ST_WAVES = 4;
constexpr int ST_SLICE = 512;                    // assignments per wave
constexpr int ST_CHUNK = ST_WAVES * ST_SLICE;    // per block

static inline int sort_blocks(int64_t n) { return (int)((n + ST_CHUNK - 1) / ST_CHUNK); }

__device__ __forceinline__ int sort_bucket(const int64_t* idx, int64_t i, int nb) {
  const int64_t v = idx[i];
  return v < 0 ? 0 : (v >= nb ? nb - 1 : (int)v);  // out-of-range input cannot leave the LDS tables
}

__global__ void __launch_bounds__(256) moe_sort_hist_kernel(const int64_t* __restrict__ idx, int64_t n, int nb,
                                                           int* __restrict__ hist) {
  __shared__ int cnt[ST_WAVES][ST_MAXNB];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int e = lane; e < nb; e += 64) cnt[wid][e] = 0;
  __syncthreads();
  const int64_t unit = (int64_t)blockIdx.x * ST_WAVES + wid;
  const int64_t start = unit * ST_SLICE;
  const int64_t end = start + ST_SLICE < n ? start + ST_SLICE : n;
  for (int64_t i = start + lane; i < end; i += 64) atomicAdd(&cnt[wid][sort_bucket(idx, i, nb)], 1);
  __syncthreads();
  for (int e = lane; e < nb; e += 64) hist[unit * nb + e] = cnt[wid][e];
}

// hist[u][e] -> number of bucket-e assignments in slices before u; base[e] ->
// first grouped row of bucket e; counts[e] (int64).
__global__ void __launch_bounds__(256) moe_sort_scan_kernel(int* __restrict__ hist, int units, int nb,
                                                           int* __restrict__ base, int64_t* __restrict__ counts) {
  __shared__ int tot[5 * 256];
  __shared__ int wtot[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int e = tid; e < 5 * 256; e += 256) {
    int run = 0;
    if (e < nb) {
      for (int u = 0; u < units; ++u) {
        const int c = hist[(int64_t)u * nb + e];
        hist[(int64_t)u * nb + e] = run;
        run += c;
      }
      counts[e] = run;
    }
    tot[e] = run;
  }
  __syncthreads();
  int loc[5], s = 0;
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    loc[q] = tot[5 * tid + q];
    s += loc[q];
  }
  int inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wtot[wid] = inc;
  __syncthreads();
  int run = inc - s;
  for (int wv = 0; wv < wid; ++wv) run += wtot[wv];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const int e = 5 * tid + q;
    if (e < nb) base[e] = run;
    run += loc[q];
  }
}

__global__ void __launch_bounds__(256) moe_sort_rank_kernel(const int64_t* __restrict__ idx, int64_t n, int nb,
                                                           const int* __restrict__ hist,
                                                           const int* __restrict__ base, int* __restrict__ order,
                                                           int* __restrict__ pos) {
  __shared__ int cur_s[ST_WAVES][ST_MAXNB];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t unit = (int64_t)blockIdx.x * ST_WAVES + wid;
  for (int e = lane; e < nb; e += 64) cur_s[wid][e] = base[e] + hist[unit * nb + e];
  __syncthreads();
  volatile int* cur = cur_s[wid];
  const int64_t start = unit * ST_SLICE;
  const int64_t end = start + ST_SLICE < n ? start + ST_SLICE : n;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t r0 = start; r0 < end; r0 += 64) {
    const int64_t i = r0 + lane;
    const bool active = i < end;
    const int v = active ? sort_bucket(idx, i, nb) : -1;
    unsigned long long todo = __ballot(active);
    int r = 0;
    while (todo) {  // one round per distinct bucket among the 64, wave-uniform
      const int leader = __ffsll(todo) - 1;
      const int bv = __shfl(v, leader, 64);
      const unsigned long long m = __ballot(v == bv);
      const int c = cur[bv];
      if (v == bv) r = c + __popcll(m & below);
      if (lane == leader) cur[bv] = c + __popcll(m);
      todo &= ~m;
    }
    if (active) {
      order[r] = (int)i;
      pos[i] = r;
    }
  }
}

// SCALE = 0: plain row copy.  SCALE = 1: rows scaled by scale[order[r]] and,
// when y / dw are given, dw[order[r]] = <y[r], src row>.
template <int SCALE>
__global__ void __launch_bounds__(256) moe_gather_rows_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ out,
                                                             const int* __restrict__ order,
                                                             const float* __restrict__ scale,
                                                             const bf16_t* __restrict__ y, float* __restrict__ dw,
                                                             const int64_t* __restrict__ counts, int sentinel,
                                                             int64_t n_rows, int64_t n, int k, int H) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int64_t n_valid = counts ? n - counts[sentinel] : n;
  const int nvec = H >> 3;
  for (int64_t r = wave; r < n_rows; r += nwaves) {
    const int a = order[r];
    u32x4* d = (u32x4*)(out + r * H);
    if (r >= n_valid) {
      const u32x4 z = {0u, 0u, 0u, 0u};
      for (int v = lane; v < nvec; v += 64) d[v] = z;
      if (SCALE && dw && lane == 0) dw[a] = 0.f;
      continue;
    }
    const u32x4* s = (const u32x4*)(src + (int64_t)(a / k) * H);
    if (!SCALE) {
      for (int v = lane; v < nvec; v += 64) d[v] = s[v];
    } else {
      const float sc = scale[a];
      const u32x4* yr = y ? (const u32x4*)(y + r * H) : nullptr;
      float dot = 0.f;
      for (int v = lane; v < nvec; v += 64) {
        float f[8];
        unpack8(s[v], f);
        if (yr) {
          float g[8];
          unpack8(yr[v], g);
#pragma unroll
          for (int q = 0; q < 8; ++q) dot += g[q] * f[q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) f[q] *= sc;
        d[v] = pack8(f);
      }
      if (dw) {
        dot = wave_sum(dot);
        if (lane == 0) dw[a] = dot;
      }
    }
  }
}

__global__ void __launch_bounds__(256) moe_ksum_rows_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ out,
                                                           const int* __restrict__ pos,
                                                           const float* __restrict__ scale,
                                                           const int64_t* __restrict__ counts, int sentinel,
                                                           int64_t T, int64_t n, int64_t src_rows, int k, int H) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  int64_t n_valid = counts ? n - counts[sentinel] : n;
  if (n_valid > src_rows) n_valid = src_rows;
  const int nvec = H >> 3;
  for (int64_t t = wave; t < T; t += nwaves) {
    // lane j < k: the grouped row of the token's j-th assignment (-1: dropped)
    int pj = -1;
    float sj = 1.f;
    if (lane < k) {
      pj = pos[t * k + lane];
      if (scale) sj = scale[t * k + lane];
      if (pj >= n_valid) pj = -1;
    }
    u32x4* d = (u32x4*)(out + t * H);
    for (int v0 = 0; v0 < nvec; v0 += 64) {  // wave-uniform trip count: the shuffles see all lanes
      const int v = v0 + lane;
      float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < k; ++j) {
        const int p = __shfl(pj, j, 64);
        const float sc = __shfl(sj, j, 64);
        if (p >= 0 && v < nvec) {
          float f[8];
          unpack8(((const u32x4*)(src + (int64_t)p * H))[v], f);
#pragma unroll
          for (int q = 0; q < 8; ++q) acc[q] += sc * f[q];
        }
      }
      if (v < nvec) d[v] = pack8(acc);
    }
  }
}

// int32 words of the sort workspace (any content on entry)
extern "C" int64_t dw_moe_sort_ws_size(int64_t n, int nb) {
  return (int64_t)sort_blocks(n) * ST_WAVES * nb + nb;
}
extern "C" int dw_moe_sort_chunk_size() { return ST_CHUNK; }

// idx [n] int64 in [0, nb); counts [nb] int64; order / pos [n] int32; ws: dw_moe_sort_ws_size int32 words.
extern "C" int dw_moe_sort(const void* idx, int64_t n, int nb, void* counts, void* order, void* pos, void* ws,
                           void* stream) {
  if (n <= 0 || n > 0x7fffffffLL - ST_CHUNK || nb < 1 || nb > ST_MAXNB) return (int)hipErrorInvalidValue;
  const int blocks = sort_blocks(n), units = blocks * ST_WAVES;
  int* hist = (int*)ws;
  int* base = hist + (int64_t)units * nb;
  hipLaunchKernelGGL(moe_sort_hist_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const int64_t*)idx, n,
                     nb, hist);
  hipLaunchKernelGGL(moe_sort_scan_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, hist, units, nb, base,
                     (int64_t*)counts);
  hipLaunchKernelGGL(moe_sort_rank_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const int64_t*)idx, n,
                     nb, (const int*)hist, (const int*)base, (int*)order, (int*)pos);
  DW_LAUNCH_RET;
}

// out [n_rows, H] bf16 (n_rows <= n); src [*, H] bf16, row order[r] / k of it feeds row r; scale [n] fp32 or null;
// y [n_rows, H] + dw [n] fp32 (both or neither, only with scale); counts int64 with the sentinel bucket at
// counts[sentinel], or null when every row is valid.
extern "C" int dw_moe_gather_rows(const void* src, void* out, const void* order, const void* scale, const void* y,
                                  void* dw, const void* counts, int sentinel, int64_t n_rows, int64_t n, int k,
                                  int H, void* stream) {
  if (n_rows < 0 || n_rows > n || k < 1 || H < 8 || (H & 7) || ((y != nullptr) != (dw != nullptr)) ||
      (y && !scale))
    return (int)hipErrorInvalidValue;
  if (n_rows == 0) return 0;
  const int grid = dw_grid_for(n_rows, 4, 4096);
  if (scale)
    hipLaunchKernelGGL(moe_gather_rows_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)src, (bf16_t*)out, (const int*)order, (const float*)scale, (const bf16_t*)y,
                       (float*)dw, (const int64_t*)counts, sentinel, n_rows, n, k, H);
  else
    hipLaunchKernelGGL(moe_gather_rows_kernel<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)src, (bf16_t*)out, (const int*)order, (const float*)nullptr,
                       (const bf16_t*)nullptr, (float*)nullptr, (const int64_t*)counts, sentinel, n_rows, n, k, H);
  DW_LAUNCH_RET;
}

// out [T, H] bf16; src [src_rows, H] bf16; pos [T k] int32; scale [T k] fp32 or null (1).
extern "C" int dw_moe_ksum_rows(const void* src, void* out, const void* pos, const void* scale, const void* counts,
                                int sentinel, int64_t T, int64_t src_rows, int k, int H, void* stream) {
  if (T < 0 || src_rows < 0 || k < 1 || k > 64 || H < 8 || (H & 7)) return (int)hipErrorInvalidValue;
  if (T == 0) return 0;
  hipLaunchKernelGGL(moe_ksum_rows_kernel, dim3(dw_grid_for(T, 4, 4096)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)src, (bf16_t*)out, (const int*)pos, (const float*)scale,
                     (const int64_t*)counts, sentinel, T, T * k, src_rows, k, H);
  DW_LAUNCH_RET;
}

DW_PRELOAD(moe_sort_hist_kernel);
DW_PRELOAD(moe_sort_scan_kernel);
DW_PRELOAD(moe_sort_rank_kernel);
DW_PRELOAD(moe_gather_rows_kernel<0>);
DW_PRELOAD(moe_gather_rows_kernel<1>);
DW_PRELOAD(moe_ksum_rows_kernel);
