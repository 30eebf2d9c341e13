// Skinny-M weight-streaming GEMM for the RL decode step (ops/skinny_gemm.py,
// docs/rl_fp8_rollouts.md):
//
//   y[M, N] = (x[M, K] . W[N, K]^T) * scale[N],   1 <= M <= 64, K % 16 == 0
//
// x bf16 (rows 16-byte aligned), y bf16, W row-major [N, K] either bf16 (no
// scale) or OCP e4m3 codes with an fp32 scale per output row.  One decode
// step reads every weight once, so the kernel is a stream over W:
//
//  * a block is 4 waves = 64 rows of W (one 16-row strip per wave) over one
//    K slice; each lane reads W with 16-byte non-temporal loads straight into
//    VGPRs (8 bf16 or 16 e4m3 of one row) and keeps one whole 256-deep k tile
//    of them in flight while it computes the previous one -- no LDS for W;
//  * x is shared by the block's waves: its [M, 256] tile goes through LDS in
//    full 512-byte rows (two buffers, one barrier per tile, 16-byte groups
//    XOR-swizzled by the row so reads and writes are conflict-free) and is
//    read back as MFMA A fragments with ds_read_b128;
//  * e4m3 -> bf16 is exact (3 mantissa bits): the codes are widened in
//    registers (v_cvt_pk_f32_fp8, keep the high halves) and feed the same
//    v_mfma_f32_16x16x32_bf16 as the bf16 form.  A lane's 16 codes are 16
//    consecutive k, so the two MFMAs of a 64-deep fp8 chunk see k in the
//    order (lane group, half, element); x fragments are read to match;
//  * rows of x beyond 16 are further accumulators over the same W registers;
//  * split K (N = 4096 is only 64 blocks): slice s owns chunks
//    [nchunks s / S, nchunks (s + 1) / S) and writes an fp32 slab
//    part[s][M][N]; a second launch adds the slabs in the order s = 0..S-1,
//    scales and rounds once.  No float atomics: bit-reproducible for a given S.
//
// Edges: a W row past N and an x row past M are clamped to the last one (the
// results are not stored); a 16-byte group at k >= the slice end is read at
// the slice start and replaced by zeros in both operands.
//
// dw_quant_rows_e4m3: the per-row quantiser that fills the e4m3 copy.
#include "dw_common.h"

namespace {

constexpr int SG_BK = 256;                 // k per staged x tile
constexpr int SG_PITCH = SG_BK * 2;        // LDS row pitch in bytes; 16-byte group q of row r sits at q ^ (r & 15)
constexpr int SG_BN = 64;                  // W rows per block: 4 waves x 16

// two exact floats -> packed bf16 pair (their high halves)
__device__ __forceinline__ unsigned hi_halves(float lo, float hi) {
  return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);
}

// 8 e4m3 codes (two words) -> 8 bf16
__device__ __forceinline__ bf16x8_t e4m3x8_to_bf16(unsigned w0, unsigned w1) {
  const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, true);
  const auto c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, true);
  const u32x4 v = {hi_halves(a[0], a[1]), hi_halves(b[0], b[1]), hi_halves(c[0], c[1]), hi_halves(d[0], d[1])};
  return __builtin_bit_cast(bf16x8_t, v);
}

template <bool FP8, int MT>
__global__ void __launch_bounds__(256) skinny_gemm_kernel(const bf16_t* __restrict__ x, long long ldx,
                                                          const unsigned char* __restrict__ W,
                                                          const float* __restrict__ scale, bf16_t* __restrict__ y,
                                                          float* __restrict__ part, int M, int N, int K, int splits) {
  constexpr int EPL = FP8 ? 16 : 8;      // W elements per lane and load
  constexpr int ES = FP8 ? 1 : 2;        // bytes per W element
  constexpr int KC = 4 * EPL;            // k per chunk (one load per lane)
  constexpr int CH = SG_BK / KC;         // chunks per tile
  __shared__ __attribute__((aligned(16))) unsigned char xs[2][MT * 16 * SG_PITCH];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c16 = lane & 15;
  const int n0 = blockIdx.x * SG_BN + wave * 16;
  const int nchunks = (K + KC - 1) / KC;
  const int s = blockIdx.y;
  const int kb = (int)((long long)nchunks * s / splits) * KC;
  const int ke = min((int)((long long)nchunks * (s + 1) / splits) * KC, K);
  const int T = (ke - kb + SG_BK - 1) / SG_BK;   // >= 1: the launcher keeps splits <= nchunks

  const unsigned char* wrow = W + (long long)min(n0 + c16, N - 1) * K * ES;
  // x staging: thread -> (row tid >> 5 of an 8-row pass, 16-byte group tid & 31)
  const int xr_row = tid >> 5, xq = tid & 31;

  u32x4 w0[CH], w1[CH], xr[2 * MT];   // W of the tile in LDS buffer 0 / 1
  unsigned ok0 = 0, ok1 = 0;
  bool x_ok = false;

  // A 16-byte group past the slice end is read at the slice start instead
  // (every address stays in bounds) and zeroed later.  No load sits in a
  // branch: at a join the compiler would wait for everything outstanding.
  auto load_x = [&](int t) {
    const int k = kb + t * SG_BK + xq * 8;
    x_ok = k < ke;
    const int kk = x_ok ? k : kb;
#pragma unroll
    for (int p = 0; p < 2 * MT; ++p) {
      const int row = min(p * 8 + xr_row, M - 1);
      xr[p] = *(const u32x4*)(x + row * ldx + kk);
    }
  };
  // tail (block-uniform): the tile reaches past the slice end.  The select
  // lives only on that path, so the loads above it stay unconditional.
  auto write_x = [&](int buf, bool tail) {
    unsigned char* dst = xs[buf] + xr_row * SG_PITCH;
    if (tail) {
#pragma unroll
      for (int p = 0; p < 2 * MT; ++p)
        *(u32x4*)(dst + p * 8 * SG_PITCH + ((xq ^ ((p * 8 + xr_row) & 15)) * 16)) =
            x_ok ? xr[p] : (u32x4){0u, 0u, 0u, 0u};
    } else {
#pragma unroll
      for (int p = 0; p < 2 * MT; ++p)
        *(u32x4*)(dst + p * 8 * SG_PITCH + ((xq ^ ((p * 8 + xr_row) & 15)) * 16)) = xr[p];
    }
  };
  auto load_w = [&](int t, u32x4* w, unsigned& ok) {
    ok = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int k = kb + t * SG_BK + c * KC + g * EPL;
      const bool v = k < ke;
      ok |= (unsigned)v << c;
      w[c] = __builtin_nontemporal_load((const u32x4*)(wrow + (long long)(v ? k : kb) * ES));
    }
  };

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int buf, const u32x4* w, unsigned ok, bool tail) {
    // fragment rows are 16 mt + c16: the swizzle term is c16 for every mt
    const unsigned char* xa = xs[buf] + c16 * SG_PITCH;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const u32x4 wv = (!tail || ((ok >> c) & 1u)) ? w[c] : (u32x4){0u, 0u, 0u, 0u};
      if (FP8) {
        const bf16x8_t b0 = e4m3x8_to_bf16(wv[0], wv[1]), b1 = e4m3x8_to_bf16(wv[2], wv[3]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const unsigned char* p = xa + mt * 16 * SG_PITCH;
          const int q = c * 8 + g * 2;   // 16-byte groups q, q + 1: k = 64 c + 16 g + {0..7, 8..15}
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)(p + ((q ^ c16) * 16)), b0, acc[mt],
                                                            0, 0, 0);
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)(p + (((q + 1) ^ c16) * 16)), b1,
                                                            acc[mt], 0, 0, 0);
        }
      } else {
        const bf16x8_t b = __builtin_bit_cast(bf16x8_t, wv);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              *(const bf16x8_t*)(xa + mt * 16 * SG_PITCH + (((c * 4 + g) ^ c16) * 16)), b, acc[mt], 0, 0, 0);
      }
    }
  };

  // x first, W behind it: the wait for x then leaves the W loads in flight.
  // No branch around a load (a wave past N streams row N - 1 again): at a
  // join the compiler would have to wait for everything outstanding.
  const bool partial = (ke - kb) % SG_BK != 0;   // only the slice's last tile can be
  load_x(0);
  load_w(0, w0, ok0);
  write_x(0, T == 1 && partial);
  __syncthreads();
  // two tiles per trip, so the W registers alternate without a copy (a copy
  // would wait for the loads it moves)
  for (int t = 0;;) {
    if (t + 1 == T) {
      compute(0, w0, ok0, partial);
      break;
    }
    load_x(t + 1);
    load_w(t + 1, w1, ok1);
    compute(0, w0, ok0, false);
    write_x(1, t + 2 == T && partial);   // buffer 1 was last read before the previous barrier
    __syncthreads();
    ++t;
    if (t + 1 == T) {
      compute(1, w1, ok1, partial);
      break;
    }
    load_x(t + 1);
    load_w(t + 1, w0, ok0);
    compute(1, w1, ok1, false);
    write_x(0, t + 2 == T && partial);
    __syncthreads();
    ++t;
  }

  // C layout: column (n) = lane & 15, row (m) = 4 (lane >> 4) + r
  const int n = n0 + c16;
  if (n >= N) return;
  const float sc = scale ? scale[n] : 1.f;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = mt * 16 + g * 4 + r;
      if (m >= M) continue;
      if (splits == 1)
        y[(long long)m * N + n] = f2bf(acc[mt][r] * sc);
      else
        part[((long long)s * M + m) * N + n] = acc[mt][r];
    }
}

// y = bf16((sum over slabs in order) * scale)
__global__ void __launch_bounds__(256) skinny_gemm_combine_kernel(const float* __restrict__ part,
                                                                  const float* __restrict__ scale,
                                                                  bf16_t* __restrict__ y, long long MN, int N,
                                                                  int splits) {
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < MN; i += (long long)gridDim.x * 256) {
    float a = part[i];
    for (int s = 1; s < splits; ++s) a += part[(long long)s * MN + i];
    y[i] = f2bf(a * (scale ? scale[i % N] : 1.f));
  }
}

__device__ __forceinline__ unsigned e4m3x4(float a, float b, float c, float d) {
  unsigned w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return w;
}
// saturate, NaN passes through (as fp8.hip)
__device__ __forceinline__ float sat448(float v) { return v != v ? v : fminf(fmaxf(v, -448.f), 448.f); }

// One block per row (grid-stride): amax of the row, scale = amax / 448 (1 for
// an all-zero row), then the row again (from L2) -> codes.
__global__ void __launch_bounds__(256) quant_rows_e4m3_kernel(const bf16_t* __restrict__ w,
                                                              unsigned char* __restrict__ codes,
                                                              float* __restrict__ scale, int N, int K) {
  __shared__ float red[4];
  const int nvec = K >> 3;
  for (int row = blockIdx.x; row < N; row += gridDim.x) {
    const u32x4* src = (const u32x4*)(w + (long long)row * K);
    float f[8], m = 0.f;
    for (int v = threadIdx.x; v < nvec; v += 256) {
      unpack8(src[v], f);
#pragma unroll
      for (int i = 0; i < 8; ++i) m = fmaxf(m, fabsf(f[i]));
    }
    m = block_max<256>(m, red);
    const float sc = m > 0.f ? m / 448.f : 1.f;
    if (threadIdx.x == 0) scale[row] = sc;
    uint2* dst = (uint2*)(codes + (long long)row * K);
    for (int v = threadIdx.x; v < nvec; v += 256) {
      unpack8(src[v], f);
#pragma unroll
      for (int i = 0; i < 8; ++i) f[i] = sat448(f[i] / sc);
      dst[v] = make_uint2(e4m3x4(f[0], f[1], f[2], f[3]), e4m3x4(f[4], f[5], f[6], f[7]));
    }
  }
}

}  // namespace

// The kernel's own K split: a function of (M, N, K) only (today of N and K).
// About one block per CU: a block keeps a whole k tile per wave in flight, and
// blocks beyond the 256 CUs run as a second, partly empty round (measured:
// N = 4096 is fastest at 4 slices = 256 blocks, N = 6144 at 4 = 384, N = 28672
// at 1 = 448; docs/rl_fp8_rollouts.md).  A power of two, so that the usual K
// gives every slice the same number of tiles; never fewer than two x tiles
// per slice, at most 16 slices.
extern "C" int dw_skinny_gemm_splits(int M, int N, int K) {
  (void)M;
  const int nb = (N + SG_BN - 1) / SG_BN, ntiles = (K + SG_BK - 1) / SG_BK;
  int s = 1;
  while (s < 16 && nb * (2 * s) <= 384 && 2 * s <= ntiles / 2) s *= 2;
  return s;
}

// The number of K slices a launch runs: the request (0 = dw_skinny_gemm_splits)
// clamped to the number of k chunks (32 k bf16, 64 k e4m3).  The one place the
// rule lives: the launcher and the workspace sizing of ops/skinny_gemm.py
// (splits * M * N floats when it is above 1) both ask here.
extern "C" int dw_skinny_gemm_plan(int M, int N, int K, int w_fp8, int splits) {
  const int kc = w_fp8 ? 64 : 32, nchunks = (K + kc - 1) / kc;
  if (splits <= 0) splits = dw_skinny_gemm_splits(M, N, K);
  if (splits > nchunks) splits = nchunks;
  return splits < 1 ? 1 : splits;
}

// x [M, K] bf16 with row stride ldx elements (ldx % 8 == 0, 16-byte aligned),
// w [N, K] bf16 (w_fp8 = 0) or e4m3 codes (1), 16-byte aligned; scale fp32 [N]
// or null; y [M, N] bf16 contiguous.  splits: as dw_skinny_gemm_plan.  ws: fp32
// scratch of ws_floats >= plan * M * N (unused when the plan is 1).
extern "C" int dw_skinny_gemm(const void* x, long long ldx, const void* w, int w_fp8, const float* scale, void* y,
                              float* ws, long long ws_floats, int M, int N, int K, int splits, void* stream) {
  if (M < 1 || M > 64 || N < 1 || K < 16 || K % 16 || ldx % 8 || ldx < K || splits < 0)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)x | (uintptr_t)w) & 15) return (int)hipErrorInvalidValue;
  splits = dw_skinny_gemm_plan(M, N, K, w_fp8, splits);
  if (splits > 1 && (!ws || ws_floats < (long long)splits * M * N)) return (int)hipErrorInvalidValue;
  const dim3 grid((N + SG_BN - 1) / SG_BN, splits);
  hipStream_t st = (hipStream_t)stream;
  const int mt = (M + 15) / 16;
#define L(F, T)                                                                                              \
  hipLaunchKernelGGL((skinny_gemm_kernel<F, T>), grid, dim3(256), 0, st, (const bf16_t*)x, ldx,              \
                     (const unsigned char*)w, scale, (bf16_t*)y, ws, M, N, K, splits)
#define LM(F)                                                                                                \
  switch (mt) {                                                                                              \
    case 1: L(F, 1); break;                                                                                  \
    case 2: L(F, 2); break;                                                                                  \
    case 3: L(F, 3); break;                                                                                  \
    default: L(F, 4); break;                                                                                 \
  }
  if (w_fp8) { LM(true) } else { LM(false) }
#undef LM
#undef L
  if (splits > 1) {
    const long long MN = (long long)M * N;
    hipLaunchKernelGGL(skinny_gemm_combine_kernel, dim3(dw_grid_for(MN, 256, 1024)), dim3(256), 0, st, ws, scale,
                       (bf16_t*)y, MN, N, splits);
  }
  DW_LAUNCH_RET;
}

// w [N, K] bf16 contiguous (K % 8 == 0, 16-byte aligned) -> codes [N, K] e4m3
// (8-byte aligned), scale fp32 [N]; one launch.
extern "C" int dw_quant_rows_e4m3(const void* w, void* codes, float* scale, int N, int K, void* stream) {
  if (N <= 0 || K <= 0) return 0;
  if (K % 8 || ((uintptr_t)w & 15) || ((uintptr_t)codes & 7)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(quant_rows_e4m3_kernel, dim3(N < 4096 ? N : 4096), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)w, (unsigned char*)codes, scale, N, K);
  DW_LAUNCH_RET;
}

DW_PRELOAD(skinny_gemm_combine_kernel);
