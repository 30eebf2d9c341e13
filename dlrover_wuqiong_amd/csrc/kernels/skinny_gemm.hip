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
//  * mxfp4 (docs/rl_mxfp4_rollouts.md): W is e2m1 codes [N, K/2], two per
//    byte, and the scale pointer carries e8m0 bytes [N, K/32].  A 16-byte load
//    is the 32 codes of one MX block of the lane's row, so the k chunk is 128
//    and each load has one scale byte, fetched beside it; 16
//    v_cvt_scalef32_pk_bf16_fp4 per load (exact, block scale applied) feed
//    four MFMAs, MFMA j of chunk c seeing k = 128 c + 32 g + 8 j .. + 7 from
//    lane group g.  Up to 32 rows of x the tile is 512 deep (four loads per
//    lane in flight, 1 KiB LDS rows); no scale in the epilogue or the combine.
//
// Edges: a W row past N and an x row past M are clamped to the last one (the
// results are not stored); a 16-byte group at k >= the slice end is read at
// the slice start and replaced by zeros in both operands.
//
// dw_quant_rows_e4m3: the per-row quantiser that fills the e4m3 copy.
#include "dw_common.h"

namespace {

constexpr int SG_BK = 256;                 // k per staged x tile (bf16, e4m3; mxfp4 above 32 rows of x)
constexpr int SG_BK_MX = 512;              // ... of the mxfp4 form up to 32 rows of x: four W loads per lane in flight
constexpr int SG_BN = 64;                  // W rows per block: 4 waves x 16
constexpr int SG_BF16 = 0, SG_E4M3 = 1, SG_MXFP4 = 2;   // the W format codes of dw_skinny_gemm

// k per staged x tile.  The LDS row pitch is twice that in bytes, and 16-byte
// group q of row r sits at q ^ (r & 15): the XOR touches the low four bits
// only, so it stays inside a row of 32 or of 64 groups, and the pitch (512 /
// 1024 B) is a multiple of the 256-byte bank period, so 16 lanes with 16
// different c16 read 16 different bank quads at either depth.
__host__ __device__ constexpr int sg_bk(int fmt, int mt) { return fmt == SG_MXFP4 && mt <= 2 ? SG_BK_MX : SG_BK; }

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

// 8 e2m1 codes (one dword: byte b holds element 2b in its low nibble, 2b + 1
// in its high one, the order v_cvt_scalef32_pk_bf16_fp4 decodes a byte in)
// times the block scale -> 8 bf16, exact.
__device__ __forceinline__ bf16x8_t mxfp4x8_to_bf16(unsigned w, float s) {
  const u32x4 v = {__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 0)),
                   __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 1)),
                   __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 2)),
                   __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, s, 3))};
  return __builtin_bit_cast(bf16x8_t, v);
}

template <int FMT, int MT>
__global__ void __launch_bounds__(256) skinny_gemm_kernel(const bf16_t* __restrict__ x, long long ldx,
                                                          const unsigned char* __restrict__ W,
                                                          const float* __restrict__ scale, bf16_t* __restrict__ y,
                                                          float* __restrict__ part, int M, int N, int K, int splits) {
  constexpr bool MX = FMT == SG_MXFP4;
  constexpr int EPL = MX ? 32 : FMT == SG_E4M3 ? 16 : 8;   // W elements per lane and load
  constexpr int ES = FMT == SG_BF16 ? 2 : 1;   // bytes per W element (mxfp4: per two)
  constexpr int KC = 4 * EPL;            // k per chunk (one load per lane)
  constexpr int BK = sg_bk(FMT, MT);     // k per staged x tile
  constexpr int CH = BK / KC;            // chunks per tile
  constexpr int PITCH = BK * 2;          // LDS row pitch in bytes
  constexpr int XQ = BK / 8;             // 16-byte groups per x row
  constexpr int XR = 256 / XQ;           // x rows per staging pass
  constexpr int XP = MT * 16 / XR;       // staging passes
  auto wbytes = [](long long k) { return MX ? k >> 1 : k * ES; };
  __shared__ __attribute__((aligned(16))) unsigned char xs[2][MT * 16 * PITCH];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c16 = lane & 15;
  const int n0 = blockIdx.x * SG_BN + wave * 16;
  const int nchunks = (K + KC - 1) / KC;
  const int s = blockIdx.y;
  const int kb = (int)((long long)nchunks * s / splits) * KC;
  const int ke = min((int)((long long)nchunks * (s + 1) / splits) * KC, K);
  const int T = (ke - kb + BK - 1) / BK;   // >= 1: the launcher keeps splits <= nchunks

  const unsigned char* wrow = W + wbytes((long long)min(n0 + c16, N - 1) * K);
  // mxfp4: the row's e8m0 bytes, one per 32 k (the scale pointer carries them)
  const unsigned char* srow = (const unsigned char*)scale + (MX ? (long long)min(n0 + c16, N - 1) * (K >> 5) : 0);
  // x staging: thread -> (row tid / XQ of an XR-row pass, 16-byte group tid % XQ)
  const int xr_row = tid / XQ, xq = tid % XQ;

  u32x4 w0[CH], w1[CH], xr[XP];   // W of the tile in LDS buffer 0 / 1
  unsigned sb0[MX ? CH : 1], sb1[MX ? CH : 1];   // mxfp4: the scale byte of each load
  unsigned ok0 = 0, ok1 = 0;
  bool x_ok = false;

  // A 16-byte group past the slice end is read at the slice start instead
  // (every address stays in bounds) and zeroed later.  No load sits in a
  // branch: at a join the compiler would wait for everything outstanding.
  auto load_x = [&](int t) {
    const int k = kb + t * BK + xq * 8;
    x_ok = k < ke;
    const int kk = x_ok ? k : kb;
#pragma unroll
    for (int p = 0; p < XP; ++p) {
      const int row = min(p * XR + xr_row, M - 1);
      xr[p] = *(const u32x4*)(x + row * ldx + kk);
    }
  };
  // tail (block-uniform): the tile reaches past the slice end.  The select
  // lives only on that path, so the loads above it stay unconditional.
  auto write_x = [&](int buf, bool tail) {
    unsigned char* dst = xs[buf] + xr_row * PITCH;
    if (tail) {
#pragma unroll
      for (int p = 0; p < XP; ++p)
        *(u32x4*)(dst + p * XR * PITCH + ((xq ^ ((p * XR + xr_row) & 15)) * 16)) =
            x_ok ? xr[p] : (u32x4){0u, 0u, 0u, 0u};
    } else {
#pragma unroll
      for (int p = 0; p < XP; ++p)
        *(u32x4*)(dst + p * XR * PITCH + ((xq ^ ((p * XR + xr_row) & 15)) * 16)) = xr[p];
    }
  };
  // mxfp4: a load is the 32 codes of one MX block of the lane's row, so its
  // scale is one byte, fetched beside it at the same (clamped) k.
  auto load_w = [&](int t, u32x4* w, unsigned* sb, unsigned& ok) {
    ok = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int k = kb + t * BK + c * KC + g * EPL;
      const bool v = k < ke;
      ok |= (unsigned)v << c;
      w[c] = __builtin_nontemporal_load((const u32x4*)(wrow + wbytes(v ? k : kb)));
      if constexpr (MX) sb[c] = srow[(v ? k : kb) >> 5];
    }
  };

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int buf, const u32x4* w, const unsigned* sb, unsigned ok, bool tail) {
    // fragment rows are 16 mt + c16: the swizzle term is c16 for every mt
    const unsigned char* xa = xs[buf] + c16 * PITCH;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const u32x4 wv = (!tail || ((ok >> c) & 1u)) ? w[c] : (u32x4){0u, 0u, 0u, 0u};
      if constexpr (MX) {
        // a group past the slice end: zero codes under scale 2^0.  MFMA j of
        // the chunk sees k = 128 c + 32 g + 8 j .. + 7 from lane group g.
        const float sf = __uint_as_float(((!tail || ((ok >> c) & 1u)) ? sb[c] : 127u) << 23);
        bf16x8_t b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = mxfp4x8_to_bf16(wv[j], sf);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const unsigned char* p = xa + mt * 16 * PITCH;
          const int q = c * 16 + g * 4;   // 16-byte groups q .. q + 3
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8_t*)(p + (((q + j) ^ c16) * 16)), b[j],
                                                              acc[mt], 0, 0, 0);
        }
      } else if constexpr (FMT == SG_E4M3) {
        const bf16x8_t b0 = e4m3x8_to_bf16(wv[0], wv[1]), b1 = e4m3x8_to_bf16(wv[2], wv[3]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const unsigned char* p = xa + mt * 16 * PITCH;
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
              *(const bf16x8_t*)(xa + mt * 16 * PITCH + (((c * 4 + g) ^ c16) * 16)), b, acc[mt], 0, 0, 0);
      }
    }
  };

  // x first, W behind it: the wait for x then leaves the W loads in flight.
  // No branch around a load (a wave past N streams row N - 1 again): at a
  // join the compiler would have to wait for everything outstanding.
  const bool partial = (ke - kb) % BK != 0;   // only the slice's last tile can be
  load_x(0);
  load_w(0, w0, sb0, ok0);
  write_x(0, T == 1 && partial);
  __syncthreads();
  // two tiles per trip, so the W registers alternate without a copy (a copy
  // would wait for the loads it moves)
  for (int t = 0;;) {
    if (t + 1 == T) {
      compute(0, w0, sb0, ok0, partial);
      break;
    }
    load_x(t + 1);
    load_w(t + 1, w1, sb1, ok1);
    compute(0, w0, sb0, ok0, false);
    write_x(1, t + 2 == T && partial);   // buffer 1 was last read before the previous barrier
    __syncthreads();
    ++t;
    if (t + 1 == T) {
      compute(1, w1, sb1, ok1, partial);
      break;
    }
    load_x(t + 1);
    load_w(t + 1, w0, sb0, ok0);
    compute(1, w1, sb1, ok1, false);
    write_x(0, t + 2 == T && partial);
    __syncthreads();
    ++t;
  }

  // C layout: column (n) = lane & 15, row (m) = 4 (lane >> 4) + r
  const int n = n0 + c16;
  if (n >= N) return;
  const float sc = !MX && scale ? scale[n] : 1.f;   // mxfp4: the block scales went into the convert
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

// MXFP4 (OCP: e2m1 elements, one e8m0 scale per 32 along K), one pass, one
// block per row (grid-stride).  A thread owns 8 consecutive bf16 (one 16-byte
// load), a lane quad one MX block: amax over the quad by two cross-lane steps
// (K % 32 == 0, so a quad is whole in every trip), scale code = the fp32
// exponent field of amax - 2 clamped to [1, 254] (127 for an all-zero block),
// v = w * 2^(127 - code) exactly, magnitude = the nearest of {0, .5, 1, 1.5, 2,
// 3, 4, 6}, ties to the even code, saturated: the count of the midpoints below
// |v|, a tie counting only at an odd midpoint.  A lane writes its 4 code bytes
// (the quad 16 contiguous ones), the quad's first lane the scale byte.
__global__ void __launch_bounds__(256) quant_rows_mxfp4_kernel(const bf16_t* __restrict__ w,
                                                               unsigned* __restrict__ codes,
                                                               unsigned char* __restrict__ scale, int N, int K) {
  const int nvec = K >> 3;
  for (int row = blockIdx.x; row < N; row += gridDim.x) {
    const u32x4* src = (const u32x4*)(w + (long long)row * K);
    unsigned* dst = codes + (long long)row * nvec;
    unsigned char* sdst = scale + (long long)row * (K >> 5);
    for (int v = threadIdx.x; v < nvec; v += 256) {
      const u32x4 in = src[v];
      float f[8], m = 0.f;
      unpack8(in, f);
#pragma unroll
      for (int i = 0; i < 8; ++i) m = fmaxf(m, fabsf(f[i]));
      m = fmaxf(m, __shfl_xor(m, 1));
      m = fmaxf(m, __shfl_xor(m, 2));
      const int e = (int)(__float_as_uint(m) >> 23);
      const int code = m > 0.f ? min(max(e - 2, 1), 254) : 127;
      const float inv = __uint_as_float((unsigned)(254 - code) << 23);
      unsigned out = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float a = fabsf(f[i]) * inv;
        const unsigned mag = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) +
                             (a > 5.f);
        // bf16 i sits in half i & 1 of dword i >> 1: its sign is bit 15 or 31
        const unsigned sign = (in[i >> 1] >> ((i & 1) * 16 + 15)) & 1u;
        out |= (sign << 3 | mag) << (4 * i);
      }
      dst[v] = out;
      if ((v & 3) == 0) sdst[v >> 2] = (unsigned char)code;
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
// per slice (bk: the form's tile depth), at most 16 slices.
static int sg_splits(int N, int K, int bk) {
  const int nb = (N + SG_BN - 1) / SG_BN, ntiles = (K + bk - 1) / bk;
  int s = 1;
  while (s < 16 && nb * (2 * s) <= 384 && 2 * s <= ntiles / 2) s *= 2;
  return s;
}

// ... of the bf16 and e4m3 forms.
extern "C" int dw_skinny_gemm_splits(int M, int N, int K) {
  (void)M;
  return sg_splits(N, K, SG_BK);
}

// The number of K slices a launch runs: the request (0 = dw_skinny_gemm_splits)
// clamped to the number of k chunks (32 k bf16, 64 k e4m3, 128 k mxfp4).  The
// one place the rule lives: the launcher and the workspace sizing of
// ops/skinny_gemm.py (splits * M * N floats when it is above 1) both ask here.
// w_fmt: 0 bf16, 1 e4m3, 2 mxfp4 (whose tile is 512 deep up to 32 rows of x).
extern "C" int dw_skinny_gemm_plan(int M, int N, int K, int w_fmt, int splits) {
  const int kc = w_fmt == SG_MXFP4 ? 128 : w_fmt ? 64 : 32, nchunks = (K + kc - 1) / kc;
  if (splits <= 0) splits = sg_splits(N, K, sg_bk(w_fmt, (M + 15) / 16));
  if (splits > nchunks) splits = nchunks;
  return splits < 1 ? 1 : splits;
}

// x [M, K] bf16 with row stride ldx elements (ldx % 8 == 0, 16-byte aligned),
// w [N, K] bf16 (w_fmt = 0) or e4m3 codes (1), 16-byte aligned; scale fp32 [N]
// or null; y [M, N] bf16 contiguous.  w_fmt = 2: w is the mxfp4 codes
// [N, K / 2] (K % 32 == 0) and scale carries their e8m0 bytes [N, K / 32].
// splits: as dw_skinny_gemm_plan.  ws: fp32 scratch of ws_floats >= plan * M * N
// (unused when the plan is 1).
extern "C" int dw_skinny_gemm(const void* x, long long ldx, const void* w, int w_fmt, const float* scale, void* y,
                              float* ws, long long ws_floats, int M, int N, int K, int splits, void* stream) {
  if (M < 1 || M > 64 || N < 1 || K < 16 || K % 16 || ldx % 8 || ldx < K || splits < 0)
    return (int)hipErrorInvalidValue;
  if (w_fmt < SG_BF16 || w_fmt > SG_MXFP4 || (w_fmt == SG_MXFP4 && (K % 32 || !scale)))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)x | (uintptr_t)w) & 15) return (int)hipErrorInvalidValue;
  splits = dw_skinny_gemm_plan(M, N, K, w_fmt, splits);
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
  if (w_fmt == SG_MXFP4) { LM(SG_MXFP4) } else if (w_fmt) { LM(SG_E4M3) } else { LM(SG_BF16) }
#undef LM
#undef L
  if (splits > 1) {
    const long long MN = (long long)M * N;
    hipLaunchKernelGGL(skinny_gemm_combine_kernel, dim3(dw_grid_for(MN, 256, 1024)), dim3(256), 0, st, ws,
                       w_fmt == SG_MXFP4 ? nullptr : scale, (bf16_t*)y, MN, N, splits);
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

// w [N, K] bf16 contiguous (K % 32 == 0, 16-byte aligned) -> codes [N, K / 2]
// (4-byte aligned), scale e8m0 [N, K / 32]; one launch.
extern "C" int dw_quant_rows_mxfp4(const void* w, void* codes, void* scale, int N, int K, void* stream) {
  if (N <= 0 || K <= 0) return 0;
  if (K % 32 || ((uintptr_t)w & 15) || ((uintptr_t)codes & 3)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(quant_rows_mxfp4_kernel, dim3(N < 4096 ? N : 4096), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)w, (unsigned*)codes, (unsigned char*)scale, N, K);
  DW_LAUNCH_RET;
}

DW_PRELOAD(skinny_gemm_combine_kernel);
