// Weight-streaming expert FFN for the decode step of a top-k MoE layer
// (ops/moe_stream.py, docs/rl_moe_decode.md):
//
//   y[t] = sum_j w[t,j] * ( silu(x[t] W1[e]^T) * (x[t] W3[e]^T) ) W2[e]^T,   e = idx[t,j]
//
// x [T, H] bf16 with 1 <= T <= 64, idx [T, k] int64 (a token's k experts are
// distinct; a value outside [0, E) is a dropped assignment), w [T, k] fp32,
// W1 / W3 [E, F, H] and W2 [E, H, F] bf16 or OCP e4m3 codes with one fp32
// scale per output row, H % 16 == 0, F % 16 == 0, k <= 8, T k <= 512.  At
// decode an expert sees a handful of rows, so the layer is a stream over the
// weights of the experts that were routed to, and nothing else is read:
//
//  * assignment (t, j) is slot a = t k + j.  Nothing is sorted beforehand: a
//    block of expert e reads the <= 512 entries of idx and builds in LDS the
//    ascending list of the slots routed to e (ballot + wave prefix counts);
//    a block whose expert has none returns (block-uniform, after the scan's
//    barrier), so an idle expert costs one pass over idx;
//  * kernel A, grid (F / 64, E): the stream of skinny_gemm.hip over the same
//    16-row strip of W1[e] and of W3[e] per wave -- 16-byte non-temporal loads
//    straight into VGPRs, one 128-deep k tile of both matrices in flight while
//    the previous one is computed.  The expert's x rows (row slot / k) are
//    gathered into the XOR-swizzled LDS tile (two buffers, one barrier per
//    tile); only the ceil(count / 16) 16-row groups that exist are staged and
//    multiplied (v_mfma_f32_16x16x32_bf16, e4m3 widened in registers).  The
//    epilogue stays in the lane: hbuf[a][n] = bf16(silu(acc1 s1) * (acc3 s3));
//  * kernel B, grid (H / 64, E, S): the same stream over W2[e] (one matrix:
//    a 256-deep tile), its x rows are hbuf[a]; slice s of K = F writes the
//    fp32 rows part[s][a][:], each valid slot row exactly once per slice;
//  * kernel C: y[t][n] = bf16(sum_j w[t,j] s2[e][n] sum_s part[s][t k + j][n])
//    in that order.  No float atomics: bit-reproducible for given shapes.
//
// Edges as in skinny_gemm.hip: a W row past N and a list row past the count
// are clamped to the last one (the results are not stored); a 16-byte k group
// past the slice end is read at the slice start and zeroed in both operands;
// no load sits in a branch.
#include "dw_common.h"

namespace {

constexpr int MS_BN = 64;            // W rows per block: 4 waves x 16
constexpr int MS_MAX_SLOTS = 512;    // T k: two entries of idx per thread
constexpr int MS_MAX_K = 8, MS_MAX_E = 256, MS_MAX_T = 64;
constexpr int MS_E4M3 = 1;           // the W format codes of dw_moe_stream_mlp: 0 bf16, 1 e4m3

// k per staged x tile: two W matrices in flight halve the depth, so that the
// W registers of a lane are those of the dense kernel (docs/rl_moe_decode.md).
__host__ __device__ constexpr int ms_bk(bool glu) { return glu ? 128 : 256; }

// The ascending list of the slots whose idx is e, into slots[]; returns its
// length.  Chunk q = 4 p + wave holds slots 64 q .. 64 q + 63, so chunk order
// then lane order is slot order.  Every thread passes both barriers.
__device__ __forceinline__ int ms_scan_slots(const long long* __restrict__ idx, int n, int e, unsigned short* slots,
                                             int* wcnt) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  bool hit[2];
  unsigned long long bal[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int a = p * 256 + tid;
    hit[p] = idx[min(a, n - 1)] == (long long)e && a < n;
    bal[p] = __ballot(hit[p]);
    if (lane == 0) wcnt[p * 4 + wave] = __popcll(bal[p]);
  }
  __syncthreads();
  int total = 0, base[2] = {0, 0};
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    if (q == wave) base[0] = total;
    if (q == 4 + wave) base[1] = total;
    total += wcnt[q];
  }
#pragma unroll
  for (int p = 0; p < 2; ++p)
    if (hit[p]) slots[base[p] + __popcll(bal[p] & ((1ull << lane) - 1ull))] = (unsigned short)(p * 256 + tid);
  __syncthreads();
  return total;
}

// GLU (kernel A): xin = x [T, K], row slot / topk; Wa, Wb = W1, W3 [E, N, K];
// writes hbuf [n_slots, N].  Otherwise (kernel B): xin = hbuf [n_slots, K],
// row slot; Wa = W2 [E, N, K]; writes part [splits, n_slots, N] (no scale:
// kernel C applies it).
template <int FMT, int MT, bool GLU>
__global__ void __launch_bounds__(256) moe_stream_kernel(const bf16_t* __restrict__ xin,
                                                         const long long* __restrict__ idx, int n_slots, int topk,
                                                         const unsigned char* __restrict__ Wa,
                                                         const unsigned char* __restrict__ Wb,
                                                         const float* __restrict__ sa, const float* __restrict__ sb,
                                                         bf16_t* __restrict__ hbuf, float* __restrict__ part, int N,
                                                         int K, int splits) {
  constexpr int NW = GLU ? 2 : 1;        // W matrices streamed
  constexpr int EPL = FMT == MS_E4M3 ? 16 : 8;   // W elements per lane and load
  constexpr int ES = FMT == MS_E4M3 ? 1 : 2;     // bytes per W element
  constexpr int KC = 4 * EPL;            // k per chunk (one load per lane and matrix)
  constexpr int BK = ms_bk(GLU);         // k per staged x tile
  constexpr int CH = BK / KC;            // chunks per tile
  constexpr int PITCH = BK * 2;          // LDS row pitch in bytes: a multiple of the 256-byte bank period
  constexpr int XQ = BK / 8;             // 16-byte groups per x row (16 or 32: the XOR of the low four bits stays inside)
  constexpr int XR = 256 / XQ;           // x rows per staging pass
  constexpr int XP = MT * 16 / XR;       // staging passes
  constexpr int PPG = 16 / XR;           // ... per 16-row group
  __shared__ __attribute__((aligned(16))) unsigned char xs[2][MT * 16 * PITCH];
  __shared__ unsigned short slots[MS_MAX_SLOTS];
  __shared__ int wcnt[8];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c16 = lane & 15;
  const int e = blockIdx.y, s = blockIdx.z;
  const int cnt = ms_scan_slots(idx, n_slots, e, slots, wcnt);
  if (cnt == 0) return;
  // <= MT: a token's experts are distinct, so cnt <= T; the min keeps the
  // staged rows inside xs whatever idx holds
  const int ng = min((cnt + 15) >> 4, MT);
  const int rows = min(cnt, MT * 16);

  const int n0 = blockIdx.x * MS_BN + wave * 16;
  const int nchunks = (K + KC - 1) / KC;
  const int kb = (int)((long long)nchunks * s / splits) * KC;
  const int ke = min((int)((long long)nchunks * (s + 1) / splits) * KC, K);
  const int T = (ke - kb + BK - 1) / BK;   // >= 1: the plan keeps splits <= nchunks

  const long long wrow = ((long long)e * N + min(n0 + c16, N - 1)) * K * ES;
  const unsigned char* wp[NW];
  wp[0] = Wa + wrow;
  if constexpr (GLU) wp[1] = Wb + wrow;
  // x staging: thread -> (row tid / XQ of an XR-row pass, 16-byte group tid % XQ)
  const int xr_row = tid / XQ, xq = tid % XQ;
  const bf16_t* xrow[XP];
#pragma unroll
  for (int p = 0; p < XP; ++p) {
    const int a = slots[min(p * XR + xr_row, rows - 1)];
    xrow[p] = xin + (long long)(GLU ? a / topk : a) * K;
  }

  u32x4 w0[NW][CH], w1[NW][CH], xr[XP];   // W of the tile in LDS buffer 0 / 1
  unsigned ok0 = 0, ok1 = 0;
  bool x_ok = false;

  // Every load is unconditional (a group past the slice end is read at the
  // slice start, a row past the count is the last one again): at the join of
  // a branch the compiler would wait for everything outstanding.
  auto load_x = [&](int t) {
    const int k = kb + t * BK + xq * 8;
    x_ok = k < ke;
    const int kk = x_ok ? k : kb;
#pragma unroll
    for (int p = 0; p < XP; ++p) xr[p] = *(const u32x4*)(xrow[p] + kk);
  };
  // tail (block-uniform): the tile reaches past the slice end.  Groups past
  // the expert's count are not staged (block-uniform too).
  auto write_x = [&](int buf, bool tail) {
    unsigned char* dst = xs[buf] + xr_row * PITCH;
#pragma unroll
    for (int p = 0; p < XP; ++p) {
      if (p / PPG >= ng) continue;
      *(u32x4*)(dst + p * XR * PITCH + ((xq ^ ((p * XR + xr_row) & 15)) * 16)) =
          (!tail || x_ok) ? xr[p] : (u32x4){0u, 0u, 0u, 0u};
    }
  };
  auto load_w = [&](int t, u32x4 (*w)[CH], unsigned& ok) {
    ok = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int k = kb + t * BK + c * KC + g * EPL;
      const bool v = k < ke;
      ok |= (unsigned)v << c;
#pragma unroll
      for (int m = 0; m < NW; ++m)
        w[m][c] = __builtin_nontemporal_load((const u32x4*)(wp[m] + (long long)(v ? k : kb) * ES));
    }
  };

  f32x4 acc[NW][MT];
#pragma unroll
  for (int m = 0; m < NW; ++m)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[m][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int buf, const u32x4 (*w)[CH], unsigned ok, bool tail) {
    // fragment rows are 16 mt + c16: the swizzle term is c16 for every mt
    const unsigned char* xa = xs[buf] + c16 * PITCH;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const bool zero = tail && !((ok >> c) & 1u);
      if constexpr (FMT == MS_E4M3) {
        // a lane's 16 codes are 16 consecutive k: the two MFMAs of a 64-deep
        // chunk see k = 64 c + 16 g + {0..7, 8..15} (the order of skinny_gemm.hip)
        bf16x8_t b0[NW], b1[NW];
#pragma unroll
        for (int m = 0; m < NW; ++m) {
          const u32x4 wv = zero ? (u32x4){0u, 0u, 0u, 0u} : w[m][c];
          b0[m] = e4m3x8_to_bf16(wv[0], wv[1]);
          b1[m] = e4m3x8_to_bf16(wv[2], wv[3]);
        }
        const int q = c * 8 + g * 2;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          if (mt >= ng) continue;
          const unsigned char* p = xa + mt * 16 * PITCH;
          const bf16x8_t a0 = *(const bf16x8_t*)(p + ((q ^ c16) * 16));
          const bf16x8_t a1 = *(const bf16x8_t*)(p + (((q + 1) ^ c16) * 16));
#pragma unroll
          for (int m = 0; m < NW; ++m) {
            acc[m][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0[m], acc[m][mt], 0, 0, 0);
            acc[m][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1[m], acc[m][mt], 0, 0, 0);
          }
        }
      } else {
        bf16x8_t b[NW];
#pragma unroll
        for (int m = 0; m < NW; ++m) b[m] = __builtin_bit_cast(bf16x8_t, zero ? (u32x4){0u, 0u, 0u, 0u} : w[m][c]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          if (mt >= ng) continue;
          const bf16x8_t a = *(const bf16x8_t*)(xa + mt * 16 * PITCH + (((c * 4 + g) ^ c16) * 16));
#pragma unroll
          for (int m = 0; m < NW; ++m)
            acc[m][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[m], acc[m][mt], 0, 0, 0);
        }
      }
    }
  };

  // x first, W behind it: the wait for x then leaves the W loads in flight
  const bool partial = (ke - kb) % BK != 0;   // only the slice's last tile can be
  load_x(0);
  load_w(0, w0, ok0);
  write_x(0, T == 1 && partial);
  __syncthreads();
  // two tiles per trip, so the W registers alternate without a copy
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

  // C layout: column (n) = lane & 15, row (list position) = 16 mt + 4 (lane >> 4) + r
  const int n = n0 + c16;
  if (n >= N) return;
  float s1 = 1.f, s3 = 1.f;
  if constexpr (GLU) {
    if (sa) s1 = sa[(long long)e * N + n], s3 = sb[(long long)e * N + n];
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = mt * 16 + g * 4 + r;
      if (i >= rows) continue;
      const long long a = slots[i];
      if constexpr (GLU)
        hbuf[a * N + n] = f2bf(silu(acc[0][mt][r] * s1) * (acc[NW - 1][mt][r] * s3));
      else
        part[((long long)s * n_slots + a) * N + n] = acc[0][mt][r];
    }
}

// y[t][n .. n + 3] = bf16(sum_j w[t,j] s2[e][n] sum_s part[s][t k + j][n]); a
// dropped slot's part row was never written and is not read.
__global__ void __launch_bounds__(256) moe_stream_combine_kernel(const float* __restrict__ part,
                                                                 const long long* __restrict__ idx,
                                                                 const float* __restrict__ w,
                                                                 const float* __restrict__ s2, bf16_t* __restrict__ y,
                                                                 int T, int topk, int E, int H, int splits) {
  const int hq = H >> 2;
  const long long slab = (long long)T * topk * H, total = (long long)T * hq;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int t = (int)(i / hq), n = (int)(i % hq) * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < topk; ++j) {
      const long long a = (long long)t * topk + j, e = idx[a];
      if (e < 0 || e >= E) continue;
      const float* p = part + a * H + n;
      f32x4 sum = *(const f32x4*)p;
      for (int s = 1; s < splits; ++s) sum += *(const f32x4*)(p + s * slab);
      const f32x4 sc = s2 ? *(const f32x4*)(s2 + e * H + n) : (f32x4){1.f, 1.f, 1.f, 1.f};
      acc += w[a] * sc * sum;
    }
    *(uint2*)(y + (long long)t * H + n) = make_uint2(f2bf(acc[0]) | ((unsigned)f2bf(acc[1]) << 16),
                                                     f2bf(acc[2]) | ((unsigned)f2bf(acc[3]) << 16));
  }
}

long long ms_hbuf_bytes(int T, int k, int F) { return ((long long)T * k * F * 2 + 15) & ~15ll; }

}  // namespace

// The number of K = F slices of the down projection: a function of the shapes
// only (never of idx, and the same for both formats), so a captured step stays
// valid.  About one block per CU over the experts a step can reach, min(E,
// T k); a power of two, never fewer than two 256-deep tiles per slice (so
// never more slices than 64-deep k chunks), at most 16.
extern "C" int dw_moe_stream_plan(int T, int k, int E, int H, int F) {
  if (T < 1 || k < 1 || E < 1 || H < 1 || F < 1) return 1;
  const long long reach = (long long)T * k < E ? (long long)T * k : E;
  const long long nb = (H + MS_BN - 1) / MS_BN * reach;
  const int ntiles = (F + ms_bk(false) - 1) / ms_bk(false);
  int s = 1;
  while (s < 16 && nb * (2 * s) <= 384 && 2 * s <= ntiles / 2) s *= 2;
  return s;
}

// Bytes of the workspace: hbuf bf16 [T k, F] (padded to 16 bytes), then part
// fp32 [plan, T k, H] (ops/moe_stream.py workspace_bytes is the same sum).
static long long ms_ws_bytes(int T, int k, int E, int H, int F) {
  return ms_hbuf_bytes(T, k, F) + (long long)dw_moe_stream_plan(T, k, E, H, F) * T * k * H * 4;
}

// x [T, H] bf16 contiguous, w [T, k] fp32, idx [T, k] int64, w1 / w3 [E, F, H]
// and w2 [E, H, F] contiguous bf16 (w_fmt 0; s1 = s3 = s2 = null) or e4m3
// codes (1) with fp32 scales s1, s3 [E, F] and s2 [E, H]; y [T, H] bf16; ws:
// ws_bytes >= ms_ws_bytes, 16-byte aligned like x and the weights.
// Three launches (A, B, C) on the stream.
extern "C" int dw_moe_stream_mlp(const void* x, const float* w, const void* idx, const void* w1, const void* w3,
                                 const void* w2, const float* s1, const float* s3, const float* s2, int w_fmt,
                                 void* y, void* ws, long long ws_bytes, int T, int k, int E, int H, int F,
                                 void* stream) {
  if (T < 1 || T > MS_MAX_T || k < 1 || k > MS_MAX_K || T * k > MS_MAX_SLOTS || E < 1 || E > MS_MAX_E || H < 16 ||
      H % 16 || F < 16 || F % 16)
    return (int)hipErrorInvalidValue;
  if (w_fmt < 0 || w_fmt > MS_E4M3 || (w_fmt == MS_E4M3) != (s1 != nullptr) || (s1 != nullptr) != (s3 != nullptr) ||
      (s1 != nullptr) != (s2 != nullptr))
    return (int)hipErrorInvalidValue;
  if (!ws || ws_bytes < ms_ws_bytes(T, k, E, H, F)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)x | (uintptr_t)w1 | (uintptr_t)w3 | (uintptr_t)w2 | (uintptr_t)ws | (uintptr_t)y |
       (uintptr_t)s2) & 15)
    return (int)hipErrorInvalidValue;
  const int splits = dw_moe_stream_plan(T, k, E, H, F), n_slots = T * k, mt = (T + 15) / 16;
  bf16_t* hbuf = (bf16_t*)ws;
  float* part = (float*)((unsigned char*)ws + ms_hbuf_bytes(T, k, F));
  hipStream_t st = (hipStream_t)stream;
  const dim3 ga((F + MS_BN - 1) / MS_BN, E), gb((H + MS_BN - 1) / MS_BN, E, splits);
#define LA(FM, M)                                                                                             \
  hipLaunchKernelGGL((moe_stream_kernel<FM, M, true>), ga, dim3(256), 0, st, (const bf16_t*)x,               \
                     (const long long*)idx, n_slots, k, (const unsigned char*)w1, (const unsigned char*)w3,  \
                     s1, s3, hbuf, (float*)nullptr, F, H, 1)
#define LB(FM, M)                                                                                             \
  hipLaunchKernelGGL((moe_stream_kernel<FM, M, false>), gb, dim3(256), 0, st, (const bf16_t*)hbuf,           \
                     (const long long*)idx, n_slots, k, (const unsigned char*)w2,                            \
                     (const unsigned char*)nullptr, (const float*)nullptr, (const float*)nullptr,            \
                     (bf16_t*)nullptr, part, H, F, splits)
#define LM(L, FM)                                                                                             \
  switch (mt) {                                                                                              \
    case 1: L(FM, 1); break;                                                                                 \
    case 2: L(FM, 2); break;                                                                                 \
    case 3: L(FM, 3); break;                                                                                 \
    default: L(FM, 4); break;                                                                                \
  }
  if (w_fmt) { LM(LA, 1) } else { LM(LA, 0) }
  if (w_fmt) { LM(LB, 1) } else { LM(LB, 0) }
#undef LM
#undef LB
#undef LA
  hipLaunchKernelGGL(moe_stream_combine_kernel, dim3(dw_grid_for((long long)T * (H >> 2), 256, 1024)), dim3(256), 0,
                     st, part, (const long long*)idx, w, s2, (bf16_t*)y, T, k, E, H, splits);
  DW_LAUNCH_RET;
}

DW_PRELOAD(moe_stream_combine_kernel);
