// LM head + token statistics in one pass, the logits never stored (RL scoring:
// the log-prob of each response token under the actor / reference model and
// the entropy of its distribution):
//
//   x = X W^T  (fp32 accumulators),  lse = log sum_v e^x,
//   logp = x[label] - lse,  ent = lse - sum_v p_v x_v.
//
// X [rows, H] bf16 with the two-level row addressing of token_logprob.hip
// (base + (row / R) * bs + (row % R) * rs, so hidden[:, P-1:-1, :] is read in
// place), W [V, H] bf16 contiguous (the nn.Linear / tied embedding weight),
// labels int64 [rows] or null.
//
// Pass 1 computes the TRANSPOSED product S^T = W X^T on the 128x128x64 tile of
// gemm_tile.h: vocabulary entries are MFMA rows, tokens are MFMA columns, so a
// v_mfma_f32_32x32x16_bf16 accumulator lane holds 16 vocabulary entries of ONE
// token and the online (m, s, t, x_label) update of token_logprob.hip runs in
// the lane, without a shuffle.  A workgroup owns one 128-token block and a
// contiguous range of vocabulary tiles (a vocab split); per tile it runs the
// whole H loop (both operands are ROW images, register-staged and double
// buffered; the loads of the next tile's first K block are in flight during
// the statistics epilogue) and then folds the 2x2x16 accumulators of each of
// its lane's two tokens into the lane's state.  The four lanes that share a
// token (2 waves x 2 wave halves) meet once, after the last tile, through LDS
// in a fixed order, and the workgroup writes one (m, s, t, x_label) per token
// to ws[split][row].  Pass 2 merges the splits in split order: no atomics,
// bit-reproducible.
//
// Grid order: workgroups are numbered token block fastest within a band of 8
// token blocks, then vocab split, then band, and xcd_block hands each XCD a
// contiguous run of that order.  The 64 workgroups resident on an XCD are then
// about 8 token blocks x 8 splits: per K step they request 64 x 32 KiB but only
// 8 X chunks + 8 W chunks are distinct, so 7/8 of the operand traffic is served
// by the XCD's L2.  (Token block fastest over the whole grid shares W alone and
// misses on every X chunk; split fastest the reverse.)
//
// Tails, all on wave-uniform branches: token rows and vocabulary rows past the
// end are CLAMPED in the loads (their lanes compute on a copy of the last
// row); vocabulary rows >= V are set to -inf before the statistics of the one
// tail tile; token rows >= rows are not written; the K tail (H % 64) zero-fills
// in the last K iteration only.  Conventions of token_logprob.hip: a label
// outside [0, V) gives logp = 0, null labels give statistics only, x = -inf
// adds 0 to t, rows == 0 launches nothing, no host synchronisation.
#include <float.h>

#include "gemm_tile.h"

namespace {

constexpr int BAND = 8;           // token blocks per band of the grid order
constexpr int TARGET_WGS = 1024;  // 256 CUs x 2 resident workgroups, twice over

struct LLArgs {
  const bf16_t* X;
  const bf16_t* W;
  const int64_t* labels;
  float4* ws;  // [nsplit][rows] partial (m, s, t, x_label)
  long long R, bs, rs;
  int rows, H, V;
  int nblk, nsplit, ntiles;
};

// (m, s, t) of two disjoint vocabulary sets -> of their union; x_label is in
// at most one of them (0 elsewhere).  m = -inf (an empty or all -inf set)
// carries s = t = 0: the scale is taken against max(m, -FLT_MAX), so
// e^(-inf - that) = 0 and no inf - inf arises.
__device__ __forceinline__ void part_merge(float4& a, const float4& b) {
  const float mn = fmaxf(a.x, b.x);
  const float ms = fmaxf(mn, -FLT_MAX);
  const float ra = __expf(a.x - ms), rb = __expf(b.x - ms);
  a.y = a.y * ra + b.y * rb;
  a.z = a.z * ra + b.z * rb;
  a.w += b.w;
  a.x = mn;
}

}  // namespace

__global__ void __launch_bounds__(NTHR, 2) linear_logprob_kernel(LLArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int hh = lane >> 5;
  const int wm = wid >> 1, wn = wid & 1;  // wave: vocabulary rows 64 wm .., tokens 64 wn ..

  // ---- which (token block, vocab split)
  const int l = xcd_block((int)gridDim.x, 1).x;
  const int per_band = BAND * a.nsplit;
  const int band = l / per_band, rem = l - band * per_band;
  const int bw = min(BAND, a.nblk - band * BAND);  // the last band may be narrower
  const int split = rem / bw;
  const int tok0 = (band * BAND + rem % bw) * BN;
  const int t0 = (int)((long long)split * a.ntiles / a.nsplit);
  const int t1 = (int)((long long)(split + 1) * a.ntiles / a.nsplit);
  const int H = a.H, V = a.V;
  const int n_it = (H + BK - 1) / BK;
  const int total = (t1 - t0) * n_it;

  // ---- staged loads: vector i of this thread is chunk tid & 7 of image row (tid >> 3) + 32 i
  const int srow = tid >> 3, scol = 8 * (tid & 7);
  long long xo[4], wo[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long row = min(tok0 + srow + 32 * i, a.rows - 1);
    xo[i] = (row / a.R) * a.bs + (row % a.R) * a.rs + scol;
  }
  auto set_tile = [&](int tile) {
#pragma unroll
    for (int i = 0; i < 4; ++i) wo[i] = (long long)min(tile * BM + srow + 32 * i, V - 1) * H + scol;
  };
  Stage sa, sb;  // A = W tile (vocabulary rows), B = X block (token rows)
  int ik = 0, itile = t0;
  auto issue = [&]() {
    const int r0 = ik * BK;
    if (r0 + BK <= H) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sa.v[i] = *(const u32x4*)(a.W + wo[i] + r0);
        sb.v[i] = *(const u32x4*)(a.X + xo[i] + r0);
      }
    } else {  // K tail: H % 8 == 0, so a 16-byte chunk is inside or outside
      const bool ok = r0 + scol < H;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sa.v[i] = ok ? *(const u32x4*)(a.W + wo[i] + r0) : (u32x4){0, 0, 0, 0};
        sb.v[i] = ok ? *(const u32x4*)(a.X + xo[i] + r0) : (u32x4){0, 0, 0, 0};
      }
    }
    if (++ik == n_it) {
      ik = 0;
      if (++itile < t1) set_tile(itile);
    }
  };
  auto write = [&](int buf) {
    char* ai = smem + buf * 2 * IMG;
    store_row(sa, ai, tid);
    store_row(sb, ai + IMG, tid);
  };

  // ---- this lane's two tokens (j = 0, 1) and their online state
  int lab[2];
  float m[2], s[2], t[2], xl[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int tok = tok0 + wn * 64 + j * 32 + (lane & 31);
    const int64_t lb = (a.labels && tok < a.rows) ? a.labels[tok] : -1;
    lab[j] = (lb >= 0 && lb < V) ? (int)lb : -1;
    m[j] = -INFINITY;
    s[j] = t[j] = xl[j] = 0.f;
  }

  f32x16 acc[2][2];  // [i: vocabulary 32-row tile][j: token 32-column tile]
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  };
  // accumulator r of tile i is vocabulary row vrow(i, r) of this wave's 64
  auto vrow = [&](int i, int r) { return i * 32 + 8 * (r >> 2) + 4 * hh + (r & 3); };

  auto epilogue = [&](int tile) {
    const int v0 = tile * BM + wm * 64;
    if (tile * BM + BM > V) {  // the vocabulary tail tile
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (v0 + vrow(i, r) >= V) acc[i][0][r] = acc[i][1][r] = -INFINITY;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float vm = acc[0][j][0];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) vm = fmaxf(vm, acc[i][j][r]);
      const float mn = fmaxf(m[j], vm);
      const float ms = fmaxf(mn, -FLT_MAX);  // all -inf so far: e^(x - ms) = 0, not e^(inf - inf)
      const float rs = __expf(m[j] - ms);
      float ss[2] = {s[j] * rs, 0.f}, tt[2] = {t[j] * rs, 0.f};
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float x = acc[i][j][r];
          const float e = __expf(x - ms);
          ss[i] += e;
          tt[i] = fmaf(e, fmaxf(x, -FLT_MAX), tt[i]);  // x = -inf: e = 0 adds 0
        }
      m[j] = mn;
      s[j] = ss[0] + ss[1];
      t[j] = tt[0] + tt[1];
      const int d = lab[j] - v0 - 4 * hh;
      if ((unsigned)d < 64u) {  // the label is one of this wave's rows of this tile (rare)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (d == i * 32 + 8 * (r >> 2) + (r & 3)) xl[j] = acc[i][j][r];
      }
    }
  };

  // ---- main loop over (tile, K block), flattened so the prefetch crosses tiles
  zero_acc();
  set_tile(t0);
  issue();
  write(0);
  if (total > 1) issue();
  __syncthreads();
  int kc = 0, tile = t0;
  for (int g = 0; g < total; ++g) {
    const char* ai = smem + (g & 1) * 2 * IMG;
    const char* bi = ai + IMG;
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      u32x4 fa[2], fb[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        fa[q] = frag_row(ai, wm * 64 + q * 32 + (lane & 31), kk, hh);
        fb[q] = frag_row(bi, wn * 64 + q * 32 + (lane & 31), kk, hh);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf(fa[i]), as_bf(fb[j]), acc[i][j], 0, 0, 0);
    }
    if (g + 1 < total) {
      write((g + 1) & 1);
      if (g + 2 < total) issue();
    }
    if (++kc == n_it) {
      epilogue(tile);
      zero_acc();
      kc = 0;
      ++tile;
    }
    __syncthreads();
  }

  // ---- the four lanes of a token (wm, hh) meet in LDS, fixed order
  float4* st = (float4*)smem;  // [4][128]
#pragma unroll
  for (int j = 0; j < 2; ++j)
    st[(wm * 2 + hh) * BN + wn * 64 + j * 32 + (lane & 31)] = make_float4(m[j], s[j], t[j], xl[j]);
  __syncthreads();
  if (tid < BN && tok0 + tid < a.rows) {
    float4 p = st[tid];
#pragma unroll
    for (int c = 1; c < 4; ++c) part_merge(p, st[c * BN + tid]);
    a.ws[(long long)split * a.rows + tok0 + tid] = p;
  }
}

static_assert(4 * BN * (int)sizeof(float4) <= 4 * IMG, "merge staging must fit the operand LDS");

__global__ void __launch_bounds__(256) linear_logprob_merge_kernel(const float4* __restrict__ ws,
                                                                   const int64_t* __restrict__ labels,
                                                                   float* __restrict__ logp, float* __restrict__ lse_out,
                                                                   float* __restrict__ ent_out, int rows, int nsplit,
                                                                   int V) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  float4 p = ws[row];
  for (int sp = 1; sp < nsplit; ++sp) part_merge(p, ws[(long long)sp * rows + row]);
  const float lse = p.x + logf(p.y);
  const int64_t lab = labels ? labels[row] : -1;
  logp[row] = (lab >= 0 && lab < V) ? p.w - lse : 0.f;
  lse_out[row] = lse;
  ent_out[row] = lse - p.z / p.y;
}

// Vocab splits of a call: enough workgroups (token blocks x splits) to cover
// the 256 CUs, two resident each, about twice; at least one tile per split.
// The workspace holds dw_linear_logprob_splits(rows, V) * rows * 4 floats.
extern "C" int dw_linear_logprob_splits(int64_t rows, int V) {
  if (rows <= 0 || V <= 0) return 1;
  const int64_t nblk = (rows + BN - 1) / BN;
  const int64_t ntiles = ((int64_t)V + BM - 1) / BM;
  int64_t ns = (TARGET_WGS + nblk - 1) / nblk;
  if (ns > ntiles) ns = ntiles;
  return (int)(ns < 1 ? 1 : ns);
}

// x [rows, H] bf16 addressed by (R, bs, rs) elements (bs, rs % 8 == 0, base
// 16-byte aligned), w [V, H] bf16 contiguous, H % 8 == 0; logp / lse / ent
// fp32 [rows]; ws: see dw_linear_logprob_splits.
extern "C" int dw_linear_logprob_fwd(const void* x, const void* w, const void* labels, void* logp, void* lse,
                                     void* ent, void* ws, int64_t rows, int64_t R, int64_t bs, int64_t rs, int H,
                                     int V, void* stream) {
  if (rows <= 0) return 0;
  if (H <= 0 || V <= 0 || R <= 0 || H % 8 || bs % 8 || rs % 8 || rows > (int64_t)INT32_MAX - BN ||
      ((uintptr_t)x | (uintptr_t)w | (uintptr_t)ws) % 16)
    return (int)hipErrorInvalidValue;
  LLArgs a;
  a.X = (const bf16_t*)x;
  a.W = (const bf16_t*)w;
  a.labels = (const int64_t*)labels;
  a.ws = (float4*)ws;
  a.R = R;
  a.bs = bs;
  a.rs = rs;
  a.rows = (int)rows;
  a.H = H;
  a.V = V;
  a.nblk = (int)((rows + BN - 1) / BN);
  a.ntiles = (V + BM - 1) / BM;
  a.nsplit = dw_linear_logprob_splits(rows, V);
  if ((int64_t)a.nblk * a.nsplit > INT32_MAX) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(linear_logprob_kernel, dim3((unsigned)(a.nblk * a.nsplit)), dim3(NTHR), 4 * IMG, s, a);
  hipLaunchKernelGGL(linear_logprob_merge_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s,
                     (const float4*)ws, (const int64_t*)labels, (float*)logp, (float*)lse, (float*)ent, (int)rows,
                     a.nsplit, V);
  DW_LAUNCH_RET;
}

DW_PRELOAD(linear_logprob_kernel);
