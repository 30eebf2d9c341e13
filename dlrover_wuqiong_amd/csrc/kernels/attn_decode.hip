// Split-KV decode attention over a static KV cache (gfx950, bf16 in/out).
//
// q [B, H, D] (one new token per sequence), k/v cache [B, Smax, Hkv, D] with
// arbitrary batch / row strides, lens [B] int32 ON THE DEVICE (keys 0..len-1
// are valid), out [B, H, D].  D in {64, 128}; GQA group G = H / Hkv.
//
// Decode is HBM-bound: every cached K/V byte is read exactly once per step.
//  * pass 1: grid (split, head group, b * Hkv); a 4-wave block owns a
//    `chunk`-key slice of one KV head and up to 8 of its query heads.  D/8
//    lanes cover one key row with 16-byte loads, so a wave streams 64/(D/8)
//    keys per step; the q.k partial dots reduce over those lanes with xor
//    shuffles, each lane group keeps an online softmax (m, l) and its 8-wide
//    slice of the output per head; lane groups, then waves (through LDS),
//    merge their states and the block writes (m, l, o) partials (fp32);
//  * pass 2: per (b, h) merge the splits' partials -> out.
// Lengths come from device memory and the grid depends only on Smax, so a
// decode step is capturable in a HIP graph and replayed as the cache grows.
//
// dw_attn_decode_q8 is the same operation over an e4m3 cache with per-(token,
// head) scales: its pass 1 (attn_decode_q8_kernel, below) runs on the MFMA
// units, pass 2 is shared.  dw_attn_decode_mfma (opt-in) reads the bf16 cache
// with an MFMA pass 1 of the same shape (attn_decode_mfma_kernel).
// dw_attn_decode_shared (opt-in) serves n samples per prompt: a prefix pass
// over the prompts' cache with the samples' heads side by side in the MFMA
// tiles (attn_decode_prefix_kernel), that MFMA pass 1 over the samples' own
// suffix caches, one merge.
#include "dw_common.h"

namespace {

constexpr int DEC_WAVES = 4;
constexpr int DEC_GMAX = 8;  // query heads per block

template <int D>
struct DecCfg {
  static constexpr int LPK = D / 8;        // lanes per key row
  static constexpr int KPW = 64 / LPK;     // keys a wave handles per step
};

template <int D>
__global__ void __launch_bounds__(64 * DEC_WAVES) attn_decode_split_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
    const int* __restrict__ lens, float* __restrict__ part_o, float* __restrict__ part_ml, int H, int HKV,
    int nsplit, int chunk, float scale_log2, long long q_bs, long long k_bs, long long k_rs, long long v_bs,
    long long v_rs) {
  using C = DecCfg<D>;
  __shared__ float sm_ml[DEC_WAVES][DEC_GMAX][2];
  __shared__ float sm_o[DEC_WAVES][DEC_GMAX][D];

  const int split = blockIdx.x, hg = blockIdx.y;
  const int b = blockIdx.z / HKV, hk = blockIdx.z % HKV;
  const int G = H / HKV;
  const int g0 = hg * DEC_GMAX;
  const int ng = min(DEC_GMAX, G - g0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = lane / C::LPK, sl = lane % C::LPK;  // key slot in the wave, 8-wide d slice
  const int len = lens[b];
  const int k_lo = split * chunk, k_hi = min(len, k_lo + chunk);

  float qv[DEC_GMAX][8];
#pragma unroll
  for (int g = 0; g < DEC_GMAX; ++g) {
    if (g < ng) {
      const u32x4 w = *(const u32x4*)(Q + (long long)b * q_bs + (long long)(hk * G + g0 + g) * D + 8 * sl);
      unpack8(w, qv[g]);
#pragma unroll
      for (int i = 0; i < 8; ++i) qv[g][i] *= scale_log2;  // scores in log2 units
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) qv[g][i] = 0.f;
    }
  }
  float m[DEC_GMAX], l[DEC_GMAX], acc[DEC_GMAX][8];
#pragma unroll
  for (int g = 0; g < DEC_GMAX; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[g][i] = 0.f;
  }

  const bf16_t* Kb = K + (long long)b * k_bs + (long long)hk * D + 8 * sl;
  const bf16_t* Vb = V + (long long)b * v_bs + (long long)hk * D + 8 * sl;
  // U keys per lane group per step, all their loads issued before any math
  // (8 x 16 B in flight per lane instead of 2)
  constexpr int U = 4;
  constexpr int STEP = DEC_WAVES * C::KPW;
  for (int key0 = k_lo + wid * C::KPW + grp; key0 < k_hi; key0 += U * STEP) {
    u32x4 kw[U], vw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = key0 + u * STEP;
      if (key < k_hi) {
        kw[u] = *(const u32x4*)(Kb + (long long)key * k_rs);
        vw[u] = *(const u32x4*)(Vb + (long long)key * v_rs);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (key0 + u * STEP >= k_hi) break;  // uniform within the lane group
      float kf[8], vf[8];
      unpack8(kw[u], kf);
      unpack8(vw[u], vf);
#pragma unroll
      for (int g = 0; g < DEC_GMAX; ++g) {
        if (g >= ng) break;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s = __builtin_fmaf(qv[g][i], kf[i], s);
#pragma unroll
        for (int off = C::LPK / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        const float mn = fmaxf(m[g], s);
        const float alpha = __builtin_amdgcn_exp2f(m[g] - mn);  // m = -inf -> 0
        const float p = __builtin_amdgcn_exp2f(s - mn);
        l[g] = l[g] * alpha + p;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[g][i] = __builtin_fmaf(p, vf[i], acc[g][i] * alpha);
        m[g] = mn;
      }
    }
  }

  // merge the KPW key slots of this wave (lanes sl, sl + LPK, ...)
#pragma unroll
  for (int g = 0; g < DEC_GMAX; ++g) {
    if (g >= ng) break;
#pragma unroll
    for (int off = C::LPK; off < 64; off <<= 1) {
      const float mo = __shfl_xor(m[g], off, 64), lo = __shfl_xor(l[g], off, 64);
      const float mn = fmaxf(m[g], mo);
      const float a = mn == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m[g] - mn);
      const float c = mn == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mo - mn);
      l[g] = l[g] * a + lo * c;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float ao = __shfl_xor(acc[g][i], off, 64);
        acc[g][i] = acc[g][i] * a + ao * c;
      }
      m[g] = mn;
    }
    if (grp == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) sm_o[wid][g][8 * sl + i] = acc[g][i];
      if (sl == 0) {
        sm_ml[wid][g][0] = m[g];
        sm_ml[wid][g][1] = l[g];
      }
    }
  }
  __syncthreads();

  // merge the waves: thread t handles (head g, d) pairs
  const long long pbase = (((long long)b * H + hk * G + g0) * nsplit + split);
  for (int e = tid; e < ng * D; e += 64 * DEC_WAVES) {
    const int g = e / D, d = e % D;
    float mx = -INFINITY;
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w) mx = fmaxf(mx, sm_ml[w][g][0]);
    float lt = 0.f, ot = 0.f;
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w) {
      const float c = mx == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(sm_ml[w][g][0] - mx);
      lt += sm_ml[w][g][1] * c;
      ot += sm_o[w][g][d] * c;
    }
    const long long pi = pbase + (long long)g * nsplit;  // row (b, h, split)
    part_o[pi * D + d] = ot;
    if (d == 0) {
      part_ml[2 * pi] = mx;
      part_ml[2 * pi + 1] = lt;
    }
  }
}

// one wave per (b, h): lanes over d (D/64 values each)
template <int D>
__global__ void __launch_bounds__(64) attn_decode_merge_kernel(const float* __restrict__ part_o,
                                                               const float* __restrict__ part_ml,
                                                               bf16_t* __restrict__ O, int nsplit,
                                                               long long o_bs, int H) {
  const int bh = blockIdx.x, lane = threadIdx.x;
  const int b = bh / H, h = bh % H;
  const long long base = (long long)bh * nsplit;
  float mx = -INFINITY;
  for (int s = 0; s < nsplit; ++s) mx = fmaxf(mx, part_ml[2 * (base + s)]);
  constexpr int PER = D / 64;
  float o[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) o[i] = 0.f;
  float lt = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float ms = part_ml[2 * (base + s)];
    if (ms == -INFINITY) continue;
    const float c = __builtin_amdgcn_exp2f(ms - mx);
    lt += part_ml[2 * (base + s) + 1] * c;
#pragma unroll
    for (int i = 0; i < PER; ++i) o[i] += part_o[(base + s) * D + lane + 64 * i] * c;
  }
  const float inv = lt > 0.f ? 1.f / lt : 0.f;
  bf16_t* Ob = O + (long long)b * o_bs + (long long)h * D;
#pragma unroll
  for (int i = 0; i < PER; ++i) Ob[lane + 64 * i] = f2bf(o[i] * inv);
}

// ---------------------------------------------------------------------------
// e4m3 KV cache (docs/rl_fp8_kv_cache.md): codes [B, Smax, Hkv, D] with one
// fp32 scale per (token, KV head), k_scale / v_scale [B, Hkv, Smax].  Pass 1
// on the MFMA units; pass 2 is attn_decode_merge_kernel above.
//
// A 4-wave block owns a `chunk`-key slice of one KV head and up to 16 of its
// query heads (the columns of one 16x16 MFMA tile; unused columns are zero);
// the waves take the slice's 32-key tiles round-robin.  Per tile and wave:
//  * S^T = K Q^T, two 16-key MFMA tiles.  The contraction index is permuted:
//    slot (g, j) of MFMA i is d = g D/4 + 8 i + j (g = lane / 16), so lane
//    (g, c) reads the contiguous D/4 bytes [g D/4, (g + 1) D/4) of key row c
//    from global memory straight into VGPRs; the Q fragments carry the same
//    permutation and live in registers for the whole slice.  Codes widen to
//    bf16 in registers (exact) and feed v_mfma_f32_16x16x32_bf16.
//  * lane (g, c) then holds the scores of head c for the keys 16 t + 4 g + r
//    (t < 2, r < 4): its 8 values are one B fragment of P^T, so P never moves
//    between lanes.  Online softmax per head: 8 values, then the 4 lanes g.
//  * O^T += V^T P^T: the wave's V tile goes global -> VGPR -> bf16 -> its own
//    LDS region (row pitch 2 D + 32 bytes: the 8 rows a half-wave reads fall
//    in 8 different bank groups), and the V^T fragments are formed with
//    ds_read_b64_tr_b16; slot (g, j) is key 16 (j / 4) + 4 g + (j % 4).
// Row addresses are clamped to the last valid key, so every load is
// unconditional and in bounds and no stale code is ever read; stale scales
// can arrive (the 4-wide scale load of the group that straddles k_hi).  Only
// the tile that straddles k_hi (a wave-uniform branch) selects: scores to
// -inf and p v_scale to 0.  It also zeroes its V rows past k_hi (copies of the
// last valid row after the clamp), so those rows are zeros as well as p.
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

constexpr int Q8_HEADS = 16;  // query heads per block
constexpr int Q8_TILE = 32;   // keys per wave step

// Epilogue of the MFMA pass-1 kernels (attn_decode_q8_kernel,
// attn_decode_mfma_kernel): the block's waves merge their states through LDS
// (`smem`, at least DEC_WAVES * Q8_HEADS * (D + 2) floats, the V staging of
// the loop) and write the partials of split `split` in the layout that
// attn_decode_merge_kernel reads.  Lane (g, c16) of wave `wid` holds
// O^T[16 dt + 4 g + r][head c16] in o, and m, l of head c16 (l summed over g).
// `row(hh)` is the partial row (b, h, split) of the tile's column hh.
template <int D, class RowFn>
__device__ __forceinline__ void mfma_wave_merge_rows(unsigned char* smem, const f32x4 (&o)[D / 16], float m, float l,
                                                     int tid, int wid, int g, int c16, int ng, RowFn row,
                                                     float* __restrict__ part_o, float* __restrict__ part_ml) {
  constexpr int DT = D / 16;
  __syncthreads();  // nothing in flight into the V staging, no wave reads it: it becomes the waves' states
  float* sm_o = (float*)smem;                          // [wave][head][D]
  float* sm_ml = sm_o + DEC_WAVES * Q8_HEADS * D;      // [wave][head][2]
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) *(f32x4*)(sm_o + (wid * Q8_HEADS + c16) * D + 16 * dt + 4 * g) = o[dt];
  if (g == 0) {
    sm_ml[(wid * Q8_HEADS + c16) * 2] = m;
    sm_ml[(wid * Q8_HEADS + c16) * 2 + 1] = l;
  }
  __syncthreads();

  // merge the waves: thread t handles (head hh, d) pairs
  for (int e = tid; e < ng * D; e += 64 * DEC_WAVES) {
    const int hh = e / D, d = e % D;
    float mxw = -INFINITY;
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w) mxw = fmaxf(mxw, sm_ml[(w * Q8_HEADS + hh) * 2]);
    float lt = 0.f, ot = 0.f;
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w) {
      const float c = mxw == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(sm_ml[(w * Q8_HEADS + hh) * 2] - mxw);
      lt += sm_ml[(w * Q8_HEADS + hh) * 2 + 1] * c;
      ot += sm_o[(w * Q8_HEADS + hh) * D + d] * c;
    }
    const long long pi = row(hh);
    part_o[pi * D + d] = ot;
    if (d == 0) {
      part_ml[2 * pi] = mxw;
      part_ml[2 * pi + 1] = lt;
    }
  }
}

// The columns of a tile are the query heads g0 .. of one (b, KV head): rows
// pbase + hh * nsplit.
template <int D>
__device__ __forceinline__ void mfma_wave_merge(unsigned char* smem, const f32x4 (&o)[D / 16], float m, float l,
                                                int tid, int wid, int g, int c16, int ng, long long pbase,
                                                int nsplit, float* __restrict__ part_o,
                                                float* __restrict__ part_ml) {
  mfma_wave_merge_rows<D>(
      smem, o, m, l, tid, wid, g, c16, ng, [=](int hh) { return pbase + (long long)hh * nsplit; }, part_o, part_ml);
}

template <int D>
__global__ void __launch_bounds__(64 * DEC_WAVES) DW_NO_PK_F32 attn_decode_q8_kernel(
    const bf16_t* __restrict__ Q, const unsigned char* __restrict__ K, const unsigned char* __restrict__ V,
    const float* __restrict__ KS, const float* __restrict__ VS, const int* __restrict__ lens,
    float* __restrict__ part_o, float* __restrict__ part_ml, int H, int HKV, int Smax, int nsplit, int chunk,
    float scale_log2, long long q_bs, long long k_bs, long long k_rs, long long v_bs, long long v_rs,
    long long ks_bs, long long ks_hs, long long vs_bs, long long vs_hs) {
  constexpr int PITCH = 2 * D + 32;          // bytes of one bf16 V row in LDS
  constexpr int VBYTES = Q8_TILE * PITCH;    // one wave's V tile
  constexpr int NM = D / 32;                 // MFMAs per 16-key score tile
  constexpr int DT = D / 16;                 // 16-row tiles of O^T
  constexpr int KV4 = D / 64;                // 16-byte loads of a lane's D/4-byte K piece
  constexpr int LPR = D / 16;                // lanes per V row (16 codes each)
  constexpr int RPL = 64 / LPR;              // V rows per load
  constexpr int NVL = Q8_TILE / RPL;         // V loads per tile
  constexpr int MERGE = DEC_WAVES * Q8_HEADS * (D + 2) * 4;
  constexpr int SMEM = DEC_WAVES * VBYTES > MERGE ? DEC_WAVES * VBYTES : MERGE;
  // the V staging of the steady loop, then (after a barrier) the waves' states
  __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];

  const int split = blockIdx.x, hg = blockIdx.y;
  const int b = blockIdx.z / HKV, hk = blockIdx.z % HKV;
  const int G = H / HKV;
  const int g0 = hg * Q8_HEADS;
  const int ng = min(Q8_HEADS, G - g0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const int len = min(lens[b], Smax);
  const int k_lo = split * chunk, k_hi = min(len, k_lo + chunk);
  const int ntiles = k_hi > k_lo ? (k_hi - k_lo + Q8_TILE - 1) / Q8_TILE : 0;
  const int last = k_hi - 1;

  // Q^T fragments (B operand: column = head c16), permuted like K
  bf16x8_t qf[NM];
  {
    const bool hv = c16 < ng;
    const bf16_t* qp = Q + (long long)b * q_bs + (long long)(hk * G + g0 + (hv ? c16 : 0)) * D + g * (D / 4);
#pragma unroll
    for (int i = 0; i < NM; ++i) {
      const u32x4 w = *(const u32x4*)(qp + 8 * i);
      qf[i] = __builtin_bit_cast(bf16x8_t, hv ? w : (u32x4){0u, 0u, 0u, 0u});
    }
  }
  float m = -INFINITY, l = 0.f;  // m: of head c16 (same in the 4 lanes g); l: this lane's keys only
  f32x4 o[DT];                   // O^T[16 dt + 4 g + r][head c16]
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const unsigned char* Kb = K + (long long)b * k_bs + (long long)hk * D + g * (D / 4);
  const unsigned char* Vb = V + (long long)b * v_bs + (long long)hk * D + (lane % LPR) * 16;
  const float* ksb = KS + (long long)b * ks_bs + (long long)hk * ks_hs;
  const float* vsb = VS + (long long)b * vs_bs + (long long)hk * vs_hs;
  unsigned char* vl = smem + wid * VBYTES;
  const int vrow = lane / LPR;
  // transposed read: lane li of a 16-lane group points at row li / 4, columns 4 (li % 4) .. + 3
  const unsigned char* vtr = vl + (4 * g + (c16 >> 2)) * PITCH + 8 * (c16 & 3);

  for (int tile = wid; tile < ntiles; tile += DEC_WAVES) {
    const int kb = k_lo + Q8_TILE * tile;
    const bool tail = kb + Q8_TILE > k_hi;  // wave-uniform
    // every load of the tile before any math
    u32x4 kw[2][KV4], vw[NVL];
    f32x4 ks[2], vs[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const unsigned char* kr = Kb + (long long)min(kb + 16 * t + c16, last) * k_rs;
#pragma unroll
      for (int h = 0; h < KV4; ++h) kw[t][h] = __builtin_nontemporal_load((const u32x4*)(kr + 16 * h));
    }
#pragma unroll
    for (int u = 0; u < NVL; ++u)
      vw[u] = __builtin_nontemporal_load((const u32x4*)(Vb + (long long)min(kb + u * RPL + vrow, last) * v_rs));
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int kc = min(kb + 16 * t + 4 * g, last & ~3);
      ks[t] = *(const f32x4*)(ksb + kc);
      vs[t] = *(const f32x4*)(vsb + kc);
    }

    // S^T = K Q^T
    float sv[8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < NM; ++i)
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            e4m3x8_to_bf16(kw[t][i / 2][2 * (i & 1)], kw[t][i / 2][2 * (i & 1) + 1]), qf[i], s, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) sv[4 * t + r] = s[r] * ks[t][r] * scale_log2;
    }
    if (tail) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (kb + 16 * (j >> 2) + 4 * g + (j & 3) >= k_hi) sv[j] = -INFINITY;
    }
    float mx = sv[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) mx = fmaxf(mx, sv[j]);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);
    const float mref = mn == -INFINITY ? 0.f : mn;
    const float alpha = __builtin_amdgcn_exp2f(m - mref);  // m = -inf -> 0
    float pv[8], psum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float p = __builtin_amdgcn_exp2f(sv[j] - mref);
      psum += p;
      pv[j] = p * vs[j >> 2][j & 3];
    }
    l = l * alpha + psum;
    m = mn;
    if (tail) {  // p = 0 there, but 0 * (a stale NaN scale) is NaN
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (kb + 16 * (j >> 2) + 4 * g + (j & 3) >= k_hi) pv[j] = 0.f;
    }
    const u32x4 pw = pack8(pv);  // one rounding of p * v_scale

    // V codes -> bf16 rows in this wave's LDS region
#pragma unroll
    for (int u = 0; u < NVL; ++u) {
      u32x4 w = vw[u];
      if (tail && kb + u * RPL + vrow >= k_hi) w = (u32x4){0u, 0u, 0u, 0u};
      unsigned char* dst = vl + (u * RPL + vrow) * PITCH + (lane % LPR) * 32;
      *(bf16x8_t*)dst = e4m3x8_to_bf16(w[0], w[1]);
      *(bf16x8_t*)(dst + 16) = e4m3x8_to_bf16(w[2], w[3]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's own writes have landed

    // O^T = alpha O^T + V^T P^T
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)LDS_PTR(vtr + 32 * dt));
      const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)LDS_PTR(vtr + 32 * dt + 16 * PITCH));
      typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
      const u32x2_t x = __builtin_bit_cast(u32x2_t, v0), y = __builtin_bit_cast(u32x2_t, v1);
      const u32x4 vf = {x[0], x[1], y[0], y[1]};
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, vf),
                                                      __builtin_bit_cast(bf16x8_t, pw), o[dt] * alpha, 0, 0, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the next tile overwrites
  }

  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  mfma_wave_merge<D>(smem, o, m, l, tid, wid, g, c16, ng, ((long long)b * H + hk * G + g0) * nsplit + split, nsplit,
                     part_o, part_ml);
}

// ---------------------------------------------------------------------------
// bf16 KV cache on the MFMA units (docs/rl_mfma_decode.md, opt-in through
// dw_attn_decode_mfma).  Work split, score / softmax dataflow and the wave
// merge are those of attn_decode_q8_kernel above; the data movement is its
// own, because bf16 rows feed the MFMAs as they lie in memory:
//  * K: lane (g, c) reads the contiguous D/2 bytes [g D/2, (g + 1) D/2) of key
//    row c straight into the A fragments (slot (g, j) of MFMA i is
//    d = g D/4 + 8 i + j, the Q fragments carry the same permutation).
//  * V: global -> LDS by DMA (global_load_lds_dwordx4), no staging registers
//    and no ds_write.  One wave instruction writes 1 KiB lane-linearly, so the
//    image keeps row-major rows of 2 D bytes and permutes the 32-byte columns
//    of a row: column c32 of row r lies at c32 ^ s(r), s(r) = r & 7 (D = 128),
//    (r >> 1) & 3 (D = 64).  The permutation lives in the per-lane SOURCE
//    address.  A half-wave's ds_read_b64_tr_b16 reads one 32-byte column of 8
//    consecutive rows: with s they fall in 8 different 32-byte bank groups.
//  * each wave owns two V buffers and prefetches across tiles: the DMA and
//    the K loads of its tile n + 1 are issued right behind the score MFMAs of
//    tile n (the K fragments are dead from there on, so tile n + 1 loads into
//    the same registers) and fly under tile n's softmax and V^T P^T; the only
//    vmcnt wait of the loop is the one at the top of a tile, on the wave's own
//    regions: no block barrier in the loop.  Two things keep it that way.  The
//    transposed reads are inline asm with their own lgkmcnt wait: the compiler
//    puts a vmcnt(0) in front of every LDS read it can see while a DMA is in
//    flight.  And the softmax reduces across lanes with v_permlane16_swap /
//    v_permlane32_swap (swap_rows16, swap_halves32 below), not __shfl_xor,
//    which is a call here and waits for every counter on entry.
// Row addresses are clamped to the last valid key of the slice: every load is
// unconditional and in bounds, no row at or past len is read.  Only the tile
// that straddles k_hi selects (wave-uniform): scores to -inf.  V needs no
// zeroing: the clamped rows are copies of a valid row and meet p = 0.

// Four V^T fragments of attn_decode_mfma_kernel (16 x 32 each: the rows at
// a[i] and the 16 rows OFF16 bytes further) with ds_read_b64_tr_b16, and the
// wait for them.  Inline asm: see the prefetch note above.
template <int OFF16>
__device__ __forceinline__ void tr_read4(const unsigned (&a)[4], u32x4 (&vf)[4]) {
  typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
  u32x2_t x[4], y[4];
  asm volatile(
      "ds_read_b64_tr_b16 %0, %8\n\tds_read_b64_tr_b16 %1, %8 offset:%12\n\t"
      "ds_read_b64_tr_b16 %2, %9\n\tds_read_b64_tr_b16 %3, %9 offset:%12\n\t"
      "ds_read_b64_tr_b16 %4, %10\n\tds_read_b64_tr_b16 %5, %10 offset:%12\n\t"
      "ds_read_b64_tr_b16 %6, %11\n\tds_read_b64_tr_b16 %7, %11 offset:%12\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(x[0]), "=&v"(y[0]), "=&v"(x[1]), "=&v"(y[1]), "=&v"(x[2]), "=&v"(y[2]), "=&v"(x[3]), "=&v"(y[3])
      : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "n"(OFF16)
      : "memory");
#pragma unroll
  for (int i = 0; i < 4; ++i) vf[i] = (u32x4){x[i][0], x[i][1], y[i][0], y[i][1]};
}

// The reductions over the 4 lanes (g, c) of a head, on the VALU alone.
// swap_rows16: r = {x of lane c + 32 (g / 2), x of lane c + 32 (g / 2) + 16}
// (v_permlane16_swap of x with itself); swap_halves32: r = {x of lane c + 16
// (g % 2), x of that lane + 32} (v_permlane32_swap).  Both values reach every
// lane of the pair, so max / sum of r is the pair's, identical in both lanes.
// No call and no LDS instruction, so nothing waits for the loads in flight
// (__shfl_xor is not inlined into a DW_NO_PK_F32 kernel, and the called
// function begins with a wait for everything).
__device__ __forceinline__ void swap_rows16(float x, float (&r)[2]) {
  const unsigned u = __float_as_uint(x);
  const auto s = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  r[0] = __uint_as_float(s[0]);
  r[1] = __uint_as_float(s[1]);
}
__device__ __forceinline__ void swap_halves32(float x, float (&r)[2]) {
  const unsigned u = __float_as_uint(x);
  const auto s = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  r[0] = __uint_as_float(s[0]);
  r[1] = __uint_as_float(s[1]);
}

template <int D>
__global__ void __launch_bounds__(64 * DEC_WAVES) DW_NO_PK_F32 attn_decode_mfma_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
    const int* __restrict__ lens, float* __restrict__ part_o, float* __restrict__ part_ml, int H, int HKV, int Smax,
    int split0, int nsplit, int chunk, float scale_log2, long long q_bs, long long k_bs, long long k_rs,
    long long v_bs, long long v_rs) {
  // the block's partials go to split slot split0 + blockIdx.x of `nsplit` (dw_attn_decode_shared puts the
  // suffix behind the prefix splits; dw_attn_decode_mfma passes 0 and its grid's x)
  constexpr int ROWB = 2 * D;                // bytes of one V row in LDS (no padding)
  constexpr int VBYTES = Q8_TILE * ROWB;     // one V tile
  constexpr int NM = D / 32;                 // MFMAs per 16-key score tile = 16-byte loads of a lane's K piece
  constexpr int DT = D / 16;                 // 16-row tiles of O^T
  constexpr int NDMA = VBYTES / 1024;        // DMA instructions per V tile
  constexpr int CPR = D / 8;                 // 16-byte chunks per V row
  constexpr int RPI = 64 / CPR;              // V rows per DMA instruction
  constexpr int MERGE = DEC_WAVES * Q8_HEADS * (D + 2) * 4;
  constexpr int SMEM = 2 * DEC_WAVES * VBYTES;
  static_assert(SMEM >= MERGE && SMEM <= 65536, "V staging holds the merge state and fits static LDS");
  // two V tiles per wave in the steady loop, then (after a barrier) the waves' states
  __shared__ __attribute__((aligned(1024))) unsigned char smem[SMEM];

  const int split = blockIdx.x, hg = blockIdx.y;
  const int b = blockIdx.z / HKV, hk = blockIdx.z % HKV;
  const int G = H / HKV;
  const int g0 = hg * Q8_HEADS;
  const int ng = min(Q8_HEADS, G - g0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const int len = min(lens[b], Smax);
  const int k_lo = split * chunk, k_hi = min(len, k_lo + chunk);
  const int ntiles = k_hi > k_lo ? (k_hi - k_lo + Q8_TILE - 1) / Q8_TILE : 0;
  const int last = k_hi - 1;

  // Q^T fragments (B operand: column = head c16), permuted like K
  bf16x8_t qf[NM];
  {
    const bool hv = c16 < ng;
    const bf16_t* qp = Q + (long long)b * q_bs + (long long)(hk * G + g0 + (hv ? c16 : 0)) * D + g * (D / 4);
#pragma unroll
    for (int i = 0; i < NM; ++i) {
      const u32x4 w = *(const u32x4*)(qp + 8 * i);
      qf[i] = __builtin_bit_cast(bf16x8_t, hv ? w : (u32x4){0u, 0u, 0u, 0u});
    }
  }
  float m = -INFINITY, l = 0.f;  // m: of head c16 (same in the 4 lanes g); l: this lane's keys only
  f32x4 o[DT];                   // O^T[16 dt + 4 g + r][head c16]
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const bf16_t* Kb = K + (long long)b * k_bs + (long long)hk * D + g * (D / 4);
  const bf16_t* Vb = V + (long long)b * v_bs + (long long)hk * D;
  unsigned char* vl = smem + wid * 2 * VBYTES;
  // DMA source of this lane: row lane / CPR of the instruction's RPI rows, the
  // chunk whose image position is lane % CPR (D = 128: s depends on the
  // instruction's parity, two offsets; D = 64: one)
  const int drow = lane / CPR;
  int dcol[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int r = RPI * par + drow;
    const int s = D == 128 ? (r & 7) : ((r >> 1) & 3);
    dcol[par] = 8 * ((lane % CPR) ^ (2 * s));
  }
  // transposed read: lane li of a 16-lane group points at row li / 4, columns
  // 4 (li % 4) .. + 3 of the 16-column tile dt; (32 dt) ^ (32 s) = 32 (dt ^ s)
  const int trow = 4 * g + (c16 >> 2);
  const int ts = D == 128 ? (trow & 7) : ((trow >> 1) & 3);  // the same for row + 16
  // (smem is 1 KiB aligned, so the xor with 32 dt touches only the bits of 32 s)
  const unsigned vtr = (unsigned)(uintptr_t)LDS_PTR(vl) + (unsigned)(trow * ROWB + 32 * ts + 8 * (c16 & 3));

  u32x4 kw[2][NM];  // the K fragments of the tile about to be scored
  auto load_tile = [&](int tile, int buf) __attribute__((always_inline)) {
    const int kb = k_lo + Q8_TILE * tile;
#pragma unroll
    for (int ci = 0; ci < NDMA; ++ci) {
      const bf16_t* src = Vb + (long long)min(kb + RPI * ci + drow, last) * v_rs + dcol[ci & 1];
      __builtin_amdgcn_global_load_lds((const void*)src, LDS_PTR(vl + buf * VBYTES + 1024 * ci), 16, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bf16_t* kr = Kb + (long long)min(kb + 16 * t + c16, last) * k_rs;
#pragma unroll
      for (int h = 0; h < NM; ++h) kw[t][h] = __builtin_nontemporal_load((const u32x4*)(kr + 8 * h));
    }
  };

  const int nw = wid < ntiles ? (ntiles - wid + DEC_WAVES - 1) / DEC_WAVES : 0;  // this wave's tiles
  if (nw > 0) load_tile(wid, 0);
  for (int n = 0; n < nw; ++n) {
    const int tile = wid + DEC_WAVES * n, buf = n & 1;
    const int kb = k_lo + Q8_TILE * tile;
    const bool tail = kb + Q8_TILE > k_hi;  // wave-uniform
    // tile n has landed, registers and LDS (nothing else of this wave is in flight)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // S^T = K Q^T
    float sv[8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < NM; ++i)
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, kw[t][i]), qf[i], s, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) sv[4 * t + r] = s[r] * scale_log2;
    }
    // the other buffer's reads ended with tile n - 1 (tr_read4 waits for them)
    if (n + 1 < nw) load_tile(tile + DEC_WAVES, buf ^ 1);
    if (tail) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (kb + 16 * (j >> 2) + 4 * g + (j & 3) >= k_hi) sv[j] = -INFINITY;
    }
    float mx = sv[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) mx = fmaxf(mx, sv[j]);
    float mo[2];
    swap_rows16(mx, mo);
    mx = fmaxf(mo[0], mo[1]);
    swap_halves32(mx, mo);
    mx = fmaxf(mo[0], mo[1]);
    const float mn = fmaxf(m, mx);
    const float mref = mn == -INFINITY ? 0.f : mn;  // all scores -inf (q.k overflowed): p = 0, not NaN
    const float alpha = __builtin_amdgcn_exp2f(m - mref);  // m = -inf -> 0
    float pv[8], psum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      pv[j] = __builtin_amdgcn_exp2f(sv[j] - mref);
      psum += pv[j];
    }
    l = l * alpha + psum;
    m = mn;
    const u32x4 pw = pack8(pv);  // one rounding of p

    // O^T = alpha O^T + V^T P^T, four 16-row tiles of O^T per group of reads
#pragma unroll
    for (int d4 = 0; d4 < DT; d4 += 4) {
      unsigned a[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = (vtr ^ (32u * (d4 + i))) + buf * VBYTES;
      u32x4 vf[4];
      tr_read4<16 * ROWB>(a, vf);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        o[d4 + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, vf[i]),
                                                            __builtin_bit_cast(bf16x8_t, pw), o[d4 + i] * alpha, 0, 0, 0);
    }
  }

  float lx[2];
  swap_rows16(l, lx);
  l = lx[0] + lx[1];
  swap_halves32(l, lx);
  l = lx[0] + lx[1];
  // every tile was waited for at the top of its iteration: no DMA is in flight at the merge's barrier
  mfma_wave_merge<D>(smem, o, m, l, tid, wid, g, c16, ng, ((long long)b * H + hk * G + g0) * nsplit + split0 + split,
                     nsplit, part_o, part_ml);
}

// ---------------------------------------------------------------------------
// Shared-prefix ("cascade") decode, prefix pass (docs/rl_shared_prefix.md,
// dw_attn_decode_shared).  q [B, H, D] with B = Bp * NS: row p * NS + j is
// sample j of prompt p, and the NS samples of a prompt attend to the same
// prefix cache row K / V [Bp, Pmax, Hkv, D].  A block owns a `chunk`-key slice
// of one KV head of one PROMPT: the query columns of (p, hk) are c = j G + g,
// NC = NS G in all, and column c reads q[p NS + c / G, hk G + c % G].  The
// block serves CT column tiles of 16 (columns 16 CT blockIdx.y ..); columns
// >= NC are zero.
//
// Per 32-key tile and wave the data movement is attn_decode_mfma_kernel's: K
// global -> VGPR as A fragments, V by DMA into the swizzled two-buffer image,
// cross-tile prefetch behind the score MFMAs, ds_read_b64_tr_b16, permlane
// swaps.  The K fragments and each group of four V^T fragments are loaded
// ONCE and feed the MFMAs of all CT column tiles; every column tile keeps its
// own Q fragments, online-softmax state (m, l) and O^T accumulators, which is
// what bounds CT.  The waves' states merge one column tile at a time through
// the V staging; a column's partial row is its own (b, h), split slot
// blockIdx.x of nsplit_total (the suffix pass fills the slots behind).
template <int D, int CT>
__global__ void __launch_bounds__(64 * DEC_WAVES) DW_NO_PK_F32 attn_decode_prefix_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
    const int* __restrict__ prefix_lens, float* __restrict__ part_o, float* __restrict__ part_ml, int H, int HKV,
    int NS, int Pmax, int nsplit_total, int chunk, float scale_log2, long long q_bs, long long k_bs, long long k_rs,
    long long v_bs, long long v_rs) {
  constexpr int ROWB = 2 * D;
  constexpr int VBYTES = Q8_TILE * ROWB;
  constexpr int NM = D / 32;
  constexpr int DT = D / 16;
  constexpr int NDMA = VBYTES / 1024;
  constexpr int CPR = D / 8;
  constexpr int RPI = 64 / CPR;
  constexpr int MERGE = DEC_WAVES * Q8_HEADS * (D + 2) * 4;
  constexpr int SMEM = 2 * DEC_WAVES * VBYTES;
  static_assert(SMEM >= MERGE && SMEM <= 65536, "V staging holds one column tile's merge state and fits static LDS");
  __shared__ __attribute__((aligned(1024))) unsigned char smem[SMEM];

  const int split = blockIdx.x;
  const int p = blockIdx.z / HKV, hk = blockIdx.z % HKV;
  const int G = H / HKV, NC = NS * G;
  const int col0 = blockIdx.y * (CT * Q8_HEADS);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const int len = min(prefix_lens[p], Pmax);
  const int k_lo = split * chunk, k_hi = min(len, k_lo + chunk);
  const int ntiles = k_hi > k_lo ? (k_hi - k_lo + Q8_TILE - 1) / Q8_TILE : 0;
  const int last = k_hi - 1;

  // Q^T fragments per column tile (B operand: column c16 of tile ct), permuted like K
  bf16x8_t qf[CT][NM];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int c = col0 + Q8_HEADS * ct + c16;
    const bool hv = c < NC;
    const int cc = hv ? c : 0;
    const bf16_t* qp =
        Q + (long long)(p * NS + cc / G) * q_bs + (long long)(hk * G + cc % G) * D + g * (D / 4);
#pragma unroll
    for (int i = 0; i < NM; ++i) {
      const u32x4 w = *(const u32x4*)(qp + 8 * i);
      qf[ct][i] = __builtin_bit_cast(bf16x8_t, hv ? w : (u32x4){0u, 0u, 0u, 0u});
    }
  }
  float m[CT], l[CT];  // as in attn_decode_mfma_kernel, per column tile
  f32x4 o[CT][DT];     // O^T[16 dt + 4 g + r][column c16 of tile ct]
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    m[ct] = -INFINITY;
    l[ct] = 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[ct][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  const bf16_t* Kb = K + (long long)p * k_bs + (long long)hk * D + g * (D / 4);
  const bf16_t* Vb = V + (long long)p * v_bs + (long long)hk * D;
  unsigned char* vl = smem + wid * 2 * VBYTES;
  const int drow = lane / CPR;
  int dcol[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int r = RPI * par + drow;
    const int s = D == 128 ? (r & 7) : ((r >> 1) & 3);
    dcol[par] = 8 * ((lane % CPR) ^ (2 * s));
  }
  const int trow = 4 * g + (c16 >> 2);
  const int ts = D == 128 ? (trow & 7) : ((trow >> 1) & 3);
  const unsigned vtr = (unsigned)(uintptr_t)LDS_PTR(vl) + (unsigned)(trow * ROWB + 32 * ts + 8 * (c16 & 3));

  u32x4 kw[2][NM];
  auto load_tile = [&](int tile, int buf) __attribute__((always_inline)) {
    const int kb = k_lo + Q8_TILE * tile;
#pragma unroll
    for (int ci = 0; ci < NDMA; ++ci) {
      const bf16_t* src = Vb + (long long)min(kb + RPI * ci + drow, last) * v_rs + dcol[ci & 1];
      __builtin_amdgcn_global_load_lds((const void*)src, LDS_PTR(vl + buf * VBYTES + 1024 * ci), 16, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const bf16_t* kr = Kb + (long long)min(kb + 16 * t + c16, last) * k_rs;
#pragma unroll
      for (int h = 0; h < NM; ++h) kw[t][h] = __builtin_nontemporal_load((const u32x4*)(kr + 8 * h));
    }
  };

  const int nw = wid < ntiles ? (ntiles - wid + DEC_WAVES - 1) / DEC_WAVES : 0;
  if (nw > 0) load_tile(wid, 0);
  for (int n = 0; n < nw; ++n) {
    const int tile = wid + DEC_WAVES * n, buf = n & 1;
    const int kb = k_lo + Q8_TILE * tile;
    const bool tail = kb + Q8_TILE > k_hi;  // wave-uniform
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // S^T = K Q^T of every column tile from the one set of K fragments
    float sv[CT][8];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NM; ++i)
          s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, kw[t][i]), qf[ct][i], s, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) sv[ct][4 * t + r] = s[r] * scale_log2;
      }
    }
    // the K fragments are dead; the other buffer's reads ended with tile n - 1
    if (n + 1 < nw) load_tile(tile + DEC_WAVES, buf ^ 1);
    float alpha[CT];
    u32x4 pw[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      if (tail) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (kb + 16 * (j >> 2) + 4 * g + (j & 3) >= k_hi) sv[ct][j] = -INFINITY;
      }
      float mx = sv[ct][0];
#pragma unroll
      for (int j = 1; j < 8; ++j) mx = fmaxf(mx, sv[ct][j]);
      float mo[2];
      swap_rows16(mx, mo);
      mx = fmaxf(mo[0], mo[1]);
      swap_halves32(mx, mo);
      mx = fmaxf(mo[0], mo[1]);
      const float mn = fmaxf(m[ct], mx);
      const float mref = mn == -INFINITY ? 0.f : mn;
      alpha[ct] = __builtin_amdgcn_exp2f(m[ct] - mref);  // m = -inf -> 0
      float pv[8], psum = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        pv[j] = __builtin_amdgcn_exp2f(sv[ct][j] - mref);
        psum += pv[j];
      }
      l[ct] = l[ct] * alpha[ct] + psum;
      m[ct] = mn;
      pw[ct] = pack8(pv);  // one rounding of p
    }

    // O^T = alpha O^T + V^T P^T: four V^T fragments per group of reads, each used by all column tiles
#pragma unroll
    for (int d4 = 0; d4 < DT; d4 += 4) {
      unsigned a[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = (vtr ^ (32u * (d4 + i))) + buf * VBYTES;
      u32x4 vf[4];
      tr_read4<16 * ROWB>(a, vf);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          o[ct][d4 + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              __builtin_bit_cast(bf16x8_t, vf[i]), __builtin_bit_cast(bf16x8_t, pw[ct]), o[ct][d4 + i] * alpha[ct], 0,
              0, 0);
      }
    }
  }

  // no DMA is in flight (every tile was waited for); the merge's barriers order the reuse of the staging
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    float lx[2];
    swap_rows16(l[ct], lx);
    float lt = lx[0] + lx[1];
    swap_halves32(lt, lx);
    lt = lx[0] + lx[1];
    const int cb = col0 + Q8_HEADS * ct;
    mfma_wave_merge_rows<D>(
        smem, o[ct], m[ct], lt, tid, wid, g, c16, min(Q8_HEADS, max(NC - cb, 0)),
        [=](int hh) {
          const int c = cb + hh;  // < NC
          return ((long long)(p * NS + c / G) * H + hk * G + c % G) * nsplit_total + split;
        },
        part_o, part_ml);
  }
}

}  // namespace

// Workspace: part_o float [B*H*nsplit*D], part_ml float [B*H*nsplit*2].
// strides (elements): q_bs, k_bs, k_rs, v_bs, v_rs, o_bs.
extern "C" int dw_attn_decode(const void* q, const void* k, const void* v, const void* lens, void* out,
                              void* part_o, void* part_ml, int B, int H, int HKV, int D, int nsplit, int chunk,
                              const long long* strides, float softmax_scale, void* stream) {
  if (H % HKV != 0 || nsplit <= 0 || chunk <= 0) return (int)hipErrorInvalidValue;
  const float scale_log2 = softmax_scale * 1.4426950408889634f;
  const int G = H / HKV;
  dim3 grid((unsigned)nsplit, (unsigned)((G + DEC_GMAX - 1) / DEC_GMAX), (unsigned)(B * HKV));
  hipStream_t s = (hipStream_t)stream;
  const long long q_bs = strides[0], k_bs = strides[1], k_rs = strides[2], v_bs = strides[3], v_rs = strides[4],
                  o_bs = strides[5];
  if (D == 128) {
    hipLaunchKernelGGL(attn_decode_split_kernel<128>, grid, dim3(64 * DEC_WAVES), 0, s, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)v, (const int*)lens, (float*)part_o, (float*)part_ml, H,
                       HKV, nsplit, chunk, scale_log2, q_bs, k_bs, k_rs, v_bs, v_rs);
    hipLaunchKernelGGL(attn_decode_merge_kernel<128>, dim3(B * H), dim3(64), 0, s, (const float*)part_o,
                       (const float*)part_ml, (bf16_t*)out, nsplit, o_bs, H);
  } else if (D == 64) {
    hipLaunchKernelGGL(attn_decode_split_kernel<64>, grid, dim3(64 * DEC_WAVES), 0, s, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)v, (const int*)lens, (float*)part_o, (float*)part_ml, H,
                       HKV, nsplit, chunk, scale_log2, q_bs, k_bs, k_rs, v_bs, v_rs);
    hipLaunchKernelGGL(attn_decode_merge_kernel<64>, dim3(B * H), dim3(64), 0, s, (const float*)part_o,
                       (const float*)part_ml, (bf16_t*)out, nsplit, o_bs, H);
  } else {
    return (int)hipErrorInvalidValue;
  }
  DW_LAUNCH_RET;
}

// e4m3 cache: k / v codes [B, Smax, HKV, D] (byte strides k_bs, k_rs, v_bs,
// v_rs, multiples of 16, 16-byte aligned bases), k_scale / v_scale fp32
// [B, HKV, Smax] (element strides ks_bs, ks_hs, vs_bs, vs_hs, multiples of 4,
// 16-byte aligned bases, readable up to the next multiple of 4 past Smax).
// strides: q_bs, k_bs, k_rs, v_bs, v_rs, o_bs, ks_bs, ks_hs, vs_bs, vs_hs.
// Workspace as dw_attn_decode; chunk % 32 == 0.
extern "C" int dw_attn_decode_q8(const void* q, const void* k, const void* v, const void* k_scale,
                                 const void* v_scale, const void* lens, void* out, void* part_o, void* part_ml,
                                 int B, int H, int HKV, int D, int Smax, int nsplit, int chunk,
                                 const long long* strides, float softmax_scale, void* stream) {
  if (H % HKV != 0 || nsplit <= 0 || chunk <= 0 || chunk % Q8_TILE || Smax < 1 ||
      (long long)nsplit * chunk < Smax)
    return (int)hipErrorInvalidValue;
  const long long* st = strides;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)k_scale | (uintptr_t)v_scale) & 15)
    return (int)hipErrorInvalidValue;
  if ((st[0] % 8) || ((st[1] | st[2] | st[3] | st[4]) % 16) || ((st[6] | st[7] | st[8] | st[9]) % 4))
    return (int)hipErrorInvalidValue;
  const float scale_log2 = softmax_scale * 1.4426950408889634f;
  const int G = H / HKV;
  dim3 grid((unsigned)nsplit, (unsigned)((G + Q8_HEADS - 1) / Q8_HEADS), (unsigned)(B * HKV));
  hipStream_t s = (hipStream_t)stream;
#define DW_DEC_Q8(DD)                                                                                              \
  hipLaunchKernelGGL(attn_decode_q8_kernel<DD>, grid, dim3(64 * DEC_WAVES), 0, s, (const bf16_t*)q,                \
                     (const unsigned char*)k, (const unsigned char*)v, (const float*)k_scale,                      \
                     (const float*)v_scale, (const int*)lens, (float*)part_o, (float*)part_ml, H, HKV, Smax,       \
                     nsplit, chunk, scale_log2, st[0], st[1], st[2], st[3], st[4], st[6], st[7], st[8], st[9]);    \
  hipLaunchKernelGGL(attn_decode_merge_kernel<DD>, dim3(B * H), dim3(64), 0, s, (const float*)part_o,              \
                     (const float*)part_ml, (bf16_t*)out, nsplit, st[5], H)
  if (D == 128) {
    DW_DEC_Q8(128);
  } else if (D == 64) {
    DW_DEC_Q8(64);
  } else {
    return (int)hipErrorInvalidValue;
  }
#undef DW_DEC_Q8
  DW_LAUNCH_RET;
}

// bf16 cache, pass 1 on the MFMA units (attn_decode_mfma_kernel); arguments
// and workspace as dw_attn_decode, plus Smax.  chunk % 32 == 0,
// nsplit * chunk >= Smax >= 1, q / k / v 16-byte aligned, q_bs and the K / V
// batch and row strides multiples of 8 elements.
extern "C" int dw_attn_decode_mfma(const void* q, const void* k, const void* v, const void* lens, void* out,
                                   void* part_o, void* part_ml, int B, int H, int HKV, int D, int Smax, int nsplit,
                                   int chunk, const long long* strides, float softmax_scale, void* stream) {
  if (HKV <= 0 || H % HKV != 0 || nsplit <= 0 || chunk <= 0 || chunk % Q8_TILE || Smax < 1 ||
      (long long)nsplit * chunk < Smax)
    return (int)hipErrorInvalidValue;
  const long long* st = strides;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) return (int)hipErrorInvalidValue;
  if ((st[0] | st[1] | st[2] | st[3] | st[4]) % 8) return (int)hipErrorInvalidValue;
  const float scale_log2 = softmax_scale * 1.4426950408889634f;
  const int G = H / HKV;
  dim3 grid((unsigned)nsplit, (unsigned)((G + Q8_HEADS - 1) / Q8_HEADS), (unsigned)(B * HKV));
  hipStream_t s = (hipStream_t)stream;
#define DW_DEC_MFMA(DD)                                                                                            \
  hipLaunchKernelGGL(attn_decode_mfma_kernel<DD>, grid, dim3(64 * DEC_WAVES), 0, s, (const bf16_t*)q,              \
                     (const bf16_t*)k, (const bf16_t*)v, (const int*)lens, (float*)part_o, (float*)part_ml, H,     \
                     HKV, Smax, 0, nsplit, chunk, scale_log2, st[0], st[1], st[2], st[3], st[4]);                  \
  hipLaunchKernelGGL(attn_decode_merge_kernel<DD>, dim3(B * H), dim3(64), 0, s, (const float*)part_o,              \
                     (const float*)part_ml, (bf16_t*)out, nsplit, st[5], H)
  if (D == 128) {
    DW_DEC_MFMA(128);
  } else if (D == 64) {
    DW_DEC_MFMA(64);
  } else {
    return (int)hipErrorInvalidValue;
  }
#undef DW_DEC_MFMA
  DW_LAUNCH_RET;
}

// Shared-prefix decode (docs/rl_shared_prefix.md): q [Bp * NS, H, D], row
// p * NS + j is sample j of prompt p; kp / vp [Bp, Pmax, HKV, D] with
// prefix_lens [Bp], ks / vs [Bp * NS, Ssuf, HKV, D] with suffix_lens [Bp * NS]
// (int32, device; clamped to Pmax / Ssuf).  out[b, h] attends to the prefix
// keys of prompt b / NS, then to the suffix keys of row b.  Three launches:
// attn_decode_prefix_kernel -> split slots [0, np), attn_decode_mfma_kernel
// over the suffix -> slots [np, np + ns), attn_decode_merge_kernel over all.
// np = ceil(Pmax / chunk), ns = ceil(Ssuf / chunk); workspace as
// dw_attn_decode with nsplit = np + ns.  chunk % 32 == 0, Pmax, Ssuf >= 1,
// q / caches 16-byte aligned, q_bs and the cache batch / row strides multiples
// of 8 elements.
// strides: q_bs, kp_bs, kp_rs, vp_bs, vp_rs, ks_bs, ks_rs, vs_bs, vs_rs, o_bs.
extern "C" int dw_attn_decode_shared(const void* q, const void* kp, const void* vp, const void* prefix_lens,
                                     const void* ks, const void* vs, const void* suffix_lens, void* out,
                                     void* part_o, void* part_ml, int Bp, int NS, int H, int HKV, int D, int Pmax,
                                     int Ssuf, int chunk, const long long* strides, float softmax_scale,
                                     void* stream) {
  if (Bp <= 0 || NS <= 0 || HKV <= 0 || H % HKV != 0 || chunk <= 0 || chunk % Q8_TILE || Pmax < 1 || Ssuf < 1)
    return (int)hipErrorInvalidValue;
  const long long* st = strides;
  if (((uintptr_t)q | (uintptr_t)kp | (uintptr_t)vp | (uintptr_t)ks | (uintptr_t)vs) & 15)
    return (int)hipErrorInvalidValue;
  if ((st[0] | st[1] | st[2] | st[3] | st[4] | st[5] | st[6] | st[7] | st[8]) % 8) return (int)hipErrorInvalidValue;
  const float scale_log2 = softmax_scale * 1.4426950408889634f;
  const int G = H / HKV, B = Bp * NS;
  const int np = (Pmax + chunk - 1) / chunk, ns = (Ssuf + chunk - 1) / chunk, nt = np + ns;
  const int nct = (NS * G + Q8_HEADS - 1) / Q8_HEADS;  // column tiles of a (prompt, KV head)
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(64 * DEC_WAVES);
#define DW_DEC_PREFIX(DD, CC)                                                                                      \
  hipLaunchKernelGGL((attn_decode_prefix_kernel<DD, CC>), dim3((unsigned)np, (unsigned)((nct + CC - 1) / CC),     \
                                                               (unsigned)(Bp * HKV)),                             \
                     blk, 0, s, (const bf16_t*)q, (const bf16_t*)kp, (const bf16_t*)vp, (const int*)prefix_lens,  \
                     (float*)part_o, (float*)part_ml, H, HKV, NS, Pmax, nt, chunk, scale_log2, st[0], st[1],      \
                     st[2], st[3], st[4])
#define DW_DEC_SHARED(DD)                                                                                          \
  if (nct == 1) {                                                                                                  \
    DW_DEC_PREFIX(DD, 1);                                                                                          \
  } else if (nct == 2) {                                                                                           \
    DW_DEC_PREFIX(DD, 2);                                                                                          \
  } else {                                                                                                         \
    DW_DEC_PREFIX(DD, 4);                                                                                          \
  }                                                                                                                \
  hipLaunchKernelGGL(attn_decode_mfma_kernel<DD>,                                                                  \
                     dim3((unsigned)ns, (unsigned)((G + Q8_HEADS - 1) / Q8_HEADS), (unsigned)(B * HKV)), blk, 0,  \
                     s, (const bf16_t*)q, (const bf16_t*)ks, (const bf16_t*)vs, (const int*)suffix_lens,           \
                     (float*)part_o, (float*)part_ml, H, HKV, Ssuf, np, nt, chunk, scale_log2, st[0], st[5],       \
                     st[6], st[7], st[8]);                                                                         \
  hipLaunchKernelGGL(attn_decode_merge_kernel<DD>, dim3(B * H), dim3(64), 0, s, (const float*)part_o,              \
                     (const float*)part_ml, (bf16_t*)out, nt, st[9], H)
  if (D == 128) {
    DW_DEC_SHARED(128);
  } else if (D == 64) {
    DW_DEC_SHARED(64);
  } else {
    return (int)hipErrorInvalidValue;
  }
#undef DW_DEC_SHARED
#undef DW_DEC_PREFIX
  DW_LAUNCH_RET;
}

DW_PRELOAD(attn_decode_merge_kernel<128>);
