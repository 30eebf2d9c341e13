// Flat fused AdamW / Adam-L2 with 8-/4-bit block-quantized moments
// (optimizers/fused.py FusedQAdamW).
//
// The fp32-moment flat update (optim.hip adam_flat_kernel) runs at the HBM
// copy rate of its 28 B/element (bf16 param + grad, fp32 master, m, v); the
// only lever left is moving fewer bytes.  Here m and v are kept in the codec
// of the low-bit optimizers (lowbit_codec.h: groups of 128 consecutive flat
// elements, one fp32 scale each; linear / table map for m, zero-point-free
// quadratic map for v):
//   8 bit: 2 + 4+4 + 2 + 1+1 + 1+1 = 16 B/element + 16 B of scales per group
//   4 bit: 14 B/element + the scales.
//
// One pass per element: load gradient, master and codes, decode, the SAME
// adam_elem as the fp32 kernels (optim_elem.h), write master and parameter,
// group absmax / max of the new moments by xor-shuffles over the lanes that
// own the group (no LDS), encode, store codes and -- one lane per group --
// the two scales.  The update is VALU-bound before it is HBM-bound (three
// IEEE divisions and square roots per element next to 14-16 B of traffic), so
// the second-moment encoder reuses the square root the update took
// (lowbit_codec.h q_v_sqrt) instead of dividing and rooting again.
//
// Lane mapping: a lane owns 8 consecutive elements and 16 consecutive lanes a
// group, as in qadamw_kernel: gradient and master accesses are 16 B per lane
// and contiguous across the wave; the code accesses are 8 B (8 bit) or 4 B (4
// bit) per lane.  Giving a lane 16 / 32 consecutive elements makes the code
// accesses 16 B but strides the master and gradient accesses by 64 / 128 B
// across lanes: measured 1.27x (8 bit) and 1.86x (4 bit) SLOWER at 1.56e9
// elements (profiles/r7/qadam_flat_lane_mapping.jsonl,
// docs/quantized_flat_adam.md), so only this mapping is built.
//
// The state arrays are padded to a multiple of 128 elements; elements >= n
// count as m = v = 0 (their codes come out 0) and are never read or written
// in grad / master / param.  A group may span two parameters and two decay
// blocks: decay is decided per 64-element block, as in adam_flat_kernel.
#include "optim_elem.h"
#include "lowbit_codec.h"

template <int W> struct CodeWords { unsigned int w[W]; };

template <int W>
__device__ __forceinline__ CodeWords<W> ld_codes(const unsigned char* p) {
  CodeWords<W> c;
  if constexpr (W == 4) {
    const u32x4 v = *(const u32x4*)p;
    c.w[0] = v[0]; c.w[1] = v[1]; c.w[2] = v[2]; c.w[3] = v[3];
  } else if constexpr (W == 2) {
    const uint2 v = *(const uint2*)p;
    c.w[0] = v.x; c.w[1] = v.y;
  } else {
    c.w[0] = *(const unsigned int*)p;
  }
  return c;
}
template <int W>
__device__ __forceinline__ void st_codes(unsigned char* p, const CodeWords<W>& c) {
  if constexpr (W == 4) {
    const u32x4 v = {c.w[0], c.w[1], c.w[2], c.w[3]};
    *(u32x4*)p = v;
  } else if constexpr (W == 2) {
    *(uint2*)p = make_uint2(c.w[0], c.w[1]);
  } else {
    *(unsigned int*)p = c.w[0];
  }
}

// master == nullptr: the param itself is the fp32 master (P must be float)
template <int BITS, typename G, typename P>
__global__ void __launch_bounds__(256) qadam_flat_kernel(P* __restrict__ param, float* __restrict__ master,
                                                         const G* __restrict__ grad, unsigned char* __restrict__ mq,
                                                         unsigned char* __restrict__ vq, float* __restrict__ ms,
                                                         float* __restrict__ vs, const float* __restrict__ gscale,
                                                         AdamArgs a) {
  constexpr int LPG = 16;               // lanes per group: 8 elements each
  constexpr int GPB = 256 / LPG;        // groups per block and iteration
  constexpr int CPW = 32 / BITS;        // codes per 32-bit word
  constexpr int W = 8 / CPW;            // code words per lane
  constexpr unsigned int CMASK = (1u << BITS) - 1u;
  const float gs = gscale ? *gscale : 1.f;
  const float step_size = a.lr / a.bc1;
  const float rbc2 = rsqrtf(a.bc2);
  const int64_t n_groups = (a.n + 127) >> 7;
  const int sub = threadIdx.x & (LPG - 1);
  // the LPG lanes of a group share grp, so they enter and leave the loop
  // together: the shuffles below only ever pair active lanes
  for (int64_t grp = blockIdx.x * (int64_t)GPB + threadIdx.x / LPG; grp < n_groups;
       grp += (int64_t)gridDim.x * GPB) {
    const int64_t i = (grp << 7) + sub * 8;
    const int64_t cbyte = i * BITS / 8;
    const CodeWords<W> mw = ld_codes<W>(mq + cbyte), vw = ld_codes<W>(vq + cbyte);
    const float msc = ms[grp], vsc = vs[grp];
    float mm[8], sv[8];  // first moment; second moment, then its square root
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      mm[k] = deq_m<BITS>((mw.w[k / CPW] >> (BITS * (k % CPW))) & CMASK, msc);
      sv[k] = deq_v<BITS>((vw.w[k / CPW] >> (BITS * (k % CPW))) & CMASK, vsc);
    }
    float g[8], w[8];
    // one update path; only the loads and stores of the buffer's last,
    // partly filled 8-vector (or of pure padding) are per element
    const bool full = i + 8 <= a.n;
    if (full) {
      ld8<G>(grad, i, g);
      if (master) ld8<float>(master, i, w); else ld8<P>(param, i, w);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const bool in = i + k < a.n;
        g[k] = in ? ld<G>(grad, i + k) : 0.f;
        w[k] = in ? (master ? master[i + k] : ld<P>(param, i + k)) : 0.f;
        // padding counts as m = v = 0, and with g = 0 the update keeps it so
        if (!in) mm[k] = sv[k] = 0.f;
      }
    }
    // an 8-vector never straddles a 64-block; the mask ends with the buffer
    const bool dblk = i < a.n && decays(a.decay_mask, a.n_decay, i);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool decay = a.decay_mask ? dblk : (i + k) < a.n_decay;
      adam_elem(g[k], gs, decay, a, step_size, rbc2, w[k], mm[k], sv[k]);
    }
    if (full) {
      if (master) st8<float>(master, i, w);
      st8<P>(param, i, w);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (i + k < a.n) {
          if (master) master[i + k] = w[k];
          st<P>(param, i + k, w[k]);
        }
      }
    }
    float amax = 0.f, vmax = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      amax = fmaxf(amax, fabsf(mm[k]));
      vmax = fmaxf(vmax, sv[k]);
      sv[k] = sqrtf(sv[k]);  // the square root adam_elem took: the encoder reuses it (q_v_sqrt)
    }
#pragma unroll
    for (int o = 1; o < LPG; o <<= 1) {
      amax = fmaxf(amax, __shfl_xor(amax, o, 64));
      vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
    }
    const float inv = amax > 0.f ? 1.f / amax : 0.f;
    const float vlev = v_levels_per_sqrt<BITS>(vmax);
    CodeWords<W> mo, vo;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      unsigned int wm = 0, wv = 0;
#pragma unroll
      for (int k = 0; k < CPW; ++k) {
        wm |= (unsigned int)q_m<BITS>(mm[j * CPW + k], inv) << (BITS * k);
        wv |= (unsigned int)q_v_sqrt<BITS>(sv[j * CPW + k], vlev) << (BITS * k);
      }
      mo.w[j] = wm;
      vo.w[j] = wv;
    }
    st_codes<W>(mq + cbyte, mo);
    st_codes<W>(vq + cbyte, vo);
    if (sub == 0) {
      ms[grp] = amax;
      vs[grp] = vmax;
    }
  }
}

template <int BITS, typename G, typename P>
static int launch_qadam(void* param, void* master, const void* grad, void* mq, void* vq, void* ms, void* vs,
                        const void* gscale, const AdamArgs& a, hipStream_t s) {
  // capped grid with a group-strided loop, as dw_adam_flat: 16 groups per block and iteration
  const int grid = dw_grid_for((a.n + 127) / 128, 16, 8192);
  hipLaunchKernelGGL((qadam_flat_kernel<BITS, G, P>), dim3(grid), dim3(256), 0, s, (P*)param, (float*)master,
                     (const G*)grad, (unsigned char*)mq, (unsigned char*)vq, (float*)ms, (float*)vs,
                     (const float*)gscale, a);
  DW_LAUNCH_RET;
}

// dtype codes: 0 fp32, 1 bf16.  A sub-range [lo, hi) with lo % 128 == 0 is
// launched by offsetting every pointer (lo elements for param / master /
// grad, lo or lo / 2 bytes for the codes, lo / 128 scales, lo / 64 mask
// bytes): groups are independent, so the split equals one launch bit for bit.
extern "C" int dw_qadam_flat(void* param, int param_dtype, void* master, const void* grad, int grad_dtype, void* mq,
                             void* vq, void* mscale, void* vscale, const void* gscale, int64_t n, int64_t n_decay,
                             float lr, float beta1, float beta2, float eps, float wd, float bc1, float bc2, int adamw,
                             const void* decay_mask, int bits, void* stream) {
  if ((bits != 4 && bits != 8) || n < 0) return (int)hipErrorInvalidValue;
  AdamArgs a{lr, beta1, beta2, eps, wd, bc1, bc2, n, n_decay, adamw, (const unsigned char*)decay_mask};
  hipStream_t s = (hipStream_t)stream;
  return dispatch_dtypes(param_dtype, grad_dtype, master != nullptr, [&](auto pt, auto gt) {
    using P = decltype(pt);
    using G = decltype(gt);
    if (n == 0) return 0;
    if (bits == 8) return launch_qadam<8, G, P>(param, master, grad, mq, vq, mscale, vscale, gscale, a, s);
    return launch_qadam<4, G, P>(param, master, grad, mq, vq, mscale, vscale, gscale, a, s);
  });
}

DW_PRELOAD((qadam_flat_kernel<8, bf16_t, bf16_t>));
