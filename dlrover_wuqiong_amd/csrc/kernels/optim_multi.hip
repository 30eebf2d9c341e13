// Multi-tensor fused optimizers: one launch updates every parameter of an
// optimizer, whatever its storage (FSDP2 DTensor local shards, TP shards, plain
// DDP parameters), without first packing them into a flat buffer.
//
// The host builds two device tables once per step (re-uploaded only when a
// gradient pointer changes):
//   MTDesc  per tensor : param / grad / fp32 master / exp_avg / exp_avg_sq
//                        pointers, element count, dtype + alignment flags,
//                        param-group index, weight in the global grad norm;
//   MTChunk per chunk  : (tensor, chunk) pairs of MT_CHUNK elements.
// Workgroups grid-stride over the chunk table; a chunk lives in one tensor, so
// the dtype/alignment branches are uniform per workgroup (no divergence) and
// a 16-byte aligned tensor streams through 8-element vectors (28 B/elem for
// bf16 params + fp32 master/moments, 32 B/elem with an fp32 grad).
//
// The element update is the flat kernels' (optim_elem.h adam_elem / agd_elem):
// from the same inputs this kernel and dw_adam_flat / dw_agd_flat write the
// same bits (tests/test_multi_tensor_optim.py).  Timed against the private
// update it replaced: profiles/optim_shared_elem_ab.jsonl.
//
// Hyper-parameters are per param group (<= MT_MAX_GROUPS) and passed by value,
// so an LR scheduler changing group["lr"] costs no upload.  The gradient scale
// (1/world, global-norm clip coefficient) is a device scalar: no host sync.
//
// Parity: torch.optim.AdamW / Adam math (decoupled or L2 decay) and ATorch
// AGD (atorch/atorch/optimizers/agd.py:84-150), as in optim.hip; the apex /
// DeepSpeed multi_tensor_apply they replace in atorch/atorch/optimizers/*.
#include "optim_elem.h"  // ld / st, adam_elem, agd_elem

#define MT_MAX_GROUPS 16
#define MT_CHUNK 16384
#define MT_THREADS 256

struct MTDesc {
  void* p;
  const void* g;
  float* master;
  float* m;
  float* v;
  int64_t n;
  int32_t flags;  // bit0: param bf16, bit1: grad bf16, bit2: all pointers 16 B aligned
  int32_t group;
  float norm_w;   // weight of this tensor's squared grad in the global norm
  int32_t pad;
};
static_assert(sizeof(MTDesc) == 64, "MTDesc layout is shared with python");

struct MTChunk {
  int32_t t;
  int32_t c;
};

struct MTHyper {
  float lr[MT_MAX_GROUPS], wd[MT_MAX_GROUPS], b1[MT_MAX_GROUPS], b2[MT_MAX_GROUPS];
  float eps[MT_MAX_GROUPS];   // Adam eps / AGD delta
  float bc1[MT_MAX_GROUPS], bc2[MT_MAX_GROUPS], bc1_prev[MT_MAX_GROUPS];
  float clip[MT_MAX_GROUPS];  // AGD update clip (0: off)
  int adamw;                  // Adam: 1 decoupled decay, 0 L2 in the gradient
};

// The update of one chunk [start, end) of tensor d; P / G: the tensor's
// parameter and gradient element types; elem(g, w, m, v): adam_elem or
// agd_elem with the chunk's hyper-parameters.
template <typename P, typename G, typename Elem>
__device__ __forceinline__ void mt_chunk(const MTDesc& d, int64_t start, int64_t end, const Elem& elem) {
  P* param = (P*)d.p;
  const G* grad = (const G*)d.g;
  float* master = d.master;
  int64_t vend = start;
  if (d.flags & 4) {
    vend = start + ((end - start) & ~(int64_t)7);
    for (int64_t i = start + threadIdx.x * 8; i < vend; i += MT_THREADS * 8) {
      float g[8], w[8], m[8], v[8];
      ld8<G>(grad, i, g);
      if (master) ld8<float>(master, i, w); else ld8<P>(param, i, w);
      ld8<float>(d.m, i, m);
      ld8<float>(d.v, i, v);
#pragma unroll
      for (int k = 0; k < 8; ++k) elem(g[k], w[k], m[k], v[k]);
      st8<float>(d.m, i, m);
      st8<float>(d.v, i, v);
      if (master) st8<float>(master, i, w);
      st8<P>(param, i, w);
    }
  }
  for (int64_t i = vend + threadIdx.x; i < end; i += MT_THREADS) {
    float w = master ? master[i] : ld<P>(param, i);
    float m = d.m[i], v = d.v[i];
    elem(ld<G>(grad, i), w, m, v);
    d.m[i] = m;
    d.v[i] = v;
    if (master) master[i] = w;
    st<P>(param, i, w);
  }
}

template <bool AGD>
__global__ void __launch_bounds__(MT_THREADS) mt_step_kernel(const MTDesc* __restrict__ descs,
                                                             const MTChunk* __restrict__ chunks, int64_t nchunks,
                                                             const float* __restrict__ gscale, MTHyper h) {
  const float gs = gscale ? *gscale : 1.f;
  for (int64_t ci = blockIdx.x; ci < nchunks; ci += gridDim.x) {
    const MTChunk ch = chunks[ci];
    const MTDesc d = descs[ch.t];
    const int gi = d.group;
    const int64_t start = (int64_t)ch.c * MT_CHUNK;
    const int64_t end = min(start + (int64_t)MT_CHUNK, d.n);
    // a chunk lives in one tensor: one dtype branch per chunk
    auto run = [&](const auto& elem) {
      switch (d.flags & 3) {
        case 0: mt_chunk<float, float>(d, start, end, elem); break;
        case 1: mt_chunk<bf16_t, float>(d, start, end, elem); break;
        case 2: mt_chunk<float, bf16_t>(d, start, end, elem); break;
        default: mt_chunk<bf16_t, bf16_t>(d, start, end, elem);
      }
    };
    // every element of a tensor decays (a group without decay has wd = 0)
    if constexpr (AGD) {
      const AgdArgs a{h.lr[gi], h.b1[gi], h.b2[gi], h.eps[gi], h.wd[gi], h.bc1[gi], h.bc1_prev[gi], h.bc2[gi],
                      h.clip[gi], d.n, d.n, nullptr};
      const float sqbc2 = sqrtf(a.bc2);
      const float delta_adj = a.delta * sqbc2;
      const float lr_adj = a.lr * sqbc2 / a.bc1;
      run([&](float g, float& w, float& m, float& v) { agd_elem(g, gs, true, a, delta_adj, lr_adj, w, m, v); });
    } else {
      const AdamArgs a{h.lr[gi], h.b1[gi], h.b2[gi], h.eps[gi], h.wd[gi], h.bc1[gi], h.bc2[gi], d.n, d.n, h.adamw,
                       nullptr};
      const float step_size = a.lr / a.bc1;
      const float rbc2 = rsqrtf(a.bc2);
      run([&](float g, float& w, float& m, float& v) { adam_elem(g, gs, true, a, step_size, rbc2, w, m, v); });
    }
  }
}

// sum over tensors of norm_w * ||grad||^2 -> added to *out (zeroed by the
// caller on the stream) by a deterministic fixed-order grid sum.
__global__ void __launch_bounds__(MT_THREADS) mt_sumsq_kernel(const MTDesc* __restrict__ descs,
                                                              const MTChunk* __restrict__ chunks, int64_t nchunks,
                                                              float* out, float* ws) {
  __shared__ float red[MT_THREADS / 64];
  float acc = 0.f;
  for (int64_t ci = blockIdx.x; ci < nchunks; ci += gridDim.x) {
    const MTChunk ch = chunks[ci];
    const MTDesc d = descs[ch.t];
    const bool gbf = d.flags & 2, vec = d.flags & 4;
    const int64_t start = (int64_t)ch.c * MT_CHUNK;
    const int64_t end = min(start + (int64_t)MT_CHUNK, d.n);
    float a = 0.f;
    int64_t vend = start;
    if (vec) {
      vend = start + ((end - start) & ~(int64_t)7);
      for (int64_t i = start + threadIdx.x * 8; i < vend; i += MT_THREADS * 8) {
        float g[8];
        if (gbf) ld8<bf16_t>((const bf16_t*)d.g, i, g); else ld8<float>((const float*)d.g, i, g);
#pragma unroll
        for (int k = 0; k < 8; ++k) a += g[k] * g[k];
      }
    }
    for (int64_t i = vend + threadIdx.x; i < end; i += MT_THREADS) {
      const float x = gbf ? ld<bf16_t>((const bf16_t*)d.g, i) : ld<float>((const float*)d.g, i);
      a += x * x;
    }
    acc += a * d.norm_w;
  }
  acc = block_sum<MT_THREADS>(acc, red);
  __syncthreads();  // red is reused by the finish
  grid_sum_finish<MT_THREADS>(acc, ws, out, red);
}

static int mt_grid(int64_t nchunks) {
  // enough workgroups to cover 256 CUs x 8 waves several times; each walks
  // a strided subset of the chunk table
  int64_t g = nchunks < 8192 ? nchunks : 8192;
  return (int)(g < 1 ? 1 : g);
}

// max_blocks > 0 caps the grid: an update running beside other work (the
// optimizer inside the FSDP backward, optimizers/in_backward.py) then holds
// at most that many workgroups' worth of CUs at a time
extern "C" int dw_mt_adam_grid(const void* descs, const void* chunks, int64_t nchunks, const void* gscale,
                               const void* hyper, int agd, int max_blocks, void* stream) {
  if (nchunks <= 0) return 0;
  const MTHyper h = *(const MTHyper*)hyper;
  hipStream_t s = (hipStream_t)stream;
  int g = mt_grid(nchunks);
  if (max_blocks > 0 && g > max_blocks) g = max_blocks;
  if (agd)
    hipLaunchKernelGGL(mt_step_kernel<true>, dim3(g), dim3(MT_THREADS), 0, s, (const MTDesc*)descs,
                       (const MTChunk*)chunks, nchunks, (const float*)gscale, h);
  else
    hipLaunchKernelGGL(mt_step_kernel<false>, dim3(g), dim3(MT_THREADS), 0, s, (const MTDesc*)descs,
                       (const MTChunk*)chunks, nchunks, (const float*)gscale, h);
  DW_LAUNCH_RET;
}

extern "C" int dw_mt_adam(const void* descs, const void* chunks, int64_t nchunks, const void* gscale,
                          const void* hyper, int agd, void* stream) {
  return dw_mt_adam_grid(descs, chunks, nchunks, gscale, hyper, agd, 0, stream);
}

// ws: float[GRID_SUM_MAX + 1] (see grid_sum_finish)
extern "C" int dw_mt_sumsq(const void* descs, const void* chunks, int64_t nchunks, void* out, void* ws,
                           void* stream) {
  if (nchunks <= 0) return 0;
  const int grid = mt_grid(nchunks) < GRID_SUM_MAX ? mt_grid(nchunks) : GRID_SUM_MAX;
  hipLaunchKernelGGL(mt_sumsq_kernel, dim3(grid), dim3(MT_THREADS), 0, (hipStream_t)stream, (const MTDesc*)descs,
                     (const MTChunk*)chunks, nchunks, (float*)out, (float*)ws);
  DW_LAUNCH_RET;
}

extern "C" int dw_mt_hyper_size() { return (int)sizeof(MTHyper); }
extern "C" int dw_mt_chunk() { return MT_CHUNK; }

DW_PRELOAD(mt_sumsq_kernel);
