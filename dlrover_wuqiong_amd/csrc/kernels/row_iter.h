// One block walks one row of a [*, V] bf16 / fp32 tensor (the RL token ops:
// token_logprob.hip, sample.hip).
//
// 16-byte vector loads (8 bf16 / 4 fp32 per lane) are used only when the row
// starts on a 16-byte boundary; otherwise (odd V in bf16, a sliced base) every
// element is loaded on its own.  The tail after the vector part is scalar.
#pragma once
#include "dw_common.h"

template <typename T>
struct RowVec;

template <>
struct RowVec<bf16_t> {
  static constexpr int W = 8;
  static __device__ __forceinline__ void load(const bf16_t* p, float* f) { unpack8(*(const u32x4*)p, f); }
  static __device__ __forceinline__ void store(bf16_t* p, const float* f) { *(u32x4*)p = pack8(f); }
  static __device__ __forceinline__ float load1(const bf16_t* p) { return bf2f(*p); }
  static __device__ __forceinline__ void store1(bf16_t* p, float f) { *p = f2bf(f); }
};

template <>
struct RowVec<float> {
  static constexpr int W = 4;
  static __device__ __forceinline__ void load(const float* p, float* f) {
    const f32x4 v = *(const f32x4*)p;
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = v[i];
  }
  static __device__ __forceinline__ void store(float* p, const float* f) {
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = f[i];
    *(f32x4*)p = v;
  }
  static __device__ __forceinline__ float load1(const float* p) { return *p; }
  static __device__ __forceinline__ void store1(float* p, float f) { *p = f; }
};

__device__ __forceinline__ bool row_aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// f(j0, v): v is float[W] (vector part) or float[1] (scalar part / tail),
// holding the elements j0 .. j0 + N - 1 of the row.
template <typename T, int NT, typename F>
__device__ __forceinline__ void row_foreach(const T* __restrict__ x, int V, F&& f) {
  constexpr int W = RowVec<T>::W;
  const int nv = row_aligned16(x) ? V / W : 0;
  for (int c = threadIdx.x; c < nv; c += NT) {
    float v[W];
    RowVec<T>::load(x + (int64_t)c * W, v);
    f(c * W, v);
  }
  for (int j = nv * W + threadIdx.x; j < V; j += NT) {
    float v[1] = {RowVec<T>::load1(x + j)};
    f(j, v);
  }
}
