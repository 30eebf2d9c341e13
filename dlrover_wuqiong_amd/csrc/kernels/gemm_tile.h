// The 128x128x64 MFMA tile shared by grouped_gemm.hip and linear_logprob.hip:
// 4 waves (2x2 of 64x64 = 2x2 v_mfma_f32_32x32x16_bf16 tiles), BK = 64,
// register-staged LDS images in the img_off layout of attn_common.h.  An
// operand whose reduction index is contiguous in memory is a ROW image
// [128 rows][64 cols] read with ds_read_b128 (frag_row).
#pragma once
#include "attn_common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64, NTHR = 256;
constexpr int IMG = BM * BK * 2;  // bytes of one operand image (both shapes)

__device__ __forceinline__ bf16x8_t as_bf(const u32x4& v) { return __builtin_bit_cast(bf16x8_t, v); }

// ROW image: [128 rows][64 cols], img_off<64>.
__device__ __forceinline__ u32x4 frag_row(const char* img, int row, int kk, int hh) {
  return *(const u32x4*)(img + img_off<64>(row, 2 * kk + hh));
}

// Staged global loads of one operand tile (4 x 16 B per thread): vector
// q = tid + NTHR * i is chunk q & 7 of row q >> 3 of a ROW image.
struct Stage {
  u32x4 v[4];
};

__device__ __forceinline__ void store_row(const Stage& s, char* img, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = tid + NTHR * i;
    *(u32x4*)(img + img_off<64>(q >> 3, q & 7)) = s.v[i];
  }
}

}  // namespace
