// Rotary-embedding register helpers shared by the RoPE + GQA attention kernels
// (gqattn.hip for 64-wide heads, gqattn128.hip for 128-wide heads).
#pragma once
#include "common.h"
#include "gemm_common.h"

namespace tfsk {
namespace rope {

constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ void unpack_bf16x8(const u32x4& v, float (&f)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[2 * e] = __uint_as_float(v[e] << 16);
    f[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u);
  }
}

// (x1, x2) -> (x1 c - x2 s, x2 c + x1 s) for eight pairs, fp32, one rounding to bf16
__device__ __forceinline__ void rotate8(u32x4& lo, u32x4& hi, const u32x4 (&c)[2], const u32x4 (&s)[2]) {
  float x1[8], x2[8], y1[8], y2[8];
  unpack_bf16x8(lo, x1);
  unpack_bf16x8(hi, x2);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float ce = __uint_as_float(c[e >> 2][e & 3]), se = __uint_as_float(s[e >> 2][e & 3]);
    y1[e] = x1[e] * ce - x2[e] * se;
    y2[e] = x2[e] * ce + x1[e] * se;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    lo[e] = gemm::pack_bf16x2(y1[2 * e], y1[2 * e + 1]);
    hi[e] = gemm::pack_bf16x2(y2[2 * e], y2[2 * e + 1]);
  }
}

// QK-norm (Qwen3, OLMo-2, Gemma-3): a head's row is RMS-normalised before the rotation.
// sumsq16: this lane's share of the row's sum of squares, the sixteen values of one chunk pair.
__device__ __forceinline__ float sumsq16(const u32x4& lo, const u32x4& hi) {
  float x1[8], x2[8], ss = 0.f;
  unpack_bf16x8(lo, x1);
  unpack_bf16x8(hi, x2);
#pragma unroll
  for (int e = 0; e < 8; ++e) ss = fmaf(x1[e], x1[e], fmaf(x2[e], x2[e], ss));
  return ss;
}

// rotate8 of x^ = x * r * gamma (r = rsqrt(mean(x^2) + eps) of the whole row; g1 / g2 the gammas
// of the two halves' dims): x^ stays in fp32, so the one rounding to bf16 is the rotation's
__device__ __forceinline__ void norm_rotate8(u32x4& lo, u32x4& hi, const u32x4 (&c)[2], const u32x4 (&s)[2], float r,
                                             const float (&g1)[8], const float (&g2)[8]) {
  float x1[8], x2[8], y1[8], y2[8];
  unpack_bf16x8(lo, x1);
  unpack_bf16x8(hi, x2);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float ce = __uint_as_float(c[e >> 2][e & 3]), se = __uint_as_float(s[e >> 2][e & 3]);
    const float n1 = x1[e] * r * g1[e], n2 = x2[e] * r * g2[e];
    y1[e] = n1 * ce - n2 * se;
    y2[e] = n2 * ce + n1 * se;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    lo[e] = gemm::pack_bf16x2(y1[2 * e], y1[2 * e + 1]);
    hi[e] = gemm::pack_bf16x2(y2[2 * e], y2[2 * e + 1]);
  }
}

}  // namespace rope
}  // namespace tfsk
