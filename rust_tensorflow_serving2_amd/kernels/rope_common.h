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

}  // namespace rope
}  // namespace tfsk
