// RMSNorm and SwiGLU for Llama-style decoders and GeGLU for ModernBERT-style
// encoders, gfx950.  All bf16 traffic is 16-B vectorised (8 elements per lane
// and access).
//
// rmsnorm: y = bf16((x + r) * rsqrt(mean((x + r)^2) + eps) * gamma), optionally
// also sum = bf16(x + r) (the residual stream the next block adds to).  A row
// is held by LPR lanes x CH chunks of 8 fp32 values, read once; the sum of
// squares (no mean is subtracted, so one pass has no cancellation) is reduced
// over the LPR lanes with xor shuffles and the row is scaled from registers.
// LPR in {16, 32, 64} by row length, so a 256-thread workgroup handles 16, 8 or
// 4 rows and short rows leave no lane idle; up to 64 x 8 x 8 = 4096 columns
// stay in registers, longer rows stream twice (one wave per row).
//
// swiglu: y[m][f] = bf16(swish(g) * u), g = gu[m][f], u = gu[m][F + f], after
// ONE GEMM over the concatenated [gate | up] weights; fp32, the sigmoid spelled
// as in the swish epilogue (common.h sigmoid()).  One 16-B chunk of each half
// per thread.
//
// geglu: the same launch with the gate's activation the erf GELU,
// y[m][f] = bf16(0.5 g (1 + erf(g / sqrt 2)) * u), spelled as the GEMM epilogues
// spell it (common.h kActGeluErf).  Its tanh-approximate form (Gemma's
// gelu_pytorch_tanh) is a second compile-time build of the same kernel with
// common.h's gelu_tanh, 0.5 g (1 + tanh(sqrt(2/pi) (g + 0.044715 g^3))) * u;
// the erf build is untouched by it.

#include "common.h"
#include "launch.h"

namespace tfsk {

namespace {

__device__ __forceinline__ void unpack8(const uint4& v, float* f) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[2 * e] = __uint_as_float(w[e] << 16);
    f[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
  }
}

__device__ __forceinline__ uint4 pack8(const float* f) {
  uint32_t w[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) w[e] = uint32_t(f32_to_bf16(f[2 * e])) | (uint32_t(f32_to_bf16(f[2 * e + 1])) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// x (+ r) chunk at column c -> f; stores the rounded sum when asked to
__device__ __forceinline__ void rms_load(const uint16_t* xr, const uint16_t* rr, uint16_t* sr, int c, float* f) {
  unpack8(*reinterpret_cast<const uint4*>(xr + c), f);
  if (rr) {
    float g[8];
    unpack8(*reinterpret_cast<const uint4*>(rr + c), g);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] += g[e];
  }
  if (sr) *reinterpret_cast<uint4*>(sr + c) = pack8(f);
}

__device__ __forceinline__ void rms_store(uint16_t* yr, int c, const float* f, float inv,
                                          const float* __restrict__ gamma) {
  const float4 g0 = *reinterpret_cast<const float4*>(gamma + c), g1 = *reinterpret_cast<const float4*>(gamma + c + 4);
  const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = f[e] * inv * g[e];
  *reinterpret_cast<uint4*>(yr + c) = pack8(o);
}

template <int LPR>
__device__ __forceinline__ float lanes_sum(float v) {
#pragma unroll
  for (int off = 1; off < LPR; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int LPR, int CH>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ r,
                                                      const float* __restrict__ gamma, uint16_t* __restrict__ y,
                                                      uint16_t* __restrict__ sum, int rows, int cols, float eps) {
  constexpr int RPB = 256 / LPR;          // rows per workgroup
  const int row = blockIdx.x * RPB + threadIdx.x / LPR;
  const int l = threadIdx.x % LPR;
  // (no barrier below: a group past the last row leaves; the shuffles stay inside a group of LPR lanes)
  if (row >= rows) return;
  const long base = long(row) * cols;
  const uint16_t* xr = x + base;
  const uint16_t* rr = r ? r + base : nullptr;
  uint16_t* sr = sum ? sum + base : nullptr;
  float v[CH][8];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int c = (k * LPR + l) * 8;
    if (c < cols) {
      rms_load(xr, rr, sr, c, v[k]);
#pragma unroll
      for (int e = 0; e < 8; ++e) ss += v[k][e] * v[k][e];
    }
  }
  const float inv = rsqrtf(lanes_sum<LPR>(ss) / cols + eps);
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int c = (k * LPR + l) * 8;
    if (c < cols) rms_store(y + base, c, v[k], inv, gamma);
  }
}

// rows longer than 4096 columns: one wave per row, the row read twice
__global__ __launch_bounds__(256) void rmsnorm_stream_kernel(const uint16_t* __restrict__ x,
                                                             const uint16_t* __restrict__ r,
                                                             const float* __restrict__ gamma,
                                                             uint16_t* __restrict__ y, uint16_t* __restrict__ sum,
                                                             int rows, int cols, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const long base = long(row) * cols;
  const uint16_t* rr = r ? r + base : nullptr;
  float ss = 0.f;
  for (int c = lane * 8; c < cols; c += 512) {
    float f[8];
    rms_load(x + base, rr, sum ? sum + base : nullptr, c, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) ss += f[e] * f[e];
  }
  const float inv = rsqrtf(lanes_sum<64>(ss) / cols + eps);
  for (int c = lane * 8; c < cols; c += 512) {
    float f[8];
    rms_load(x + base, rr, nullptr, c, f);
    rms_store(y + base, c, f, inv, gamma);
  }
}

template <int ACT>
__global__ __launch_bounds__(256) void glu_kernel(const uint16_t* __restrict__ gu, uint16_t* __restrict__ y,
                                                  long chunks, int F) {
  const long i = long(blockIdx.x) * 256 + threadIdx.x;
  if (i >= chunks) return;
  const int per_row = F / 8;
  const long m = i / per_row;
  const int c = int(i % per_row) * 8;
  const uint16_t* row = gu + m * 2 * F;
  float g[8], u[8], o[8];
  unpack8(*reinterpret_cast<const uint4*>(row + c), g);
  unpack8(*reinterpret_cast<const uint4*>(row + F + c), u);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = act_fn<ACT>(g[e]) * u[e];
  *reinterpret_cast<uint4*>(y + m * F + c) = pack8(o);
}

template <int LPR, int CH>
hipError_t rms_run(const uint16_t* x, const uint16_t* r, const float* gamma, uint16_t* y, uint16_t* sum, int rows,
                   int cols, float eps, hipStream_t s) {
  constexpr int RPB = 256 / LPR;
  hipLaunchKernelGGL((rmsnorm_kernel<LPR, CH>), dim3((rows + RPB - 1) / RPB), dim3(256), 0, s, x, r, gamma, y, sum,
                     rows, cols, eps);
  return hipGetLastError();
}

}  // namespace

hipError_t rmsnorm_launch(const uint16_t* x, const uint16_t* r, const float* gamma, uint16_t* y, uint16_t* sum,
                          int rows, int cols, float eps, hipStream_t s) {
  if (rows < 0 || cols < 8 || cols % 8 || x == nullptr || gamma == nullptr || y == nullptr) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(gamma) |
       reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(sum)) & 15)
    return hipErrorInvalidValue;
  if (rows == 0) return hipSuccess;
  if (cols <= 128) return rms_run<16, 1>(x, r, gamma, y, sum, rows, cols, eps, s);
  if (cols <= 256) return rms_run<32, 1>(x, r, gamma, y, sum, rows, cols, eps, s);
  if (cols <= 512) return rms_run<64, 1>(x, r, gamma, y, sum, rows, cols, eps, s);
  if (cols <= 1024) return rms_run<64, 2>(x, r, gamma, y, sum, rows, cols, eps, s);
  if (cols <= 2048) return rms_run<64, 4>(x, r, gamma, y, sum, rows, cols, eps, s);
  if (cols <= 4096) return rms_run<64, 8>(x, r, gamma, y, sum, rows, cols, eps, s);
  hipLaunchKernelGGL(rmsnorm_stream_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, r, gamma, y, sum, rows, cols,
                     eps);
  return hipGetLastError();
}

namespace {

template <int ACT>
hipError_t glu_run(const uint16_t* gu, uint16_t* y, long M, int F, hipStream_t s) {
  if (M < 0 || F < 8 || F % 8 || gu == nullptr || y == nullptr) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(gu) | reinterpret_cast<uintptr_t>(y)) & 15) return hipErrorInvalidValue;
  const long chunks = M * (F / 8);
  if (chunks == 0) return hipSuccess;
  const long grid = (chunks + 255) / 256;
  if (grid >= (1L << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(glu_kernel<ACT>, dim3(unsigned(grid)), dim3(256), 0, s, gu, y, chunks, F);
  return hipGetLastError();
}

}  // namespace

hipError_t swiglu_launch(const uint16_t* gu, uint16_t* y, long M, int F, hipStream_t s) {
  return glu_run<kActSwish>(gu, y, M, F, s);
}

hipError_t geglu_launch(const uint16_t* gu, uint16_t* y, long M, int F, hipStream_t s, bool approximate) {
  return approximate ? glu_run<kActGeluTanh>(gu, y, M, F, s) : glu_run<kActGeluErf>(gu, y, M, F, s);
}

}  // namespace tfsk
