// Depthwise 7 x 7 convolution + bias + LayerNorm over the channels in one launch
// (gfx950), NHWC bf16 in and out, stride 1, channel multiplier 1 -- the opening
// of every ConvNeXt block:
//   v[n][ho][wo][c] = bias[c] + sum_{kh,kw} x[n][ho-PT+kh][wo-PL+kw][c] * w[kh*7+kw][c]
//   y[n][ho][wo][:] = (v - mean_c v) * rsqrt(var_c v + eps) * gamma + beta
// The filter ([49][C]), bias, gamma and beta are fp32.  The accumulator starts
// at the bias and takes one fp32 FMA per tap; v is never rounded to bf16: the
// mean, then the centred sum of squares (two passes), the normalisation and the
// affine are fp32 on the fp32 v, and the result is rounded to bf16 once.
//
// A workgroup owns R output rows x TW output columns x ALL C channels (the
// statistics of a pixel need every chunk of it), TW * C/8 <= 256:
//   * a thread owns one 16-B chunk (8 channels) of one output column and the R
//     rows of the tile; chunks vary fastest across lanes, so a wave's loads and
//     stores are contiguous;
//   * the filter is walked column by column: the 7 x 8 weights of filter column
//     kw sit in registers while the R + 6 input rows of image column wo-PL+kw
//     are loaded once each and added into the (at most seven) output rows they
//     belong to -- (R + 6) input loads and 14 weight loads per filter column for
//     R outputs, against 7 and 14 per ONE output in the generic depthwise
//     kernel;
//   * every load is an unconditional buffer load: an out-of-range tap reads a
//     clamped in-range address and is masked by a select (never by a product
//     with 0: the clamped neighbour may hold Inf);
//   * the statistics: a thread sums its 8 channels, the C/8 partials of a pixel
//     meet in LDS and are summed by 8 lanes in a fixed order (a strided serial
//     sum each, then an xor butterfly) -- no atomics, so results repeat bit for
//     bit; the second pass does the same with the centred squares;
//   * stores are unconditional buffer stores: a row past Ho, a column past Wo or
//     a thread past the tile's last chunk gets an out-of-range offset, which the
//     descriptor drops.
// Two tile heights: R = 4 where that still fills the machine (1024 workgroups),
// else R = 2 (small maps, small batches).  (R = 8 needs 256 VGPRs + AGPR spills: one
// wave per SIMD, nothing to hide the loads behind; R = 4 runs four.)
#include "common.h"
#include "launch.h"

namespace tfsk {

namespace {

constexpr uint32_t kOob = 0x80000000u;    // beyond every descriptor below (operands are < 2 GiB)
constexpr int kThreads = 256;
constexpr int kK = 7;

struct DwLnArgs {
  const uint16_t* x;
  const float* w;
  const float* bias;
  const float* gamma;
  const float* beta;
  uint16_t* y;
  int N, H, W, C, PT, PL, Ho, Wo, TW, tilesH, tilesW;
  float eps;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(const void* p, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, int(bytes), 0x00020000);
}

__device__ __forceinline__ void load8f(const __amdgpu_buffer_rsrc_t& rs, uint32_t off, float* f) {
  const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
  const u32x4 b = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16u, 0, 0);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[e] = __uint_as_float(a[e]);
    f[4 + e] = __uint_as_float(b[e]);
  }
}

// red[p * C8 + k], k < C8, holds the partials of pixel p: their sum, the same in
// the 8 lanes that share p.  Lane i adds partials i, i + 8, ... in that order,
// then the 8 sums meet in an xor butterfly (a + b == b + a: every lane gets the
// same bits).
__device__ __forceinline__ float pixel_sum(const float* red, int p, int C8, int sub) {
  float s = 0.f;
  for (int k = sub; k < C8; k += 8) s += red[p * C8 + k];
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 4, 64);
  return s;
}

// grid: x = (n * tilesH + th) * tilesW + tw
template <int R>
__device__ __forceinline__ void dwln7x7(const DwLnArgs& p) {
  constexpr int T = R + kK - 1;            // input rows of the tile
  __shared__ float red[R * kThreads];      // [r][wl][c8]
  __shared__ float stat[R * kThreads];     // [r][wl]: the mean, later the rstd

  const int tid = threadIdx.x;
  const int C8 = p.C >> 3;
  const int items = p.TW * C8;             // <= kThreads
  // a thread past the tile's last chunk computes the last chunk again, and
  // neither joins the statistics nor stores
  const bool live = tid < items;
  const int j = min(tid, items - 1);
  const int wl = j / C8;
  const int c8 = j - wl * C8;
  int t0 = int(blockIdx.x);
  const int tw = t0 % p.tilesW;
  t0 /= p.tilesW;
  const int th = t0 % p.tilesH;
  const int n = t0 / p.tilesH;
  const int ho0 = th * R;
  const int wo = tw * p.TW + wl;           // may lie past Wo (last tile): clamped taps, dropped stores

  const __amdgpu_buffer_rsrc_t rsX = rsrc_of(p.x, long(p.N) * p.H * p.W * p.C * 2);
  const __amdgpu_buffer_rsrc_t rsW = rsrc_of(p.w, long(kK * kK) * p.C * 4);
  const __amdgpu_buffer_rsrc_t rsB = rsrc_of(p.bias, long(p.C) * 4);
  const __amdgpu_buffer_rsrc_t rsG = rsrc_of(p.gamma, long(p.C) * 4);
  const __amdgpu_buffer_rsrc_t rsBe = rsrc_of(p.beta, long(p.C) * 4);
  const __amdgpu_buffer_rsrc_t rsY = rsrc_of(p.y, long(p.N) * p.Ho * p.Wo * p.C * 2);

  // (gamma and beta are wanted last and loaded first: their latency is then nobody's)
  float ga[8], be[8];
  load8f(rsG, uint32_t(c8 * 8) * 4u, ga);
  load8f(rsBe, uint32_t(c8 * 8) * 4u, be);
  float acc[R][8];
  {
    float bf[8];
    load8f(rsB, uint32_t(c8 * 8) * 4u, bf);
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[r][e] = bf[e];
  }

  const int hi0 = ho0 - p.PT;
  const uint32_t row_bytes = uint32_t(p.W) * uint32_t(p.C) * 2u;
  uint32_t roff[T];
#pragma unroll
  for (int t = 0; t < T; ++t) roff[t] = uint32_t(n * p.H + min(max(hi0 + t, 0), p.H - 1)) * row_bytes;

  auto load_col = [&](int kw, u32x4 (&xv)[T], float (&wf)[kK][8]) __attribute__((always_inline)) {
    const int wi = wo - p.PL + kw;
    const uint32_t coff = uint32_t(min(max(wi, 0), p.W - 1) * p.C + c8 * 8) * 2u;
#pragma unroll
    for (int t = 0; t < T; ++t) xv[t] = __builtin_amdgcn_raw_buffer_load_b128(rsX, roff[t] + coff, 0, 0);
#pragma unroll
    for (int kh = 0; kh < kK; ++kh) load8f(rsW, uint32_t((kh * kK + kw) * p.C + c8 * 8) * 4u, wf[kh]);
  };
  auto fma_col = [&](int kw, const u32x4 (&xv)[T], const float (&wf)[kK][8]) __attribute__((always_inline)) {
    const bool okw = (unsigned)(wo - p.PL + kw) < (unsigned)p.W;
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const bool ok = okw && (unsigned)(hi0 + t) < (unsigned)p.H;
      float f[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        f[2 * e] = ok ? __uint_as_float(xv[t][e] << 16) : 0.f;
        f[2 * e + 1] = ok ? __uint_as_float(xv[t][e] & 0xffff0000u) : 0.f;
      }
#pragma unroll
      for (int kh = 0; kh < kK; ++kh) {
        const int r = t - kh;              // input row t is filter row kh of output row r
        if (r >= 0 && r < R) {
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[r][e] = fmaf(f[e], wf[kh][e], acc[r][e]);
        }
      }
    }
  };
  if constexpr (R == kDwLnRowsShort) {
    // the short form runs where the machine is not full: the next column's loads are issued before a
    // column's FMAs (two register sets, the loop unrolled)
    u32x4 xa[T], xb[T];
    float wa[kK][8], wb[kK][8];
    load_col(0, xa, wa);
#pragma unroll
    for (int kw = 0; kw < kK; kw += 2) {
      if (kw + 1 < kK) load_col(kw + 1, xb, wb);
      fma_col(kw, xa, wa);
      if (kw + 1 < kK) {
        load_col(kw + 2, xa, wa);          // (kK is odd: kw + 2 < kK here)
        fma_col(kw + 1, xb, wb);
      }
    }
  } else {
    // the tall form has other waves to hide its loads behind and keeps its registers for them
#pragma unroll 1
    for (int kw = 0; kw < kK; ++kw) {
      u32x4 xv[T];
      float wf[kK][8];
      load_col(kw, xv, wf);
      fma_col(kw, xv, wf);
    }
  }

  // ---- the statistics of the tile's R * TW pixels, two passes
  const int P = R * p.TW;
  const float fc = float(p.C);              // (a true division: a pixel of equal channels has exactly their value as its mean)
  const int sub = tid & 7;
  if (live) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float s = acc[r][0];
#pragma unroll
      for (int e = 1; e < 8; ++e) s += acc[r][e];
      red[r * items + j] = s;
    }
  }
  __syncthreads();
  for (int q = tid >> 3; q < P; q += kThreads / 8) {
    const float s = pixel_sum(red, q, C8, sub);
    if (sub == 0) stat[q] = s / fc;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float mean = stat[r * p.TW + wl];
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      acc[r][e] -= mean;
      s = fmaf(acc[r][e], acc[r][e], s);
    }
    if (live) red[r * items + j] = s;
  }
  __syncthreads();
  for (int q = tid >> 3; q < P; q += kThreads / 8) {
    const float s = pixel_sum(red, q, C8, sub);
    if (sub == 0) stat[q] = 1.f / sqrtf(s / fc + p.eps);
  }
  __syncthreads();

#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float rstd = stat[r * p.TW + wl];
    uint32_t b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = f32_to_bf16(fmaf(acc[r][e] * rstd, ga[e], be[e]));
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = b[2 * e] | (b[2 * e + 1] << 16);
    const int ho = ho0 + r;
    const uint32_t off = live && ho < p.Ho && wo < p.Wo
                             ? (uint32_t((n * p.Ho + ho) * p.Wo + wo) * uint32_t(C8) + uint32_t(c8)) * 16u
                             : kOob;
    __builtin_amdgcn_raw_buffer_store_b128(o, rsY, off, 0, 0);
  }
}

__global__ __launch_bounds__(kThreads) void dwln7x7_tall_kernel(DwLnArgs p) { dwln7x7<kDwLnRowsTall>(p); }
// at most 2 waves per SIMD asked for: the scheduler then keeps the prefetched column's loads where they
// were written instead of sinking them to save registers
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, 2))) void dwln7x7_short_kernel(DwLnArgs p) {
  dwln7x7<kDwLnRowsShort>(p);
}

// the tile: R rows x TW columns; equal column tiles of at most 256 / (C / 8) columns
struct DwLnTile {
  int R, TW, tilesH, tilesW;
  long blocks;
};

DwLnTile dwln_tile(long N, int Ho, int Wo, int C) {
  DwLnTile t;
  const int twmax = kThreads / (C / 8);
  t.tilesW = (Wo + twmax - 1) / twmax;
  t.TW = (Wo + t.tilesW - 1) / t.tilesW;
  // tall tiles re-read 6 rows in 10 instead of 6 in 8 and load the filter once
  // per 4 rows, but leave few workgroups on small maps: tall only where that
  // still fills every CU (4 resident workgroups each)
  const long tall = N * ((Ho + kDwLnRowsTall - 1) / kDwLnRowsTall) * t.tilesW;
  t.R = tall >= 1024 ? kDwLnRowsTall : kDwLnRowsShort;
  t.tilesH = (Ho + t.R - 1) / t.R;
  t.blocks = N * t.tilesH * t.tilesW;
  return t;
}

}  // namespace

bool dwconv_ln_supported(long N, long Ho, long Wo, long C, int KH, int KW, int SH, int SW) {
  return KH == kK && KW == kK && SH == 1 && SW == 1 && C % 8 == 0 && C >= 8 && C <= kDwLnMaxC && N >= 0 && Ho >= 0 &&
         Wo >= 0 && N * Ho * Wo * C * 2 < 0x7ffffff0L;
}

long dwconv_ln_grid(long N, long Ho, long Wo, long C) {
  if (!dwconv_ln_supported(N, Ho, Wo, C, kK, kK, 1, 1) || N == 0 || Ho == 0 || Wo == 0) return 0;
  return dwln_tile(N, int(Ho), int(Wo), int(C)).blocks;
}

hipError_t dwconv_ln_launch(const uint16_t* x, const float* w, const float* bias, const float* gamma,
                            const float* beta, uint16_t* y, int N, int H, int W, int C, int KH, int KW, int SH, int SW,
                            int PT, int PL, int Ho, int Wo, float eps, hipStream_t s) {
  if (!dwconv_ln_supported(N, Ho, Wo, C, KH, KW, SH, SW)) return hipErrorInvalidValue;
  if (PT < 0 || PL < 0 || H <= 0 || W <= 0 || !(eps >= 0.f)) return hipErrorInvalidValue;
  if (N == 0 || Ho == 0 || Wo == 0) return hipSuccess;
  // 32-bit byte offsets; kOob must lie beyond every operand
  if (long(N) * H * W * C * 2 >= 0x7ffffff0L) return hipErrorInvalidValue;
  for (const void* q : {(const void*)x, (const void*)w, (const void*)bias, (const void*)gamma, (const void*)beta,
                        (const void*)y})
    if (q == nullptr || (reinterpret_cast<uintptr_t>(q) & 15u)) return hipErrorInvalidValue;
  const DwLnTile t = dwln_tile(N, Ho, Wo, C);
  if (t.blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const DwLnArgs a{x, w, bias, gamma, beta, y, N, H, W, C, PT, PL, Ho, Wo, t.TW, t.tilesH, t.tilesW, eps};
  const dim3 grid{unsigned(t.blocks)};
  if (t.R == kDwLnRowsTall) hipLaunchKernelGGL(dwln7x7_tall_kernel, grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(dwln7x7_short_kernel, grid, dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace tfsk
