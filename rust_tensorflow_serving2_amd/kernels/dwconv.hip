// Depthwise KH x KW convolution (gfx950), NHWC bf16 in and out, channel
// multiplier 1: y[n][ho][wo][c] = act(bias[c] + sum_{kh,kw} x[n][ho*SH-PT+kh][wo*SW-PL+kw][c] * w[kh*KW+kw][c]).
// The filter ([KH*KW][C], BatchNorm folded in) and the bias stay fp32; the
// accumulation is one fp32 FMA per tap on top of the bias, then the
// activation (none, ReLU, ReLU6, hard-swish or swish) and one
// round-to-nearest-even store to bf16.
//
// The op is bandwidth-bound (KH*KW FMAs per 2 bytes in and 2 bytes out), so
// the 3x3 kernels are built around one read of the input and one write of the
// output:
//   * a thread owns one 16-B chunk (8 channels) of one output column and a
//     strip of R consecutive output rows; chunks vary fastest across lanes, so
//     a wave's loads and stores are contiguous;
//   * its 8 x 9 weights and 8 biases sit in registers for its whole life;
//   * the strip's (R - 1) S + 3 input rows are each loaded once (three taps):
//     a loaded row is added into the (at most three) output rows it belongs
//     to, and an output row is stored as soon as its last input row is in;
//   * every load is unconditional -- an out-of-range tap reads a clamped
//     in-range address and is masked by a select (never by a product with 0:
//     the clamped neighbour may hold Inf) -- and the next row's loads are
//     issued before the current row's FMAs;
//   * stores are unconditional buffer stores: a row past Ho, or a thread past
//     the row's last chunk, gets an out-of-range offset, which the descriptor
//     drops.
// The 5x5 strip kernel (equal strides 1 or 2; strips of 2 or 4 rows, on request
// only) is the same design with a thread owning an 8-B half chunk (4 channels):
// 8 x 25 weights would leave one wave per SIMD, 4 x 25 leave three.  Lanes still
// run fastest along channels, so a wave's 8-B loads and stores are contiguous.
// Its accumulation order is the generic kernel's (bias, then filter rows
// ascending, taps ascending, one FMA each), and its results are the generic
// kernel's bit for bit.
// Any other filter up to 7 x 7 or any stride pair runs the generic kernel: one
// output chunk per thread, a run-time loop over the filter rows, seven taps
// (masked beyond KW) in flight per row, weights read per tap.
#include "common.h"
#include "launch.h"

namespace tfsk {

namespace {

constexpr uint32_t kOob = 0x80000000u;    // beyond every descriptor below (operands are < 2 GiB)
constexpr int kThreads = 256;
constexpr int kMaxTaps = 7;

struct DwArgs {
  const uint16_t* x;
  const float* w;
  const float* bias;
  uint16_t* y;
  int N, H, W, C, KH, KW, SH, SW, PT, PL, Ho, Wo;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(const void* p, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, int(bytes), 0x00020000);
}

__device__ __forceinline__ void unpack8(const u32x4& v, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[2 * e] = __uint_as_float(v[e] << 16);
    f[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u);
  }
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

template <int ACT>
__device__ __forceinline__ u32x4 act_pack8(const float* v) {
  uint32_t b[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) b[e] = f32_to_bf16(act_fn<ACT>(v[e]));
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = b[2 * e] | (b[2 * e + 1] << 16);
  return o;
}

// 3 x 3, stride S in both directions, strips of R output rows.
// grid: x = N * ceil(Ho / R) strips, y = blocks of 256 of the row's Wo * C/8 chunks.
template <int S, int R, int ACT>
__global__ __launch_bounds__(kThreads) void dwconv3x3_kernel(DwArgs p) {
  const int C8 = p.C >> 3;
  // a thread past the row's last chunk computes the last chunk again and drops
  // its stores (no exec-masked region around the loads and their waits)
  const bool live = int(blockIdx.y * kThreads + threadIdx.x) < p.Wo * C8;
  const int j = min(int(blockIdx.y * kThreads + threadIdx.x), p.Wo * C8 - 1);
  const int wo = j / C8;
  const int c8 = j - wo * C8;
  const int strips = (p.Ho + R - 1) / R;
  const int n = blockIdx.x / strips;
  const int ho0 = (blockIdx.x - n * strips) * R;

  const __amdgpu_buffer_rsrc_t rsX = rsrc_of(p.x, long(p.N) * p.H * p.W * p.C * 2);
  const __amdgpu_buffer_rsrc_t rsW = rsrc_of(p.w, long(9) * p.C * 4);
  const __amdgpu_buffer_rsrc_t rsB = rsrc_of(p.bias, long(p.C) * 4);
  const __amdgpu_buffer_rsrc_t rsY = rsrc_of(p.y, long(p.N) * p.Ho * p.Wo * p.C * 2);

  float wf[9][8], bf[8];
#pragma unroll
  for (int t = 0; t < 9; ++t) load8f(rsW, uint32_t(t * p.C + c8 * 8) * 4u, wf[t]);
  load8f(rsB, uint32_t(c8 * 8) * 4u, bf);

  bool okw[3];
  uint32_t coff[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int wi = wo * S - p.PL + k;
    okw[k] = (unsigned)wi < (unsigned)p.W;
    coff[k] = uint32_t(min(max(wi, 0), p.W - 1) * p.C + c8 * 8) * 2u;
  }
  const int hi0 = ho0 * S - p.PT;
  const uint32_t row_bytes = uint32_t(p.W) * uint32_t(p.C) * 2u;
  auto load_row = [&](int t, u32x4 (&v)[3]) __attribute__((always_inline)) {
    const int hc = min(max(hi0 + t, 0), p.H - 1);
    const uint32_t roff = uint32_t(n * p.H + hc) * row_bytes;
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = __builtin_amdgcn_raw_buffer_load_b128(rsX, roff + coff[k], 0, 0);
  };

  constexpr int T = (R - 1) * S + 3;       // input rows of the strip
  float acc[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[r][e] = bf[e];
  u32x4 cur[3], nxt[3];
  load_row(0, cur);
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (t + 1 < T) load_row(t + 1, nxt);
    const bool okh = (unsigned)(hi0 + t) < (unsigned)p.H;
    float f[3][8];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      unpack8(cur[k], f[k]);
      const bool ok = okh && okw[k];
#pragma unroll
      for (int e = 0; e < 8; ++e) f[k][e] = ok ? f[k][e] : 0.f;
    }
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int d = t - kh;                // input row t is filter row kh of output row d / S
      if (d >= 0 && d % S == 0 && d / S < R) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[d / S][e] = fmaf(f[k][e], wf[kh * 3 + k][e], acc[d / S][e]);
      }
    }
    if (t >= 2 && (t - 2) % S == 0) {      // output row (t - 2) / S is complete
      const int r = (t - 2) / S;
      const int ho = ho0 + r;
      const uint32_t off = live && ho < p.Ho ? (uint32_t(n * p.Ho + ho) * uint32_t(p.Wo * C8) + uint32_t(j)) * 16u : kOob;
      __builtin_amdgcn_raw_buffer_store_b128(act_pack8<ACT>(acc[r]), rsY, off, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) cur[k] = nxt[k];
  }
}

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

// 5 x 5, stride S in both directions, strips of R output rows, 4 channels per thread.
// grid: x = N * ceil(Ho / R) strips, y = blocks of 256 of the row's Wo * C/4 half chunks.
template <int S, int R, int ACT>
__global__ __launch_bounds__(kThreads) void dwconv5x5_kernel(DwArgs p) {
  const int C4 = p.C >> 2;
  const bool live = int(blockIdx.y * kThreads + threadIdx.x) < p.Wo * C4;     // as in dwconv3x3_kernel
  const int j = min(int(blockIdx.y * kThreads + threadIdx.x), p.Wo * C4 - 1);
  const int wo = j / C4;
  const int c4 = j - wo * C4;
  const int strips = (p.Ho + R - 1) / R;
  const int n = blockIdx.x / strips;
  const int ho0 = (blockIdx.x - n * strips) * R;

  const __amdgpu_buffer_rsrc_t rsX = rsrc_of(p.x, long(p.N) * p.H * p.W * p.C * 2);
  const __amdgpu_buffer_rsrc_t rsW = rsrc_of(p.w, long(25) * p.C * 4);
  const __amdgpu_buffer_rsrc_t rsB = rsrc_of(p.bias, long(p.C) * 4);
  const __amdgpu_buffer_rsrc_t rsY = rsrc_of(p.y, long(p.N) * p.Ho * p.Wo * p.C * 2);

  float wf[25][4], bf[4];
#pragma unroll
  for (int t = 0; t < 25; ++t) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsW, uint32_t(t * p.C + c4 * 4) * 4u, 0, 0);
#pragma unroll
    for (int e = 0; e < 4; ++e) wf[t][e] = __uint_as_float(v[e]);
  }
  {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsB, uint32_t(c4 * 4) * 4u, 0, 0);
#pragma unroll
    for (int e = 0; e < 4; ++e) bf[e] = __uint_as_float(v[e]);
  }

  bool okw[5];
  uint32_t coff[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int wi = wo * S - p.PL + k;
    okw[k] = (unsigned)wi < (unsigned)p.W;
    coff[k] = uint32_t(min(max(wi, 0), p.W - 1) * p.C + c4 * 4) * 2u;
  }
  const int hi0 = ho0 * S - p.PT;
  const uint32_t row_bytes = uint32_t(p.W) * uint32_t(p.C) * 2u;
  auto load_row = [&](int t, u32x2 (&v)[5]) __attribute__((always_inline)) {
    const int hc = min(max(hi0 + t, 0), p.H - 1);
    const uint32_t roff = uint32_t(n * p.H + hc) * row_bytes;
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = __builtin_amdgcn_raw_buffer_load_b64(rsX, roff + coff[k], 0, 0);
  };

  constexpr int T = (R - 1) * S + 5;       // input rows of the strip
  float acc[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[r][e] = bf[e];
  u32x2 cur[5], nxt[5];
  load_row(0, cur);
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (t + 1 < T) load_row(t + 1, nxt);
    const bool okh = (unsigned)(hi0 + t) < (unsigned)p.H;
    float f[5][4];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const bool ok = okh && okw[k];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        f[k][2 * e] = ok ? __uint_as_float(cur[k][e] << 16) : 0.f;
        f[k][2 * e + 1] = ok ? __uint_as_float(cur[k][e] & 0xffff0000u) : 0.f;
      }
    }
    // ascending t is ascending kh for every output row: the generic kernel's order
#pragma unroll
    for (int kh = 4; kh >= 0; --kh) {
      const int d = t - kh;                // input row t is filter row kh of output row d / S
      if (d >= 0 && d % S == 0 && d / S < R) {
#pragma unroll
        for (int k = 0; k < 5; ++k)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[d / S][e] = fmaf(f[k][e], wf[kh * 5 + k][e], acc[d / S][e]);
      }
    }
    if (t >= 4 && (t - 4) % S == 0) {      // output row (t - 4) / S is complete
      const int r = (t - 4) / S;
      const int ho = ho0 + r;
      const uint32_t off = live && ho < p.Ho ? (uint32_t(n * p.Ho + ho) * uint32_t(p.Wo * C4) + uint32_t(j)) * 8u : kOob;
      uint32_t b[4];
      // + 0: the generic kernel's two masked taps per filter row (fmaf(0, 0, acc)) turn a -0 sum into +0
#pragma unroll
      for (int e = 0; e < 4; ++e) b[e] = f32_to_bf16(act_fn<ACT>(acc[r][e] + 0.f));
      u32x2 o;
      o[0] = b[0] | (b[1] << 16);
      o[1] = b[2] | (b[3] << 16);
      __builtin_amdgcn_raw_buffer_store_b64(o, rsY, off, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) cur[k] = nxt[k];
  }
}

// Any KH, KW <= 7 and any strides.  grid: x = N * Ho output rows, y as above.
template <int ACT>
__global__ __launch_bounds__(kThreads) void dwconv_generic_kernel(DwArgs p) {
  const int C8 = p.C >> 3;
  const bool live = int(blockIdx.y * kThreads + threadIdx.x) < p.Wo * C8;     // as in dwconv3x3_kernel
  const int j = min(int(blockIdx.y * kThreads + threadIdx.x), p.Wo * C8 - 1);
  const int wo = j / C8;
  const int c8 = j - wo * C8;
  const int n = blockIdx.x / p.Ho;
  const int ho = blockIdx.x - n * p.Ho;

  const __amdgpu_buffer_rsrc_t rsX = rsrc_of(p.x, long(p.N) * p.H * p.W * p.C * 2);
  const __amdgpu_buffer_rsrc_t rsW = rsrc_of(p.w, long(p.KH) * p.KW * p.C * 4);
  const __amdgpu_buffer_rsrc_t rsB = rsrc_of(p.bias, long(p.C) * 4);
  const __amdgpu_buffer_rsrc_t rsY = rsrc_of(p.y, long(p.N) * p.Ho * p.Wo * p.C * 2);

  float acc[8];
  load8f(rsB, uint32_t(c8 * 8) * 4u, acc);
  bool okw[kMaxTaps];
  uint32_t coff[kMaxTaps];
#pragma unroll
  for (int k = 0; k < kMaxTaps; ++k) {
    const int wi = wo * p.SW - p.PL + k;
    okw[k] = k < p.KW && (unsigned)wi < (unsigned)p.W;
    coff[k] = uint32_t(min(max(wi, 0), p.W - 1) * p.C + c8 * 8) * 2u;
  }
  const uint32_t row_bytes = uint32_t(p.W) * uint32_t(p.C) * 2u;
  for (int kh = 0; kh < p.KH; ++kh) {
    const int hi = ho * p.SH - p.PT + kh;
    const bool okh = (unsigned)hi < (unsigned)p.H;
    const uint32_t roff = uint32_t(n * p.H + min(max(hi, 0), p.H - 1)) * row_bytes;
    u32x4 xv[kMaxTaps];
    float wv[kMaxTaps][8];
#pragma unroll
    for (int k = 0; k < kMaxTaps; ++k) {
      xv[k] = __builtin_amdgcn_raw_buffer_load_b128(rsX, roff + coff[k], 0, 0);
      // taps beyond KW: an out-of-range offset, which reads zeros
      load8f(rsW, k < p.KW ? uint32_t((kh * p.KW + k) * p.C + c8 * 8) * 4u : kOob, wv[k]);
    }
#pragma unroll
    for (int k = 0; k < kMaxTaps; ++k) {
      float f[8];
      unpack8(xv[k], f);
      const bool ok = okh && okw[k];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(ok ? f[e] : 0.f, wv[k][e], acc[e]);
    }
  }
  const uint32_t off = live ? (uint32_t(blockIdx.x) * uint32_t(p.Wo * C8) + uint32_t(j)) * 16u : kOob;
  __builtin_amdgcn_raw_buffer_store_b128(act_pack8<ACT>(acc), rsY, off, 0, 0);
}

template <int S, int R>
void launch3x3(const DwArgs& a, int act, dim3 grid, hipStream_t s) {
  switch (act) {
    case kActRelu: hipLaunchKernelGGL((dwconv3x3_kernel<S, R, kActRelu>), grid, dim3(kThreads), 0, s, a); break;
    case kActRelu6: hipLaunchKernelGGL((dwconv3x3_kernel<S, R, kActRelu6>), grid, dim3(kThreads), 0, s, a); break;
    case kActHardSwish:
      hipLaunchKernelGGL((dwconv3x3_kernel<S, R, kActHardSwish>), grid, dim3(kThreads), 0, s, a);
      break;
    case kActSwish: hipLaunchKernelGGL((dwconv3x3_kernel<S, R, kActSwish>), grid, dim3(kThreads), 0, s, a); break;
    default: hipLaunchKernelGGL((dwconv3x3_kernel<S, R, kActNone>), grid, dim3(kThreads), 0, s, a); break;
  }
}

template <int S, int R>
void launch5x5(const DwArgs& a, int act, dim3 grid, hipStream_t s) {
  switch (act) {
    case kActRelu: hipLaunchKernelGGL((dwconv5x5_kernel<S, R, kActRelu>), grid, dim3(kThreads), 0, s, a); break;
    case kActRelu6: hipLaunchKernelGGL((dwconv5x5_kernel<S, R, kActRelu6>), grid, dim3(kThreads), 0, s, a); break;
    case kActHardSwish:
      hipLaunchKernelGGL((dwconv5x5_kernel<S, R, kActHardSwish>), grid, dim3(kThreads), 0, s, a);
      break;
    case kActSwish: hipLaunchKernelGGL((dwconv5x5_kernel<S, R, kActSwish>), grid, dim3(kThreads), 0, s, a); break;
    default: hipLaunchKernelGGL((dwconv5x5_kernel<S, R, kActNone>), grid, dim3(kThreads), 0, s, a); break;
  }
}

bool is5x5(int KH, int KW, int SH, int SW) { return KH == 5 && KW == 5 && SH == SW && (SH == 1 || SH == 2); }

}  // namespace

int dwconv_strip(int N, int Ho, int Wo, int C, int KH, int KW, int SH, int SW, int strip) {
  if (!(KH == 3 && KW == 3 && SH == SW && (SH == 1 || SH == 2))) return 0;     // the generic kernel
  if (strip == kDwStripShort || strip == kDwStripTall) return strip;
  // tall strips re-read 2 rows in 10 instead of 2 in 4, but leave few
  // workgroups on small maps: tall only where that still fills the CUs
  const long blocks = (long(Wo) * (C / 8) + kThreads - 1) / kThreads;
  const long tall = long(N) * ((Ho + kDwStripTall - 1) / kDwStripTall) * blocks;
  return tall >= 1024 ? kDwStripTall : kDwStripShort;
}

int dwconv_forms(int N, int Ho, int Wo, int C, int KH, int KW, int SH, int SW, int* forms) {
  int n = 0;
  forms[n++] = 0;
  if (dwconv_strip(N, Ho, Wo, C, KH, KW, SH, SW) != 0) {
    forms[n++] = kDwStripShort;
    forms[n++] = kDwStripTall;
  } else if (is5x5(KH, KW, SH, SW)) {
    forms[n++] = kDwStrip5Short;
    forms[n++] = kDwStrip5Tall;
  }
  return n;
}

hipError_t dwconv_nhwc_launch(const uint16_t* x, const float* w, const float* bias, uint16_t* y, int N, int H, int W,
                              int C, int KH, int KW, int SH, int SW, int PT, int PL, int Ho, int Wo, int act,
                              int strip, hipStream_t s) {
  if (act != kActNone && act != kActRelu && act != kActRelu6 && act != kActHardSwish && act != kActSwish)
    return hipErrorInvalidValue;
  // strip 4 is a 5x5 form only; 8 on a 5x5 keeps meaning the generic kernel, as before the 5x5 strips
  const bool five = is5x5(KH, KW, SH, SW) && (strip == kDwStrip5Short || strip == kDwStrip5Tall);
  if (C <= 0 || C % 8 || KH < 1 || KW < 1 || KH > kMaxTaps || KW > kMaxTaps || SH < 1 || SW < 1 || PT < 0 || PL < 0 ||
      H <= 0 || W <= 0 || N < 0 || Ho < 0 || Wo < 0 ||
      (strip != 0 && strip != kDwStripShort && strip != kDwStripTall && !five))
    return hipErrorInvalidValue;
  if (N == 0 || Ho == 0 || Wo == 0) return hipSuccess;
  // 32-bit byte offsets; kOob must lie beyond every operand
  if (long(N) * H * W * C * 2 >= 0x7ffffff0L || long(N) * Ho * Wo * C * 2 >= 0x7ffffff0L) return hipErrorInvalidValue;
  const long blocks = (long(Wo) * (C / 8) + kThreads - 1) / kThreads;
  if (blocks > 65535) return hipErrorInvalidValue;
  const DwArgs a{x, w, bias, y, N, H, W, C, KH, KW, SH, SW, PT, PL, Ho, Wo};
  if (five) {
    const long blocks5 = (long(Wo) * (C / 4) + kThreads - 1) / kThreads;
    if (blocks5 > 65535) return hipErrorInvalidValue;
    const dim3 grid5{unsigned(long(N) * ((Ho + strip - 1) / strip)), unsigned(blocks5)};
    if (SH == 1) {
      if (strip == kDwStrip5Tall) launch5x5<1, kDwStrip5Tall>(a, act, grid5, s);
      else launch5x5<1, kDwStrip5Short>(a, act, grid5, s);
    } else {
      if (strip == kDwStrip5Tall) launch5x5<2, kDwStrip5Tall>(a, act, grid5, s);
      else launch5x5<2, kDwStrip5Short>(a, act, grid5, s);
    }
    return hipGetLastError();
  }
  const int r = dwconv_strip(N, Ho, Wo, C, KH, KW, SH, SW, strip);
  const long rows = r ? long(N) * ((Ho + r - 1) / r) : long(N) * Ho;
  const dim3 grid{unsigned(rows), unsigned(blocks)};
  if (r == 0) {
    switch (act) {
      case kActRelu: hipLaunchKernelGGL(dwconv_generic_kernel<kActRelu>, grid, dim3(kThreads), 0, s, a); break;
      case kActRelu6: hipLaunchKernelGGL(dwconv_generic_kernel<kActRelu6>, grid, dim3(kThreads), 0, s, a); break;
      case kActHardSwish:
        hipLaunchKernelGGL(dwconv_generic_kernel<kActHardSwish>, grid, dim3(kThreads), 0, s, a);
        break;
      case kActSwish: hipLaunchKernelGGL(dwconv_generic_kernel<kActSwish>, grid, dim3(kThreads), 0, s, a); break;
      default: hipLaunchKernelGGL(dwconv_generic_kernel<kActNone>, grid, dim3(kThreads), 0, s, a); break;
    }
  } else if (SH == 1) {
    if (r == kDwStripTall) launch3x3<1, kDwStripTall>(a, act, grid, s);
    else launch3x3<1, kDwStripShort>(a, act, grid, s);
  } else {
    if (r == kDwStripTall) launch3x3<2, kDwStripTall>(a, act, grid, s);
    else launch3x3<2, kDwStripShort>(a, act, grid, s);
  }
  return hipGetLastError();
}

}  // namespace tfsk
