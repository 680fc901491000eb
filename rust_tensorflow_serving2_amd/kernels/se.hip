// Squeeze-and-excite (gfx950), NHWC bf16 activation, fp32 weights and gate:
//   se_gate:  gate[b][c] = gate_act(b2[c] + sum_r h[b][r] w2[r][c]),        (hard-sigmoid or sigmoid)
//             h[b][r] = act1(b1[r] + sum_c p[b][c] w1[c][r]),               (none, ReLU or swish)
//             p[b][c] = (1 / HW) sum_{h,w} x[b][h][w][c]           (fp32 throughout)
//   se_scale: y[b][h][w][c] = bf16(x[b][h][w][c] * gate[b][c])
// Two launches per block; no atomics anywhere, every sum has a fixed order, so
// the results are reproducible bit for bit.
//
// se_gate runs one 256-thread workgroup per image:
//   * pooling: a thread owns one 16-B chunk column (8 channels) and every G-th
//     pixel, G = 256 / (C / 8) pixels in flight per pass; chunks vary fastest
//     across lanes, so the live lanes of a pass read one contiguous run.  Every
//     load is unconditional: a lane past the last pixel (or past the last whole
//     pixel group) reads a clamped in-range address of the same image and is
//     masked by a select (never by a product with 0: the clamped pixel may hold
//     Inf).  Four passes are in flight at once.  The per-thread fp32 partials go
//     through LDS and are summed per channel in pixel-group order;
//   * both FCs read their input vector from LDS and their weights ([K][N], N
//     contiguous: lanes along N read contiguous floats) with fp32 FMAs.  With
//     N < 256 the K loop is split across the 256 / N lane groups (interleaved
//     k) and the partials reduced through LDS in group order -- FC1 has 8..240
//     outputs, a thread per output would idle most of the workgroup; with
//     N >= 256 a thread owns outputs j, j + 256, ...;
//   * the gate row is stored with unconditional buffer stores (a lane past C
//     gets an out-of-range offset, which the descriptor drops).
// se_scale is a full-grid, bandwidth-bound pass in the style of dwconv.hip: one
// 16-B chunk per thread, contiguous waves, unconditional loads (the dead tail
// re-reads the last chunk) and stores (the dead tail's offset is out of range).
#include "common.h"
#include "launch.h"

namespace tfsk {

namespace {

constexpr uint32_t kOob = 0x80000000u;    // beyond every descriptor below (operands are < 2 GiB)
constexpr int kThreads = 256;
constexpr int kInFlight = 4;              // pooling passes whose loads are issued together
// weight loads of an FC's K loop issued together: a thread walks up to 960 rows of w1 one 4-B load at a
// time, and with 4 in flight the loop was 240 memory round trips (168 us for 960 -> 240 -> 960)
constexpr int kFcInFlight = 16;

struct SeGateArgs {
  const uint16_t* x;
  const float* w1;
  const float* b1;
  const float* w2;
  const float* b2;
  float* gate;
  int B, HW, C, Cr, act1, gate_act;
  float inv_hw;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(const void* p, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, int(bytes), 0x00020000);
}

__device__ __forceinline__ float load_f32(const __amdgpu_buffer_rsrc_t& rs, uint32_t off) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
}

__device__ __forceinline__ void unpack8(const u32x4& v, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[2 * e] = __uint_as_float(v[e] << 16);
    f[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u);
  }
}

// out[j] = act(bias[j] + sum_k in[k] w[k][j]) for j < N, in / out / red in LDS
// (red: kThreads floats).  Ends with a barrier.
__device__ __forceinline__ void fc_lds(const float* in, const __amdgpu_buffer_rsrc_t& rsW,
                                       const __amdgpu_buffer_rsrc_t& rsB, int K, int N, float* red, float* out,
                                       int act, int tid) {
  if (N < kThreads) {
    // lane group ks takes k = ks, ks + L, ...; groups past L (256 % N lanes) are masked
    const int L = kThreads / N;
    const int j = tid % N, ks = tid / N;
    const bool live = ks < L;
    const int iters = (K + L - 1) / L;
    const float bj = load_f32(rsB, uint32_t(min(tid, N - 1)) * 4u);
    float acc = 0.f;
#pragma unroll kFcInFlight
    for (int i = 0; i < iters; ++i) {
      const int k = ks + i * L;
      const int kc = min(k, K - 1);
      const float w = load_f32(rsW, uint32_t(kc * N + j) * 4u);
      // the select is on the LDS operand, so the weight load feeds an unconditional FMA and cannot
      // sink into a branch (a masked lane adds 0 * w: the weights are a model's constants, finite)
      acc = fmaf(live && k < K ? in[kc] : 0.f, w, acc);
    }
    red[tid] = acc;                       // [ks][j]
    __syncthreads();
    if (tid < N) {
      float s = bj;
      for (int q = 0; q < L; ++q) s += red[q * N + tid];
      out[tid] = apply_act(s, act);
    }
  } else {
    for (int j0 = 0; j0 < N; j0 += kThreads) {
      const int j = j0 + tid;
      const int jc = min(j, N - 1);
      float acc = load_f32(rsB, uint32_t(jc) * 4u);
#pragma unroll kFcInFlight
      for (int k = 0; k < K; ++k) acc = fmaf(in[k], load_f32(rsW, uint32_t(k * N + jc) * 4u), acc);
      if (j < N) out[j] = apply_act(acc, act);
    }
  }
  __syncthreads();
}

// grid: x = B images.
__global__ __launch_bounds__(kThreads) void se_gate_kernel(SeGateArgs a) {
  __shared__ float s_p[2048];             // pooled vector (C <= 2048)
  __shared__ float s_part[kThreads * 8];  // pooling partials [pixel group][C]; then the FCs' [lane group][N]
  __shared__ float s_h[512];              // hidden vector (Cr <= 512)
  __shared__ float s_g[2048];             // gate row
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int C = a.C, HW = a.HW, C8 = C >> 3;

  const __amdgpu_buffer_rsrc_t rsX = rsrc_of(a.x, long(a.B) * HW * C * 2);
  const __amdgpu_buffer_rsrc_t rsW1 = rsrc_of(a.w1, long(C) * a.Cr * 4);
  const __amdgpu_buffer_rsrc_t rsB1 = rsrc_of(a.b1, long(a.Cr) * 4);
  const __amdgpu_buffer_rsrc_t rsW2 = rsrc_of(a.w2, long(a.Cr) * C * 4);
  const __amdgpu_buffer_rsrc_t rsB2 = rsrc_of(a.b2, long(C) * 4);
  const __amdgpu_buffer_rsrc_t rsG = rsrc_of(a.gate, long(a.B) * C * 4);

  // ---- pooling
  const int G = kThreads / C8;            // pixels per pass (>= 1: C8 <= 256)
  const int c8 = tid % C8, pg = tid / C8;
  const bool live = pg < G;
  const int iters = (HW + G - 1) / G;
  const uint32_t img = uint32_t(b) * uint32_t(HW) * uint32_t(C) * 2u;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i0 = 0; i0 < iters; i0 += kInFlight) {
    u32x4 v[kInFlight];
    bool ok[kInFlight];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const int px = (i0 + u) * G + pg;
      ok[u] = live && px < HW;
      v[u] = __builtin_amdgcn_raw_buffer_load_b128(rsX, img + uint32_t(min(px, HW - 1) * C8 + c8) * 16u, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      float f[8];
      unpack8(v[u], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += ok[u] ? f[e] : 0.f;
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) s_part[tid * 8 + e] = acc[e];     // [pg][c8][e]; dead lanes hold zeros past [G][C]
  __syncthreads();
  for (int c = tid; c < C; c += kThreads) {
    float s = 0.f;
    for (int q = 0; q < G; ++q) s += s_part[q * C + c];
    s_p[c] = s * a.inv_hw;
  }
  __syncthreads();

  // ---- the two FCs
  fc_lds(s_p, rsW1, rsB1, C, a.Cr, s_part, s_h, a.act1, tid);
  fc_lds(s_h, rsW2, rsB2, a.Cr, C, s_part, s_g, a.gate_act, tid);

  // ---- the gate row
  for (int c0 = 0; c0 < C; c0 += kThreads) {
    const int c = c0 + tid;
    const uint32_t off = c < C ? (uint32_t(b) * uint32_t(C) + uint32_t(c)) * 4u : kOob;
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(s_g[min(c, C - 1)]), rsG, off, 0, 0);
  }
}

struct SeScaleArgs {
  const uint16_t* x;
  const float* gate;
  uint16_t* y;
  int B, HW, C;
};

// grid: x = blocks of 256 of the B * HW * C/8 chunks.
__global__ __launch_bounds__(kThreads) void se_scale_kernel(SeScaleArgs a) {
  const int C8 = a.C >> 3;
  const uint32_t per_img = uint32_t(a.HW) * uint32_t(C8);
  const uint32_t total = uint32_t(a.B) * per_img;
  const uint32_t i = blockIdx.x * uint32_t(kThreads) + threadIdx.x;
  // a thread past the last chunk computes the last chunk again and drops its store
  const bool live = i < total;
  const uint32_t j = min(i, total - 1u);
  const uint32_t b = j / per_img;
  const uint32_t c8 = j % uint32_t(C8);

  const __amdgpu_buffer_rsrc_t rsX = rsrc_of(a.x, long(total) * 16);
  const __amdgpu_buffer_rsrc_t rsG = rsrc_of(a.gate, long(a.B) * a.C * 4);
  const __amdgpu_buffer_rsrc_t rsY = rsrc_of(a.y, long(total) * 16);

  const u32x4 xv = __builtin_amdgcn_raw_buffer_load_b128(rsX, j * 16u, 0, 0);
  const uint32_t goff = (b * uint32_t(a.C) + c8 * 8u) * 4u;
  const u32x4 g0 = __builtin_amdgcn_raw_buffer_load_b128(rsG, goff, 0, 0);
  const u32x4 g1 = __builtin_amdgcn_raw_buffer_load_b128(rsG, goff + 16u, 0, 0);
  float f[8];
  unpack8(xv, f);
  uint32_t o[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    o[e] = f32_to_bf16(f[e] * __uint_as_float(g0[e]));
    o[4 + e] = f32_to_bf16(f[4 + e] * __uint_as_float(g1[e]));
  }
  u32x4 ov;
#pragma unroll
  for (int e = 0; e < 4; ++e) ov[e] = o[2 * e] | (o[2 * e + 1] << 16);
  __builtin_amdgcn_raw_buffer_store_b128(ov, rsY, live ? j * 16u : kOob, 0, 0);
}

}  // namespace

bool se_gate_supported(long B, long HW, long C, long Cr) {
  return B >= 0 && HW >= 1 && C >= 8 && C <= kSeMaxC && C % 8 == 0 && Cr >= 1 && Cr <= kSeMaxCr &&
         B * HW * C * 2 < 0x7ffffff0L;
}

hipError_t se_gate_launch(const uint16_t* x, const float* w1, const float* b1, const float* w2, const float* b2,
                          float* gate, int B, int HW, int C, int Cr, int act1, int gate_act, hipStream_t s) {
  if (!se_gate_supported(B, HW, C, Cr)) return hipErrorInvalidValue;
  if (act1 != kActNone && act1 != kActRelu && act1 != kActSwish) return hipErrorInvalidValue;
  if (gate_act != kActHardSigmoid && gate_act != kActSigmoid) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  const SeGateArgs a{x, w1, b1, w2, b2, gate, B, HW, C, Cr, act1, gate_act, 1.f / float(HW)};
  hipLaunchKernelGGL(se_gate_kernel, dim3(unsigned(B)), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t se_scale_launch(const uint16_t* x, const float* gate, uint16_t* y, int B, int HW, int C, hipStream_t s) {
  if (B < 0 || HW < 1 || C < 8 || C % 8) return hipErrorInvalidValue;
  // 32-bit byte offsets; kOob must lie beyond every operand
  if (long(B) * HW * C * 2 >= 0x7ffffff0L) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  const long total = long(B) * HW * (C / 8);
  const SeScaleArgs a{x, gate, y, B, HW, C};
  hipLaunchKernelGGL(se_scale_kernel, dim3(unsigned((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace tfsk
