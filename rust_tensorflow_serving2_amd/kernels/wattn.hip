// Windowed multi-head self-attention (Swin), gfx950.
//
// Input is the packed output of ONE fused QKV GEMM: qkv[R][3*H*32] (bf16,
// Q | K | V column blocks, head h at columns h*32, as attention.hip takes
// them).  A window is S <= 64 tokens that attend to each other only; the score
// of (query i, key j) of head h in window w is
//     s = (q . k) * scale + bias[h][i][j] (+ mask[w][i][j])        in fp32,
// bias the relative-position table [H][S][S], mask the shifted blocks' [nW][S][S]
// adder chosen by the window's index within its image.  The arithmetic is
// attention.hip's register kernel at the padded length 64 with D = 32:
//   scores^T = K Q^T        one v_mfma_f32_16x16x32_bf16 k-step per 16-key tile
//                           (K rows by LDS-DMA, 16-B chunks XOR-swizzled on the
//                           source address)
//   keys >= S               closed by a select to -inf after the adds and before
//                           the row maximum (S >= 1: key 0 is always open)
//   p = exp(s - max)        rounded to bf16 for the P V MFMA, the unrounded p
//                           summed in fp32; P stays in registers as the B operand
//   ctx^T = V^T P^T         V transposed through LDS (Vt[d][key])
//   one division and one rounding to bf16; whole 64-B output rows leave through
//   a wave-private LDS block.
// One 256-thread workgroup per (window, head): wave w owns queries [16w, 16w+16)
// against all 64 key slots.  A wave whose rows are all >= S still stages its
// share of K / V and meets the one barrier.
//
// Row addressing (row_of): with no grid, window bw owns rows [bw*S, (bw+1)*S)
// and its mask window is bw % nW.  With grid = (Hf, Wf, ws, shift) the rows are
// in image order, S = ws*ws, and token (i, j) of window (b, wy, wx) is row
//     b*Hf*Wf + ((wy*ws + i + shift) % Hf)*Wf + ((wx*ws + j + shift) % Wf),
// read and written in place: Roll(-shift) -> partition -> attention -> reverse
// -> Roll(+shift) without one copy.  The mask window is wy*(Wf/ws) + wx.
//
// Every global access is an unconditional buffer load / store through a
// descriptor of the operand's exact byte size: token slots >= S get kOOB as
// their whole offset and read zeros (K, V, Q, bias, mask) or are dropped (the
// output); an absent mask is a 0-record descriptor (zeros).  The tables are
// read as they are, unpadded, one dword per (query, key) -- S = 49 rows are
// 196 B, not 16-B aligned -- so there is no padding to define: a closed slot's
// bias and mask are the descriptor's zeros, and its score is REPLACED by -inf
// (a select, never a product), so no value there, Inf or NaN in a neighbouring
// window included, can reach an open key.  Every element of Ks [64][32] and
// Vt [32][0, 64) that an MFMA reads is written by this launch (zeros past S),
// so a closed key's exact-zero p meets zeros, not stale LDS.  No atomics, one
// accumulation chain per output: bit-for-bit reproducible.
#include "common.h"
#include "gemm_common.h"
#include "launch.h"

namespace tfsk {

namespace {

constexpr int D = kWattnHeadDim;          // 32
constexpr int SP = kWattnMaxSeq;          // 64 key slots
constexpr int VT_LD = SP + 8;             // Vt row stride (elements): +16 B pad

struct WattnArgs {
  int S, H, nW;                           // nW = 0: no mask
  int Hf, Wf, ws, shift;                  // ws = 0: no grid
  int nwx, wpi, inv_ws;                   // windows per image row / per image; ceil(65536 / ws)
  int qkv_bytes, out_bytes, bias_bytes, mask_bytes;
  float scale;
};

__global__ __launch_bounds__(256) void window_attention_kernel(const uint16_t* __restrict__ qkv,
                                                               const float* __restrict__ bias,
                                                               const float* __restrict__ mask,
                                                               uint16_t* __restrict__ out, const WattnArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t Ks[SP * D];        // [key][32] swizzled
  __shared__ __attribute__((aligned(16))) uint16_t Vt[D * VT_LD];     // [d][key]
  __shared__ __attribute__((aligned(16))) uint16_t Os[4 * 16 * D];    // per-wave output rows

  const int S = a.S, H = a.H;
  const int bid = blockIdx.x;
  const int h = bid % H, win = bid / H;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int row_stride = 3 * H * D, out_stride = H * D;

  // ---- the window (uniform): first row / origin in the image, mask window
  int rbase, y0 = 0, x0 = 0, w;
  if (a.ws > 0) {
    const int b = win / a.wpi, wl = win - b * a.wpi;
    const int wy = wl / a.nwx, wx = wl - wy * a.nwx;
    rbase = b * a.Hf * a.Wf;
    y0 = wy * a.ws + a.shift;
    x0 = wx * a.ws + a.shift;
    w = wl;
  } else {
    rbase = win * S;
    w = a.nW > 0 ? win % a.nW : 0;
  }
  // row of token slot t (t < 64; meaningful for t < S only).  t / ws by a
  // 16-bit reciprocal: exact for t < 64, ws <= 64.
  auto row_of = [&](int t) -> int {
    if (a.ws > 0) {
      const int i = (t * a.inv_ws) >> 16, j = t - i * a.ws;
      int y = y0 + i, x = x0 + j;
      y = y >= a.Hf ? y - a.Hf : y;
      x = x >= a.Wf ? x - a.Wf : x;
      return rbase + y * a.Wf + x;
    }
    return rbase + t;
  };

  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  const __amdgpu_buffer_rsrc_t rsQ =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(qkv), 0, a.qkv_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bias), 0, a.bias_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsM =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(mask), 0, a.mask_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(out, 0, a.out_bytes, 0x00020000);

  // ---- K rows by LDS-DMA: one wave instruction lands 1 KB (16 keys x 64 B),
  // lane l at chunk position l & 3 of key row l >> 2, fetching chunk
  // (l & 3) ^ ((key >> 1) & 3) -- the swizzled row
  {
    const int key = wid * 16 + (lane >> 2);
    const uint32_t src =
        uint32_t(row_of(key) * row_stride + H * D + h * D + (((lane & 3) ^ ((key >> 1) & 3)) * 8)) * 2u;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsQ, (lds_ptr_t)(Ks + wid * 16 * D), 16, key < S ? src : gemm::kOOB, 0,
                                             0, 0);
  }
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  // ---- Q fragment (the B operand of K Q^T: column = query fr, k = d; zeros past S)
  const int q0 = wid * 16, qi = q0 + fr;
  const bf16x8 qf = __builtin_bit_cast(
      bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                  rsQ, qi < S ? uint32_t(row_of(qi) * row_stride + h * D + fq * 8) * 2u : gemm::kOOB, 0, 0));
  // ---- V: one 16-B chunk (8 dims of one key) per thread
  const int vkey = tid >> 2, vch = tid & 3;
  const u32x4 vv = __builtin_amdgcn_raw_buffer_load_b128(
      rsQ, vkey < S ? uint32_t(row_of(vkey) * row_stride + 2 * H * D + h * D + vch * 8) * 2u : gemm::kOOB, 0, 0);
  // ---- this lane's bias and mask entries: query qi, keys nt*16 + 4fq + r
  // (the offsets pass through an empty asm: hipcc otherwise splits each
  // `live ? offset : kOOB` load into two branches with a vmcnt(0) between them)
  float bb[4][4], mm[4][4];
  uint32_t boff[4][4], moff[4][4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = nt * 16 + fq * 4 + r;
      const bool live = qi < S && key < S;
      boff[nt][r] = live ? uint32_t((h * S + qi) * S + key) * 4u : gemm::kOOB;
      moff[nt][r] = live ? uint32_t((w * S + qi) * S + key) * 4u : gemm::kOOB;
      asm volatile("" : "+v"(boff[nt][r]), "+v"(moff[nt][r]));
    }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bb[nt][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsB, boff[nt][r], 0, 0));
      mm[nt][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsM, moff[nt][r], 0, 0));
    }
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  gemm::wait_vmcnt<0>();
  // ---- V transposed into LDS: Vt[vch*8 + d][vkey]
  {
    const uint32_t vw[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int d = 0; d < 8; ++d)
      Vt[(vch * 8 + d) * VT_LD + vkey] = uint16_t((d & 1) ? (vw[d >> 1] >> 16) : (vw[d >> 1] & 0xffffu));
  }
  __syncthreads();

  // ---- S^T tiles: lane holds keys nt*16 + 4fq + r of query fr
  f32x4 s[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int key = nt * 16 + fr;
    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + key * D + ((fq ^ ((key >> 1) & 3)) * 8));
    s[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  }
  // ---- softmax over the live keys
  const int lim = S - fq * 4;                 // key nt*16 + 4fq + r is live iff nt*16 + r < lim
  float mx = -INFINITY;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = (s[nt][r] * a.scale + bb[nt][r]) + mm[nt][r];
      v = nt * 16 + r < lim ? v : -INFINITY;
      s[nt][r] = v;
      mx = fmaxf(mx, v);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  bf16x8 pb[2];                               // P^T B fragments, k-slot j -> tile 2ks + (j >> 2), r = j & 3
  constexpr float kLog2e = 1.4426950408889634f;
  const float mxl = mx * kLog2e;
  typedef __attribute__((ext_vector_type(2))) float f32x2;
  f32x2 sum2 = {0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      const f32x2 v = {s[2 * ks + (j >> 2)][j & 3], s[2 * ks + (j >> 2)][(j & 3) + 1]};
      const f32x2 e2 = v * kLog2e - mxl;      // -inf for a closed key: p = 0 exactly
      const f32x2 e = {__builtin_amdgcn_exp2f(e2.x), __builtin_amdgcn_exp2f(e2.y)};
      sum2 += e;
      pb[ks][j] = static_cast<__bf16>(e.x);
      pb[ks][j + 1] = static_cast<__bf16>(e.y);
    }
  }
  float sum = sum2.x + sum2.y;
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);

  // ---- ctx^T = V^T P^T: A = Vt rows dt*16 + fr at the same permuted keys
  f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const uint16_t* vr = Vt + (dt * 16 + fr) * VT_LD + ks * 32 + fq * 4;
      const uint2 lo = *reinterpret_cast<const uint2*>(vr);
      const uint2 hi = *reinterpret_cast<const uint2*>(vr + 16);
      const bf16x8 va = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb[ks], o[dt], 0, 0, 0);
    }
  // ---- normalise; lane holds dims dt*16 + 4fq + [0, 4) of query q0 + fr.
  // Re-laid out through this wave's 16 x 32 block (16-B chunks XOR-swizzled by
  // row) and stored as whole 64-B rows; dead rows get kOOB
  const float inv = 1.f / sum;
  uint16_t* os = Os + wid * 16 * D;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    const uint32_t lo = gemm::pack_bf16x2(o[dt][0] * inv, o[dt][1] * inv);
    const uint32_t hi = gemm::pack_bf16x2(o[dt][2] * inv, o[dt][3] * inv);
    const int chunk = dt * 2 + (fq >> 1);
    *reinterpret_cast<uint2*>(os + fr * D + ((chunk ^ (fr & 3)) * 8) + (fq & 1) * 4) = make_uint2(lo, hi);
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0): this wave's LDS writes landed
  __builtin_amdgcn_wave_barrier();
  {
    const int row = lane >> 2, ch = lane & 3;
    const u32x4 v = *reinterpret_cast<const u32x4*>(os + row * D + ((ch ^ (row & 3)) * 8));
    __builtin_amdgcn_raw_buffer_store_b128(
        v, rsO, q0 + row < S ? uint32_t(row_of(q0 + row) * out_stride + h * D + ch * 8) * 2u : gemm::kOOB, 0, 0);
  }
}

}  // namespace

bool window_attention_supported(int64_t R, int64_t S, int64_t H, int64_t Dh, int64_t nW, int64_t Hf, int64_t Wf,
                                int64_t ws, int64_t shift) {
  if (Dh != D || S < 1 || S > SP || H < 1 || R < 0 || nW < 0) return false;
  const int64_t lim = int64_t(1) << 31;
  if (R * 3 * H * D * 2 >= lim || H * S * S * 4 >= lim || nW * S * S * 4 >= lim) return false;
  int64_t windows;
  if (ws > 0) {
    if (Hf < 1 || Wf < 1 || Hf % ws || Wf % ws || ws * ws != S || shift < 0 || shift >= ws) return false;
    if (R % (Hf * Wf)) return false;
    const int64_t wpi = (Hf / ws) * (Wf / ws);
    if (nW != 0 && nW != wpi) return false;
    windows = R / (Hf * Wf) * wpi;
  } else {
    if (Hf != 0 || Wf != 0 || ws != 0 || shift != 0 || R % S) return false;
    windows = R / S;
  }
  return windows * H < lim;
}

hipError_t window_attention_launch(const uint16_t* qkv, const float* bias, const float* mask, uint16_t* out, int64_t R,
                                   int S, int H, int nW, float scale, int Hf, int Wf, int ws, int shift,
                                   hipStream_t st) {
  if (mask == nullptr) nW = 0;
  if (!window_attention_supported(R, S, H, D, nW, Hf, Wf, ws, shift)) return hipErrorInvalidValue;
  const int64_t windows = ws > 0 ? R / (int64_t(Hf) * Wf) * ((Hf / ws) * (Wf / ws)) : R / S;
  if (windows == 0) return hipSuccess;
  WattnArgs a;
  a.S = S; a.H = H; a.nW = nW;
  a.Hf = Hf; a.Wf = Wf; a.ws = ws; a.shift = shift;
  a.nwx = ws > 0 ? Wf / ws : 1;
  a.wpi = ws > 0 ? (Hf / ws) * (Wf / ws) : 1;
  a.inv_ws = ws > 0 ? (65536 + ws - 1) / ws : 0;
  a.qkv_bytes = int(R * 3 * H * D * 2);
  a.out_bytes = int(R * H * D * 2);
  a.bias_bytes = H * S * S * 4;
  a.mask_bytes = nW * S * S * 4;
  a.scale = scale;
  hipLaunchKernelGGL(window_attention_kernel, dim3(unsigned(windows * H)), dim3(256), 0, st, qkv, bias, mask, out, a);
  return hipGetLastError();
}

}  // namespace tfsk
