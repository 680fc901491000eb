// Bidirectional multi-head attention with rotary position embedding applied at
// load and an optional local window, for ModernBERT-style encoders, gfx950.
//
// Input is the packed output of ONE QKV GEMM, qkv[B][S][3 * H * D] (bf16: Q heads
// | K heads | V heads, D = 64), and one half of the rotate-half tables, cos / sin
// [S][32] (f32).  q and k are rotated by their position in fp32 and rounded to
// bf16 once, exactly as gqattn.hip does it (rope_common.h), then
//     ctx[b, i, h, :] = softmax_{j open for i}(q~_i . k~_j * scale + key_adder[b][j]) V
// where key j is open for query i iff |i - j| <= window; window < 0 (or
// window >= S - 1) opens every key.  Closed keys get -inf, weight exactly 0.
// 1 <= S <= kMaxAttentionSeq.
//
// Two builds of one kernel, LOCAL a compile-time parameter: the global build
// carries no window arithmetic at all.
//
// Work split.  One 256-thread workgroup per (batch, head, block of QB = 64
// query rows); wave w owns the 16-row MFMA tile w.  There is no
// diagonal, so every workgroup of a launch walks the same number of key blocks
// (up to the clipping at the two ends of the sequence) and no longest-first
// order is needed: blockIdx counts the query blocks of one (batch, head) first,
// so the workgroups that read the same K / V head are neighbours and share it
// in L2.
//
// Block range.  The workgroup with rows [q0, q0 + QB) walks the 64-key blocks
//     jlo = max(0, q0 - window) / 64  ...  jhi = min(nb - 1, (q0 + QB - 1 + window) / 64)
// (0 ... nb - 1 in the global build).  Per 16-row tile and block, three cases,
// all wave-uniform: the block is wholly closed for the tile (possible only in
// the local build, at the ends of the range: skipped, no MFMA), wholly open (no
// mask arithmetic), or an edge block: |i - j| <= window and key < S are
// evaluated per element.  In the global build only the ragged last block is an
// edge block.
//
// Data movement, per key block (double-buffered ring, one barrier per block),
// is gqattn.hip's: K fetched with its keys' cos / sin, rotated once per
// workgroup while it is staged and stored into rows XOR-swizzled by 16-B chunk;
// V transposed into Vt[d][key]; the key adder one f32 per key; Q rotated in
// registers from the row's own table entries; P stays in registers as the B
// fragment of ctx^T = V^T P^T on v_mfma_f32_16x16x32_bf16.  Every descriptor is
// bounded to image b's S rows, rows >= S read zeros and are never stored.
// Online softmax with the guard for a row whose keys so far are all closed:
// in the local build a tile can meet a closed stretch before its first open key.
//
// LDS 43,520 B (K 2 x 8 KiB, V^T 2 x 9 KiB, adder 512 B, output strips 8 KiB):
// three workgroups per CU by LDS.  Registers as hipcc reports them for gfx950
// (-Rpass-analysis=kernel-resource-usage; no scratch, no spills in any build;
// profiles/modernbert/resources.txt):
//     global   134 VGPRs + 16 AGPRs   3 waves per SIMD
//     local    138 VGPRs + 16 AGPRs   3 waves per SIMD
// Two variants were built, measured against this one in alternating rounds at
// H = 12 and taken out again (docs/benchmarks.md, "ModernBERT"):
//   * 128 query rows per workgroup, two tiles per wave (220 + 32 / 172 + 32
//     registers): halves the re-rotation of keys, but lost on every local shape
//     (1.08-1.46x) and at batch 1 up to S = 1024 (1.25x), and won outside the
//     run-to-run spread only at 8 x 4096 global (0.83x);
//   * for window <= 64, the whole range (<= 3 blocks, 61,184 B of LDS, two
//     workgroups per CU) staged at once behind one barrier, no ring: level at
//     1 x 512 and 1 x 1024 (1.00x, 1.01x), 1.07-1.25x slower everywhere else.

#include "common.h"
#include "gemm_common.h"
#include "launch.h"
#include "rope_common.h"

namespace tfsk {

namespace {

using rope::kLog2e;
using rope::rotate8;

constexpr int D = 64;
constexpr int KB = 64;                  // keys per block
constexpr int VT_LD = KB + 8;           // Vt row stride (elements): +16 B pad
constexpr int HALF = D / 2;             // table row length

template <bool LOCAL>
__global__ __launch_bounds__(256) void rope_attention_kernel(const uint16_t* __restrict__ qkv,
                                                             const float* __restrict__ cos_t,
                                                             const float* __restrict__ sin_t,
                                                             const float* __restrict__ key_adder,
                                                             uint16_t* __restrict__ ctx, int S, int H, int qblocks,
                                                             int window, float scale, long adder_bstride) {
  constexpr int NT = 1;                   // 16-row tiles per wave (two were measured and lost: see above)
  constexpr int QB = 64 * NT;             // query rows per workgroup
  __shared__ __attribute__((aligned(16))) uint16_t Ks[2][KB * D];      // [key][64] swizzled, rotated
  __shared__ __attribute__((aligned(16))) uint16_t Vt[2][D * VT_LD];   // [d][key]
  __shared__ __attribute__((aligned(16))) float Ms[2][KB];             // key adder
  __shared__ __attribute__((aligned(16))) uint16_t Os[4][16 * D];      // per-wave output strip

  const int bid = blockIdx.x;
  const int qb = bid % qblocks;                   // the query blocks of one (batch, head) are neighbours
  const int bh = bid / qblocks;
  const int h = bh % H, b = bh / H;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const long row_stride = long(3 * H) * D;
  const int kcol = (H + h) * D, vcol = (2 * H + h) * D;
  const __amdgpu_buffer_rsrc_t rsQ = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(qkv + long(b) * S * row_stride), 0, int(S * row_stride * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsC =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(cos_t), 0, S * HALF * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsS =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(sin_t), 0, S * HALF * 4, 0x00020000);
  const bool has_adder = key_adder != nullptr;
  const __amdgpu_buffer_rsrc_t rsM = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(has_adder ? key_adder + long(b) * adder_bstride : key_adder), 0, has_adder ? S * 4 : 0,
      0x00020000);
  // key blocks this workgroup walks: jlo .. jhi (the launcher keeps 0 <= window < S - 1 in the local build)
  const int nb = (S + KB - 1) / KB;
  const int qw0 = qb * QB;
  const int jlo = LOCAL ? max(0, qw0 - window) / KB : 0;
  const int jhi = LOCAL ? min(nb - 1, (qw0 + QB - 1 + window) / KB) : nb - 1;

  // ---- staging of key block j: issue() starts its loads into registers, land()
  // rotates K, writes buffer j & 1 behind vmcnt(0) and ends with the block's one
  // barrier.  K: key kkey, chunks kc and kc + 4, stored at chunk ch ^ (key & 7)
  // of its row.  V: keys 2 kp, 2 kp + 1, dims 8 vch ..
  const int kc = tid & 3, kkey = tid >> 2;
  const int vch = tid & 7, kp = tid >> 3;
  u32x4 kreg[2], kcos[2], ksin[2], vreg[2];
  float areg = 0.f;
  auto issue = [&](int j) {
    const int k0 = j * KB;
    {
      const int key = k0 + kkey;
      const bool live = key < S;
      const uint32_t ko = uint32_t(long(key) * row_stride + kcol + kc * 8) * 2u;
      const uint32_t to = uint32_t(key * HALF + kc * 8) * 4u;
      kreg[0] = __builtin_amdgcn_raw_buffer_load_b128(rsQ, live ? ko : gemm::kOOB, 0, 0);
      kreg[1] = __builtin_amdgcn_raw_buffer_load_b128(rsQ, live ? ko + HALF * 2u : gemm::kOOB, 0, 0);
      kcos[0] = __builtin_amdgcn_raw_buffer_load_b128(rsC, live ? to : gemm::kOOB, 0, 0);
      kcos[1] = __builtin_amdgcn_raw_buffer_load_b128(rsC, live ? to + 16u : gemm::kOOB, 0, 0);
      ksin[0] = __builtin_amdgcn_raw_buffer_load_b128(rsS, live ? to : gemm::kOOB, 0, 0);
      ksin[1] = __builtin_amdgcn_raw_buffer_load_b128(rsS, live ? to + 16u : gemm::kOOB, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = k0 + kp * 2 + i;
      vreg[i] = __builtin_amdgcn_raw_buffer_load_b128(
          rsQ, key < S ? uint32_t(long(key) * row_stride + vcol + vch * 8) * 2u : gemm::kOOB, 0, 0);
    }
    if (has_adder && wid == 0)
      areg = __uint_as_float(
          __builtin_amdgcn_raw_buffer_load_b32(rsM, k0 + lane < S ? uint32_t(k0 + lane) * 4u : gemm::kOOB, 0, 0));
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  auto land = [&](int j) {
    gemm::wait_vmcnt<0>();
    rotate8(kreg[0], kreg[1], kcos, ksin);
    uint16_t* kr = &Ks[j & 1][kkey * D];
    *reinterpret_cast<u32x4*>(kr + ((kc ^ (kkey & 7)) * 8)) = kreg[0];
    *reinterpret_cast<u32x4*>(kr + (((kc + 4) ^ (kkey & 7)) * 8)) = kreg[1];
    uint16_t* vt = &Vt[j & 1][0];
    const uint32_t a[4] = {vreg[0].x, vreg[0].y, vreg[0].z, vreg[0].w};
    const uint32_t c[4] = {vreg[1].x, vreg[1].y, vreg[1].z, vreg[1].w};
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const uint32_t lo = (d & 1) ? (a[d >> 1] >> 16) : (a[d >> 1] & 0xffffu);
      const uint32_t hi = (d & 1) ? (c[d >> 1] & 0xffff0000u) : (c[d >> 1] << 16);
      *reinterpret_cast<uint32_t*>(vt + (vch * 8 + d) * VT_LD + kp * 2) = lo | hi;
    }
    if (has_adder && wid == 0) Ms[j & 1][lane] = areg;
    __syncthreads();
  };

  issue(jlo);
  // ---- Q fragments (the B operand of K Q^T: column = query fr, k = d), rotated
  // in registers with row q0 + fr's cos / sin [8 fq, 8 fq + 8); zeros for rows past S
  int q0[NT];
  bf16x8 qf[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    q0[t] = qw0 + (wid + 4 * t) * 16;
    const int row = q0[t] + fr;
    const bool live = row < S;
    const uint32_t to = uint32_t(row * HALF + fq * 8) * 4u;
    const uint32_t qo = uint32_t(long(row) * row_stride + h * D + fq * 8) * 2u;
    u32x4 qcos[2], qsin[2];
    qcos[0] = __builtin_amdgcn_raw_buffer_load_b128(rsC, live ? to : gemm::kOOB, 0, 0);
    qcos[1] = __builtin_amdgcn_raw_buffer_load_b128(rsC, live ? to + 16u : gemm::kOOB, 0, 0);
    qsin[0] = __builtin_amdgcn_raw_buffer_load_b128(rsS, live ? to : gemm::kOOB, 0, 0);
    qsin[1] = __builtin_amdgcn_raw_buffer_load_b128(rsS, live ? to + 16u : gemm::kOOB, 0, 0);
    u32x4 lo = __builtin_amdgcn_raw_buffer_load_b128(rsQ, live ? qo : gemm::kOOB, 0, 0);
    u32x4 hi = __builtin_amdgcn_raw_buffer_load_b128(rsQ, live ? qo + HALF * 2u : gemm::kOOB, 0, 0);
    rotate8(lo, hi, qcos, qsin);
    qf[t][0] = __builtin_bit_cast(bf16x8, lo);
    qf[t][1] = __builtin_bit_cast(bf16x8, hi);
  }
  float m[NT], l[NT];
  f32x4 o[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    m[t] = -INFINITY;
    l[t] = 0.f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  land(jlo);

  for (int j = jlo; j <= jhi; ++j) {
    const int k0 = j * KB;
    if (j < jhi) issue(j + 1);
    const uint16_t* ks = &Ks[j & 1][0];
    const uint16_t* vt = &Vt[j & 1][0];
    // this lane's key adders (keys 16 nt + 4 fq + r): shared by the tiles
    f32x4 mb[KB / 16];
    if (has_adder) {
#pragma unroll
      for (int nt = 0; nt < KB / 16; ++nt) mb[nt] = *reinterpret_cast<const f32x4*>(&Ms[j & 1][nt * 16 + fq * 4]);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      // the block against this tile's rows [q0, q0 + 16): wholly closed blocks are
      // skipped, edge blocks take the mask arithmetic (all wave-uniform)
      bool edge = k0 + KB > S;
      if (LOCAL) {
        if (k0 > q0[t] + 15 + window || k0 + KB - 1 < q0[t] - window) continue;
        edge = edge || k0 + KB - 1 - q0[t] > window || q0[t] + 15 - k0 > window;
      }
      // ---- S^T tiles: lane holds keys k0 + nt*16 + 4fq + r of query q0 + fr
      f32x4 sc[KB / 16];
#pragma unroll
      for (int nt = 0; nt < KB / 16; ++nt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int key = nt * 16 + fr;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int ch = kk * 4 + fq;
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(ks + key * D + ((ch ^ (key & 7)) * 8));
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[t][kk], acc, 0, 0, 0);
        }
        sc[nt] = acc;
      }
      // ---- scale, key adder, and in an edge block the select: key k0 + 4fq + e,
      // e = nt*16 + r, is closed iff it is past S or its distance dlt + e to row
      // q0 + fr exceeds the window
      const int klim = S - k0 - fq * 4;
      const int dlt = k0 + fq * 4 - q0[t] - fr;
      float bm = -INFINITY;
#pragma unroll
      for (int nt = 0; nt < KB / 16; ++nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = sc[nt][r] * scale;
          if (has_adder) v += mb[nt][r];
          if (edge) {
            bool closed = nt * 16 + r >= klim;
            if (LOCAL) {
              const int d = dlt + nt * 16 + r;
              closed = closed || d > window || d < -window;
            }
            v = closed ? -INFINITY : v;
          }
          sc[nt][r] = v;
          bm = fmaxf(bm, v);
        }
      }
      bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
      bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
      // ms: the max the exponentials subtract.  A row whose keys so far are all
      // closed (by the window in an edge block, or by a -inf adder) has mn = -inf;
      // (-inf) - (-inf) would be NaN in alpha and in every p of the block.
      // Subtracting 0 instead gives alpha = 0 and p = exp(-inf) = 0, and the
      // first block with an open key rescales.
      const float mn = fmaxf(m[t], bm);
      const float ms = mn == -INFINITY ? 0.f : mn;
      const float alpha = __builtin_amdgcn_exp2f((m[t] - ms) * kLog2e);
      m[t] = mn;
      const float msl = ms * kLog2e;
      float bs = 0.f;
      bf16x8 pb[KB / 32];                        // P^T B fragments, k-slot i -> tile 2ks + (i >> 2), r = i & 3
#pragma unroll
      for (int ks2 = 0; ks2 < KB / 32; ++ks2) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float e = __builtin_amdgcn_exp2f(sc[2 * ks2 + (i >> 2)][i & 3] * kLog2e - msl);
          bs += e;
          pb[ks2][i] = static_cast<__bf16>(e);
        }
      }
      bs += __shfl_xor(bs, 16, 64);
      bs += __shfl_xor(bs, 32, 64);
      l[t] = l[t] * alpha + bs;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[t][dt][r] *= alpha;
      // ---- ctx^T += V^T P^T: A = Vt rows dt*16 + fr at the same permuted keys
#pragma unroll
      for (int ks2 = 0; ks2 < KB / 32; ++ks2) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const uint16_t* vr = vt + (dt * 16 + fr) * VT_LD + ks2 * 32 + fq * 4;
          const uint2 lo = *reinterpret_cast<const uint2*>(vr);
          const uint2 hi = *reinterpret_cast<const uint2*>(vr + 16);
          const bf16x8 va = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
          o[t][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb[ks2], o[t][dt], 0, 0, 0);
        }
      }
    }
    if (j < jhi) land(j + 1);
  }

  // ---- normalise; lane holds dims dt*16 + 4fq + [0, 4) of query q0 + fr.
  // Re-laid out through this wave's 16 x 64 strip (16-B chunks XOR-swizzled by
  // row) and stored as whole 128-B rows through a descriptor bounded to image
  // b's S rows; rows past S get kOOB
  const long out_stride = long(H) * D;
  const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(ctx + long(b) * S * out_stride, 0,
                                                                       int(S * out_stride * 2), 0x00020000);
  uint16_t* os = &Os[wid][0];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float inv = 1.f / l[t];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const uint32_t lo = gemm::pack_bf16x2(o[t][dt][0] * inv, o[t][dt][1] * inv);
      const uint32_t hi = gemm::pack_bf16x2(o[t][dt][2] * inv, o[t][dt][3] * inv);
      const int chunk = dt * 2 + (fq >> 1);
      *reinterpret_cast<uint2*>(os + fr * D + ((chunk ^ (fr & 7)) * 8) + (fq & 1) * 4) = make_uint2(lo, hi);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0): this wave's LDS writes landed
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = i * 64 + lane, row = c >> 3, ch = c & 7;
      const u32x4 v = *reinterpret_cast<const u32x4*>(os + row * D + ((ch ^ (row & 7)) * 8));
      __builtin_amdgcn_raw_buffer_store_b128(
          v, rsO, q0[t] + row < S ? uint32_t(long(q0[t] + row) * out_stride + h * D + ch * 8) * 2u : gemm::kOOB, 0, 0);
    }
    if (t + 1 < NT) {
      __builtin_amdgcn_s_waitcnt(0xc07f);        // the strip's reads are done before the next tile overwrites it
      __builtin_amdgcn_wave_barrier();
    }
  }
}

template <bool LOCAL>
hipError_t launch_rope(const uint16_t* qkv, const float* cos_t, const float* sin_t, const float* adder, uint16_t* ctx,
                       long BH, int S, int H, int window, float scale, long adder_bstride, hipStream_t st) {
  const int qblocks = (S + 63) / 64;
  const long grid = BH * qblocks;
  if (grid >= (1L << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rope_attention_kernel<LOCAL>, dim3(unsigned(grid)), dim3(256), 0, st, qkv, cos_t, sin_t,
                     adder, ctx, S, H, qblocks, window, scale, adder_bstride);
  return hipGetLastError();
}

}  // namespace

hipError_t rope_attention_launch(const uint16_t* qkv, const float* cos_t, const float* sin_t, const float* key_adder,
                                 uint16_t* ctx, int B, int S, int H, int Dh, int window, float scale,
                                 long adder_bstride, hipStream_t st) {
  if (!rope_attention_supported(S, Dh, H, window) || B < 0 || qkv == nullptr || ctx == nullptr || cos_t == nullptr ||
      sin_t == nullptr)
    return hipErrorInvalidValue;
  if (adder_bstride != 0 && adder_bstride != S) return hipErrorInvalidValue;
  // the descriptors count bytes in 32 bits: one image's qkv rows must fit
  const long BH = long(B) * H;
  if (long(S) * 3 * H * D * 2 >= (1L << 31) || BH >= (1L << 31)) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(ctx) | reinterpret_cast<uintptr_t>(cos_t) |
       reinterpret_cast<uintptr_t>(sin_t)) & 15)
    return hipErrorInvalidValue;
  if (BH == 0) return hipSuccess;
  const bool local = window >= 0 && window < S - 1;   // a window that reaches every key is the global form
  if (local) return launch_rope<true>(qkv, cos_t, sin_t, key_adder, ctx, BH, S, H, window, scale, adder_bstride, st);
  return launch_rope<false>(qkv, cos_t, sin_t, key_adder, ctx, BH, S, H, -1, scale, adder_bstride, st);
}

}  // namespace tfsk
