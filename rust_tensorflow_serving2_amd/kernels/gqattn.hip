// Causal grouped-query attention with rotary position embedding applied at
// load, for Llama-style decoders, gfx950.
//
// Input is the packed output of ONE QKV GEMM, qkv[B][S][(H + 2 Hkv) * D] (bf16:
// H query heads | Hkv key heads | Hkv value heads, D = 64), and one half of the
// rotate-half tables, cos / sin [S][32] (f32).  G = H / Hkv in {1, 2, 4, 8};
// query head h reads K / V head h / G.  For x in {q, k} at position p, with
// x1 = x[:32], x2 = x[32:]:
//     x~1 = x1 cos[p] - x2 sin[p],   x~2 = x2 cos[p] + x1 sin[p]
// in fp32, rounded to bf16 once (what the graph's Mul / AddV2 would have handed
// the MFMA), then ctx[b, q, h, :] = softmax_{key <= q}(q~ . k~ * scale +
// key_adder[b][key]) V with V as the GEMM left it.  1 <= S <= kMaxAttentionSeq.
//
// Work split.  One 256-thread workgroup per (batch, K/V head, block of QB query
// rows) serves ALL G query heads of that K/V head, so each 64-key K block and V
// block is fetched, rotated and written to LDS once for the whole group instead
// of once per query head.  The workgroup's 16-row MFMA tiles are numbered
// idx = wave + 4 t (t < NT tiles per wave) and tile idx is (head idx % G of the
// group, row tile idx / G):
//     G = 8   NT = 2  QB = 16   wave w: heads w and w + 4, the same 16 rows
//     G = 4   NT = 1  QB = 16   wave w: head w, the same 16 rows
//     G = 2   NT = 1  QB = 32   wave w: head w & 1, rows 16 (w >> 1)
//     G = 1   NT = 1  QB = 64   wave w: rows 16 w            (cattn.hip's split)
// The heads of a group go across the waves first because they share the causal
// range by construction: for G >= 4 every tile of the workgroup has the same
// rows, hence the same diagonal block and the same MFMA count, and a staged
// block feeds 4 * NT tiles (64 or 128 query rows' worth of MFMAs, as in
// cattn.hip) although only 16 positions are in flight.  QB divides 64, so a
// workgroup's rows lie in ONE key block and no tile ever sees a block that is
// wholly above it.  Two tiles per wave only for G = 8 (it is what covers the
// group; 2 x 16 accumulators); G <= 2 takes more row tiles rather than a
// second tile per wave, which keeps the registers of the G = 4 build.
// blockIdx counts the query blocks from the LAST one down, all (batch, K/V
// head) pairs of one query block next to each other: longest key range first.
//
// Data movement, per key block j (double-buffered, one barrier per block):
//   K    thread tid holds 16-B chunks c = tid & 3 and c + 4 of key tid >> 2,
//        i.e. dims 8c .. 8c + 7 and 32 + 8c .. 32 + 8c + 7: both halves of
//        eight rotation pairs, with that key's eight cos and eight sin values
//        (four 16-B table loads; the tables stay in L2).  Issued at the top of
//        block j for block j + 1; at the bottom of block j the thread rotates
//        its pairs in fp32, rounds once and stores the two chunks into rows
//        XOR-swizzled by 16-B chunk.  Each key is rotated once per workgroup.
//   V    two 16-B rows-of-8-dims per thread, transposed into Vt[d][key] (rows
//        padded by 16 B) as eight 4-B stores, as in cattn.hip
//   key adder   one f32 per key (wave 0), only when given
//   vmcnt(0) + the LDS stores + ONE barrier end the block; the barrier also
//   retires buffer j & 1 for every wave, which block j + 1 refills.
//   Q    a lane's two B fragments hold dims 8 fq .. and 32 + 8 fq .. of row
//        q0 + fr: it loads that row's cos / sin [8 fq, 8 fq + 8) and rotates in
//        registers; nothing crosses lanes.  The tiles of a wave share the row.
//   Keys and query rows >= S are never read: every descriptor is bounded to
//   image b's S rows (the tables' to S rows) and such rows get kOOB (zeros).
//   Rows >= S are never stored.
//
// Math.  cattn.hip's: S^T = K~ Q~^T on v_mfma_f32_16x16x32_bf16, P in registers
// as the B fragment of ctx^T = V^T P^T, online softmax with the guard for a row
// whose keys so far are all closed by a -inf adder, mask arithmetic only in the
// block that straddles the diagonal (the last one a workgroup walks).
//
// LDS 43,520 B (K 2 x 8 KiB, V^T 2 x 9 KiB, adder 512 B, output strips 8 KiB):
// three workgroups per CU by LDS.  Registers as hipcc reports them for gfx950
// (-Rpass-analysis=kernel-resource-usage; no scratch, no spills in any build):
//     G = 1, 2, 4   136 VGPRs + 16 AGPRs   3 waves per SIMD
//     G = 8         220 VGPRs + 32 AGPRs   2 waves per SIMD
// (cattn.hip: 120 at one tile per wave, 150 at two; the 16 staged cos / sin
// values per thread live across a block's MFMAs).  Measured against the
// composition torch RoPE + torch K / V repeat + causal_attention and against
// that attention launch alone: docs/benchmarks.md, "Llama".

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

template <int G>
__global__ __launch_bounds__(256) void rope_gqa_attention_kernel(const uint16_t* __restrict__ qkv,
                                                                 const float* __restrict__ cos_t,
                                                                 const float* __restrict__ sin_t,
                                                                 const float* __restrict__ key_adder,
                                                                 uint16_t* __restrict__ ctx, int S, int H, int Hkv,
                                                                 int BK, float scale, long adder_bstride) {
  constexpr int NT = G == 8 ? 2 : 1;      // tiles per wave
  constexpr int QB = 16 * (4 * NT / G);   // query rows per workgroup
  static_assert(KB % QB == 0, "a workgroup's rows lie in one key block");
  __shared__ __attribute__((aligned(16))) uint16_t Ks[2][KB * D];      // [key][64] swizzled, rotated
  __shared__ __attribute__((aligned(16))) uint16_t Vt[2][D * VT_LD];   // [d][key]
  __shared__ __attribute__((aligned(16))) float Ms[2][KB];             // key adder
  __shared__ __attribute__((aligned(16))) uint16_t Os[4][16 * D];      // per-wave output strip

  const int qblocks = (S + QB - 1) / QB;
  const int bid = blockIdx.x;
  const int qb = qblocks - 1 - bid / BK;          // longest key range first
  const int bk = bid % BK;
  const int hk = bk % Hkv, b = bk / Hkv;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const long row_stride = long(H + 2 * Hkv) * D;
  const int kcol = (H + hk) * D, vcol = (H + Hkv + hk) * D;
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
  // key blocks this workgroup walks: up to the one holding its rows (or key S - 1)
  const int nb = min((S + KB - 1) / KB, (qb * QB) / KB + 1);

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

  issue(0);
  // ---- Q fragments (the B operand of K Q^T: column = query fr, k = d), rotated
  // in registers with row q0 + fr's cos / sin [8 fq, 8 fq + 8); zeros for rows past S
  int q0[NT], hq[NT];
  bf16x8 qf[NT][2];
  {
    const int rt = wid / G;                        // (wid + 4 t) / G is the same for every t: NT = 2 only for G = 8
    const int row = qb * QB + rt * 16 + fr;
    const bool live = row < S;
    const uint32_t to = uint32_t(row * HALF + fq * 8) * 4u;
    u32x4 qcos[2], qsin[2];
    qcos[0] = __builtin_amdgcn_raw_buffer_load_b128(rsC, live ? to : gemm::kOOB, 0, 0);
    qcos[1] = __builtin_amdgcn_raw_buffer_load_b128(rsC, live ? to + 16u : gemm::kOOB, 0, 0);
    qsin[0] = __builtin_amdgcn_raw_buffer_load_b128(rsS, live ? to : gemm::kOOB, 0, 0);
    qsin[1] = __builtin_amdgcn_raw_buffer_load_b128(rsS, live ? to + 16u : gemm::kOOB, 0, 0);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      q0[t] = qb * QB + rt * 16;
      hq[t] = hk * G + (wid + 4 * t) % G;
      const uint32_t qo = uint32_t(long(row) * row_stride + hq[t] * D + fq * 8) * 2u;
      u32x4 lo = __builtin_amdgcn_raw_buffer_load_b128(rsQ, live ? qo : gemm::kOOB, 0, 0);
      u32x4 hi = __builtin_amdgcn_raw_buffer_load_b128(rsQ, live ? qo + HALF * 2u : gemm::kOOB, 0, 0);
      rotate8(lo, hi, qcos, qsin);
      qf[t][0] = __builtin_bit_cast(bf16x8, lo);
      qf[t][1] = __builtin_bit_cast(bf16x8, hi);
    }
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
  land(0);

  for (int j = 0; j < nb; ++j) {
    const int k0 = j * KB;
    if (j + 1 < nb) issue(j + 1);
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
      // ---- scale, key adder, and in the block that straddles the diagonal the
      // causal select: key k0 + nt*16 + 4fq + r is closed iff nt*16 + r > lim
      const bool diag = k0 + KB - 1 > q0[t];
      const int lim = q0[t] + fr - k0 - fq * 4;
      float bm = -INFINITY;
#pragma unroll
      for (int nt = 0; nt < KB / 16; ++nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = sc[nt][r] * scale;
          if (has_adder) v += mb[nt][r];
          if (diag) v = nt * 16 + r > lim ? -INFINITY : v;
          sc[nt][r] = v;
          bm = fmaxf(bm, v);
        }
      }
      bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
      bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
      // ms: the max the exponentials subtract.  A row whose keys so far are all
      // closed by a -inf adder has mn = -inf; (-inf) - (-inf) would be NaN in
      // alpha and in every p of the block.  Subtracting 0 instead gives alpha =
      // 0 and p = exp(-inf) = 0, and the first block with an open key rescales.
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
    if (j + 1 < nb) land(j + 1);
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
          v, rsO, q0[t] + row < S ? uint32_t(long(q0[t] + row) * out_stride + hq[t] * D + ch * 8) * 2u : gemm::kOOB, 0,
          0);
    }
    if (t + 1 < NT) {
      __builtin_amdgcn_s_waitcnt(0xc07f);        // the strip's reads are done before the next tile overwrites it
      __builtin_amdgcn_wave_barrier();
    }
  }
}

template <int G>
hipError_t launch_gqa(const uint16_t* qkv, const float* cos_t, const float* sin_t, const float* adder, uint16_t* ctx,
                      long BK, int S, int H, int Hkv, float scale, long adder_bstride, hipStream_t st) {
  constexpr int QB = 16 * (4 * (G == 8 ? 2 : 1) / G);
  const long grid = BK * ((S + QB - 1) / QB);
  if (grid >= (1L << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rope_gqa_attention_kernel<G>, dim3(unsigned(grid)), dim3(256), 0, st, qkv, cos_t, sin_t, adder,
                     ctx, S, H, Hkv, int(BK), scale, adder_bstride);
  return hipGetLastError();
}

}  // namespace

hipError_t rope_gqa_attention_launch(const uint16_t* qkv, const float* cos_t, const float* sin_t,
                                     const float* key_adder, uint16_t* ctx, int B, int S, int H, int Hkv, int Dh,
                                     float scale, long adder_bstride, hipStream_t st, const float* q_gamma,
                                     const float* k_gamma, float eps) {
  if (Dh == 128)                                 // 128-wide heads: gqattn128.hip
    return rope_gqa_attention128_launch(qkv, cos_t, sin_t, key_adder, ctx, B, S, H, Hkv, scale, adder_bstride, st,
                                        q_gamma, k_gamma, eps);
  if (q_gamma != nullptr || k_gamma != nullptr) return hipErrorInvalidValue;   // QK-norm: D = 128 only
  if (Dh != D || !rope_gqa_attention_supported(S, Dh, H, Hkv) || B < 0 || qkv == nullptr || ctx == nullptr ||
      cos_t == nullptr || sin_t == nullptr)
    return hipErrorInvalidValue;
  if (adder_bstride != 0 && adder_bstride != S) return hipErrorInvalidValue;
  // the descriptors count bytes in 32 bits: one image's qkv rows must fit
  const long BK = long(B) * Hkv;
  if (long(S) * (H + 2 * Hkv) * D * 2 >= (1L << 31) || BK >= (1L << 31)) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(ctx) | reinterpret_cast<uintptr_t>(cos_t) |
       reinterpret_cast<uintptr_t>(sin_t)) & 15)
    return hipErrorInvalidValue;
  if (BK == 0) return hipSuccess;
  switch (H / Hkv) {
    case 1: return launch_gqa<1>(qkv, cos_t, sin_t, key_adder, ctx, BK, S, H, Hkv, scale, adder_bstride, st);
    case 2: return launch_gqa<2>(qkv, cos_t, sin_t, key_adder, ctx, BK, S, H, Hkv, scale, adder_bstride, st);
    case 4: return launch_gqa<4>(qkv, cos_t, sin_t, key_adder, ctx, BK, S, H, Hkv, scale, adder_bstride, st);
    default: return launch_gqa<8>(qkv, cos_t, sin_t, key_adder, ctx, BK, S, H, Hkv, scale, adder_bstride, st);
  }
}

}  // namespace tfsk
