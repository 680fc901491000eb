// Causal multi-head self-attention for decoder models (GPT-2), gfx950.
//
// Input is the packed output of ONE QKV GEMM, qkv[B][S][3*H*D] (bf16, Q | K | V
// column blocks, head h at columns h*D), D = 64, any 1 <= S <= kMaxAttentionSeq.
// ctx[b, q, h, :] = softmax_{key <= q}(Q K^T * scale + key_adder[b][key]) V: the
// mask is index arithmetic, never memory, and the key blocks above the diagonal
// are never loaded or multiplied.
//
// Work split.  One 256-thread workgroup per (batch, head, block of QB = 64 * TQ
// query rows), TQ in {1, 2}.  Wave w owns the 16-row tiles at rows
// 64 t + 16 w of the block (t < TQ): with TQ = 2 every wave has one tile in
// the upper and one in the lower half, so the four waves do the same number of
// MFMAs although the diagonal cuts the block.  The workgroup walks the 64-key
// blocks 0 .. (last row of the block) / 64 and stops there; a tile skips the
// one block that lies wholly above its rows (TQ = 2: the upper tiles skip the
// last block).  blockIdx counts the query blocks from the LAST one down, all
// (batch, head) pairs of one query block next to each other: the workgroups
// with the longest key range are dispatched first and the one-block workgroups
// fill the tail of the grid.
//
// Data movement, per key block j (double-buffered, one barrier per block):
//   K    two 16-B chunks per thread into registers, issued at the top of block
//        j for block j + 1 and stored at the bottom of block j into rows
//        XOR-swizzled by 16-B chunk as in attention.hip (conflict-free b128
//        fragment reads)
//   V    two 16-B rows-of-8-dims per thread the same way, transposed into
//        Vt[d][key] (rows padded by 16 B) as eight 4-B stores
//   key adder   one f32 per key (wave 0), only when given
//   The loads of block j + 1 are in flight during the MFMAs and the softmax of
//   block j; vmcnt(0) + the LDS stores + ONE barrier end the block.  The barrier
//   also retires buffer j & 1 for every wave, which block j + 1 refills.
//   (Register-staged, not buffer_load ... lds: with the direct-to-LDS form the
//   compiler cannot tell the DMA's target buffer from the one being read and
//   puts a vmcnt wait for block j + 1's K in front of block j's first LDS read
//   -- seen in the gfx950 ISA -- which serialises the fetch with the MFMAs.)
//   Keys and query rows >= S are never read: the descriptors span image b's S
//   rows and such rows get kOOB (zeros).  Rows >= S are never stored.
//
// Math.  Scores transposed, S^T = K Q^T on v_mfma_f32_16x16x32_bf16 (keys on
// the MFMA rows, queries on the columns): a lane holds, for ONE query (column
// lane & 15), keys 16 nt + 4 (lane >> 4) + r of the block.  Row max / sum are
// two xor shuffles, the running max m and sum l are one scalar per tile and
// lane, and after exp the lane holds exactly a B fragment of ctx^T = V^T P^T
// (k slots permuted; the A side reads V^T rows with the same permutation), so
// P never goes through LDS.  Online softmax as in attention_flash_kernel: O
// and l rescaled by exp(m_old - m_new) per block, with its guard for a row
// whose keys so far are all -inf (only a -inf key adder can make one: key 0 is
// causally open to every query).  Mask arithmetic (key > query -> -inf, from
// lane indices) runs only in a block that straddles the tile's diagonal; the
// block holding keys >= S always does for a tile with a live row, so those
// keys need no test of their own.
//
// Query block height.  QB = 128 reads each K / V block once per 128 rows
// instead of per 64; QB = 64 gives twice the workgroups and three workgroups
// per CU instead of two (120 vs 150 VGPRs).  Measured on an MI355X with
// scripts/cattn_bench.py (H = 12, us, qb 64 / qb 128): B = 1: S 128 7.8 / 9.1,
// 512 15.6 / 22.2, 2048 50.2 / 75.0; B = 32: S 128 11.3 / 13.1, 256 20.4 /
// 23.0, 512 49.9 / 53.3, 1024 156.8 / 157.6, 2048 571.3 / 565.8 (spread of
// the repeated medians 0.2 - 2.7 %).  64 wins or ties everywhere, so the
// launcher takes 64 and 128 runs only when asked for (qb = 128).

#include "common.h"
#include "gemm_common.h"
#include "launch.h"

namespace tfsk {

namespace {

constexpr int D = 64;
constexpr int KB = 64;                  // keys per block
constexpr int VT_LD = KB + 8;           // Vt row stride (elements): +16 B pad
constexpr float kLog2e = 1.4426950408889634f;

template <int TQ>
__global__ __launch_bounds__(256) void causal_attention_kernel(const uint16_t* __restrict__ qkv,
                                                               const float* __restrict__ key_adder,
                                                               uint16_t* __restrict__ ctx, int S, int H, int BH,
                                                               float scale, long adder_bstride) {
  constexpr int QB = 64 * TQ;
  __shared__ __attribute__((aligned(16))) uint16_t Ks[2][KB * D];      // [key][64] swizzled
  __shared__ __attribute__((aligned(16))) uint16_t Vt[2][D * VT_LD];   // [d][key]
  __shared__ __attribute__((aligned(16))) float Ms[2][KB];             // key adder
  __shared__ __attribute__((aligned(16))) uint16_t Os[4][16 * D];      // per-wave output strip

  const int qblocks = (S + QB - 1) / QB;
  const int bid = blockIdx.x;
  const int qb = qblocks - 1 - bid / BH;          // longest key range first
  const int bh = bid % BH;
  const int h = bh % H, b = bh / H;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const long row_stride = 3L * H * D;
  const __amdgpu_buffer_rsrc_t rsQ = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(qkv + long(b) * S * row_stride), 0, int(S * row_stride * 2), 0x00020000);
  const bool has_adder = key_adder != nullptr;
  const __amdgpu_buffer_rsrc_t rsM = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(has_adder ? key_adder + long(b) * adder_bstride : key_adder), 0, has_adder ? S * 4 : 0,
      0x00020000);
  // key blocks this workgroup walks: up to the one holding its last row (or key S - 1)
  const int nb = min((S + KB - 1) / KB, (qb * QB + QB - 1) / KB + 1);

  // ---- staging of key block j: issue() starts its loads into registers, land()
  // writes them into buffer j & 1 behind vmcnt(0) and ends with the block's one
  // barrier.  K: 16-B chunk c = tid + 256 i of the block's 64 x 8 chunks, stored
  // at chunk (c & 7) ^ (key & 7) of its row.  V: keys 2 kp, 2 kp + 1, dims 8 vch ..
  const int vch = tid & 7, kp = tid >> 3;
  u32x4 kreg[2], vreg[2];
  float areg = 0.f;
  auto issue = [&](int j) {
    const int k0 = j * KB;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = k0 + i * 32 + kp;
      kreg[i] = __builtin_amdgcn_raw_buffer_load_b128(
          rsQ, key < S ? uint32_t(long(key) * row_stride + H * D + h * D + vch * 8) * 2u : gemm::kOOB, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = k0 + kp * 2 + i;
      vreg[i] = __builtin_amdgcn_raw_buffer_load_b128(
          rsQ, key < S ? uint32_t(long(key) * row_stride + 2 * H * D + h * D + vch * 8) * 2u : gemm::kOOB, 0, 0);
    }
    if (has_adder && wid == 0)
      areg = __uint_as_float(
          __builtin_amdgcn_raw_buffer_load_b32(rsM, k0 + lane < S ? uint32_t(k0 + lane) * 4u : gemm::kOOB, 0, 0));
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  auto land = [&](int j) {
    gemm::wait_vmcnt<0>();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = i * 32 + kp;
      *reinterpret_cast<u32x4*>(&Ks[j & 1][key * D + ((vch ^ (key & 7)) * 8)]) = kreg[i];
    }
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
  // ---- Q fragments (the B operand of K Q^T: column = query fr, k = d); zeros for rows past S
  int q0[TQ];
  bf16x8 qf[TQ][2];
#pragma unroll
  for (int t = 0; t < TQ; ++t) {
    q0[t] = qb * QB + t * 64 + wid * 16;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
      qf[t][kk] = __builtin_bit_cast(
          bf16x8,
          __builtin_amdgcn_raw_buffer_load_b128(
              rsQ, q0[t] + fr < S ? uint32_t(long(q0[t] + fr) * row_stride + h * D + kk * 32 + fq * 8) * 2u : gemm::kOOB,
              0, 0));
  }
  float m[TQ], l[TQ];
  f32x4 o[TQ][4];
#pragma unroll
  for (int t = 0; t < TQ; ++t) {
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
    for (int t = 0; t < TQ; ++t) {
      if (k0 > q0[t] + 15) continue;             // the block lies above every row of the tile (wave-uniform)
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
      // ---- scale, key adder, and in a block that straddles the diagonal the
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
  for (int t = 0; t < TQ; ++t) {
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
    if (t + 1 < TQ) {
      __builtin_amdgcn_s_waitcnt(0xc07f);        // the strip's reads are done before the next tile overwrites it
      __builtin_amdgcn_wave_barrier();
    }
  }
}

template <int TQ>
hipError_t launch_causal(const uint16_t* qkv, const float* adder, uint16_t* ctx, long BH, int S, int H, float scale,
                         long adder_bstride, hipStream_t st) {
  constexpr int QB = 64 * TQ;
  const long grid = BH * ((S + QB - 1) / QB);
  if (grid >= (1L << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(causal_attention_kernel<TQ>, dim3(unsigned(grid)), dim3(256), 0, st, qkv, adder, ctx, S, H,
                     int(BH), scale, adder_bstride);
  return hipGetLastError();
}

}  // namespace

hipError_t causal_attention_launch(const uint16_t* qkv, const float* key_adder, uint16_t* ctx, int B, int S, int H,
                                   int Dh, float scale, long adder_bstride, hipStream_t st, int qb) {
  if (!causal_attention_supported(S, Dh) || B < 0 || H < 1 || qkv == nullptr || ctx == nullptr)
    return hipErrorInvalidValue;
  if (qb != 0 && qb != 64 && qb != 128) return hipErrorInvalidValue;
  if (adder_bstride != 0 && adder_bstride != S) return hipErrorInvalidValue;
  // the descriptors count bytes in 32 bits: one image's qkv rows must fit
  const long BH = long(B) * H;
  if (long(S) * 3 * H * D * 2 >= (1L << 31) || BH >= (1L << 31)) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(ctx)) & 15) return hipErrorInvalidValue;
  if (BH == 0) return hipSuccess;
  return qb == 128 ? launch_causal<2>(qkv, key_adder, ctx, BH, S, H, scale, adder_bstride, st)
                                : launch_causal<1>(qkv, key_adder, ctx, BH, S, H, scale, adder_bstride, st);
}

}  // namespace tfsk
