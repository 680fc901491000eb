// Bidirectional multi-head attention with a learned relative-position bias, for
// T5-style encoders (T5, Flan-T5, sentence-T5, GTR, ALiBi-style encoders), gfx950.
//
// Input is the packed output of ONE QKV GEMM, qkv[B][S][3 * H * D] (bf16: Q heads
// | K heads | V heads, D = 64), and the bias as what it is, a function of j - i
// only: table T[H][2 S - 1] (f32), entry j - i + S - 1 of head h.  Then
//     ctx[b, i, h, :] = softmax_j((q_i . k_j) * scale + T[h][j - i + S - 1] + key_adder[b][j]) V
// with key_adder an optional f32 [B | 1][S].  1 <= S <= kMaxAttentionSeq.  The
// S x S bias of a head is never formed, in HBM or in LDS: a (64 query rows, 64
// keys) pair of blocks needs the 127 consecutive table entries of its offsets.
//
// Work split (rattn.hip's).  One 256-thread workgroup per (batch, head, block of
// 64 query rows); wave w owns the 16-row MFMA tile w.  Every workgroup walks all
// nb = ceil(S / 64) key blocks, so no longest-first order is needed: blockIdx
// counts the query blocks of one (batch, head) first, and the workgroups that
// read the same K / V head and the same table row are neighbours and share them
// in L2.
//
// Data movement, per key block (two-deep ring, one barrier per block).  What
// differs from rattn.hip: nothing has to be rotated, so K never passes through
// registers.  Its rows land by buffer_load ... lds DMA, 16 B per lane, each wave
// instruction 8 keys x 128 B, with the XOR swizzle applied on the SOURCE address
// (lane l of a row fetches chunk (l & 7) ^ (key & 7)), as attention.hip stages its
// one block; here the DMA of block j + 1 runs under the MFMAs of block j.  The key
// adder (wave 2) and the bias slice (waves 0 and 1) land the same way, 4 B per
// lane.  That leaves V as the only operand held in registers across a block (2
// b128 per thread, against rattn.hip's 8 for K, its tables and V); it is
// transposed into Vt[d][key] as there.  Q is the B operand of S^T = K Q^T, loaded
// once; P stays in registers as the B fragment of ctx^T = V^T P^T on
// v_mfma_f32_16x16x32_bf16; online softmax with the guard for a row whose keys so
// far are all closed (a -inf adder); one rounding of the output, which leaves as
// whole 128-B rows through wave-private LDS strips.
//
// Bias slice.  For query rows [q0, q0 + 64) and keys [k0, k0 + 64) the offsets
// j - i span [k0 - q0 - 63, k0 - q0 + 63].  Slot x of Bs, 0 <= x < 128, holds
//     T[h][k0 - q0 + x - 64 + S]        (zero when that index is outside [0, 2 S - 2])
// so the pair (ql, kl) of in-block indices reads x = kl - ql + 63, in [0, 126]
// (slot 127 is staged and never read).  An index outside the table row can only
// belong to a pair with a key or a row >= S: the key is closed by the select, the
// row is never stored.  The loads are unconditional: such a lane gets kOOB.
//
// Bank conflicts of the bias reads, on paper.  The scores are held transposed
// (MFMA rows are keys): lane (fr, fq) of wave w holds, for query ql = 16 w + fr,
// the keys kl = 16 nt + 4 fq + r, r = 0..3, of each tile nt.  One ds_read_b32
// (fixed nt, r) therefore reads x = c + 4 fq - fr, c = 16 nt + r - 16 w + 63 wave-
// uniform: over the 64 lanes x takes the values c - 15 .. c + 12, a range of 28
// dwords.  LDS has 64 banks of 4 B, so two lanes meet in a bank only if their x
// are equal (|dx| <= 27 < 64), and equal addresses are one broadcast read.  Paired
// into ds_read2_b32 (offsets r, r + 1) the range is 29 dwords: the same argument.
// No padding is needed.  The reads are 16 dwords per lane and block, against the
// key adder's 4 b128.
//
// Closed keys.  Only the ragged last block holds keys >= S: there every score is
// selected to -inf after the adds (weight exactly 0), whatever the adder holds.
// Every global access is an unconditional buffer load or store through a
// descriptor bounded to image b's S rows, the table's H (2 S - 1) floats or image
// b's adder row; every LDS element an MFMA or the softmax reads is written by the
// same launch (K rows and V columns of keys >= S as zeros).  No atomics.
//
// LDS 44,544 B (K 2 x 8 KiB, V^T 2 x 9 KiB, key adder 512 B, bias 1 KiB, output
// strips 8 KiB): three workgroups per CU by LDS.  Registers as hipcc reports them
// for gfx950 (-Rpass-analysis=kernel-resource-usage, profiles/t5/resources.txt):
//     110 VGPRs + 16 AGPRs, 57 SGPRs, no scratch, no spills, 3 waves per SIMD
// (rattn.hip's global build: 134 + 16; K, its tables and V wait in registers
// there, only V here).  The optional variant of the design (a block pair wholly
// inside T5's saturated far bucket adds one scalar instead of reading the slice)
// was not built: it needs the bucket layout as a second contract beside the table.

#include "common.h"
#include "gemm_common.h"
#include "launch.h"

namespace tfsk {

namespace {

constexpr int D = 64;
constexpr int KB = 64;                  // keys per block
constexpr int QB = 64;                  // query rows per workgroup
constexpr int VT_LD = KB + 8;           // Vt row stride (elements): +16 B pad
constexpr int BS_N = 2 * KB;            // bias slots per block pair (127 read)
constexpr float kLog2e = 1.4426950408889634f;

typedef __attribute__((address_space(3))) void* lds_ptr_t;

__global__ __launch_bounds__(256) void bias_attention_kernel(const uint16_t* __restrict__ qkv,
                                                             const float* __restrict__ table,
                                                             const float* __restrict__ key_adder,
                                                             uint16_t* __restrict__ ctx, int S, int H, int qblocks,
                                                             float scale, long adder_bstride) {
  __shared__ __attribute__((aligned(16))) uint16_t Ks[2][KB * D];      // [key][64] swizzled
  __shared__ __attribute__((aligned(16))) uint16_t Vt[2][D * VT_LD];   // [d][key]
  __shared__ __attribute__((aligned(16))) float Ms[2][KB];             // key adder
  __shared__ __attribute__((aligned(16))) float Bs[2][BS_N];           // bias slice, slot kl - ql + 63
  __shared__ __attribute__((aligned(16))) uint16_t Os[4][16 * D];      // per-wave output strip

  const int bid = blockIdx.x;
  const int qb = bid % qblocks;                   // the query blocks of one (batch, head) are neighbours
  const int bh = bid / qblocks;
  const int h = bh % H, b = bh / H;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const long row_stride = long(3 * H) * D;
  const int kcol = (H + h) * D, vcol = (2 * H + h) * D;
  const int tlen = 2 * S - 1;                     // table row length
  const __amdgpu_buffer_rsrc_t rsQ = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(qkv + long(b) * S * row_stride), 0, int(S * row_stride * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsT =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(table), 0, int(long(H) * tlen * 4), 0x00020000);
  const bool has_adder = key_adder != nullptr;
  const __amdgpu_buffer_rsrc_t rsM = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(has_adder ? key_adder + long(b) * adder_bstride : key_adder), 0, has_adder ? S * 4 : 0,
      0x00020000);
  const int nb = (S + KB - 1) / KB;
  const int qw0 = qb * QB;

  // ---- staging of key block j into ring slot j & 1.  issue() starts the DMA of
  // K (two 1-KB pieces per wave: keys 8 pc + (lane >> 3), pc = wid and wid + 4),
  // of the bias slice (waves 0, 1) and of the key adder (wave 2), and V's loads
  // into registers (keys 2 kp, 2 kp + 1, dims 8 vch ..); land() transposes V
  // behind vmcnt(0), which also covers this wave's DMA, and ends with the
  // block's one barrier.
  const int vch = tid & 7, kp = tid >> 3;
  const int ksub = lane >> 3, kch = lane & 7;
  u32x4 vreg[2];
  auto issue = [&](int j) {
    const int k0 = j * KB, slot = j & 1;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pc = wid + i * 4, kl = pc * 8 + ksub, key = k0 + kl;
      const uint32_t src = uint32_t(long(key) * row_stride + kcol + ((kch ^ (kl & 7)) * 8)) * 2u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsQ, (lds_ptr_t)(&Ks[slot][pc * 512]), 16, key < S ? src : gemm::kOOB, 0,
                                               0, 0);
    }
    if (wid < 2) {
      const int idx = k0 - qw0 + wid * 64 + lane - KB + S;          // T[h][idx] -> slot wid * 64 + lane
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsT, (lds_ptr_t)(&Bs[slot][wid * 64]), 4,
                                               idx >= 0 && idx < tlen ? uint32_t(h * tlen + idx) * 4u : gemm::kOOB, 0,
                                               0, 0);
    } else if (wid == 2 && has_adder) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsM, (lds_ptr_t)(&Ms[slot][0]), 4,
                                               k0 + lane < S ? uint32_t(k0 + lane) * 4u : gemm::kOOB, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = k0 + kp * 2 + i;
      vreg[i] = __builtin_amdgcn_raw_buffer_load_b128(
          rsQ, key < S ? uint32_t(long(key) * row_stride + vcol + vch * 8) * 2u : gemm::kOOB, 0, 0);
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  auto land = [&](int j) {
    gemm::wait_vmcnt<0>();
    uint16_t* vt = &Vt[j & 1][0];
    const uint32_t a[4] = {vreg[0].x, vreg[0].y, vreg[0].z, vreg[0].w};
    const uint32_t c[4] = {vreg[1].x, vreg[1].y, vreg[1].z, vreg[1].w};
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const uint32_t lo = (d & 1) ? (a[d >> 1] >> 16) : (a[d >> 1] & 0xffffu);
      const uint32_t hi = (d & 1) ? (c[d >> 1] & 0xffff0000u) : (c[d >> 1] << 16);
      *reinterpret_cast<uint32_t*>(vt + (vch * 8 + d) * VT_LD + kp * 2) = lo | hi;
    }
    asm volatile("" ::: "memory");
    __syncthreads();
  };

  issue(0);
  // ---- Q fragments (the B operand of K Q^T: column = query fr, k = d); zeros for rows past S
  const int q0 = qw0 + wid * 16;
  bf16x8 qf[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
    qf[kk] = __builtin_bit_cast(
        bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                    rsQ, q0 + fr < S ? uint32_t(long(q0 + fr) * row_stride + h * D + kk * 32 + fq * 8) * 2u : gemm::kOOB,
                    0, 0));
  float m = -INFINITY, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // this lane's first bias slot: x = kl - ql + 63 with kl = 16 nt + 4 fq + r, ql = 16 wid + fr
  const int bx = 63 + fq * 4 - wid * 16 - fr;
  land(0);

  for (int j = 0; j < nb; ++j) {
    const int k0 = j * KB;
    if (j + 1 < nb) issue(j + 1);
    const uint16_t* ks = &Ks[j & 1][0];
    const uint16_t* vt = &Vt[j & 1][0];
    const float* bs = &Bs[j & 1][bx];
    const bool edge = k0 + KB > S;                 // the ragged last block: wave-uniform
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
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], acc, 0, 0, 0);
      }
      sc[nt] = acc;
    }
    // ---- t = score * scale + bias, then + key adder, then in the edge block the select
    const int klim = S - k0 - fq * 4;              // key 16 nt + r of this lane is live iff 16 nt + r < klim
    float bm = -INFINITY;
#pragma unroll
    for (int nt = 0; nt < KB / 16; ++nt) {
      f32x4 mb = {0.f, 0.f, 0.f, 0.f};
      if (has_adder) mb = *reinterpret_cast<const f32x4*>(&Ms[j & 1][nt * 16 + fq * 4]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = sc[nt][r] * scale + bs[nt * 16 + r];
        if (has_adder) v += mb[r];
        if (edge) v = nt * 16 + r >= klim ? -INFINITY : v;
        sc[nt][r] = v;
        bm = fmaxf(bm, v);
      }
    }
    bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
    bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
    // ms: the max the exponentials subtract.  A row whose keys so far are all
    // closed by a -inf adder has mn = -inf; (-inf) - (-inf) would be NaN in alpha
    // and in every p of the block.  Subtracting 0 instead gives alpha = 0 and
    // p = exp(-inf) = 0, and the first block with an open key rescales.
    const float mn = fmaxf(m, bm);
    const float ms = mn == -INFINITY ? 0.f : mn;
    const float alpha = __builtin_amdgcn_exp2f((m - ms) * kLog2e);
    m = mn;
    const float msl = ms * kLog2e;
    float bsum = 0.f;
    bf16x8 pb[KB / 32];                          // P^T B fragments, k-slot i -> tile 2ks + (i >> 2), r = i & 3
#pragma unroll
    for (int ks2 = 0; ks2 < KB / 32; ++ks2) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float e = __builtin_amdgcn_exp2f(sc[2 * ks2 + (i >> 2)][i & 3] * kLog2e - msl);
        bsum += e;
        pb[ks2][i] = static_cast<__bf16>(e);
      }
    }
    bsum += __shfl_xor(bsum, 16, 64);
    bsum += __shfl_xor(bsum, 32, 64);
    l = l * alpha + bsum;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
    // ---- ctx^T += V^T P^T: A = Vt rows dt*16 + fr at the same permuted keys
#pragma unroll
    for (int ks2 = 0; ks2 < KB / 32; ++ks2) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const uint16_t* vr = vt + (dt * 16 + fr) * VT_LD + ks2 * 32 + fq * 4;
        const uint2 lo = *reinterpret_cast<const uint2*>(vr);
        const uint2 hi = *reinterpret_cast<const uint2*>(vr + 16);
        const bf16x8 va = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb[ks2], o[dt], 0, 0, 0);
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
  const float inv = 1.f / l;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const uint32_t lo = gemm::pack_bf16x2(o[dt][0] * inv, o[dt][1] * inv);
    const uint32_t hi = gemm::pack_bf16x2(o[dt][2] * inv, o[dt][3] * inv);
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
        v, rsO, q0 + row < S ? uint32_t(long(q0 + row) * out_stride + h * D + ch * 8) * 2u : gemm::kOOB, 0, 0);
  }
}

}  // namespace

hipError_t bias_attention_launch(const uint16_t* qkv, const float* table, const float* key_adder, uint16_t* ctx, int B,
                                 int S, int H, int Dh, float scale, long adder_bstride, hipStream_t st) {
  if (!bias_attention_supported(S, Dh, H) || B < 0 || qkv == nullptr || ctx == nullptr || table == nullptr)
    return hipErrorInvalidValue;
  if (adder_bstride != 0 && adder_bstride != S) return hipErrorInvalidValue;
  // the descriptors count bytes in 32 bits: one image's qkv rows and the table must fit
  const long BH = long(B) * H;
  if (long(S) * 3 * H * D * 2 >= (1L << 31) || long(H) * (2 * S - 1) * 4 >= (1L << 31) || BH >= (1L << 31))
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(ctx)) & 15) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(key_adder)) & 3) return hipErrorInvalidValue;
  if (BH == 0) return hipSuccess;
  const int qblocks = (S + QB - 1) / QB;
  const long grid = BH * qblocks;
  if (grid >= (1L << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bias_attention_kernel, dim3(unsigned(grid)), dim3(256), 0, st, qkv, table, key_adder, ctx, S, H,
                     qblocks, scale, adder_bstride);
  return hipGetLastError();
}

}  // namespace tfsk
