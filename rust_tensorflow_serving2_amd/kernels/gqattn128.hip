// Causal grouped-query attention with rotary position embedding applied at
// load for 128-wide heads (Llama-2 / 3, Mistral, Qwen), gfx950.  The semantics
// are gqattn.hip's with D = 128: qkv[B][S][(H + 2 Hkv) * 128] bf16 (Q heads |
// K heads | V heads), cos / sin [S][64] f32 (one half of the rotate-half
// tables), rotation pairs (i, i + 64) rotated in fp32 and rounded to bf16 once,
// query head h reads K / V head h / G with G = H / Hkv in {1, 2, 4, 8}, then
// ctx[b, q, h, :] = softmax_{key <= q}(q~ . k~ * scale + key_adder[b][key]) V.
// 1 <= S <= kMaxAttentionSeq.
//
// What is kept from gqattn.hip: one workgroup per (batch, K/V head, block of QB
// query rows) serves all G query heads, so a 64-key K block and V block is
// fetched, rotated and written to LDS once per group; QB divides 64, so a
// workgroup's rows lie in one key block and only the blocks up to its diagonal
// are walked, longest ranges first; S^T = K~ Q~^T and ctx^T = V^T P^T on
// v_mfma_f32_16x16x32_bf16 with P in registers; online softmax with the guard
// for a row whose keys so far are all closed; mask arithmetic only in the block
// that straddles the diagonal; every load and store unconditional through
// descriptors bounded to image b's S rows (kOOB for dead rows); no atomics and
// one accumulation chain per output, so reruns are bit-equal.
//
// What D = 128 decides anew.
//
// Work split: ONE 16-row tile per wave in every build.  A tile costs 32
// accumulators, 16 Q registers, 16 scores and 8 for P, twice gqattn.hip's, so
// the G = 8 build does not take two tiles per wave as it does at D = 64: it
// takes a 512-thread workgroup (8 waves, wave w = head w of the group, the
// same 16 rows), which also halves what a thread stages.  Tile w of a
// workgroup is (head w % G, row tile w / G):
//     G = 8   512 threads  QB = 16     G = 2   256 threads  QB = 32
//     G = 4   256 threads  QB = 16     G = 1   256 threads  QB = 64 (cattn.hip's split)
//
// Staging, per key block (double-buffered, one barrier per block).  A K block
// is 64 keys x 16 chunks of 16 B.  The unit of K staging is a rotation-pair
// chunk (key p >> 3, chunks c = p & 7 and c + 8, i.e. dims 8c .. 8c + 7 and
// 64 + 8c ..: both halves of eight pairs) with that key's eight cos and eight
// sin values; thread tid takes units tid + i T, 512 / T of them (2 at 256
// threads, 1 at 512).  Eight neighbouring threads read one key's 128
// contiguous bytes twice.  The loads of block j + 1 are issued at the top of
// block j; at the bottom the thread rotates in fp32, rounds once and stores.
// Each key is rotated once per workgroup.  V: unit u = (chunk u & 15, key pair
// u >> 4), two 16-B loads, transposed into Vt[d][key] (rows padded by 16 B) as
// eight 4-B stores, as in cattn.hip.  Q is rotated in registers: a lane's four
// B fragments are chunks fq, 4 + fq, 8 + fq, 12 + fq of row q0 + fr, i.e. the
// pairs (fq, 8 + fq) and (4 + fq, 12 + fq), with that row's table values.
//
// K swizzle.  A K row is 256 B = 16 chunks = all 64 LDS banks, so unswizzled
// every key's chunk c sits on the same four banks.  Chunk ch of key k is
// stored at slot ch ^ f(k), f(k) = ((k & 1) << 3) | ((k >> 1) & 7), a
// bijection of k & 15.  Fragment reads: the 16 lanes of a quarter wave (one
// ds_read_b128 pass: 16 x 16 B = the 64 banks) hold keys 16 nt + fr, fr = 0 ..
// 15, at one chunk 4 kk + fq, so their slots ch ^ f(fr) are the 16 distinct
// ones: conflict-free.  Staging stores: 16 neighbouring lanes hold keys 2 m and
// 2 m + 1 at chunks c = 0 .. 7 (then c + 8): f(2 m) and f(2 m + 1) differ in
// bit 3 only, so key 2 m fills the eight slots of one half row and key 2 m + 1
// the eight of the other: the 64 banks once, conflict-free.  (XOR by k & 15
// itself would serve the reads but put both keys' chunks in the same half.)
//
// LDS 70,144 B, dynamic (above 64 KiB: ensure_dyn_lds): K 2 x 16 KiB, V^T 2 x
// 18 KiB, adder 512 B.  The per-wave 16 x 128 output strips (4 KiB each, 16 or
// 32 KiB) are NOT added: they overlay the K buffers, which are dead after the
// last block, behind one barrier.  Two workgroups of 256 threads per CU
// (140,288 of 163,840 B); with the strips on top it would be one.  The G = 8
// build's one 512-thread workgroup per CU is the same two waves per SIMD.
//
// Registers as hipcc reports them for gfx950 (-Rpass-analysis=kernel-resource-
// usage, -packed-fp32-ops as built; no scratch in any build):
//     G    threads  VGPRs  AGPRs  scratch  LDS      waves / SIMD
//     1    256      188    32     0        70,144   2 by registers; 2 workgroups per CU
//     2    256      188    32     0        70,144   2 by registers; 2 workgroups per CU
//     4    256      188    32     0        70,144   2 by registers; 2 workgroups per CU
//     8    512      150    0      0        70,144   3 by registers; 1 workgroup per CU
//
// QK-norm (NORM builds; Qwen3, OLMo-2, Gemma-3): each head's q row and k row is
// RMS-normalised over its 128 dims, x^ = x * rsqrt(mean(x^2) + eps) * gamma with
// q_gamma / k_gamma f32 [128], before it is rotated; x^ stays in fp32 and the
// rotation's rounding to bf16 is the only one (rope::norm_rotate8).  It rides on
// the staging above and reads qkv no second time.  K: a key's 128 dims are the
// registers of the eight lanes tid ^ 0 .. 7 in land(), so the sum of squares is
// 16 FMAs and three __shfl_xor steps (1, 2, 4): no LDS, no further barrier, once
// per key and workgroup.  Q: a row's dims are in the four lanes fr + 16 fq; both
// chunk pairs are loaded before either is rotated and the sum crosses fq (16,
// 32).  A dead row's zeros stay zero: 0 * rsqrt(eps), eps > 0.  k_gamma: a
// thread's kc is fixed, so its 16 values are read once and kept in registers.
// The other choice, a 512-B LDS array, was not needed: the register builds
// below have no scratch and keep two waves per SIMD, and LDS reads would sit
// between land()'s wait and its barrier, the one place all waves wait on.
//     G    threads  VGPRs  AGPRs  scratch  LDS      waves / SIMD          (NORM)
//     1    256      214    32     0        70,144   2 by registers; 2 workgroups per CU
//     2    256      214    32     0        70,144   2 by registers; 2 workgroups per CU
//     4    256      214    32     0        70,144   2 by registers; 2 workgroups per CU
//     8    512      206    0      0        70,144   2 by registers; 1 workgroup per CU
// The NORM = false builds are instruction for instruction what they were before
// the parameter existed (scripts/isa_audit.py --resources, the code digest).
// Measured against what the op ran before (torch, fp32) and against torch RoPE
// + scaled_dot_product_attention: docs/benchmarks.md, "Llama", D = 128.

#include "common.h"
#include "gemm_common.h"
#include "launch.h"
#include "rope_common.h"

namespace tfsk {

namespace {

using rope::kLog2e;
using rope::norm_rotate8;
using rope::rotate8;
using rope::sumsq16;

constexpr int D = 128;
constexpr int KB = 64;                  // keys per block
constexpr int VT_LD = KB + 8;           // Vt row stride (elements): +16 B pad
constexpr int HALF = D / 2;             // table row length
constexpr int KS_BYTES = KB * D * 2;    // one K buffer
constexpr int VT_BYTES = D * VT_LD * 2; // one V^T buffer
constexpr int LDS_BYTES = 2 * KS_BYTES + 2 * VT_BYTES + 2 * KB * 4;

// the slot XOR of key k's row: a bijection of k & 15 whose bit 3 is k's bit 0
__device__ __forceinline__ int kswz(int key) { return ((key & 1) << 3) | ((key >> 1) & 7); }

template <int G>
struct Split {
  static constexpr int T = G == 8 ? 512 : 256;   // threads
  static constexpr int NW = T / 64;              // waves = 16-row tiles
  static constexpr int QB = 16 * (NW / G);       // query rows per workgroup
  static constexpr int NU = 512 / T;             // K units and V units per thread
  static_assert(KB % QB == 0, "a workgroup's rows lie in one key block");
  static_assert(NW * 16 * D * 2 <= 2 * KS_BYTES, "the output strips fit in the K buffers");
};

template <int G, bool NORM>
__global__ __launch_bounds__(Split<G>::T) void rope_gqa_attention128_kernel(
    const uint16_t* __restrict__ qkv, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    const float* __restrict__ key_adder, uint16_t* __restrict__ ctx, int S, int H, int Hkv, int BK, float scale,
    long adder_bstride, const float* __restrict__ q_gamma, const float* __restrict__ k_gamma, float eps) {
  constexpr int T = Split<G>::T, QB = Split<G>::QB, NU = Split<G>::NU;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* const Ks = reinterpret_cast<uint16_t*>(smem);                                  // [2][key][128] swizzled, rotated
  uint16_t* const Vt = reinterpret_cast<uint16_t*>(smem + 2 * KS_BYTES);                   // [2][d][VT_LD]
  float* const Ms = reinterpret_cast<float*>(smem + 2 * KS_BYTES + 2 * VT_BYTES);          // [2][KB] key adder

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
  // barrier.  K unit i: key (tid + i T) >> 3, chunks kc and kc + 8.  V unit i:
  // keys 2 kp, 2 kp + 1 with kp = (tid + i T) >> 4, dims 8 vch ..
  const int kc = tid & 7, vch = tid & 15;
  u32x4 klo[NU], khi[NU], kcos[NU][2], ksin[NU][2], vreg[NU][2];
  float areg = 0.f;
  // QK-norm: the thread's kc never changes, so its sixteen k_gamma values (dims 8 kc .. and 64 + 8 kc ..)
  // are read once and stay in registers for the whole walk
  float kg[NORM ? 2 : 1][8];
  if constexpr (NORM) {
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(k_gamma + hf * HALF + kc * 8);
      const f32x4 c = *reinterpret_cast<const f32x4*>(k_gamma + hf * HALF + kc * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) kg[hf][e] = a[e], kg[hf][4 + e] = c[e];
    }
  }
  auto issue = [&](int j) {
    const int k0 = j * KB;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int key = k0 + ((tid + i * T) >> 3);
      const bool live = key < S;
      const uint32_t ko = uint32_t(long(key) * row_stride + kcol + kc * 8) * 2u;
      const uint32_t to = uint32_t(key * HALF + kc * 8) * 4u;
      klo[i] = __builtin_amdgcn_raw_buffer_load_b128(rsQ, live ? ko : gemm::kOOB, 0, 0);
      khi[i] = __builtin_amdgcn_raw_buffer_load_b128(rsQ, live ? ko + HALF * 2u : gemm::kOOB, 0, 0);
      kcos[i][0] = __builtin_amdgcn_raw_buffer_load_b128(rsC, live ? to : gemm::kOOB, 0, 0);
      kcos[i][1] = __builtin_amdgcn_raw_buffer_load_b128(rsC, live ? to + 16u : gemm::kOOB, 0, 0);
      ksin[i][0] = __builtin_amdgcn_raw_buffer_load_b128(rsS, live ? to : gemm::kOOB, 0, 0);
      ksin[i][1] = __builtin_amdgcn_raw_buffer_load_b128(rsS, live ? to + 16u : gemm::kOOB, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int kp = (tid + i * T) >> 4;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int key = k0 + kp * 2 + e;
        vreg[i][e] = __builtin_amdgcn_raw_buffer_load_b128(
            rsQ, key < S ? uint32_t(long(key) * row_stride + vcol + vch * 8) * 2u : gemm::kOOB, 0, 0);
      }
    }
    if (has_adder && wid == 0)
      areg = __uint_as_float(
          __builtin_amdgcn_raw_buffer_load_b32(rsM, k0 + lane < S ? uint32_t(k0 + lane) * 4u : gemm::kOOB, 0, 0));
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  auto land = [&](int j) {
    gemm::wait_vmcnt<0>();
    uint16_t* kbuf = Ks + (j & 1) * (KB * D);
    uint16_t* vt = Vt + (j & 1) * (D * VT_LD);
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int key = (tid + i * T) >> 3;
      if constexpr (NORM) {
        // the key's 128 dims lie in the eight lanes tid ^ 0 .. 7: its sum of squares without LDS.
        // A dead key's zeros give 0 * rsqrt(eps) = 0.
        float ss = sumsq16(klo[i], khi[i]);
        ss += __shfl_xor(ss, 1, 64);
        ss += __shfl_xor(ss, 2, 64);
        ss += __shfl_xor(ss, 4, 64);
        norm_rotate8(klo[i], khi[i], kcos[i], ksin[i], __builtin_amdgcn_rsqf(ss * (1.f / D) + eps), kg[0], kg[1]);
      } else {
        rotate8(klo[i], khi[i], kcos[i], ksin[i]);
      }
      uint16_t* kr = kbuf + key * D;
      *reinterpret_cast<u32x4*>(kr + ((kc ^ kswz(key)) * 8)) = klo[i];
      *reinterpret_cast<u32x4*>(kr + (((kc + 8) ^ kswz(key)) * 8)) = khi[i];
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int kp = (tid + i * T) >> 4;
      const uint32_t a[4] = {vreg[i][0].x, vreg[i][0].y, vreg[i][0].z, vreg[i][0].w};
      const uint32_t c[4] = {vreg[i][1].x, vreg[i][1].y, vreg[i][1].z, vreg[i][1].w};
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const uint32_t lo = (d & 1) ? (a[d >> 1] >> 16) : (a[d >> 1] & 0xffffu);
        const uint32_t hi = (d & 1) ? (c[d >> 1] & 0xffff0000u) : (c[d >> 1] << 16);
        *reinterpret_cast<uint32_t*>(vt + (vch * 8 + d) * VT_LD + kp * 2) = lo | hi;
      }
    }
    if (has_adder && wid == 0) Ms[(j & 1) * KB + lane] = areg;
    __syncthreads();
  };

  issue(0);
  // ---- Q fragments (the B operand of K Q^T: column = query fr, k = d): chunks
  // 4 kk + fq of row q0 + fr, the pairs (kk, kk + 2) rotated in registers with
  // that row's cos / sin [8 (4 kk + fq), + 8); zeros for rows past S
  const int q0 = qb * QB + (wid / G) * 16;
  const int hq = hk * G + wid % G;
  bf16x8 qf[4];
  if constexpr (NORM) {
    // a row's 128 dims lie in the four lanes fr + 16 fq: both chunk pairs are loaded before either is
    // rotated, and the sum of squares crosses fq in two steps
    const int row = q0 + fr;
    const bool live = row < S;
    u32x4 lo[2], hi[2], qcos[2][2], qsin[2][2];
    float qg[2][2][8];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int ch = 4 * kk + fq;
      const uint32_t to = uint32_t(row * HALF + ch * 8) * 4u;
      const uint32_t qo = uint32_t(long(row) * row_stride + hq * D + ch * 8) * 2u;
      qcos[kk][0] = __builtin_amdgcn_raw_buffer_load_b128(rsC, live ? to : gemm::kOOB, 0, 0);
      qcos[kk][1] = __builtin_amdgcn_raw_buffer_load_b128(rsC, live ? to + 16u : gemm::kOOB, 0, 0);
      qsin[kk][0] = __builtin_amdgcn_raw_buffer_load_b128(rsS, live ? to : gemm::kOOB, 0, 0);
      qsin[kk][1] = __builtin_amdgcn_raw_buffer_load_b128(rsS, live ? to + 16u : gemm::kOOB, 0, 0);
      lo[kk] = __builtin_amdgcn_raw_buffer_load_b128(rsQ, live ? qo : gemm::kOOB, 0, 0);
      hi[kk] = __builtin_amdgcn_raw_buffer_load_b128(rsQ, live ? qo + HALF * 2u : gemm::kOOB, 0, 0);
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(q_gamma + hf * HALF + ch * 8);
        const f32x4 c = *reinterpret_cast<const f32x4*>(q_gamma + hf * HALF + ch * 8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) qg[kk][hf][e] = a[e], qg[kk][hf][4 + e] = c[e];
      }
    }
    float ss = sumsq16(lo[0], hi[0]) + sumsq16(lo[1], hi[1]);
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    const float r = __builtin_amdgcn_rsqf(ss * (1.f / D) + eps);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      norm_rotate8(lo[kk], hi[kk], qcos[kk], qsin[kk], r, qg[kk][0], qg[kk][1]);
      qf[kk] = __builtin_bit_cast(bf16x8, lo[kk]);
      qf[kk + 2] = __builtin_bit_cast(bf16x8, hi[kk]);
    }
  } else {
    const int row = q0 + fr;
    const bool live = row < S;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int ch = 4 * kk + fq;
      const uint32_t to = uint32_t(row * HALF + ch * 8) * 4u;
      const uint32_t qo = uint32_t(long(row) * row_stride + hq * D + ch * 8) * 2u;
      u32x4 qcos[2], qsin[2];
      qcos[0] = __builtin_amdgcn_raw_buffer_load_b128(rsC, live ? to : gemm::kOOB, 0, 0);
      qcos[1] = __builtin_amdgcn_raw_buffer_load_b128(rsC, live ? to + 16u : gemm::kOOB, 0, 0);
      qsin[0] = __builtin_amdgcn_raw_buffer_load_b128(rsS, live ? to : gemm::kOOB, 0, 0);
      qsin[1] = __builtin_amdgcn_raw_buffer_load_b128(rsS, live ? to + 16u : gemm::kOOB, 0, 0);
      u32x4 lo = __builtin_amdgcn_raw_buffer_load_b128(rsQ, live ? qo : gemm::kOOB, 0, 0);
      u32x4 hi = __builtin_amdgcn_raw_buffer_load_b128(rsQ, live ? qo + HALF * 2u : gemm::kOOB, 0, 0);
      rotate8(lo, hi, qcos, qsin);
      qf[kk] = __builtin_bit_cast(bf16x8, lo);
      qf[kk + 2] = __builtin_bit_cast(bf16x8, hi);
    }
  }
  float m = -INFINITY, l = 0.f;
  f32x4 o[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int fsw = kswz(fr);                        // the keys a lane reads are 16 nt + fr
  land(0);

  for (int j = 0; j < nb; ++j) {
    const int k0 = j * KB;
    if (j + 1 < nb) issue(j + 1);
    const uint16_t* ks = Ks + (j & 1) * (KB * D);
    const uint16_t* vt = Vt + (j & 1) * (D * VT_LD);
    // ---- S^T tiles: lane holds keys k0 + nt*16 + 4fq + r of query q0 + fr
    f32x4 sc[KB / 16];
#pragma unroll
    for (int nt = 0; nt < KB / 16; ++nt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const uint16_t* kr = ks + (nt * 16 + fr) * D;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(kr + (((kk * 4 + fq) ^ fsw) * 8));
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], acc, 0, 0, 0);
      }
      sc[nt] = acc;
    }
    // ---- scale, key adder (this lane's keys 16 nt + 4 fq + r), and in the block
    // that straddles the diagonal the causal select: key k0 + nt*16 + 4fq + r is
    // closed iff nt*16 + r > lim
    const bool diag = k0 + KB - 1 > q0;
    const int lim = q0 + fr - k0 - fq * 4;
    float bm = -INFINITY;
#pragma unroll
    for (int nt = 0; nt < KB / 16; ++nt) {
      f32x4 mb = {0.f, 0.f, 0.f, 0.f};
      if (has_adder) mb = *reinterpret_cast<const f32x4*>(&Ms[(j & 1) * KB + nt * 16 + fq * 4]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = sc[nt][r] * scale;
        if (has_adder) v += mb[r];
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
    const float mn = fmaxf(m, bm);
    const float ms = mn == -INFINITY ? 0.f : mn;
    const float alpha = __builtin_amdgcn_exp2f((m - ms) * kLog2e);
    m = mn;
    const float msl = ms * kLog2e;
    float bs = 0.f;
    bf16x8 pb[KB / 32];                        // P^T B fragments, k-slot i -> tile 2ks + (i >> 2), r = i & 3
#pragma unroll
    for (int ks2 = 0; ks2 < KB / 32; ++ks2) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float e = __builtin_amdgcn_exp2f(sc[2 * ks2 + (i >> 2)][i & 3] * kLog2e - msl);
        bs += e;                               // the unrounded p feeds the denominator
        pb[ks2][i] = static_cast<__bf16>(e);
      }
    }
    bs += __shfl_xor(bs, 16, 64);
    bs += __shfl_xor(bs, 32, 64);
    l = l * alpha + bs;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
    // ---- ctx^T += V^T P^T: A = Vt rows dt*16 + fr at the same permuted keys
#pragma unroll
    for (int ks2 = 0; ks2 < KB / 32; ++ks2) {
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
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
  // Re-laid out through this wave's 16 x 128 strip (16-B chunks XOR-swizzled by
  // row) and stored as whole 256-B rows through a descriptor bounded to image
  // b's S rows; rows past S get kOOB.  The strips overlay the K buffers: the
  // barrier is the point after which no wave reads a K block any more.
  __syncthreads();
  const long out_stride = long(H) * D;
  const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(ctx + long(b) * S * out_stride, 0,
                                                                       int(S * out_stride * 2), 0x00020000);
  uint16_t* os = Ks + wid * (16 * D);
  const float inv = 1.f / l;
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    const uint32_t lo = gemm::pack_bf16x2(o[dt][0] * inv, o[dt][1] * inv);
    const uint32_t hi = gemm::pack_bf16x2(o[dt][2] * inv, o[dt][3] * inv);
    const int chunk = dt * 2 + (fq >> 1);
    *reinterpret_cast<uint2*>(os + fr * D + ((chunk ^ fr) * 8) + (fq & 1) * 4) = make_uint2(lo, hi);
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0): this wave's LDS writes landed
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = i * 64 + lane, row = c >> 4, ch = c & 15;
    const u32x4 v = *reinterpret_cast<const u32x4*>(os + row * D + ((ch ^ row) * 8));
    __builtin_amdgcn_raw_buffer_store_b128(
        v, rsO, q0 + row < S ? uint32_t(long(q0 + row) * out_stride + hq * D + ch * 8) * 2u : gemm::kOOB, 0, 0);
  }
}

template <int G, bool NORM>
hipError_t launch_gqa128(const uint16_t* qkv, const float* cos_t, const float* sin_t, const float* adder,
                         uint16_t* ctx, long BK, int S, int H, int Hkv, float scale, long adder_bstride,
                         const float* q_gamma, const float* k_gamma, float eps, hipStream_t st) {
  const long grid = BK * ((S + Split<G>::QB - 1) / Split<G>::QB);
  if (grid >= (1L << 31)) return hipErrorInvalidValue;
  constexpr auto kernel = &rope_gqa_attention128_kernel<G, NORM>;
  hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(kernel), LDS_BYTES);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(unsigned(grid)), dim3(Split<G>::T), LDS_BYTES, st, qkv, cos_t, sin_t, adder, ctx, S,
                     H, Hkv, int(BK), scale, adder_bstride, q_gamma, k_gamma, eps);
  return hipGetLastError();
}

}  // namespace

hipError_t rope_gqa_attention128_launch(const uint16_t* qkv, const float* cos_t, const float* sin_t,
                                        const float* key_adder, uint16_t* ctx, int B, int S, int H, int Hkv,
                                        float scale, long adder_bstride, hipStream_t st, const float* q_gamma,
                                        const float* k_gamma, float eps) {
  if (!rope_gqa_attention_supported(S, D, H, Hkv) || B < 0 || qkv == nullptr || ctx == nullptr || cos_t == nullptr ||
      sin_t == nullptr)
    return hipErrorInvalidValue;
  if (adder_bstride != 0 && adder_bstride != S) return hipErrorInvalidValue;
  // the descriptors count bytes in 32 bits: one image's qkv rows must fit
  const long BK = long(B) * Hkv;
  if (long(S) * (H + 2 * Hkv) * D * 2 >= (1L << 31) || BK >= (1L << 31)) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(ctx) | reinterpret_cast<uintptr_t>(cos_t) |
       reinterpret_cast<uintptr_t>(sin_t)) & 15)
    return hipErrorInvalidValue;
  // QK-norm: both gammas or neither, 16-B aligned (the kernel reads them as float4), eps > 0
  const bool norm = q_gamma != nullptr || k_gamma != nullptr;
  if (norm && (q_gamma == nullptr || k_gamma == nullptr || !(eps > 0.f) ||
               ((reinterpret_cast<uintptr_t>(q_gamma) | reinterpret_cast<uintptr_t>(k_gamma)) & 15)))
    return hipErrorInvalidValue;
  if (BK == 0) return hipSuccess;
#define TFSK_GQA128(G_)                                                                                        \
  return norm ? launch_gqa128<G_, true>(qkv, cos_t, sin_t, key_adder, ctx, BK, S, H, Hkv, scale, adder_bstride, \
                                        q_gamma, k_gamma, eps, st)                                             \
              : launch_gqa128<G_, false>(qkv, cos_t, sin_t, key_adder, ctx, BK, S, H, Hkv, scale, adder_bstride, \
                                         nullptr, nullptr, 0.f, st)
  switch (H / Hkv) {
    case 1: TFSK_GQA128(1);
    case 2: TFSK_GQA128(2);
    case 4: TFSK_GQA128(4);
    default: TFSK_GQA128(8);
  }
#undef TFSK_GQA128
}

}  // namespace tfsk
