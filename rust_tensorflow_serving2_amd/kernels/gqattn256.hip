// Causal grouped-query attention with rotary position embedding applied at
// load for 256-wide heads, with an optional sliding window (Gemma-2 / Gemma-3),
// gfx950.  The operation is gqattn128.hip's with D = 256 and a window:
// qkv[B][S][(H + 2 Hkv) * 256] bf16 (Q heads | K heads | V heads), cos / sin
// [S][128] f32, rotation pairs (i, i + 128) rotated in fp32 and rounded to bf16
// once, query head h reads K / V head h / G with G = H / Hkv in {1, 2, 4, 8},
// optional QK-norm before the rotation (q_gamma / k_gamma f32 [256], eps), then
// ctx[b, i, h, :] = softmax_{j open}(q~ . k~ * scale + key_adder[b][j]) V with
// key j open for query i iff 0 <= i - j <= window (LOCAL builds) or j <= i.
// Closed keys weigh exactly 0.  1 <= S <= kMaxAttentionSeq.
//
// What is kept from gqattn128.hip: one workgroup per (batch, K/V head, block of
// QB query rows) serves all G query heads, so each key is fetched, normalised
// and rotated once per group; one 16-row tile per wave, tile w = (head w % G,
// row tile w / G); S^T = K~ Q~^T and
// ctx^T = V^T P^T on v_mfma_f32_16x16x32_bf16 with P in registers; the online
// softmax with the guard for a row whose keys so far are all closed; K / V
// double-buffered behind one barrier per block; every load and store
// unconditional through descriptors bounded to image b's S rows (kOOB for dead
// rows); no atomics and one accumulation chain per output, so reruns are
// bit-equal.
//
// What D = 256 decides anew.
//
// Key block and workgroup: KB = 32 keys and 512 threads (8 waves) in every
// build.  A 16-row tile now costs 64 fp32 accumulators and 32 Q registers
// before anything is staged.  The staging unit is still a rotation-pair chunk
// (key u >> 4, chunks kc = u & 15 and kc + 16, i.e. dims 8 kc .. and 128 + 8 kc
// ..) with that key's eight cos and eight sin values: 24 registers.  A 64-key
// block is 1024 units, four per thread at 256 threads (96 + 32 for V), twice
// gqattn128.hip's staging on top of a tile twice as large, and its 136 KiB of
// LDS is one workgroup per CU.  A 32-key block is 512 units; the scores of a
// block shrink to 8 registers and P to 4, and P V is one k-step per tile.  The
// price is a barrier every 32 keys instead of 64, with 16 + 16 MFMAs per wave
// between barriers, the count D = 128 has per 64 keys.  With 256 threads (two
// units per thread, D = 128's 48 + 16 staging registers) the G <= 4 builds came
// out at 232 VGPRs + 64 AGPRs: one wave per SIMD, so the second workgroup the
// LDS has room for could not be resident.  With 512 threads a thread stages ONE
// K unit and ONE V unit (24 + 8 registers) and every build fits the 256
// registers that two waves per SIMD leave (table below), which is what a
// 512-thread workgroup needs to launch at all; one workgroup per CU, eight
// waves.  The discarded variant's numbers are in docs/benchmarks.md, "Gemma-3".
//
// Rows per workgroup: QB = 16 * 8 / G = 128, 64, 32, 16 for G = 1, 2, 4, 8.
// QB > 32 spans several key blocks, so "a workgroup's rows lie in one key block"
// no longer holds: a workgroup walks up to the block of its LAST row, and a
// wave skips (wave-uniformly, outside the staging and its barrier) the MFMAs
// and softmax of a block that lies wholly after its tile's rows or, in LOCAL
// builds, wholly before every row's window.  A skipped block is one whose keys
// all weigh 0, so skipping changes no bit.
//
// Window (LOCAL builds).  A workgroup walks key blocks max(0, first_row -
// window) / KB .. (last_row / KB), at most window / KB + 1 + QB / KB blocks.  The causal select runs only in blocks with a key past the tile's
// first row, the low-side select only in blocks with a key before the low edge
// of the tile's last row (k0 < q0 + 15 - window).  Rows of one tile have
// different low edges: in the first block walked the tile's later rows can be
// wholly closed while its first row is not, and the softmax guard (max of
// -inf: subtract 0, alpha = 0, p = 0) carries those rows to their first open
// key.  The dispatch order stays "last query block first"; with a window every
// range has nearly the same length (only the first window / QB query blocks
// are shorter), so the order balances nothing there and costs nothing.
// window < 0 or >= S - 1 takes the LOCAL = false build, which has no window
// arithmetic in it.
//
// K swizzle.  A K row is 512 B = 32 chunks of 16 B = two passes over the 64
// LDS banks: chunk slot s lies on banks 4 (s & 15) .. + 3.  Chunk ch of key k
// is stored at slot ch ^ (k & 15): bit 4 of ch (which half of the rotation
// pair) is kept, the low four bits are permuted by the key.  Fragment reads:
// the 16 lanes of a quarter wave (one ds_read_b128 pass) hold keys 16 nt + fr,
// fr = 0 .. 15, at one chunk 4 kk + fq, so their slots' low four bits
// (ch & 15) ^ fr are the 16 distinct values: the 64 banks once.  Staging
// stores: 16 neighbouring lanes hold ONE key at chunks kc = 0 .. 15 (then kc +
// 16), a whole half row, so kc ^ (k & 15) is again a permutation of 0 .. 15:
// the 64 banks once.  D = 128's f(k) had to move bit 0 of the key to bit 3
// because there 16 lanes stored two keys' half rows; here a quarter wave stores
// one key, and the plain XOR serves both sides.
//
// V^T staging.  Vt[d][key] rows are padded by 16 B (40 elements = 20 dwords).
// P V reads row 16 dt + fr at keys 4 fq .. (8 B): 20 fr mod 64 are 16 distinct
// multiples of 4, and fq = 0, 1 fill the other pair of dwords, so a half wave's
// ds_read_b64 touches the 64 banks once.  The transposing 4-B stores at D = 128
// put neighbouring lanes on neighbouring chunks of one key pair: 8 dims apart
// is 8 * 20 dwords = 32 banks apart, so with 32 chunks per key a wave would hit
// four banks, 16 ways each.  Here unit u is (chunk (u & 3) | (u >> 6) << 2, key
// pair (u >> 2) & 15): a wave holds 16 key pairs (16 neighbouring dwords) at
// four neighbouring chunks (two bank offsets), 32 banks two ways, and a quarter
// wave still loads 64 contiguous bytes of each of its eight keys.
//
// LDS 75,008 B, dynamic (ensure_dyn_lds): K 2 x 16 KiB, V^T 2 x 20 KiB, adder
// 256 B, k_gamma 1 KiB.  The eight per-wave 16 x 256 output strips (8 KiB each,
// 64 KiB) are not added: they overlay the K buffers and the V^T buffers after
// them, all dead after the last block, behind one barrier.
//
// QK-norm (NORM builds).  K: a key's 256 dims are the registers of the 16
// lanes tid ^ 0 .. 15 in land(), so the sum of squares is 16 FMAs and four
// __shfl_xor steps (1, 2, 4, 8): no further barrier.  A thread's kc is fixed
// for the whole walk, so its k_gamma slice is 16 values, not 32.  They live in
// a 1 KiB LDS array written once, not in registers: the NORM builds are the
// ones near the 256-register line (236 against 185), 16 registers held across
// the whole walk are what they can least afford, and the four 16-B LDS reads in
// land() sit under the shuffles of the sum.  Q: a row's dims are in the four
// lanes fr + 16 fq, four chunk pairs each; all eight chunks are loaded and
// summed (across fq: 16, 32) before the tables and gammas of one pair at a time
// are loaded and rotated.  The packed chunks are made opaque between the two
// steps: otherwise the compiler keeps the sum's 64 unpacked floats for the
// rotation and the build spills.  A dead row's zeros stay zero: 0 * rsqrt(eps),
// eps > 0.
//
// Registers as hipcc reports them for gfx950 (-Rpass-analysis=kernel-resource-
// usage, -packed-fp32-ops as built); the same for every G:
//     NORM   LOCAL   VGPRs  AGPRs  scratch  LDS      waves / SIMD
//     no     no      185    0      0        75,008   2 (one 512-thread workgroup per CU)
//     no     yes     186    0      0        75,008   2
//     yes    no      236    0      0        75,008   2
//     yes    yes     234    0      0        75,008   2

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

constexpr int D = 256;
constexpr int KB = 32;                  // keys per block
constexpr int VT_LD = KB + 8;           // Vt row stride (elements): +16 B pad
constexpr int HALF = D / 2;             // table row length
constexpr int NCH = D / 8;              // 16-B chunks per row
constexpr int KS_BYTES = KB * D * 2;    // one K buffer
constexpr int VT_BYTES = D * VT_LD * 2; // one V^T buffer
constexpr int LDS_BYTES = 2 * KS_BYTES + 2 * VT_BYTES + 2 * KB * 4 + D * 4;

template <int G>
struct Split {
  static constexpr int T = 512;                  // threads, every G
  static constexpr int NW = T / 64;              // waves = 16-row tiles
  static constexpr int QB = 16 * (NW / G);       // query rows per workgroup
  static constexpr int NU = 512 / T;             // K units and V units per thread
  static_assert(T % 64 == 0 && NU * T == KB * (NCH / 2), "a block is 512 K units and 512 V units");
  static_assert(NW * 16 * D * 2 <= 2 * KS_BYTES + 2 * VT_BYTES, "the output strips fit in the dead K / V^T buffers");
};

template <int G, bool NORM, bool LOCAL>
__global__ __launch_bounds__(Split<G>::T) void rope_gqa_attention256_kernel(
    const uint16_t* __restrict__ qkv, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    const float* __restrict__ key_adder, uint16_t* __restrict__ ctx, int S, int H, int Hkv, int BK, float scale,
    int window, long adder_bstride, const float* __restrict__ q_gamma, const float* __restrict__ k_gamma, float eps) {
  constexpr int T = Split<G>::T, QB = Split<G>::QB, NU = Split<G>::NU;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* const Ks = reinterpret_cast<uint16_t*>(smem);                                  // [2][key][256] swizzled, rotated
  uint16_t* const Vt = reinterpret_cast<uint16_t*>(smem + 2 * KS_BYTES);                   // [2][d][VT_LD]
  float* const Ms = reinterpret_cast<float*>(smem + 2 * KS_BYTES + 2 * VT_BYTES);          // [2][KB] key adder
  float* const Gs = Ms + 2 * KB;                                                           // [256] k_gamma (NORM)

  const int qblocks = (S + QB - 1) / QB;
  const int bid = blockIdx.x;
  const int qb = qblocks - 1 - bid / BK;          // last query block first
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
  // key blocks this workgroup walks: from the one holding its first row's lowest open key to
  // the one holding its last row (or key S - 1)
  const int jlo = LOCAL ? max(0, qb * QB - window) / KB : 0;
  const int jhi = min(S - 1, qb * QB + QB - 1) / KB;

  // ---- staging of key block j: issue() starts its loads into registers, land()
  // rotates K, writes buffer j & 1 behind vmcnt(0) and ends with the block's one
  // barrier.  K unit i: key (tid + i T) >> 4, chunks kc and kc + 16.  V unit i:
  // u = tid + i T, keys 2 kp, 2 kp + 1 with kp = (u >> 2) & 15, dims 8 vch .. with
  // vch = (u & 3) | (u >> 6) << 2.
  const int kc = tid & 15, kp = (tid >> 2) & 15;
  u32x4 klo[NU], khi[NU], kcos[NU][2], ksin[NU][2], vreg[NU][2];
  float areg = 0.f;
  // QK-norm: k_gamma goes to the LDS array Gs once; land() reads the thread's sixteen values (dims 8 kc ..
  // and 128 + 8 kc ..) from there for every block instead of holding them in registers (file header)
  if constexpr (NORM) {
    if (tid < D / 4) *reinterpret_cast<f32x4*>(Gs + tid * 4) = *reinterpret_cast<const f32x4*>(k_gamma + tid * 4);
    __syncthreads();
  }
  auto issue = [&](int j) {
    const int k0 = j * KB;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int key = k0 + ((tid + i * T) >> 4);
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
      const int vch = (tid & 3) | (((tid + i * T) >> 6) << 2);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int key = k0 + kp * 2 + e;
        vreg[i][e] = __builtin_amdgcn_raw_buffer_load_b128(
            rsQ, key < S ? uint32_t(long(key) * row_stride + vcol + vch * 8) * 2u : gemm::kOOB, 0, 0);
      }
    }
    if (has_adder && wid == 0)
      areg = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
          rsM, lane < KB && k0 + lane < S ? uint32_t(k0 + lane) * 4u : gemm::kOOB, 0, 0));
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  auto land = [&](int j) {
    gemm::wait_vmcnt<0>();
    uint16_t* kbuf = Ks + (j & 1) * (KB * D);
    uint16_t* vt = Vt + (j & 1) * (D * VT_LD);
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int key = (tid + i * T) >> 4;
      if constexpr (NORM) {
        // the key's 256 dims lie in the sixteen lanes tid ^ 0 .. 15: its sum of squares without LDS.
        // A dead key's zeros give 0 * rsqrt(eps) = 0.
        float ss = sumsq16(klo[i], khi[i]);
        ss += __shfl_xor(ss, 1, 64);
        ss += __shfl_xor(ss, 2, 64);
        ss += __shfl_xor(ss, 4, 64);
        ss += __shfl_xor(ss, 8, 64);
        float kg[2][8];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(Gs + hf * HALF + kc * 8);
          const f32x4 c = *reinterpret_cast<const f32x4*>(Gs + hf * HALF + kc * 8 + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) kg[hf][e] = a[e], kg[hf][4 + e] = c[e];
        }
        norm_rotate8(klo[i], khi[i], kcos[i], ksin[i], __builtin_amdgcn_rsqf(ss * (1.f / D) + eps), kg[0], kg[1]);
      } else {
        rotate8(klo[i], khi[i], kcos[i], ksin[i]);
      }
      uint16_t* kr = kbuf + key * D;
      const int slot = kc ^ (key & 15);
      *reinterpret_cast<u32x4*>(kr + slot * 8) = klo[i];
      *reinterpret_cast<u32x4*>(kr + (slot + NCH / 2) * 8) = khi[i];
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int vch = (tid & 3) | (((tid + i * T) >> 6) << 2);
      const uint32_t a[4] = {vreg[i][0].x, vreg[i][0].y, vreg[i][0].z, vreg[i][0].w};
      const uint32_t c[4] = {vreg[i][1].x, vreg[i][1].y, vreg[i][1].z, vreg[i][1].w};
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const uint32_t lo = (d & 1) ? (a[d >> 1] >> 16) : (a[d >> 1] & 0xffffu);
        const uint32_t hi = (d & 1) ? (c[d >> 1] & 0xffff0000u) : (c[d >> 1] << 16);
        *reinterpret_cast<uint32_t*>(vt + (vch * 8 + d) * VT_LD + kp * 2) = lo | hi;
      }
    }
    if (has_adder && wid == 0 && lane < KB) Ms[(j & 1) * KB + lane] = areg;
    __syncthreads();
  };

  issue(jlo);
  // ---- Q fragments (the B operand of K Q^T: column = query fr, k = d): chunks
  // 4 kk + fq of row q0 + fr, the pairs (kk, kk + 4) rotated in registers with
  // that row's cos / sin [8 (4 kk + fq), + 8); zeros for rows past S
  const int q0 = qb * QB + (wid / G) * 16;
  const int hq = hk * G + wid % G;
  bf16x8 qf[8];
  {
    const int row = q0 + fr;
    const bool live = row < S;
    u32x4 lo[4], hi[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const uint32_t qo = uint32_t(long(row) * row_stride + hq * D + (4 * kk + fq) * 8) * 2u;
      lo[kk] = __builtin_amdgcn_raw_buffer_load_b128(rsQ, live ? qo : gemm::kOOB, 0, 0);
      hi[kk] = __builtin_amdgcn_raw_buffer_load_b128(rsQ, live ? qo + HALF * 2u : gemm::kOOB, 0, 0);
    }
    float r = 0.f;
    if constexpr (NORM) {
      // a row's 256 dims lie in the four lanes fr + 16 fq: the sum of squares crosses fq in two steps
      float ss = 0.f;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) ss += sumsq16(lo[kk], hi[kk]);
      ss += __shfl_xor(ss, 16, 64);
      ss += __shfl_xor(ss, 32, 64);
      r = __builtin_amdgcn_rsqf(ss * (1.f / D) + eps);
      // the packed chunks are what stays live: without this the 64 unpacked floats of the sum are kept for
      // the rotation below, next to every pair's tables and gammas, and the build spills
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) asm volatile("" : "+v"(lo[kk]), "+v"(hi[kk]));
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int ch = 4 * kk + fq;
      const uint32_t to = uint32_t(row * HALF + ch * 8) * 4u;
      u32x4 qcos[2], qsin[2];
      qcos[0] = __builtin_amdgcn_raw_buffer_load_b128(rsC, live ? to : gemm::kOOB, 0, 0);
      qcos[1] = __builtin_amdgcn_raw_buffer_load_b128(rsC, live ? to + 16u : gemm::kOOB, 0, 0);
      qsin[0] = __builtin_amdgcn_raw_buffer_load_b128(rsS, live ? to : gemm::kOOB, 0, 0);
      qsin[1] = __builtin_amdgcn_raw_buffer_load_b128(rsS, live ? to + 16u : gemm::kOOB, 0, 0);
      if constexpr (NORM) {
        float qg[2][8];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(q_gamma + hf * HALF + ch * 8);
          const f32x4 c = *reinterpret_cast<const f32x4*>(q_gamma + hf * HALF + ch * 8 + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) qg[hf][e] = a[e], qg[hf][4 + e] = c[e];
        }
        norm_rotate8(lo[kk], hi[kk], qcos, qsin, r, qg[0], qg[1]);
        // one pair's tables and gammas at a time: hoisting all four pairs' loads costs 128 registers here
        __builtin_amdgcn_sched_barrier(0);
      } else {
        rotate8(lo[kk], hi[kk], qcos, qsin);
      }
      qf[kk] = __builtin_bit_cast(bf16x8, lo[kk]);
      qf[kk + 4] = __builtin_bit_cast(bf16x8, hi[kk]);
    }
  }
  float m = -INFINITY, l = 0.f;
  f32x4 o[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  land(jlo);

  for (int j = jlo; j <= jhi; ++j) {
    const int k0 = j * KB;
    if (j < jhi) issue(j + 1);
    // a block wholly after this tile's rows, or wholly before every row's window, weighs 0: the wave
    // passes it by (q0 and k0 are wave-uniform) and only stages
    const bool pass = k0 > q0 + 15 || (LOCAL && k0 + KB - 1 < q0 - window);
    if (!pass) {
      const uint16_t* ks = Ks + (j & 1) * (KB * D);
      const uint16_t* vt = Vt + (j & 1) * (D * VT_LD);
      // ---- S^T tiles: lane holds keys k0 + nt*16 + 4fq + r of query q0 + fr
      f32x4 sc[KB / 16];
#pragma unroll
      for (int nt = 0; nt < KB / 16; ++nt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const uint16_t* kr = ks + (nt * 16 + fr) * D;      // the keys a lane reads are 16 nt + fr: slot XOR fr
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(kr + (((kk * 4 + fq) ^ fr) * 8));
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], acc, 0, 0, 0);
        }
        sc[nt] = acc;
      }
      // ---- scale, key adder (this lane's keys 16 nt + 4 fq + r) and the selects: key k0 + nt*16 + 4fq
      // + r is after the row iff nt*16 + r > lim (only in a block with a key past the tile's first row)
      // and before the row's window iff nt*16 + r < lim - window (only in a block with a key before the
      // low edge of the tile's last row)
      const bool diag = k0 + KB - 1 > q0;
      const bool low = LOCAL && k0 < q0 + 15 - window;
      const int lim = q0 + fr - k0 - fq * 4;
      const int llim = lim - window;
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
          if constexpr (LOCAL) {
            if (low) v = nt * 16 + r < llim ? -INFINITY : v;
          }
          sc[nt][r] = v;
          bm = fmaxf(bm, v);
        }
      }
      bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
      bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
      // ms: the max the exponentials subtract.  A row whose keys so far are all
      // closed (by a -inf adder, or by the window in the first block walked) has
      // mn = -inf; (-inf) - (-inf) would be NaN in alpha and in every p of the
      // block.  Subtracting 0 instead gives alpha = 0 and p = exp(-inf) = 0, and
      // the first block with an open key rescales.
      const float mn = fmaxf(m, bm);
      const float ms = mn == -INFINITY ? 0.f : mn;
      const float alpha = __builtin_amdgcn_exp2f((m - ms) * kLog2e);
      m = mn;
      const float msl = ms * kLog2e;
      float bs = 0.f;
      bf16x8 pb;                                 // P^T B fragment, k-slot i -> tile i >> 2, r = i & 3
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float e = __builtin_amdgcn_exp2f(sc[i >> 2][i & 3] * kLog2e - msl);
        bs += e;                                 // the unrounded p feeds the denominator
        pb[i] = static_cast<__bf16>(e);
      }
      bs += __shfl_xor(bs, 16, 64);
      bs += __shfl_xor(bs, 32, 64);
      l = l * alpha + bs;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
      // ---- ctx^T += V^T P^T: A = Vt rows dt*16 + fr at the same permuted keys, one k-step per tile
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
        const uint16_t* vr = vt + (dt * 16 + fr) * VT_LD + fq * 4;
        const uint2 lo = *reinterpret_cast<const uint2*>(vr);
        const uint2 hi = *reinterpret_cast<const uint2*>(vr + 16);
        const bf16x8 va = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb, o[dt], 0, 0, 0);
      }
    }
    if (j < jhi) land(j + 1);
  }

  // ---- normalise; lane holds dims dt*16 + 4fq + [0, 4) of query q0 + fr.
  // Re-laid out through this wave's 16 x 256 strip (16-B chunks XOR-swizzled by
  // row) and stored as whole 512-B rows through a descriptor bounded to image
  // b's S rows; rows past S get kOOB.  The strips overlay the K (and V^T)
  // buffers: the barrier is the point after which no wave reads a block any more.
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
  for (int i = 0; i < 16 * NCH / 64; ++i) {
    const int c = i * 64 + lane, row = c >> 5, ch = c & 31;
    const u32x4 v = *reinterpret_cast<const u32x4*>(os + row * D + ((ch ^ row) * 8));
    __builtin_amdgcn_raw_buffer_store_b128(
        v, rsO, q0 + row < S ? uint32_t(long(q0 + row) * out_stride + hq * D + ch * 8) * 2u : gemm::kOOB, 0, 0);
  }
}

template <int G, bool NORM, bool LOCAL>
hipError_t launch_gqa256(const uint16_t* qkv, const float* cos_t, const float* sin_t, const float* adder,
                         uint16_t* ctx, long BK, int S, int H, int Hkv, float scale, int window, long adder_bstride,
                         const float* q_gamma, const float* k_gamma, float eps, hipStream_t st) {
  const long grid = BK * ((S + Split<G>::QB - 1) / Split<G>::QB);
  if (grid >= (1L << 31)) return hipErrorInvalidValue;
  constexpr auto kernel = &rope_gqa_attention256_kernel<G, NORM, LOCAL>;
  hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(kernel), LDS_BYTES);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3(unsigned(grid)), dim3(Split<G>::T), LDS_BYTES, st, qkv, cos_t, sin_t, adder, ctx, S,
                     H, Hkv, int(BK), scale, window, adder_bstride, q_gamma, k_gamma, eps);
  return hipGetLastError();
}

template <int G>
hipError_t pick_gqa256(bool norm, bool local, const uint16_t* qkv, const float* cos_t, const float* sin_t,
                       const float* adder, uint16_t* ctx, long BK, int S, int H, int Hkv, float scale, int window,
                       long adder_bstride, const float* q_gamma, const float* k_gamma, float eps, hipStream_t st) {
#define TFSK_GQA256(N_, L_) \
  launch_gqa256<G, N_, L_>(qkv, cos_t, sin_t, adder, ctx, BK, S, H, Hkv, scale, window, adder_bstride, q_gamma, \
                           k_gamma, eps, st)
  if (norm) return local ? TFSK_GQA256(true, true) : TFSK_GQA256(true, false);
  return local ? TFSK_GQA256(false, true) : TFSK_GQA256(false, false);
#undef TFSK_GQA256
}

}  // namespace

hipError_t rope_gqa_attention256_launch(const uint16_t* qkv, const float* cos_t, const float* sin_t,
                                        const float* key_adder, uint16_t* ctx, int B, int S, int H, int Hkv,
                                        float scale, int window, long adder_bstride, hipStream_t st,
                                        const float* q_gamma, const float* k_gamma, float eps) {
  if (!rope_gqa_attention256_supported(S, H, Hkv) || B < 0 || qkv == nullptr || ctx == nullptr || cos_t == nullptr ||
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
  // a window that reaches key 0 from the last row closes nothing: the causal build
  const bool local = window >= 0 && window < S - 1;
  if (!norm) q_gamma = k_gamma = nullptr, eps = 0.f;
  if (!local) window = -1;
  switch (H / Hkv) {
    case 1: return pick_gqa256<1>(norm, local, qkv, cos_t, sin_t, key_adder, ctx, BK, S, H, Hkv, scale, window,
                                  adder_bstride, q_gamma, k_gamma, eps, st);
    case 2: return pick_gqa256<2>(norm, local, qkv, cos_t, sin_t, key_adder, ctx, BK, S, H, Hkv, scale, window,
                                  adder_bstride, q_gamma, k_gamma, eps, st);
    case 4: return pick_gqa256<4>(norm, local, qkv, cos_t, sin_t, key_adder, ctx, BK, S, H, Hkv, scale, window,
                                  adder_bstride, q_gamma, k_gamma, eps, st);
    default: return pick_gqa256<8>(norm, local, qkv, cos_t, sin_t, key_adder, ctx, BK, S, H, Hkv, scale, window,
                                   adder_bstride, q_gamma, k_gamma, eps, st);
  }
}

}  // namespace tfsk
