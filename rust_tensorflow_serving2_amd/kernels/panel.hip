// Row-panel 1x1 conv (a plain GEMM on NHWC rows) for the wide expand convs:
//
//   out[M][N] = act(A[M][K] W[N][ldw]^T + bias (+ residual[M][N]))     bf16 in / out, fp32 accumulate
//
// With one workgroup per (64-row, 64-column) tile (cgemm<64,64,...>) every
// N-tile of a row block loads the same [64][K] A tile again: N / 64 reads of A
// and a prologue + exposed epilogue per K loop of 2-8 steps.  Here a workgroup
// owns BM rows x one span of N / nsplit columns and walks the span's 64-column
// n-tiles itself:
//
//   * A: each of the 4 waves owns BM / 4 rows and holds their MFMA fragments in
//     registers for the whole walk (16-B buffer loads straight into the
//     v_mfma_f32_16x16x32_bf16 operand layout: K / 8 VGPRs at BM = 64, K / 4 at
//     BM = 128).  A is read once per span.
//   * W: one LDS-DMA ring of S = 4 slots of [64 columns][64 k] (8 KB, 16-B
//     chunks XOR-swizzled by row & 7 as in chain.hip).  The ring runs over
//     (n-tile, k-tile) as ONE sequence: it does not drain at an n-tile boundary.
//   * the bias and residual chunks of n-tile j + 1 are loaded into registers
//     while n-tile j computes (two register sets, ping-pong);
//   * epilogue per n-tile as chain.hip phase 2: each wave stages its
//     accumulators through a private fp32 LDS slab (wave barrier only),
//     (acc + bias) + residual -> act -> one rounding to bf16 (gemm::epi_chunk's
//     order with alpha = 1), unconditional 16-B buffer stores (rows past M go
//     to kOOB).  The stores drain under the next n-tile's MFMAs.
//
// vmcnt discipline.  Every step issues the same memory operations (slots past
// the sequence and prefetches past the span go to kOOB), so the operations
// younger than a ring slot are a compile-time count per k-step.  Stores count
// in vmcnt too and may complete out of order with the DMAs, so the wait before
// slot t is vmcnt(L) with L = the LOADS certainly issued after slot t's DMAs,
// stores left out: loads return in order among themselves, so "at most L
// outstanding" cannot hold while slot t and its L younger loads are all in
// flight, whatever the stores did.  (If stores do complete in order the wait
// asks for up to one younger slot early; the ring is three slots ahead.)  The
// prefetch issued in the same step as slot t's DMAs is not counted either, so
// the count holds whichever way the compiler orders the two.
//
// LDS: 32 KB ring + 17 KB slabs = 49 KB, three workgroups per CU by LDS.
#include <type_traits>
#include <utility>

#include "gemm_common.h"

namespace tfsk {
namespace {

using namespace gemm;

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): an unrolled loop whose index is a constant
// expression (the counted vmcnt waits take an immediate)
template <class F, int... I>
__device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}

// 8 consecutive floats of this wave's epilogue slab.  Inline asm, with its own lgkmcnt wait: before a
// compiler-visible read of the slab hipcc waits vmcnt(0) -- any LDS read it can name may alias the ring's
// LDS-DMAs in flight -- which drained the ring at every n-tile (seen in the gfx950 ISA).  The slab is written
// and read by this wave only, and a wave's LDS operations execute in order.
__device__ __forceinline__ void slab_read8(const float* src, f32x4& lo, f32x4& hi) {
  typedef __attribute__((address_space(3))) const float* lds_cfp_t;
  const uint32_t addr = uint32_t(reinterpret_cast<uintptr_t>((lds_cfp_t)src));
  asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(lo), "=&v"(hi)
               : "v"(addr)
               : "memory");
}

struct PanelArgs {
  const uint16_t* a;     // [M][K] bf16
  const uint16_t* w;     // [N][ldw] bf16
  const float* bias;     // [N]
  const uint16_t* res;   // [M][N] bf16 or nullptr
  uint16_t* out;         // [M][N] bf16
  int M, N, ldw;
  int ns_log2;           // nsplit = 1 << ns_log2 column spans per row panel
  float lo;              // activation floor: 0 (ReLU) or -inf (none)
};

constexpr int kPanelNT = 256, kPanelStgLd = 68;   // fp32 slab row stride (floats): 16-B aligned rows

template <int K, int BM>
struct PN {
  static constexpr int KT1 = K / KT;                  // k-tiles per n-tile
  static constexpr int KS = K / 32;                   // MFMA k-steps
  static constexpr int RPW = BM / 4, TM = RPW / 16;   // rows per wave, 16-row fragments per wave
  static constexpr int S = 4;                         // ring depth
  static constexpr int SLOT = 64 * KT * 2;            // [64 cols][64 k] bf16
  static constexpr int WPW = 64 / 8 / 4;              // 8-row DMA pieces per wave per slot
  static constexpr int RING = S * SLOT;
  static constexpr int STG = 4 * 16 * kPanelStgLd * 4;   // one 16-row slab per wave
  static constexpr int LDS = RING + STG;
  static constexpr int EPI = 2 * TM + 2;              // prefetch loads per lane per n-tile: residual + bias
  static constexpr int STORES = 2 * TM;               // 16-B stores per lane per n-tile
  // loads certainly younger than slot t at the wait of k-step u of an n-tile:
  // the S - 2 slots after it, and the prefetches of the steps t - S + 2 .. t - 1
  static constexpr int younger(int u) {
    int pf = 0;
    for (int d = 1; d <= S - 2; ++d) pf += ((u - d) % KT1 + KT1) % KT1 == 0;
    return (S - 2) * WPW + pf * EPI;
  }
  static_assert(K % KT == 0 && (KT1 & (KT1 - 1)) == 0 && (BM == 64 || BM == 128), "panel shape");
  static_assert((S & (S - 1)) == 0, "slot = t & (S - 1)");
  static_assert(LDS <= 80 * 1024, "two workgroups per CU");
  static_assert((S - 2) * WPW + (S - 2) * EPI < 64, "vmcnt range");
};

template <int K, int BM>
__global__ __launch_bounds__(kPanelNT, 2) void conv1x1_panel_kernel(PanelArgs p) {
  using G = PN<K, BM>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int prow = lane >> 3;
  const uint32_t kc = uint32_t(((lane & 7) ^ prow) * 8);
  const int c8 = lane & 7, rl = lane >> 3;
  const int M = p.M, N = p.N;

  // spans of one row panel are adjacent logical ids: they share an XCD's L2
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int panel = id >> p.ns_log2, span = id - (panel << p.ns_log2);
  const int m0 = panel * BM;
  const int NS = N >> p.ns_log2;
  const int n0 = span * NS;
  const int ntiles = NS >> 6;
  const int T = ntiles * G::KT1;

  const __amdgpu_buffer_rsrc_t rsA =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(p.a), 0, int(long(M) * K * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsW =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(p.w), 0, int(long(N) * p.ldw * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias), 0, N * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(p.res), 0, p.res ? int(long(M) * N * 2) : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, int(long(M) * N * 2), 0x00020000);

  // ---- the A panel: this wave's rows as MFMA fragments (row fr, k chunk fq of each 32-deep k-step)
  bf16x8 af[G::TM][G::KS];
#pragma unroll
  for (int i = 0; i < G::TM; ++i) {
    const int m = m0 + wid * G::RPW + i * 16 + fr;
#pragma unroll
    for (int ks = 0; ks < G::KS; ++ks) {
      const uint32_t v = m < M ? (uint32_t(m) * uint32_t(K) + uint32_t(ks * 32 + fq * 8)) * 2u : kOOB;
      af[i][ks] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsA, v, 0, 0));
    }
  }

  // ---- ring slot t = (n-tile t / KT1, k-tile t % KT1): piece q (8 rows x 128 B) lands at rows [8q, 8q + 8)
  auto issue_w = [&](int t) {
    const int j = t / G::KT1, kt = t % G::KT1;
    char* slot = smem + (t & (G::S - 1)) * G::SLOT;
    // past the sequence: bit 31 sends the offset out of range (an OR, not a select of two offsets, which the
    // compiler turned into a scalar branch around each DMA -- and then lost count of them in its own waits)
    const uint32_t past = t < T ? 0u : kOOB;
#pragma unroll
    for (int q = 0; q < G::WPW; ++q) {
      const int pc = wid * G::WPW + q;
      const int n = n0 + j * 64 + pc * 8 + prow;
      const uint32_t v = ((uint32_t(n) * uint32_t(p.ldw) + uint32_t(kt * KT) + kc) * 2u) | past;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (lds_ptr_t)(slot + pc * 1024), 16, v, 0, 0, 0);
    }
  };

  // ---- this lane's epilogue operands of n-tile j: chunk column c8 of rows rl and rl + 8 of each 16-row unit
  auto load_epi = [&](int j, u32x4 (&rr)[G::TM][2], u32x4 (&bb)[2]) {
    const uint32_t past = j < ntiles ? 0u : kOOB;
    const uint32_t n = uint32_t(n0 + j * 64 + c8 * 8);
    bb[0] = __builtin_amdgcn_raw_buffer_load_b128(rsB, (n * 4u) | past, 0, 0);
    bb[1] = __builtin_amdgcn_raw_buffer_load_b128(rsB, (n * 4u + 16u) | past, 0, 0);
#pragma unroll
    for (int i = 0; i < G::TM; ++i)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int m = m0 + wid * G::RPW + i * 16 + rl + 8 * k;
        rr[i][k] = __builtin_amdgcn_raw_buffer_load_b128(
            rsR, (m < M ? (uint32_t(m) * uint32_t(N) + n) * 2u : kOOB) | past, 0, 0);
      }
  };

  float* stg = reinterpret_cast<float*>(smem + G::RING) + wid * 16 * kPanelStgLd;
  const uint32_t ro0 = uint32_t((fr * KT + ((fq ^ (fr & 7)) * 8)) * 2);
  const uint32_t ro1 = uint32_t((fr * KT + (((4 + fq) ^ (fr & 7)) * 8)) * 2);
  const float lo_act = p.lo;

  // n-tile j: its K loop over the ring, then its epilogue with (rc, bc); the
  // operands of n-tile j + 1 are loaded into (rn, bn) meanwhile
  auto tile = [&](int j, u32x4 (&rc)[G::TM][2], u32x4 (&bc)[2], u32x4 (&rn)[G::TM][2], u32x4 (&bn)[2]) {
    f32x4 acc[G::TM][4];
#pragma unroll
    for (int i = 0; i < G::TM; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) acc[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
    static_for([&](auto uc) __attribute__((always_inline)) {
      constexpr int u = decltype(uc)::value;
      const int t = j * G::KT1 + u;
      // slot t landed (see the header), and every wave is done reading slot t - 1, which the issue below refills
      wait_vmcnt<G::younger(u)>();
      lds_barrier();
      issue_w(t + G::S - 1);
      if (u == 0) load_epi(j + 1, rn, bn);
      const char* sb = smem + (t & (G::S - 1)) * G::SLOT;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 bfr[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
          bfr[jj] = *reinterpret_cast<const bf16x8*>(sb + (kk ? ro1 : ro0) + jj * 16 * KT * 2);
#pragma unroll
        for (int i = 0; i < G::TM; ++i)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
            acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][u * 2 + kk], bfr[jj], acc[i][jj], 0, 0, 0);
      }
    }, std::make_integer_sequence<int, G::KT1>{});
    // ---- epilogue through this wave's fp32 slab, 16 rows x 64 columns at a time
    const float bv[8] = {__uint_as_float(bc[0].x), __uint_as_float(bc[0].y), __uint_as_float(bc[0].z),
                         __uint_as_float(bc[0].w), __uint_as_float(bc[1].x), __uint_as_float(bc[1].y),
                         __uint_as_float(bc[1].z), __uint_as_float(bc[1].w)};
    const uint32_t n = uint32_t(n0 + j * 64 + c8 * 8);
#pragma unroll
    for (int i = 0; i < G::TM; ++i) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int r = 0; r < 4; ++r) stg[(fq * 4 + r) * kPanelStgLd + jj * 16 + fr] = acc[i][jj][r];
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const float* src = stg + (rl + 8 * k) * kPanelStgLd + c8 * 8;
        f32x4 lo, hi;
        slab_read8(src, lo, hi);
        const float a[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        const u32x4 w = rc[i][k];
        const uint32_t rw[4] = {w.x, w.y, w.z, w.w};
        u32x4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v0 = fmaxf(a[2 * e] + bv[2 * e] + __uint_as_float(rw[e] << 16), lo_act);
          const float v1 = fmaxf(a[2 * e + 1] + bv[2 * e + 1] + __uint_as_float(rw[e] & 0xffff0000u), lo_act);
          ov[e] = pack_bf16x2(v0, v1);
        }
        const int m = m0 + wid * G::RPW + i * 16 + rl + 8 * k;
        // unconditional store: rows past M go to a dropped out-of-range offset
        __builtin_amdgcn_raw_buffer_store_b128(ov, rsO, m < M ? (uint32_t(m) * uint32_t(N) + n) * 2u : kOOB, 0, 0);
      }
      __builtin_amdgcn_wave_barrier();   // slab reads done before the next unit overwrites it
    }
  };

  // ---- ring prologue and n-tile 0's epilogue operands; everything issued so far lands here
#pragma unroll
  for (int s = 0; s < G::S - 1; ++s) issue_w(s);
  u32x4 r0[G::TM][2], b0[2], r1[G::TM][2], b1[2];
  load_epi(0, r0, b0);
  wait_vmcnt<0>();
  __syncthreads();

  // (an odd last n-tile after the loop, not under a branch inside it: with the branch hipcc waited at the loop
  // head for the prefetch that only the skipped tile would have consumed)
  int j = 0;
  for (; j + 1 < ntiles; j += 2) {
    tile(j, r0, b0, r1, b1);
    tile(j + 1, r1, b1, r0, b0);
  }
  if (j < ntiles) tile(j, r0, b0, r1, b1);
  // the ring's tail DMAs (kOOB) and the last stores are done before the LDS is released
  wait_vmcnt<0>();
}

template <int K, int BM>
hipError_t launch_panel(const PanelArgs& a, int nsplit, hipStream_t s) {
  using G = PN<K, BM>;
  hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(&conv1x1_panel_kernel<K, BM>), G::LDS);
  if (e != hipSuccess) return e;
  const int grid = ((a.M + BM - 1) / BM) * nsplit;
  hipLaunchKernelGGL((conv1x1_panel_kernel<K, BM>), dim3(grid), dim3(kPanelNT), G::LDS, s, a);
  return hipGetLastError();
}

}  // namespace

bool conv1x1_panel_supported(int M, int N, int K, int bm, int nsplit) {
  if (M <= 0 || (K != 128 && K != 256 && K != 512) || N <= 0 || N % 64) return false;
  if (nsplit != 1 && nsplit != 2 && nsplit != 4 && nsplit != 8) return false;
  if (N % nsplit || (N / nsplit) % 64) return false;
  if (bm != 64 && !(bm == 128 && K <= 256)) return false;
  // 32-bit buffer offsets (N >= 64 and K <= 512: the output bounds A as well unless N < K)
  return long(M) * N * 2 < 0x7fffffffL && long(M) * K * 2 < 0x7fffffffL;
}

int conv1x1_panel_forms(int M, int N, int K, int* bm, int* nsplit) {
  // by fewer spans first (fewer reads of A), 64 rows before 128: the forms
  // with at least 128 workgroups, or every form when none has that many
  int count = 0;
  for (int pass = 0; pass < 2 && count == 0; ++pass)
    for (int ns = 1; ns <= 8; ns *= 2)
      for (int b = 64; b <= 128; b += 64) {
        if (!conv1x1_panel_supported(M, N, K, b, ns)) continue;
        const long wgs = long((M + b - 1) / b) * ns;
        if ((pass == 0 && wgs < 128) || count == kPanelMaxForms) continue;
        bm[count] = b;
        nsplit[count] = ns;
        ++count;
      }
  return count;
}

hipError_t conv1x1_panel_launch(const uint16_t* a, const uint16_t* w, int ldw, const float* bias, const uint16_t* res,
                                uint16_t* out, int M, int N, int K, int bm, int nsplit, int act, hipStream_t s) {
  if (M == 0) return hipSuccess;
  if (!conv1x1_panel_supported(M, N, K, bm, nsplit) || ldw < K || ldw % 8) return hipErrorInvalidValue;
  if (act != kActNone && act != kActRelu) return hipErrorInvalidValue;
  // (the ring's tail slots compute offsets up to S - 1 n-tiles past the span before they are sent out of range)
  if (long(N + 256) * ldw * 2 >= 0x7fffffffL) return hipErrorInvalidValue;
  const int ns_log2 = nsplit == 1 ? 0 : nsplit == 2 ? 1 : nsplit == 4 ? 2 : 3;
  const PanelArgs p{a, w, bias, res, out, M, N, ldw, ns_log2, act == kActRelu ? 0.f : -INFINITY};
  if (bm == 128) return K == 128 ? launch_panel<128, 128>(p, nsplit, s) : launch_panel<256, 128>(p, nsplit, s);
  if (K == 128) return launch_panel<128, 64>(p, nsplit, s);
  if (K == 256) return launch_panel<256, 64>(p, nsplit, s);
  return launch_panel<512, 64>(p, nsplit, s);
}

}  // namespace tfsk
