// The epilogue pieces shared by igemm.hip, bgemm.hip and halo.hip: activation
// dispatch, the guard of the one-pass bf16 epilogue, the split-K slab store and
// in-kernel finish, the row-chunk loop around epi_chunk and the residual
// prefetch.  Accumulator staging into LDS stays with each kernel (their
// layouts differ), and so does the one-pass bf16 epilogue itself.
// cgemm_impl.h does not use this header: with any of these pieces, the
// dispatch alone included, some of its 254 kernels spill more SGPRs or lose
// occupancy (docs/benchmarks.md, "One epilogue for the GEMM / conv kernels"),
// so it keeps its own switches, prefetch_residual, epilogue_rows, slab store
// and finish.  A fix to the epilogue goes here, into gemm_common.h epi_chunk
// and into cgemm_impl.h.
#pragma once
#include <type_traits>

#include "gemm_common.h"

namespace tfsk {
namespace gemm {

// Runtime activation code -> compile-time tag: f(std::integral_constant<int, ACT>{}).
// WITH_ERF = false: erf GELU takes the default (none) -- the callers that
// exclude erf beforehand do not pay for its expansion.
// WITH_RELU6: the kernel also builds the ReLU6, hard-swish and swish epilogues
// (the "igemm-only" activations).  igemm only: it takes every shape, so a
// relu6, hard-swish or swish conv always has a kernel.  bgemm and halo keep the
// four-case switch (their code is unchanged by any of them), and the bindings
// reject all three on their configs as they do on cgemm's.
template <bool WITH_ERF = true, bool WITH_RELU6 = false, class F>
__device__ __forceinline__ void dispatch_act(int act, F&& f) {
  if constexpr (WITH_RELU6) {
    if (act == kActRelu6) {
      f(std::integral_constant<int, kActRelu6>{});
      return;
    }
    if (act == kActHardSwish) {
      f(std::integral_constant<int, kActHardSwish>{});
      return;
    }
    if (act == kActSwish) {
      f(std::integral_constant<int, kActSwish>{});
      return;
    }
  }
  if constexpr (WITH_ERF) {
    switch (act) {
      case kActRelu: f(std::integral_constant<int, kActRelu>{}); break;
      case kActGeluTanh: f(std::integral_constant<int, kActGeluTanh>{}); break;
      case kActGeluErf: f(std::integral_constant<int, kActGeluErf>{}); break;
      case kActTanh: f(std::integral_constant<int, kActTanh>{}); break;
      default: f(std::integral_constant<int, kActNone>{}); break;
    }
  } else {
    switch (act) {
      case kActRelu: f(std::integral_constant<int, kActRelu>{}); break;
      case kActGeluTanh: f(std::integral_constant<int, kActGeluTanh>{}); break;
      case kActTanh: f(std::integral_constant<int, kActTanh>{}); break;
      default: f(std::integral_constant<int, kActNone>{}); break;
    }
  }
}

// Row map of a dense tile (or of one row pass of it): tile row -> global GEMM
// row, -1 past M.  The epilogue pieces below take any such callable; the halo
// kernel passes its output-pixel map.
struct DenseRows {
  int m0, M;
  __device__ __forceinline__ int operator()(int row) const { return m0 + row < M ? m0 + row : -1; }
};

// Issue the residual loads of this thread's epilogue chunks early (before the
// K loop) so their latency hides under the operand DMA and the MFMAs.
template <int BM, int BN, int NT>
__device__ __forceinline__ void prefetch_residual(const IGemmArgs& p, int m0, int n0, int tid,
                                                  uint4 (&rpre)[Epi<BM, BN, NT>::PRE > 0 ? Epi<BM, BN, NT>::PRE : 1]) {
  using E = Epi<BM, BN, NT>;
  if (E::PRE == 0 || !p.residual || p.splits > 1 || (p.N % 8) || (p.ldr % 8)) return;
#pragma unroll
  for (int it = 0; it < E::PRE; ++it) {
    int row, col;
    const bool in = epi_rowcol<BM, BN, NT>(tid, it, row, col);
    const int m = m0 + row, n = n0 + col;
    rpre[it] = (in && m < p.M && n + 8 <= p.N) ? *reinterpret_cast<const uint4*>(p.residual + size_t(m) * p.ldr + n)
                                          : make_uint4(0, 0, 0, 0);
  }
}

// Row chunks of the fp32 tile in Cs through epi_chunk, residual loaded per
// chunk.  `rows`: tile row -> global row or -1.  UNROLL: the `#pragma unroll`
// count of the chunk loop, for every activation (halo and bgemm: 2).
template <int BM, int BN, int NT, int CS_LD, int ACT, int UNROLL, class Rows>
__device__ __forceinline__ void epilogue_rows(const IGemmArgs& p, const float* Cs, int n0, int tid, const Rows& rows,
                                              const float4 b0, const float4 b1) {
  using E = Epi<BM, BN, NT>;
  const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll UNROLL
  for (int it = 0; it < E::ITERS; ++it) {
    int row, col;
    if (!epi_rowcol<BM, BN, NT>(tid, it, row, col)) continue;
    const int m = rows(row), n = n0 + col;
    if (m < 0 || n >= p.N) continue;
    const uint4 rr = p.residual ? *reinterpret_cast<const uint4*>(p.residual + size_t(m) * p.ldr + n)
                                : make_uint4(0, 0, 0, 0);
    epi_chunk<ACT>(p, Cs + row * CS_LD + col, m, n, bv, rr);
  }
}

// True when the launch takes a kernel's one-pass bf16 epilogue: plain bf16
// output, one K slice, no residual / second output, any activation but erf.
// bgemm's kernel and the persistent halo launcher call it; halo_epilogue and
// cgemm write the same seven terms out (as a call they changed those kernels'
// branch layout and cost registers, see halo.hip).
__host__ __device__ __forceinline__ bool plain_bf16_epilogue(const IGemmArgs& p) {
  return p.splits <= 1 && p.residual == nullptr && p.out2 == nullptr && !p.out_f32 && p.out != nullptr &&
         p.act != kActGeluErf && !p.epi_f32;
}

// Split-K: the raw (alpha-scaled) partial slab of this K slice (blockIdx.y)
// from the fp32 tile in Cs; splitk_reduce or the last slice (splitk_finish)
// applies the epilogue.  OPTS, a sum of:
//   kSlabTail: the scalar path for N % 4 != 0 is compiled in (the kernels
//     without it are only launched with N % 8 == 0);
//   kSlabFixup: the kernel has the in-kernel finish, so with p.counters set
//     the stores are the agent-coherent ones its last slice reads back;
//   kSlabRolled: `#pragma unroll 1` (the halo kernels' loop; the others leave
//     the unrolling to the compiler).
enum SlabOpt : int { kSlabTail = 1, kSlabFixup = 2, kSlabRolled = 4 };

template <int BM, int BN, int NT, int CS_LD, int OPTS, class Rows>
__device__ __forceinline__ void splitk_store_slab(const IGemmArgs& p, const float* Cs, int n0, int tid,
                                                  const Rows& rows) {
  using E = Epi<BM, BN, NT>;
  constexpr bool TAIL = OPTS & kSlabTail, FIXUP = OPTS & kSlabFixup;
  const int N = p.N;
  const float alpha = p.alpha;
  float* ws = p.ws + size_t(blockIdx.y) * p.M * N;
  const bool v4 = (N % 4 == 0);
  auto chunk = [&](int it) __attribute__((always_inline)) {
    int row, col;
    if (!epi_rowcol<BM, BN, NT>(tid, it, row, col)) return;
    const int m = rows(row), n = n0 + col;
    if (m < 0 || n >= N) return;
    const float* src = Cs + row * CS_LD + col;
    float* dst = ws + size_t(m) * N + n;
    if (!TAIL || (v4 && n + 8 <= N)) {
      float4 a = *reinterpret_cast<const float4*>(src);
      float4 b = *reinterpret_cast<const float4*>(src + 4);
      a.x *= alpha; a.y *= alpha; a.z *= alpha; a.w *= alpha;
      b.x *= alpha; b.y *= alpha; b.z *= alpha; b.w *= alpha;
      if constexpr (FIXUP) {
        if (p.counters != nullptr) {
          splitk_store8(p, splitk_rsrc(p), m, n, a, b);
          return;
        }
      }
      *reinterpret_cast<float4*>(dst) = a;
      *reinterpret_cast<float4*>(dst + 4) = b;
    } else {
      for (int e = 0; e < 8 && n + e < N; ++e) dst[e] = src[e] * alpha;
    }
  };
  if constexpr (OPTS & kSlabRolled) {
#pragma unroll 1
    for (int it = 0; it < E::ITERS; ++it) chunk(it);
  } else {
    for (int it = 0; it < E::ITERS; ++it) chunk(it);
  }
}

// The last slice of a fixed-up tile (splitk_arrive returned true): every slab
// of the tile summed back into Cs (unrolled: every chunk's slab loads in
// flight together), then `q` -- a copy of the launch's arguments -- becomes
// the epilogue's view: one slice, alpha 1 (the slabs carry alpha already), and
// the bias the split path did not prefetch in b0 / b1.
template <int BM, int BN, int NT, int CS_LD, class Rows>
__device__ __forceinline__ void splitk_finish(IGemmArgs& q, float* Cs, int n0, int tid, const Rows& rows, float4& b0,
                                              float4& b1) {
  using E = Epi<BM, BN, NT>;
  const __amdgpu_buffer_rsrc_t wsr = splitk_rsrc(q);
#pragma unroll
  for (int it = 0; it < E::ITERS; ++it) {
    int row, col;
    if (!epi_rowcol<BM, BN, NT>(tid, it, row, col)) continue;
    const int m = rows(row), n = n0 + col;
    if (m < 0 || n >= q.N) continue;
    float4 lo, hi;
    splitk_sum8(q, wsr, m, n, lo, hi);
    *reinterpret_cast<float4*>(Cs + row * CS_LD + col) = lo;
    *reinterpret_cast<float4*>(Cs + row * CS_LD + col + 4) = hi;
  }
  __syncthreads();
  q.splits = 1;
  q.alpha = 1.f;
  prefetch_bias<BM, BN, NT>(q, n0, tid, b0, b1);
}

}  // namespace gemm
}  // namespace tfsk
