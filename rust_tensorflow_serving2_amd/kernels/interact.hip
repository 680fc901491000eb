// DLRM dot interaction, gfx950.
//
//   out[b] = [ dense[b, 0:Dd] | z_i . z_j over np.tril_indices(F, k) | zeros ]        k = -1 or 0
//
// Z [B][F][D] bf16, dense [B][Dd] bf16 or null, out [B][Wp] bf16 with
// Wp = ceil8(Dd + P + pad), P the pair count; every column of [0, Wp) is
// written, the zero tail included.
//
// One wave per sample, four samples per 256-thread workgroup.  Z[b] is padded
// to 32 rows through the descriptor (rows >= F get kOOB and read zeros) and
// Z Z^T runs on v_mfma_f32_16x16x32_bf16.  For Z Z^T the A and the B fragment
// of a 16-row block are the same registers: lane l holds row l % 16 and the
// 16-B chunk l / 16 of the 32-deep k-step, loaded once, straight from global.
// Only the tiles on and below the diagonal run -- (0,0), (1,0), (1,1); with
// F <= 16 only (0,0) -- four k-steps' fragments in flight at a time.
//
// Tile (bi, bj) leaves entry (I, J) = (16 bi + 4 (l / 16) + r, 16 bj + l % 16)
// in register r of lane l.  The entries with J <= I + k and I < F are rounded
// once and written to position I (I + 1 + 2k) / 2 + J of the wave's own LDS row
// image (np.tril_indices order); entries of padded rows are computed and never
// written, so an Inf or NaN in feature row i reaches the outputs (i, .) and
// (., i) of its own sample and nothing else.  The image's chunks from P / 8 on
// are zeroed first; the row then leaves as 16-B chunks with unconditional
// buffer stores (kOOB for the chunks past the row and for a wave past the last
// sample).  The dense columns are copied global to global.  fp32 accumulate,
// no atomics, one chain per output: reruns are bit-equal.
#include "common.h"
#include "gemm_common.h"
#include "launch.h"

namespace tfsk {

namespace {

using gemm::kOOB;
constexpr int kImg = kInteractMaxTail;      // elements of a wave's row image (the columns behind dense)
constexpr int kSteps = 4;                   // k-steps whose fragments are loaded together

struct InteractArgs {
  int B, F, D, Dd, P, Wp, self;             // self = 1: k = 0 (the diagonal included)
  int z_bytes, dense_bytes, out_bytes;
};

template <bool TWO>
__global__ __launch_bounds__(256) void dot_interaction_kernel(const uint16_t* __restrict__ z,
                                                              const uint16_t* __restrict__ dense,
                                                              uint16_t* __restrict__ out, const InteractArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t images[4 * kImg];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int F = a.F, D = a.D, Wp = a.Wp, Dd = a.Dd;
  const int b = blockIdx.x * 4 + wid;
  const bool live = b < a.B;
  uint16_t* img = images + wid * kImg;
  const __amdgpu_buffer_rsrc_t rsZ =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(z), 0, a.z_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsD =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(dense), 0, a.dense_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(out, 0, a.out_bytes, 0x00020000);
  const uint32_t orow = uint32_t(b) * uint32_t(Wp) * 2u;          // (bytes; used when live)

  // ---- dense columns: global to global
  const int dch = Dd >> 3;
  for (int c0 = 0; c0 < dch; c0 += 64) {
    const int c = c0 + lane;
    const bool ok = live && c < dch;
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsD, ok ? uint32_t(b * dch + c) * 16u : kOOB, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b128(v, rsO, ok ? orow + uint32_t(c) * 16u : kOOB, 0, 0);
  }

  // ---- Z Z^T on and below the block diagonal
  const uint32_t zb = uint32_t(b) * uint32_t(F * D) * 2u;
  const uint32_t off0 = live && fr < F ? zb + uint32_t(fr * D + fq * 8) * 2u : kOOB;
  const uint32_t off1 = live && 16 + fr < F ? zb + uint32_t((16 + fr) * D + fq * 8) * 2u : kOOB;
  const int nks = D >> 5;
  f32x4 c00 = {0.f, 0.f, 0.f, 0.f}, c10 = c00, c11 = c00;
  for (int k0 = 0; k0 < nks; k0 += kSteps) {
    bf16x8 a0[kSteps], a1[kSteps];
#pragma unroll
    for (int j = 0; j < kSteps; ++j) {
      const bool in = k0 + j < nks;                               // a k-step past D reads zeros
      // (the offsets pass through an empty asm: hipcc otherwise splits each select into two branches
      // around the load, with a vmcnt(0) between them)
      uint32_t o0 = in ? off0 + uint32_t(k0 + j) * 64u : kOOB, o1 = in ? off1 + uint32_t(k0 + j) * 64u : kOOB;
      asm volatile("" : "+v"(o0), "+v"(o1));
      a0[j] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsZ, o0, 0, 0));
      if constexpr (TWO) a1[j] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsZ, o1, 0, 0));
    }
    __builtin_amdgcn_sched_barrier(0);       // (the scheduler otherwise sinks each load to its MFMA: two in flight)
#pragma unroll
    for (int j = 0; j < kSteps; ++j) {
      c00 =__builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[j], a0[j], c00, 0, 0, 0);
      if constexpr (TWO) {
        c10 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[j], a0[j], c10, 0, 0, 0);
        c11 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[j], a1[j], c11, 0, 0, 0);
      }
    }
  }

  // ---- the row image: zeros from chunk P / 8 on, then the pairs in tril order
  const int ichunks = (Wp - Dd) >> 3;
  for (int c0 = a.P >> 3; c0 < ichunks; c0 += 64) {
    const int c = c0 + lane;
    if (c < ichunks) *reinterpret_cast<u32x4*>(img + c * 8) = u32x4{0u, 0u, 0u, 0u};
  }
  asm volatile("" ::: "memory");             // (one wave's LDS operations complete in issue order)
  const int self = a.self;
  auto put = [&](const f32x4& c, int bi, int bj) {
    const int J = 16 * bj + fr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int I = 16 * bi + 4 * fq + r;
      if (I < F && J < I + self) img[((I * (I - 1 + 2 * self)) >> 1) + J] = f32_to_bf16(c[r]);
    }
  };
  put(c00, 0, 0);
  if constexpr (TWO) {
    put(c10, 1, 0);
    put(c11, 1, 1);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              // this wave's LDS writes landed
  __builtin_amdgcn_wave_barrier();
  for (int c0 = 0; c0 < ichunks; c0 += 64) {
    const int c = c0 + lane;
    const bool ok = live && c < ichunks;
    const u32x4 v = *reinterpret_cast<const u32x4*>(img + min(c, ichunks - 1) * 8);
    __builtin_amdgcn_raw_buffer_store_b128(v, rsO, ok ? orow + uint32_t(Dd + c * 8) * 2u : kOOB, 0, 0);
  }
}

}  // namespace

int64_t dot_interaction_pairs(int64_t F, bool self) { return self ? F * (F + 1) / 2 : F * (F - 1) / 2; }

int64_t dot_interaction_width(int64_t F, int64_t Dd, int64_t pad, bool self) {
  return (Dd + dot_interaction_pairs(F, self) + pad + 7) / 8 * 8;
}

bool dot_interaction_supported(int64_t B, int64_t F, int64_t D, int64_t Dd, int64_t pad, bool self) {
  if (B < 0 || F < 2 || F > kInteractMaxF || D % 32 != 0 || D < 32 || D > kInteractMaxD) return false;
  if (Dd < 0 || Dd % 8 != 0 || pad < 0) return false;
  const int64_t Wp = dot_interaction_width(F, Dd, pad, self);
  if (Wp - Dd > kInteractMaxTail) return false;
  const int64_t lim = int64_t(1) << 31;
  return B * F * D * 2 < lim && B * Wp * 2 < lim && B * Dd * 2 < lim;
}

hipError_t dot_interaction_launch(const uint16_t* z, const uint16_t* dense, uint16_t* out, int64_t B, int64_t F,
                                  int64_t D, int64_t Dd, int64_t pad, bool self, hipStream_t s) {
  if (dense == nullptr) Dd = 0;
  if (!dot_interaction_supported(B, F, D, Dd, pad, self)) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  InteractArgs a;
  a.B = int(B); a.F = int(F); a.D = int(D); a.Dd = int(Dd);
  a.P = int(dot_interaction_pairs(F, self));
  a.Wp = int(dot_interaction_width(F, Dd, pad, self));
  a.self = self ? 1 : 0;
  a.z_bytes = int(B * F * D * 2);
  a.dense_bytes = int(B * Dd * 2);
  a.out_bytes = int(B * a.Wp * 2);
  const dim3 grid(unsigned((B + 3) / 4));
  if (F > 16)
    hipLaunchKernelGGL(dot_interaction_kernel<true>, grid, dim3(256), 0, s, z, dense, out, a);
  else
    hipLaunchKernelGGL(dot_interaction_kernel<false>, grid, dim3(256), 0, s, z, dense, out, a);
  return hipGetLastError();
}

}  // namespace tfsk
