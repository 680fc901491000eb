// Embedding bag (DLRM's sparse features), gfx950.
//
//   out[b, F0 + f, :] = bf16( sum_{l < L_f} table_f[ ids[b, first_f + l], : ] )      f < F, one launch
//   out[b, 0, :]      = dense[b, :]                                                    when F0 == 1
//
// ids [B][T] int32 or int64 (read as they are: no cast launch), the tables one
// bf16 blob [sum V_f][D], feat [F][4] int64 = (first row of table f in the blob,
// V_f, first_f, L_f), dense [B][D] bf16 or null, out [B][F0 + F][D] bf16.
//
// A thread owns one 16-B chunk (8 channels) of one (b, f) output row, chunks
// fastest across lanes, so a wave reads whole rows of 16-B pieces.  The feature
// comes from blockIdx.y: feat[f] arrives by scalar loads and the table's buffer
// descriptor is scalar, based at table f and exactly V_f rows long (every table
// below 2 GiB; the blob may be larger).  Every global access is an
// unconditional buffer load / store:
//   * an id < 0 or >= V_f (an int64 with a non-zero high word included), a slot
//     l >= L_f of the last batch of four and a thread past the last chunk get
//     kOOB as the whole offset and read zeros -- never a clamped row times 0,
//     which would turn an Inf in that row into NaN;
//   * the row loads of up to four slots are issued together, the next four ids
//     behind them, before the first add;
//   * a dead thread's store gets kOOB and is dropped.
// The fp32 accumulator starts from the first row's value and adds the others
// in slot order: L_f = 1 is a copy (whatever the bf16 -> f32 -> bf16 round trip
// keeps, -0 included), and there is one rounding to bf16.  No atomics, no LDS,
// one chain per output: reruns are bit-equal.
#include "common.h"
#include "gemm_common.h"
#include "launch.h"

namespace tfsk {

namespace {

using gemm::kOOB;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

struct EmbagArgs {
  int B, T, CH, F, F0;                      // CH = D / 8 chunks per row
  int ids_bytes, dense_bytes, out_bytes;
};

constexpr int kAhead = 4;                   // row loads in flight per thread

template <bool I64>
__global__ __launch_bounds__(256) void embedding_bag_kernel(const void* __restrict__ ids,
                                                            const uint16_t* __restrict__ blob,
                                                            const int64_t* __restrict__ feat,
                                                            const uint16_t* __restrict__ dense,
                                                            uint16_t* __restrict__ out, const EmbagArgs a) {
  const int CH = a.CH;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;            // chunk of this slot: b * CH + ch
  const bool live = i < uint32_t(a.B) * uint32_t(CH);
  const uint32_t b = (live ? i : 0u) / uint32_t(CH), ch = (live ? i : 0u) - b * uint32_t(CH);
  const int slot = blockIdx.y;                                    // output row within a sample
  const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(out, 0, a.out_bytes, 0x00020000);
  const uint32_t ooff = live ? ((b * uint32_t(a.F0 + a.F) + uint32_t(slot)) * uint32_t(CH) + ch) * 16u : kOOB;
  if (slot < a.F0) {                                              // (uniform) the dense row
    const __amdgpu_buffer_rsrc_t rsD =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(dense), 0, a.dense_bytes, 0x00020000);
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsD, live ? i * 16u : kOOB, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b128(v, rsO, ooff, 0, 0);
    return;
  }
  const int64_t* ft = feat + long(slot - a.F0) * 4;
  const long row_base = ft[0];
  const int V = int(ft[1]), first = int(ft[2]), L = int(ft[3]);
  const uint32_t row_bytes = uint32_t(CH) * 16u;
  const __amdgpu_buffer_rsrc_t rsI = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(ids), 0, a.ids_bytes,
                                                                       0x00020000);
  const __amdgpu_buffer_rsrc_t rsT = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint16_t*>(blob) + row_base * CH * 8, 0, int(uint32_t(V) * row_bytes), 0x00020000);
  constexpr uint32_t kIdBytes = I64 ? 8u : 4u;
  const uint32_t id0 = (b * uint32_t(a.T) + uint32_t(first)) * kIdBytes;

  uint32_t lo[kAhead], hi[kAhead];
  auto load_ids = [&](int l0) {
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      uint32_t off = live & (l0 + j < L) ? id0 + uint32_t(l0 + j) * kIdBytes : kOOB;
      asm volatile("" : "+v"(off));         // (hipcc otherwise splits the select into two branches around the load)
      if constexpr (I64) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rsI, off, 0, 0);
        lo[j] = v.x;
        hi[j] = v.y;
      } else {
        lo[j] = __builtin_amdgcn_raw_buffer_load_b32(rsI, off, 0, 0);
        hi[j] = 0u;
      }
    }
  };

  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  load_ids(0);
  for (int l0 = 0; l0 < L; l0 += kAhead) {
    u32x4 r[kAhead];
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      // unsigned compare: a negative int32 is >= 2^31 > V; a negative int64 has a non-zero high word
      const bool ok = live & (l0 + j < L) & (hi[j] == 0u) & (lo[j] < uint32_t(V));
      uint32_t off = ok ? lo[j] * row_bytes + ch * 16u : kOOB;
      asm volatile("" : "+v"(off));
      r[j] = __builtin_amdgcn_raw_buffer_load_b128(rsT, off, 0, 0);
    }
    load_ids(l0 + kAhead);
    __builtin_amdgcn_sched_barrier(0);       // (every load of the batch is issued before the first add)
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      const uint32_t w[4] = {r[j].x, r[j].y, r[j].z, r[j].w};
      const bool start = l0 + j == 0, in = l0 + j < L;            // (uniform)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = __uint_as_float((e & 1) ? (w[e >> 1] & 0xffff0000u) : (w[e >> 1] << 16));
        acc[e] = start ? f : (in ? acc[e] + f : acc[e]);
      }
    }
  }
  const u32x4 o = {gemm::pack_bf16x2(acc[0], acc[1]), gemm::pack_bf16x2(acc[2], acc[3]),
                   gemm::pack_bf16x2(acc[4], acc[5]), gemm::pack_bf16x2(acc[6], acc[7])};
  __builtin_amdgcn_raw_buffer_store_b128(o, rsO, ooff, 0, 0);
}

}  // namespace

bool embedding_bag_supported(int64_t B, int64_t T, int64_t D, int64_t F, int64_t F0, bool ids64) {
  if (B < 0 || T < 1 || F < 1 || F0 < 0 || F0 > 1) return false;
  if (D % 8 != 0 || D < kEmbagMinD || D > kEmbagMaxD) return false;
  const int64_t lim = int64_t(1) << 31;
  if (F0 + F > 65535) return false;                               // gridDim.y
  return B * T * (ids64 ? 8 : 4) < lim && B * (F0 + F) * D * 2 < lim && B * (D / 8) < lim;
}

bool embedding_bag_feature_ok(int64_t row_base, int64_t V, int64_t first, int64_t L, int64_t rows, int64_t T,
                              int64_t D) {
  return row_base >= 0 && V >= 1 && row_base + V <= rows && V * D * 2 < (int64_t(1) << 31) && first >= 0 &&
         L >= 1 && L <= kEmbagMaxHot && first + L <= T;
}

hipError_t embedding_bag_launch(const void* ids, bool ids64, const uint16_t* blob, const int64_t* feat,
                                const uint16_t* dense, uint16_t* out, int64_t B, int64_t T, int64_t D, int64_t F,
                                hipStream_t s) {
  const int F0 = dense != nullptr ? 1 : 0;
  if (!embedding_bag_supported(B, T, D, F, F0, ids64)) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  EmbagArgs a;
  a.B = int(B); a.T = int(T); a.CH = int(D / 8); a.F = int(F); a.F0 = F0;
  a.ids_bytes = int(B * T * (ids64 ? 8 : 4));
  a.dense_bytes = F0 ? int(B * D * 2) : 0;
  a.out_bytes = int(B * (F0 + F) * D * 2);
  const dim3 grid(unsigned((B * (D / 8) + 255) / 256), unsigned(F0 + F));
  if (ids64)
    hipLaunchKernelGGL(embedding_bag_kernel<true>, grid, dim3(256), 0, s, ids, blob, feat, dense, out, a);
  else
    hipLaunchKernelGGL(embedding_bag_kernel<false>, grid, dim3(256), 0, s, ids, blob, feat, dense, out, a);
  return hipGetLastError();
}

}  // namespace tfsk
