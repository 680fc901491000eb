// Grouped 3 x 3 convolution on the matrix cores (gfx950), NHWC bf16 in and out:
// y[n][ho][wo][g*Cg + o] = act(bias[g*Cg + o] + sum_{kh,kw,i} x[n][ho*S-PT+kh][wo*S-PL+kw][g*Cg + i] * w[kh][kw][i][g*Cg + o])
// with Cg = C / groups inputs AND outputs per group, Cg in {4, 8, 16, 32}
// (ResNeXt 32x4d's four stages, RegNet's group widths), stride S = 1 or 2.
// The filter (BatchNorm folded in) is bf16, the bias fp32; the sums are fp32
// MFMA accumulators, then bias, activation (none or ReLU) and one
// round-to-nearest-even store to bf16.
//
// One GEMM per (16 output pixels of a row, group) on v_mfma_f32_16x16x32_bf16:
// M = 16 pixels, N = Cg (one 16-column tile, two for Cg = 32), K = 9 Cg in
// (tap, channel) order, rounded up to a multiple of 32:
//   * lane l holds A[pixel l & 15][k = 32 ks + 8 (l >> 4) + j]: for Cg >= 8 one
//     16-B chunk of one halo pixel (Cg = 8: tap 4 ks + (l >> 4); Cg = 16: half
//     a tap; Cg = 32: a quarter of tap ks), for Cg = 4 two 8-B halves (taps
//     2 c and 2 c + 1 of chunk c = 4 ks + (l >> 4));
//   * the K slots past 9 Cg are zero in BOTH operands: a select on the A side
//     (the clamped tap that was read may hold Inf), zeros packed on the host on
//     the B side;
//   * for Cg < 16 the B columns past Cg are zero and their results are never
//     stored.  A group's activations meet that group's weights only -- no
//     block-diagonal filter, no product of another group's input with a
//     structural zero (0 x Inf = NaN would leak across groups).
//
// The op is bandwidth-bound (2.9 GFLOP against 51 MB at ResNeXt-50 stage 1,
// batch 32), so a workgroup reads its input once and writes its output once:
//   * a workgroup (4 waves) owns TH x 16 output pixels (TH = 8 at stride 1, 4
//     at stride 2) of a slab of 32 channels (32 / Cg whole groups);
//   * the ((TH-1) S + 3) x (15 S + 3) halo of the slab is loaded with
//     unconditional 16-B buffer loads -- a pixel outside the image, or a chunk
//     past C in the last slab, gets an out-of-range offset and reads zeros --
//     and staged in LDS, 80 B per pixel (64 B of channels + 16 B of padding:
//     sixteen neighbouring pixels' 16-B chunks then cover all 64 banks);
//   * the nine taps are shifted LDS reads of that halo;
//   * the weights never pass through LDS: they are packed on the host in
//     fragment order, [group][k-step][column tile][lane][8], and a wave loads
//     its B fragments once per group with 16-B buffer loads, contiguous across
//     the wave (they stay L2-resident: 9 Cg C bf16 before the padding);
//   * the results go through an LDS image of the output tile so that they
//     leave as 16-B chunks, four per pixel, with unconditional buffer stores:
//     a pixel past Ho / Wo or a chunk past C gets an offset the descriptor
//     drops.
// No atomics, no split accumulation: results are bit-for-bit reproducible.
#include "common.h"
#include "launch.h"

namespace tfsk {

namespace {

constexpr uint32_t kOob = 0x80000000u;    // beyond every descriptor below (operands are < 2 GiB)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kTW = 16;                   // output pixels of a row per MFMA tile
constexpr int kPix = 80;                  // LDS bytes per pixel: kGconvSlab channels + 16 B (bank spread)

struct GcArgs {
  const uint16_t* x;
  const uint16_t* w;
  const float* bias;
  uint16_t* y;
  int N, H, W, C, PT, PL, Ho, Wo, tilesH, tilesW, slabs;
  long wbytes;
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(const void* p, long bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, int(bytes), 0x00020000);
}

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

// grid: xcd_remap(x) = ((n * tilesH + th) * tilesW + tw) * slabs + slab
template <int S, int CG, int ACT>
__global__ __launch_bounds__(kThreads) void gconv3x3_kernel(GcArgs p) {
  constexpr int TH = S == 1 ? 8 : 4;
  constexpr int HH = (TH - 1) * S + 3, HW = (kTW - 1) * S + 3;
  constexpr int HPIX = (HH * HW + 63) / 64 * 64;          // whole rounds of the 256 loader threads
  constexpr int LI = HPIX * 4 / kThreads;
  constexpr int KS = gconv_ksteps(CG);
  constexpr int NT = CG == 32 ? 2 : 1;
  constexpr int GPS = kGconvSlab / CG;                     // groups of a slab
  constexpr int RW = TH * NT / kWaves;                     // rows of a wave
  __shared__ __attribute__((aligned(16))) unsigned char halo[HPIX * kPix];
  __shared__ __attribute__((aligned(16))) unsigned char tile[TH * kTW * kPix];

  const int tid = threadIdx.x;
  // the slabs of a pixel tile share 128-B lines (a slab is 64 B of a pixel), neighbouring tiles their
  // halos: consecutive logical ids go to one XCD, so that one L2 serves them
  int t = xcd_remap(int(blockIdx.x), int(gridDim.x));
  const int slab = t % p.slabs;
  t /= p.slabs;
  const int tw = t % p.tilesW;
  t /= p.tilesW;
  const int th = t % p.tilesH;
  const int n = t / p.tilesH;
  const int ho0 = th * TH, wo0 = tw * kTW;
  const int hi0 = ho0 * S - p.PT, wi0 = wo0 * S - p.PL;
  const int c0 = slab * kGconvSlab;

  const __amdgpu_buffer_rsrc_t rsX = rsrc_of(p.x, long(p.N) * p.H * p.W * p.C * 2);
  const __amdgpu_buffer_rsrc_t rsW = rsrc_of(p.w, p.wbytes);
  const __amdgpu_buffer_rsrc_t rsB = rsrc_of(p.bias, long(p.C) * 4);
  const __amdgpu_buffer_rsrc_t rsY = rsrc_of(p.y, long(p.N) * p.Ho * p.Wo * p.C * 2);

  // ---- the halo: every load first, then the LDS writes
  u32x4 hv[LI];
#pragma unroll
  for (int it = 0; it < LI; ++it) {
    const int i = tid + it * kThreads;
    const int pix = i >> 2, ch = i & 3;
    const int hy = pix / HW, hx = pix - hy * HW;
    const int hi = hi0 + hy, wi = wi0 + hx;
    const bool ok = hy < HH && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W && c0 + ch * 8 < p.C;
    const uint32_t off = (uint32_t((n * p.H + hi) * p.W + wi) * uint32_t(p.C) + uint32_t(c0 + ch * 8)) * 2u;
    hv[it] = __builtin_amdgcn_raw_buffer_load_b128(rsX, ok ? off : kOob, 0, 0);
  }
#pragma unroll
  for (int it = 0; it < LI; ++it) {
    const int i = tid + it * kThreads;
    *reinterpret_cast<u32x4*>(halo + (i >> 2) * kPix + (i & 3) * 16) = hv[it];
  }

  const int lane = tid & (kWave - 1), wave = tid >> 6;
  const int m = lane & 15, q = lane >> 4;
  const int nt = NT == 2 ? (wave & 1) : 0;
  const int r0 = NT == 2 ? (wave >> 1) : wave;             // rows r0 + i * (kWaves / NT)

  // a lane's LDS offset and validity per k-step (second half-chunk for Cg = 4)
  uint32_t aoff[KS], aoff2[KS];
  bool aok[KS], aok2[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int ci = ks * 4 + q;
    int tap, tap2 = 0, coff;
    if constexpr (CG == 32) { tap = ks; coff = q * 16; }
    else if constexpr (CG == 16) { tap = ci >> 1; coff = (ci & 1) * 16; }
    else if constexpr (CG == 8) { tap = ci; coff = 0; }
    else { tap = 2 * ci; tap2 = 2 * ci + 1; coff = 0; }
    aok[ks] = tap < 9;
    aok2[ks] = tap2 < 9;
    tap = aok[ks] ? tap : 0;
    tap2 = aok2[ks] ? tap2 : 0;
    aoff[ks] = uint32_t(((tap / 3) * HW + tap % 3 + m * S) * kPix + coff);
    aoff2[ks] = uint32_t(((tap2 / 3) * HW + tap2 % 3 + m * S) * kPix + coff);
  }
  __syncthreads();

#pragma unroll
  for (int gi = 0; gi < GPS; ++gi) {
    const int g = slab * GPS + gi;
    const bool glive = c0 + gi * CG < p.C;                 // (the last slab may hold fewer groups)
    // B fragments of the group, and the lane's bias
    u32x4 bfr[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const uint32_t off = uint32_t(((g * KS + ks) * NT + nt) * kWave + lane) * 16u;
      bfr[ks] = __builtin_amdgcn_raw_buffer_load_b128(rsW, glive ? off : kOob, 0, 0);
    }
    const int col = nt * 16 + m;                           // the lane's output channel within the group
    const bool colok = col < CG;
    const int cs = gi * CG + col;                          // ... within the slab
    const float bv = __uint_as_float(
        __builtin_amdgcn_raw_buffer_load_b32(rsB, colok && glive ? uint32_t(c0 + cs) * 4u : kOob, 0, 0));
#pragma unroll
    for (int i = 0; i < RW; ++i) {
      const int r = r0 + i * (kWaves / NT);
      const unsigned char* base = halo + r * S * HW * kPix + gi * CG * 2;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        u32x4 a;
        if constexpr (CG == 4) {
          const u32x2 lo = *reinterpret_cast<const u32x2*>(base + aoff[ks]);
          const u32x2 hi = *reinterpret_cast<const u32x2*>(base + aoff2[ks]);
          a[0] = aok[ks] ? lo[0] : 0u;
          a[1] = aok[ks] ? lo[1] : 0u;
          a[2] = aok2[ks] ? hi[0] : 0u;
          a[3] = aok2[ks] ? hi[1] : 0u;
        } else {
          a = *reinterpret_cast<const u32x4*>(base + aoff[ks]);
          if constexpr (9 * CG % 32 != 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = aok[ks] ? a[e] : 0u;
          }
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                      __builtin_bit_cast(bf16x8, bfr[ks]), acc, 0, 0, 0);
      }
      // C: column (channel) = lane & 15, pixel = 4 (lane >> 4) + e
      if (colok) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          *reinterpret_cast<uint16_t*>(tile + (r * kTW + q * 4 + e) * kPix + cs * 2) =
              f32_to_bf16(act_fn<ACT>(acc[e] + bv));
      }
    }
  }
  __syncthreads();

  // ---- the output tile: four 16-B chunks per pixel
  constexpr int SI = TH * kTW * 4 / kThreads;
#pragma unroll
  for (int it = 0; it < SI; ++it) {
    const int i = tid + it * kThreads;
    const int pix = i >> 2, ch = i & 3;
    const int ho = ho0 + pix / kTW, wo = wo0 + pix % kTW;
    const bool live = ho < p.Ho && wo < p.Wo && c0 + ch * 8 < p.C;
    const uint32_t off = (uint32_t((n * p.Ho + ho) * p.Wo + wo) * uint32_t(p.C) + uint32_t(c0 + ch * 8)) * 2u;
    const u32x4 v = *reinterpret_cast<const u32x4*>(tile + pix * kPix + ch * 16);
    __builtin_amdgcn_raw_buffer_store_b128(v, rsY, live ? off : kOob, 0, 0);
  }
}

template <int S, int CG>
void launch_act(const GcArgs& a, int act, dim3 grid, hipStream_t s) {
  if (act == kActRelu) hipLaunchKernelGGL((gconv3x3_kernel<S, CG, kActRelu>), grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL((gconv3x3_kernel<S, CG, kActNone>), grid, dim3(kThreads), 0, s, a);
}

template <int S>
void launch_cg(const GcArgs& a, int cg, int act, dim3 grid, hipStream_t s) {
  switch (cg) {
    case 4: launch_act<S, 4>(a, act, grid, s); break;
    case 8: launch_act<S, 8>(a, act, grid, s); break;
    case 16: launch_act<S, 16>(a, act, grid, s); break;
    default: launch_act<S, 32>(a, act, grid, s); break;
  }
}

}  // namespace

bool gconv_supported(int C, int CGin, int CGout, int KH, int KW, int SH, int SW) {
  return KH == 3 && KW == 3 && SH == SW && (SH == 1 || SH == 2) && CGin == CGout &&
         (CGin == 4 || CGin == 8 || CGin == 16 || CGin == 32) && C > 0 && C % 8 == 0 && C % CGin == 0;
}

long gconv_packed_elems(int C, int CG) {
  return long(C / CG) * gconv_ksteps(CG) * (CG == 32 ? 2 : 1) * kWave * 8;
}

hipError_t gconv_nhwc_launch(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* y, int N, int H, int W,
                             int C, int CGin, int CGout, int KH, int KW, int SH, int SW, int PT, int PL, int Ho,
                             int Wo, int act, hipStream_t s) {
  if (act != kActNone && act != kActRelu) return hipErrorInvalidValue;
  if (!gconv_supported(C, CGin, CGout, KH, KW, SH, SW)) return hipErrorInvalidValue;
  if (PT < 0 || PL < 0 || H <= 0 || W <= 0 || N < 0 || Ho < 0 || Wo < 0) return hipErrorInvalidValue;
  if (N == 0 || Ho == 0 || Wo == 0) return hipSuccess;
  // 32-bit byte offsets; kOob must lie beyond every operand
  if (long(N) * H * W * C * 2 >= 0x7ffffff0L || long(N) * Ho * Wo * C * 2 >= 0x7ffffff0L) return hipErrorInvalidValue;
  const int TH = SH == 1 ? 8 : 4;
  const int tilesH = (Ho + TH - 1) / TH, tilesW = (Wo + kTW - 1) / kTW;
  const int slabs = (C + kGconvSlab - 1) / kGconvSlab;
  const long blocks = long(N) * tilesH * tilesW * slabs;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const GcArgs a{x, w, bias, y, N, H, W, C, PT, PL, Ho, Wo, tilesH, tilesW, slabs, gconv_packed_elems(C, CGin) * 2};
  const dim3 grid{unsigned(blocks)};
  if (SH == 1) launch_cg<1>(a, CGin, act, grid, s);
  else launch_cg<2>(a, CGin, act, grid, s);
  return hipGetLastError();
}

}  // namespace tfsk
