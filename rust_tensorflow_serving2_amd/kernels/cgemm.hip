// Pipelined MFMA conv / GEMM for MI355X (gfx950): bf16 operands, fp32 accumulate.
//
// C[M][N] = epilogue( A[M][K] * B[N][K]^T ), the same contract as igemm.hip, for
// the 64-aligned cases that make up almost all of ResNet-50 / BERT:
//   A dense row-major (K % 64 == 0), or the implicit im2col of an NHWC tensor
//   with C % 64 == 0, so one 64-deep k-tile is exactly one filter tap x 64
//   channels;  B = weights [Cout][ldb].
//
// Why a second kernel: rocprofv3 PMC of igemm on the ResNet 3x3 layers showed
// ~90 SALU+VALU instructions per 16 MFMAs and a vmcnt(0) drain every k-tile
// (SQ_ACTIVE_INST_ANY 44 %, SQ_WAIT_ANY 41 %, MFMA busy 11-16 % of wave
// cycles).  This kernel is built so the steady-state k-tile costs little more
// than its MFMAs:
//   * S-deep ring of direct-to-LDS DMAs (buffer_load ... lds): the wait before
//     tile t is a counted vmcnt((S-2) * pieces) — never a drain — followed by a
//     bare s_barrier;
//   * every per-lane DMA offset is precomputed once (voffset) and the k-tile
//     advance is a wave-uniform scalar (soffset): no VALU address math per tile;
//   * im2col padding = one precomputed tap-validity bit mask per DMA row
//     (3 VALU per piece), the tap walk runs in SGPRs, and the buffer
//     descriptor is rebased by the top/left padding so every in-image offset is
//     non-negative; invalid taps read through an out-of-range voffset (zeros);
//   * the loop is unrolled by S, so ring slots and all LDS fragment offsets
//     are compile-time immediates;
//   * LDS rows are 128 B with 16-B chunks XOR-swizzled by (row & 7): the DMA
//     lane writes slot l&7 of row l>>3 from source chunk (l&7)^(l>>3), the
//     ds_read_b128 fragment reads undo it (conflict-free);
//   * 4 or 8 waves per workgroup, each owning a WM x WN sub-tile of
//     v_mfma_f32_16x16x32_bf16 accumulators; bijective XCD-aware tile remap +
//     GROUP_M ordering; epilogue staged through LDS as fp32 for coalesced
//     16-B bias/residual/activation/store row chunks (residual prefetched into
//     registers before the K loop).
#include "cgemm_impl.h"

namespace tfsk {

namespace {

using namespace gemm;
using cgemm_impl::launch_cfg;

// The configs are the TFSK_CGEMM_CONFIGS / TFSK_CGEMM_PF_CONFIGS rows of
// tile_configs.h (tile BM x BN, wave grid, ring depth).
template <int AM>
hipError_t launch_mode_pf(const IGemmArgs& a, int cfg, hipStream_t s) {
  switch (cfg) {
#define TFSK_CASE(id, base, BM, BN, WGM, WGN, S) \
  case id: return launch_cfg<BM, BN, WGM, WGN, S, AM, true>(a, s);
    TFSK_CGEMM_PF_CONFIGS(TFSK_CASE)
#undef TFSK_CASE
    default: return hipErrorInvalidValue;
  }
}

template <int AM>
hipError_t launch_mode(const IGemmArgs& a, int cfg, hipStream_t s) {
  switch (cfg) {
#define TFSK_CASE(id, BM, BN, WGM, WGN, S) \
  case id: return launch_cfg<BM, BN, WGM, WGN, S, AM>(a, s);
    TFSK_CGEMM_CONFIGS(TFSK_CASE)
#undef TFSK_CASE
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

// (0 / false for an id that is not a cgemm config)
int cgemm_config_bm(int cfg) { return cgemm_cfg_id(cfg) ? tile_config(cfg)->bm : 0; }
int cgemm_config_bn(int cfg) { return cgemm_cfg_id(cfg) ? tile_config(cfg)->bn : 0; }

bool cgemm_fixup_ok(int cfg) {
  // bgemm has no in-kernel fixup
  if (!cgemm_cfg_id(cfg) || tile_config(cfg)->family == TileFamily::kBGemm) return false;
  // the in-kernel split-K fixup needs the whole fp32 tile in LDS at once (one pass)
  return size_t(cgemm_config_bm(cfg)) * (cgemm_config_bn(cfg) + 4) * 4 <= 160 * 1024;
}

bool cgemm_supported(const IGemmArgs& a, int a_mode) {
  if (a.K <= 0 || a.K % KT || a.ldb % 8 || a.ldb < a.K) return false;
  if (a.N % 8 || a.ldc % 8 || (a.residual && a.ldr % 8)) return false;   // 16-B epilogue chunks only
  if (a.M >= (1 << 23)) return false;   // fdiv() row-index decomposition is exact below 2^23
  if (a_mode == kADense) return a.lda % 8 == 0 && a.lda >= a.K;
  if (a_mode == kAIm2col)
    return a.C % KT == 0 && a.KH * a.KW <= 32 && a.K == a.KH * a.KW * a.C &&
           a.a_bytes + int64_t(a.PT * a.W + a.PL) * a.C * 2 < 0x7ffffff0LL;
  if (a_mode == kAC4)
    return a.C == 4 && a.KW == 8 && a.KH % 2 == 0 && a.K == a.KH * 32 && a.PT == 0 && a.PL == 0 &&
           a.H >= (a.Ho - 1) * a.SH + a.KH && a.W >= (a.Wo - 1) * a.SW + a.KW;
  if (a_mode == kADual)
    return a.a2 && a.K1 > 0 && a.K1 % KT == 0 && a.lda % 8 == 0 && a.lda >= a.K1 && a.C % KT == 0 &&
           a.K == a.K1 + a.C && a.KH == 1 && a.KW == 1 && a.PT == 0 && a.PL == 0 && a.a2_bytes < 0x7ffffff0LL;
  return false;
}


hipError_t cgemm_launch(const IGemmArgs& a, int a_mode, int cfg, hipStream_t s) {
  if (!cgemm_cfg_id(cfg) || !cgemm_supported(a, a_mode)) return hipErrorInvalidValue;
  const TileFamily family = tile_config(cfg)->family;
  if (family == TileFamily::kBGemm) return bgemm_launch(a, a_mode, cfg, s);
  if (family == TileFamily::kCGemm32) return cgemm32_launch(a, a_mode, cfg, s);
  if (family == TileFamily::kCGemmPf) {
    switch (a_mode) {
      case kAIm2col: return launch_mode_pf<1>(a, cfg, s);
      case kADual: return launch_mode_pf<2>(a, cfg, s);
      case kAC4: return launch_mode_pf<3>(a, cfg, s);
      default: return launch_mode_pf<0>(a, cfg, s);
    }
  }
  switch (a_mode) {
    case kAIm2col: return launch_mode<1>(a, cfg, s);
    case kADual: return launch_mode<2>(a, cfg, s);
    case kAC4: return launch_mode<3>(a, cfg, s);
    default: return launch_mode<0>(a, cfg, s);
  }
}

}  // namespace tfsk
