// Pipelined MFMA conv/GEMM (cgemm.hip): the fast path for 64-aligned operands.
#pragma once
#include "launch.h"

namespace tfsk {

// One `cfg` integer selects a config of either kernel family (and of igemm):
// the rows of tile_configs.h.  The cgemm ids cover cgemm.hip (plain and
// fragment-prefetch builds), cgemm32.hip and bgemm.hip.
inline bool cgemm_cfg_id(int cfg) {
  const TileConfig* c = tile_config(cfg);
  return c != nullptr && cgemm_family(c->family);
}

// Operand requirements (else cgemm_launch returns hipErrorInvalidValue):
//   dense (a_mode kADense): K % 64 == 0, lda % 8 == 0;
//   im2col (kAIm2col): C % 64 == 0 (a k-tile is one filter tap x 64 channels), KH*KW <= 32;
//   stem (kAC4): zero-bordered bf16 RGBA input (no conv padding), KW == 8, KH even;
//   dual (kADual): see IGemmArgs::a2;
//   weights: ldb % 8 == 0, ldb >= K;  epilogue: N, ldc (and ldr) % 8 == 0.
bool cgemm_supported(const IGemmArgs& a, int a_mode);
int cgemm_config_bm(int cfg);
int cgemm_config_bn(int cfg);
hipError_t cgemm_launch(const IGemmArgs& a, int a_mode, int cfg, hipStream_t stream);
// the 32x32x16 builds (cgemm32.hip) and the big-tile ping-pong builds
// (bgemm.hip) of their config ids; cgemm_launch dispatches to them
hipError_t cgemm32_launch(const IGemmArgs& a, int a_mode, int cfg, hipStream_t stream);
hipError_t bgemm_launch(const IGemmArgs& a, int a_mode, int cfg, hipStream_t stream);
// the config can finish split-K in-kernel (IGemmArgs::counters)
bool cgemm_fixup_ok(int cfg);
// workgroups (= tiles) of a halo launch (its split-K counters)
long halo_tiles(const IGemmArgs& a, int cfg);

// Halo-tiled 3x3 stride-1 conv (halo.hip): an NHWC bf16 input with C % 64 == 0
// and the im2col weight layout ([Cout][9 * C]); the workgroup tile is a block
// of output pixels (TH x TW, picked by the launcher) x a BN slice of Cout.
// Split-K splits the channel chunks (kt_per_split counts 64-channel chunks).
// The halo ids: the plain and fragment-prefetch builds and the persistent
// kernel (halo_persist_kernel).
inline bool halo_cfg_id(int cfg) {
  const TileConfig* c = tile_config(cfg);
  return c != nullptr && halo_family(c->family);
}
// host-only, launches nothing: the tile walk the persistent kernel's launcher
// uses for n images of ho x wo output pixels (tiles of ti images x th x tw
// pixels; the grid is min(tiles, CUs)).  false: no such launch.
bool halo_persist_tiles(int n, int ho, int wo, long& tiles, int& th, int& tw, int& ti);
bool halo_supported(const IGemmArgs& a);
int halo_config_bm(int cfg);
int halo_config_bn(int cfg);
hipError_t halo_launch(const IGemmArgs& a, int cfg, hipStream_t stream);

}  // namespace tfsk
