// 32x32x16 MFMA builds of the pipelined conv / GEMM kernel (the
// TFSK_CGEMM32_CONFIGS rows; cgemm_launch dispatches here).  Separate translation
// unit so the two families compile in parallel.
#include "cgemm_impl.h"

namespace tfsk {

namespace {

using cgemm_impl::launch_cfg;

template <int AM>
hipError_t launch_mode32(const IGemmArgs& a, int cfg, hipStream_t s) {
  switch (cfg) {
#define TFSK_CASE(id, BM, BN, WGM, WGN, S) \
  case id: return launch_cfg<BM, BN, WGM, WGN, S, AM, false, 32>(a, s);
    TFSK_CGEMM32_CONFIGS(TFSK_CASE)
#undef TFSK_CASE
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t cgemm32_launch(const IGemmArgs& a, int a_mode, int cfg, hipStream_t s) {
  switch (a_mode) {
    case kAIm2col: return launch_mode32<1>(a, cfg, s);
    case kADual: return launch_mode32<2>(a, cfg, s);
    case kAC4: return launch_mode32<3>(a, cfg, s);
    default: return launch_mode32<0>(a, cfg, s);
  }
}

}  // namespace tfsk
