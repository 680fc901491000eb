// torch bindings of the gfx950 kernels (`_hip`).  (ROCm torch exposes HIP
// devices as "cuda": guards/streams use the MasqueradingAsCUDA variants.)  Every op launches on the
// caller's current HIP stream, allocates nothing inside the launch function
// beyond the output tensor (so callers can capture them in HIP graphs with
// pre-allocated outputs via the `out=` forms), and validates shapes on the host
// before anything touches the GPU.
#include <cstdlib>
#include <cmath>
#include <algorithm>
#include <torch/extension.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include "common.h"
#include "launch.h"
#include "cgemm.h"

namespace {

using torch::Tensor;

hipStream_t cur_stream(const Tensor& t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

void check(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, what, ": ", hipGetErrorString(e));
}

// Launch with optional split-K: raw fp32 slabs in a workspace + reduce/epilogue kernel.
// `cfg` is a row of tile_configs.h: an igemm.hip config (any operand mode), a
// cgemm one (the pipelined kernels, 64-aligned operands) or a halo one (the
// halo-tiled 3x3 stride-1 conv).  nullptr: not a config.
const tfsk::TileConfig* config_of(int64_t cfg) {
  return cfg >= 0 && cfg < tfsk::kTileIdEnd ? tfsk::tile_config(int(cfg)) : nullptr;
}
bool is_cgemm_cfg(int64_t cfg) { return config_of(cfg) != nullptr && tfsk::cgemm_family(config_of(cfg)->family); }
bool is_halo_cfg(int64_t cfg) { return config_of(cfg) != nullptr && tfsk::halo_family(config_of(cfg)->family); }

hipError_t launch_any(const tfsk::IGemmArgs& a, int a_mode, int64_t cfg, hipStream_t st) {
  if (is_halo_cfg(cfg)) return tfsk::halo_launch(a, int(cfg), st);
  return is_cgemm_cfg(cfg) ? tfsk::cgemm_launch(a, a_mode, int(cfg), st) : tfsk::igemm_launch(a, a_mode, int(cfg), st);
}

// Split-K finishing in-kernel (the last slice of a tile sums the slabs and
// runs the epilogue; no reduce launch).  TFSERVE_SPLITK_FIXUP: "1" always,
// "0" never.  Otherwise the serving runtime decides per batch bucket while it
// tunes and captures (set_splitk_fixup: on for the small buckets, whose few
// workgroups each run a long K loop -- b1 0.371-0.374 vs 0.391-0.394 ms per
// replay -- off for the large ones, where the write-through slab traffic cost
// more than the reduce launch when every small launch used it: b32 0.816-0.824 vs 0.780-0.786 ms; per bucket: 0.771-0.773 vs 0.781-0.794,
// profiles/round4/s13), and outside that launches of fewer than
// kFixupAutoTiles tiles use it.
constexpr long kFixupAutoTiles = 128;
// per thread: the serving runtime sets it around ONE bucket's tuning + capture
// on the capturing thread; eager launches of other threads (another
// servable's warm-up / tuning) keep the default rule and never take eager
// ring slices under a capture's mode
thread_local int g_fixup_override = -1;
int split_fixup_mode() {
  const char* v = std::getenv("TFSERVE_SPLITK_FIXUP");
  if (v && v[0] == '1') return 1;
  if (v && v[0] == '0') return 0;
  if (g_fixup_override >= 0) return g_fixup_override;
  return 2;
}

// scripts/wg_trace.py: per-workgroup phase stamps of the next GEMM / conv
// launches (a device int64 buffer of 8 per workgroup; None turns it off)
long long* g_trace = nullptr;
int g_trace_cap = 0;

void run_igemm(tfsk::IGemmArgs& a, int a_mode, int64_t cfg, int64_t splits, const Tensor& like, hipStream_t st) {
  a.trace = g_trace;
  a.trace_cap = g_trace_cap;
  TORCH_CHECK(config_of(cfg) != nullptr, "bad tile config ", cfg);
  TORCH_CHECK(!is_cgemm_cfg(cfg) || tfsk::cgemm_supported(a, a_mode),
              "tile config ", cfg, " needs 64-aligned operands (K % 64, C % 64)");
  TORCH_CHECK(!is_halo_cfg(cfg) || (a_mode == tfsk::kAIm2col && tfsk::halo_supported(a)),
              "halo config ", cfg, " needs a 3x3 stride-1 conv with C % 64 == 0");
  // split-K granule: 64-deep k-tiles, or 64-channel chunks (9 taps each) for the halo conv
  const int nk = is_halo_cfg(cfg) ? a.C / 64 : (a.K + 63) / 64;
  if (splits > nk) splits = nk;
  if (splits <= 1) {
    a.splits = 1;
    a.kt_per_split = nk;
    a.ws = nullptr;
    TORCH_CHECK(launch_any(a, a_mode, cfg, st) == hipSuccess, "conv/GEMM launch failed");
    return;
  }
  const int per = (nk + splits - 1) / splits;
  splits = (nk + per - 1) / per;
  Tensor ws = torch::empty({splits * int64_t(a.M) * a.N}, like.options().dtype(at::kFloat));
  a.splits = int(splits);
  a.kt_per_split = per;
  a.ws = ws.data_ptr<float>();
  // With the fixup on (split_fixup_mode: launches under kFixupAutoTiles tiles by default) cgemm /
  // halo finish split-K in-kernel (the last slice of each tile reduces): one
  // launch instead of two; eager launches (autotuning) then use the fixup too,
  // so the tuner times the split-K candidates as the graph runs them.
  // Otherwise, or when no counters are left, a separate reduce launch.
  a.counters = nullptr;
  const int fixup = split_fixup_mode();
  if (fixup != 0 && a.N % 8 == 0 && ((is_cgemm_cfg(cfg) && tfsk::cgemm_fixup_ok(int(cfg))) || is_halo_cfg(cfg))) {
    long tiles = 0;
    if (is_halo_cfg(cfg)) {
      tiles = tfsk::halo_tiles(a, int(cfg));
    } else {
      const int bm = tfsk::cgemm_config_bm(int(cfg)), bn = tfsk::cgemm_config_bn(int(cfg));
      tiles = long((a.M + bm - 1) / bm) * ((a.N + bn - 1) / bn);
    }
    if (tiles > 0 && tiles < (1L << 24) && (fixup == 1 || tiles < kFixupAutoTiles)) {
      tfsk::splitk_counters_prepare(st);
      a.counters = tfsk::splitk_counters(int(tiles), st);
    }
  }
  TORCH_CHECK(launch_any(a, a_mode, cfg, st) == hipSuccess, "conv/GEMM (split-K) launch failed");
  if (a.counters == nullptr)
    TORCH_CHECK(tfsk::splitk_reduce_launch(a, st) == hipSuccess, "split-K reduce launch failed");
}

void need(const Tensor& t, at::ScalarType st, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == st, name, " has dtype ", t.scalar_type(), ", expected ", st);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

bool aligned16(const Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }

const uint16_t* bf16p(const Tensor& t) { return reinterpret_cast<const uint16_t*>(t.data_ptr()); }

// An activation code the kernels do not implement is an error, never "none"
// (their switches send unknown codes to the default case).  Every GEMM / conv
// family implements the codes up to kActTanh.  ReLU6 is built into igemm
// (which takes every shape) and the split-K reduce only: with the extra case
// in their epilogue switches 61 of the cgemm kernels spilled more registers
// (profiles/dwconv/resources_before_after.txt), and bgemm and halo are kept
// byte-identical for the ResNet / BERT engines.  A relu6 launch on one of
// their configs is rejected here, and ops.candidates(relu6=True) offers igemm
// configs only.  The deferred-LayerNorm epilogue has no ReLU6 either, and the
// post-activation outputs (act2, the max-pool's) are none / ReLU only.
// Hard-swish (code 7) shares all of this: built where ReLU6 is, rejected where
// ReLU6 is.  relu6_cfg answers for both "igemm-only" activations.  Hard-sigmoid
// (code 6) is a gate activation of se.hip: no GEMM / conv epilogue takes it.
// Swish (code 9) is the third igemm-only activation, and sigmoid (code 8) the
// second gate-only one.
bool relu6_cfg(int64_t cfg) {
  return config_of(cfg) != nullptr && config_of(cfg)->family == tfsk::TileFamily::kIGemm;
}
void need_act(int64_t act, int64_t cfg, const char* op) {
  TORCH_CHECK((act >= tfsk::kActNone && act <= tfsk::kActRelu6) || act == tfsk::kActHardSwish ||
              act == tfsk::kActSwish, op, ": unknown activation code ", act);
  const bool igemm_only = act == tfsk::kActRelu6 || act == tfsk::kActHardSwish || act == tfsk::kActSwish;
  TORCH_CHECK(!igemm_only || config_of(cfg) == nullptr || relu6_cfg(cfg), op, ": activation ",
              act == tfsk::kActRelu6 ? "relu6" : act == tfsk::kActHardSwish ? "hard_swish" : "swish",
              " is built into the igemm kernels only (tile config ", cfg, " is not one)");
}
void need_post_act(int64_t act, const char* op) {
  TORCH_CHECK(act == tfsk::kActNone || act == tfsk::kActRelu, op, ": the post activation is none (0) or relu (1), got ",
              act);
}

// Post-activation output (ResNet v2): out2 = act2(y * scale + shift) per output
// channel, written by the same GEMM epilogue.  post_only: `y` itself receives
// the post-activated values (the raw sum is not stored).  cgemm / halo configs
// (or split-K, whose reduce applies the epilogue) only.
void set_post(tfsk::IGemmArgs& a, const c10::optional<Tensor>& scale, const c10::optional<Tensor>& shift,
              int64_t act2, const c10::optional<Tensor>& out2, bool post_only, const Tensor& y, int64_t cfg,
              int64_t splits, int cout) {
  if (!scale.has_value()) {
    TORCH_CHECK(!shift.has_value() && !out2.has_value() && !post_only, "post output needs post_scale");
    return;
  }
  TORCH_CHECK(shift.has_value(), "post_scale needs post_shift");
  need_post_act(act2, "conv");
  need(*scale, at::kFloat, "post_scale");
  need(*shift, at::kFloat, "post_shift");
  TORCH_CHECK(scale->numel() == cout && shift->numel() == cout, "post scale / shift must have Cout entries");
  TORCH_CHECK(aligned16(*scale) && aligned16(*shift), "post scale / shift must be 16-B aligned");
  TORCH_CHECK(is_cgemm_cfg(cfg) || is_halo_cfg(cfg) || splits > 1,
              "the post-activation output needs a cgemm / halo config");
  a.scale2 = scale->data_ptr<float>();
  a.shift2 = shift->data_ptr<float>();
  a.act2 = int(act2);
  if (post_only) {
    TORCH_CHECK(!out2.has_value(), "post_only writes the post output to `out`");
    a.out2 = y.data_ptr();
    a.out = nullptr;
  } else {
    TORCH_CHECK(out2.has_value(), "dual output needs out2");
    TORCH_CHECK(out2->scalar_type() == y.scalar_type() && out2->numel() == y.numel() && out2->is_contiguous(),
                "out2 must match the output");
    a.out2 = out2->data_ptr();
  }
}
uint16_t* bf16p_mut(const Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

// x: NHWC bf16 (or fp32 when stem=true), w: [Cout][ldb] bf16, bias: [Cout] f32
Tensor conv2d(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& bias,
              const c10::optional<Tensor>& residual, int64_t KH, int64_t KW, int64_t SH, int64_t SW,
              int64_t PT, int64_t PB, int64_t PL, int64_t PR, int64_t act, int64_t cfg,
              const c10::optional<Tensor>& out, bool out_f32, int64_t splits,
              const c10::optional<Tensor>& post_scale, const c10::optional<Tensor>& post_shift, int64_t post_act,
              const c10::optional<Tensor>& out2, bool post_only) {
  const bool stem = x.scalar_type() == at::kFloat;
  need_act(act, cfg, "conv2d");
  need(x, stem ? at::kFloat : at::kBFloat16, "x");
  need(w, at::kBFloat16, "w");
  TORCH_CHECK(x.dim() == 4, "x must be NHWC");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int Ho = (H + PT + PB - KH) / SH + 1, Wo = (W + PL + PR - KW) / SW + 1;
  TORCH_CHECK(Ho > 0 && Wo > 0, "empty conv output");
  const int Cout = w.size(0), ldb = w.size(1);
  const bool c4 = !stem && C == 4;
  TORCH_CHECK(!c4 || KW <= 8, "4-channel (RGBA) conv supports KW <= 8");
  const int K = c4 ? KH * 32 : KH * KW * C;   // c4 weights: [Cout][kh][8 taps][4 ch]
  TORCH_CHECK(ldb >= K && ldb % 8 == 0, "weight rows must hold K=", K, " (padded to a multiple of 8)");
  int a_mode;
  if (stem) {
    a_mode = (C == 3 && KH == 7 && KW == 7) ? tfsk::kAStem7x7x3 : tfsk::kAStemF32;
  } else if (c4) {
    a_mode = tfsk::kAC4;
  } else {
    TORCH_CHECK(C % 8 == 0, "conv input channels must be a multiple of 8 (got ", C, ")");
    a_mode = (KH == 1 && KW == 1 && SH == 1 && SW == 1 && PT == 0 && PL == 0) ? tfsk::kADense : tfsk::kAIm2col;
  }
  Tensor y = out.has_value() ? *out
                             : torch::empty({N, Ho, Wo, Cout}, x.options().dtype(out_f32 ? at::kFloat : at::kBFloat16));
  need(y, out_f32 ? at::kFloat : at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == int64_t(N) * Ho * Wo * Cout, "out has the wrong size");
  tfsk::IGemmArgs a{};
  a.a = x.data_ptr();
  a.b = bf16p(w);
  a.a_bytes = x.numel() * x.element_size();
  a.b_bytes = w.numel() * 2;
  TORCH_CHECK(a.a_bytes < 0x7ffffff0LL && a.b_bytes < 0x7ffffff0LL, "conv operands must be < 2 GiB");
  a.M = N * Ho * Wo; a.N = Cout; a.K = K; a.lda = C; a.ldb = ldb;
  a.H = H; a.W = W; a.C = C; a.KH = KH; a.KW = KW; a.SH = SH; a.SW = SW; a.PT = PT; a.PL = PL;
  a.Ho = Ho; a.Wo = Wo;
  if (bias.has_value()) {
    need(*bias, at::kFloat, "bias");
    TORCH_CHECK(bias->numel() == Cout, "bias size");
    a.bias = bias->data_ptr<float>();
  }
  if (residual.has_value()) {
    need(*residual, at::kBFloat16, "residual");
    TORCH_CHECK(residual->numel() == y.numel(), "residual shape must match the output");
    a.residual = bf16p(*residual);
    a.ldr = Cout;
  }
  a.act = act; a.out = y.data_ptr(); a.ldc = Cout; a.out_f32 = out_f32; a.alpha = 1.f;
  set_post(a, post_scale, post_shift, post_act, out2, post_only, y, cfg, splits, Cout);
  run_igemm(a, a_mode, cfg, splits, x, cur_stream(x));
  return y;
}

// ResNet bottleneck tail in one GEMM: act(conv1x1(h) + conv1x1_stride(x) + bias)
// with w = [Cout][C_h + C_x] (expand weights | projection weights).
// h: NHWC [N][Ho][Wo][C_h] bf16 (dense rows), x: NHWC [N][H][W][C_x] bf16
// sampled at (ho*SH, wo*SW).  cgemm configs only (C_h, C_x % 64 == 0).
Tensor conv2d_dual(const Tensor& h, const Tensor& x, const Tensor& w, const c10::optional<Tensor>& bias,
                   int64_t SH, int64_t SW, int64_t act, int64_t cfg, const c10::optional<Tensor>& out, int64_t splits,
                   const c10::optional<Tensor>& post_scale, const c10::optional<Tensor>& post_shift,
                   int64_t post_act, const c10::optional<Tensor>& out2, bool post_only) {
  need_act(act, cfg, "conv2d_dual");
  need(h, at::kBFloat16, "h");
  need(x, at::kBFloat16, "x");
  need(w, at::kBFloat16, "w");
  TORCH_CHECK(h.dim() == 4 && x.dim() == 4 && h.size(0) == x.size(0), "conv2d_dual: NHWC h and x, same batch");
  TORCH_CHECK(is_cgemm_cfg(cfg), "conv2d_dual needs a cgemm tile config");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(h.device());
  const int N = h.size(0), Ho = h.size(1), Wo = h.size(2), C1 = h.size(3);
  const int H = x.size(1), W = x.size(2), C2 = x.size(3);
  TORCH_CHECK(SH >= 1 && SW >= 1 && (H - 1) / SH + 1 == Ho && (W - 1) / SW + 1 == Wo,
              "conv2d_dual: x sampled at stride (SH, SW) must give h's spatial size");
  const int Cout = w.size(0), ldb = w.size(1);
  TORCH_CHECK(ldb >= C1 + C2 && ldb % 8 == 0, "conv2d_dual: weights must hold K = C_h + C_x");
  Tensor y = out.has_value() ? *out : torch::empty({N, Ho, Wo, Cout}, h.options());
  need(y, at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == int64_t(N) * Ho * Wo * Cout, "out has the wrong size");
  tfsk::IGemmArgs a{};
  a.a = h.data_ptr(); a.a_bytes = h.numel() * 2;
  a.a2 = x.data_ptr(); a.a2_bytes = x.numel() * 2;
  a.b = bf16p(w); a.b_bytes = w.numel() * 2;
  TORCH_CHECK(a.a_bytes < 0x7ffffff0LL && a.a2_bytes < 0x7ffffff0LL && a.b_bytes < 0x7ffffff0LL,
              "conv2d_dual operands must be < 2 GiB");
  a.M = N * Ho * Wo; a.N = Cout; a.K = C1 + C2; a.K1 = C1; a.lda = C1; a.ldb = ldb;
  a.H = H; a.W = W; a.C = C2; a.KH = 1; a.KW = 1; a.SH = SH; a.SW = SW; a.PT = 0; a.PL = 0; a.Ho = Ho; a.Wo = Wo;
  if (bias.has_value()) {
    need(*bias, at::kFloat, "bias");
    TORCH_CHECK(bias->numel() == Cout, "bias size");
    a.bias = bias->data_ptr<float>();
  }
  a.act = act; a.out = y.data_ptr(); a.ldc = Cout; a.out_f32 = 0; a.alpha = 1.f;
  set_post(a, post_scale, post_shift, post_act, out2, post_only, y, cfg, splits, Cout);
  run_igemm(a, tfsk::kADual, cfg, splits, h, cur_stream(h));
  return y;
}

// x: [M][K] bf16 (any leading dims), w: [N][ldb] bf16 -> [.., N]
Tensor linear(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& bias,
              const c10::optional<Tensor>& residual, int64_t act, int64_t cfg, bool out_f32, double alpha,
              const c10::optional<Tensor>& out, int64_t splits) {
  // x: contiguous, or a row-strided 2-D view (x[r][k] at r * lda + k; e.g.
  // BERT's pooler reads every sequence's first token straight from [B, S, H])
  need_act(act, cfg, "linear");
  const bool strided = !x.is_contiguous();
  if (strided) {
    TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2 && x.stride(1) == 1 &&
                    x.stride(0) >= x.size(1) && x.stride(0) % 8 == 0,
                "x must be contiguous or a row-strided 2-D bf16 view");
  } else {
    need(x, at::kBFloat16, "x");
  }
  need(w, at::kBFloat16, "w");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  const int K = x.size(-1);
  const int M = x.numel() / K;
  const int lda = strided ? int(x.stride(0)) : K;
  const int N = w.size(0), ldb = w.size(1);
  TORCH_CHECK(ldb >= K && K % 8 == 0 && ldb % 8 == 0, "linear: K must be a multiple of 8 and fit in w");
  auto sizes = x.sizes().vec();
  sizes.back() = N;
  Tensor y = out.has_value() ? *out : torch::empty(sizes, x.options().dtype(out_f32 ? at::kFloat : at::kBFloat16));
  need(y, out_f32 ? at::kFloat : at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == int64_t(M) * N, "out has the wrong size");
  tfsk::IGemmArgs a{};
  a.a = x.data_ptr(); a.b = bf16p(w);
  a.a_bytes = M > 0 ? (int64_t(M - 1) * lda + K) * 2 : 0;
  a.b_bytes = w.numel() * 2;
  TORCH_CHECK(a.a_bytes < 0x7ffffff0LL && a.b_bytes < 0x7ffffff0LL, "linear operands must be < 2 GiB");
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb;
  if (bias.has_value()) {
    need(*bias, at::kFloat, "bias");
    TORCH_CHECK(bias->numel() == N, "bias size");
    a.bias = bias->data_ptr<float>();
  }
  if (residual.has_value()) {
    need(*residual, at::kBFloat16, "residual");
    TORCH_CHECK(residual->numel() == y.numel(), "residual shape must match the output");
    a.residual = bf16p(*residual);
    a.ldr = N;
  }
  a.act = act; a.out = y.data_ptr(); a.ldc = N; a.out_f32 = out_f32; a.alpha = float(alpha);
  run_igemm(a, tfsk::kADense, cfg, splits, x, cur_stream(x));
  return y;
}


// Deferred-LayerNorm GEMM (graph/fused.py defer_layernorm): y = epilogue(x @
// w^T) where the rows of x (a_st) and / or of the residual (r_st) are sums
// whose LayerNorm was never stored -- their statistics come along as [M][P][2]
// (sum, sum sq) partials and the epilogue applies the normalisation (x's via
// the gamma-folded weights w, the beta-folded bias and a_colsum = per-column
// sums of w; the residual's via r_gamma / r_beta) -- and, with stats, y's own
// row partials are returned for the next consumer.  cgemm configs (not the
// persistent ones), one K slice.  Returns {y, y's partials (empty without stats)}.
std::vector<Tensor> linear_lnx(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& bias,
                               const c10::optional<Tensor>& residual, int64_t act, int64_t cfg, bool out_f32,
                               const c10::optional<Tensor>& out, const c10::optional<Tensor>& a_st,
                               const c10::optional<Tensor>& a_colsum, double a_eps,
                               const c10::optional<Tensor>& r_st, const c10::optional<Tensor>& r_gamma,
                               const c10::optional<Tensor>& r_beta, double r_eps, bool stats) {
  TORCH_CHECK(act >= tfsk::kActNone && act <= tfsk::kActTanh, "linear_lnx: unknown activation code ", act,
              " (the deferred-LayerNorm epilogue has no relu6, no hard_swish and no swish)");
  need(x, at::kBFloat16, "x");
  need(w, at::kBFloat16, "w");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  const int K = x.size(-1);
  const int M = x.numel() / K;
  const int N = w.size(0), ldb = w.size(1);
  TORCH_CHECK(ldb >= K && K % 64 == 0 && ldb % 8 == 0 && N % 8 == 0,
              "linear_lnx: K % 64 == 0 (fitting in w), N % 8 == 0");
  TORCH_CHECK(is_cgemm_cfg(cfg) && config_of(cfg)->family != tfsk::TileFamily::kBGemm,
              "linear_lnx: a cgemm tile config");
  TORCH_CHECK(!(stats && out_f32), "linear_lnx: row statistics of bf16 outputs only");
  auto sizes = x.sizes().vec();
  sizes.back() = N;
  Tensor y = out.has_value() ? *out : torch::empty(sizes, x.options().dtype(out_f32 ? at::kFloat : at::kBFloat16));
  need(y, out_f32 ? at::kFloat : at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == int64_t(M) * N, "out has the wrong size");
  auto parts_of = [&](const Tensor& t, const char* what) {
    need(t, at::kFloat, what);
    TORCH_CHECK(t.dim() == 3 && t.size(0) == M && t.size(2) == 2 && t.size(1) >= 1,
                "linear_lnx: ", what, " must be [M][parts][2]");
    return int(t.size(1));
  };
  auto vec_n = [&](const c10::optional<Tensor>& t, const char* what) {
    TORCH_CHECK(t.has_value(), "linear_lnx: ", what, " missing");
    need(*t, at::kFloat, what);
    TORCH_CHECK(t->numel() == N && aligned16(*t), "linear_lnx: ", what, " must be N floats, 16-B aligned");
    return t->data_ptr<float>();
  };
  tfsk::IGemmArgs a{};
  a.a = x.data_ptr(); a.b = bf16p(w);
  a.a_bytes = int64_t(M) * K * 2;
  a.b_bytes = w.numel() * 2;
  TORCH_CHECK(a.a_bytes < 0x7ffffff0LL && a.b_bytes < 0x7ffffff0LL, "linear_lnx operands must be < 2 GiB");
  a.M = M; a.N = N; a.K = K; a.lda = K; a.ldb = ldb;
  if (bias.has_value()) {
    need(*bias, at::kFloat, "bias");
    TORCH_CHECK(bias->numel() == N, "bias size");
    a.bias = bias->data_ptr<float>();
  }
  if (residual.has_value()) {
    need(*residual, at::kBFloat16, "residual");
    TORCH_CHECK(residual->numel() == y.numel(), "residual shape must match the output");
    a.residual = bf16p(*residual);
    a.ldr = N;
  }
  if (a_st.has_value()) {
    a.a_parts = parts_of(*a_st, "a_st");
    a.a_st = a_st->data_ptr<float>();
    a.a_colsum = vec_n(a_colsum, "a_colsum");
    a.a_eps = float(a_eps);
  }
  if (r_st.has_value()) {
    TORCH_CHECK(residual.has_value(), "linear_lnx: r_st normalises the residual: give one");
    a.r_parts = parts_of(*r_st, "r_st");
    a.r_st = r_st->data_ptr<float>();
    a.r_gamma = vec_n(r_gamma, "r_gamma");
    a.r_beta = vec_n(r_beta, "r_beta");
    a.r_eps = float(r_eps);
  }
  Tensor st;
  if (stats) {
    const int bn = tfsk::cgemm_config_bn(int(cfg));
    st = torch::empty({M, (N + bn - 1) / bn, 2}, x.options().dtype(at::kFloat));
    a.st_out = st.data_ptr<float>();
  } else {
    st = torch::empty({0}, x.options().dtype(at::kFloat));
  }
  a.act = act; a.out = y.data_ptr(); a.ldc = N; a.out_f32 = out_f32; a.alpha = 1.f;
  run_igemm(a, tfsk::kADense, cfg, 1, x, cur_stream(x));
  return {y, st};
}

Tensor dense_softmax(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& bias, int64_t n) {
  need(x, at::kFloat, "x");
  need(w, at::kBFloat16, "w");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && w.size(1) >= x.size(1) && w.size(0) >= n && n >= 1 && n <= 16,
              "dense_softmax: x [B, K] f32, w [>= n, >= K] bf16, 1 <= n <= 16");
  TORCH_CHECK(x.size(1) % 4 == 0 && w.size(1) % 4 == 0, "dense_softmax: K % 4 == 0");
  const float* b = nullptr;
  if (bias.has_value()) {
    need(*bias, at::kFloat, "bias");
    TORCH_CHECK(bias->numel() >= n, "bias size");
    b = bias->data_ptr<float>();
  }
  Tensor probs = torch::empty({x.size(0), n}, x.options());
  TORCH_CHECK(tfsk::dense_softmax_launch(x.data_ptr<float>(), int(x.size(1)), bf16p(w), int(w.size(1)), b,
                                         probs.data_ptr<float>(), int(x.size(0)), int(n), int(x.size(1)),
                                         cur_stream(x)) == hipSuccess, "dense_softmax launch failed");
  return probs;
}

Tensor key_mask_adder(const Tensor& m, double one, double scale) {
  TORCH_CHECK(m.is_cuda() && m.is_contiguous() && (m.scalar_type() == at::kInt || m.scalar_type() == at::kFloat),
              "key mask must be a contiguous int32 / f32 GPU tensor");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(m.device());
  Tensor out = torch::empty(m.sizes(), m.options().dtype(at::kFloat));
  TORCH_CHECK(tfsk::key_mask_adder_launch(m.data_ptr(), m.scalar_type() == at::kInt, float(one), float(scale),
                                          out.data_ptr<float>(), m.numel(), cur_stream(m)) == hipSuccess,
              "key_mask_adder launch failed");
  return out;
}

Tensor maxpool(const Tensor& x, int64_t KH, int64_t KW, int64_t SH, int64_t SW, int64_t PT, int64_t PB,
               int64_t PL, int64_t PR, const c10::optional<Tensor>& out, const c10::optional<Tensor>& post_scale,
               const c10::optional<Tensor>& post_shift, int64_t post_act) {
  need(x, at::kBFloat16, "x");
  TORCH_CHECK(x.dim() == 4 && x.size(3) % 8 == 0, "maxpool: NHWC with C % 8 == 0");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  const int Ho = (H + PT + PB - KH) / SH + 1, Wo = (W + PL + PR - KW) / SW + 1;
  Tensor y = out.has_value() ? *out : torch::empty({N, Ho, Wo, C}, x.options());
  need(y, at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == int64_t(N) * Ho * Wo * C, "out has the wrong size");
  const float* sc = nullptr;
  const float* sh = nullptr;
  if (post_scale.has_value()) {
    TORCH_CHECK(post_shift.has_value(), "post_scale needs post_shift");
    need_post_act(post_act, "maxpool");
    need(*post_scale, at::kFloat, "post_scale");
    need(*post_shift, at::kFloat, "post_shift");
    TORCH_CHECK(post_scale->numel() == C && post_shift->numel() == C, "post scale / shift must have C entries");
    sc = post_scale->data_ptr<float>();
    sh = post_shift->data_ptr<float>();
  }
  check(tfsk::maxpool_nhwc_launch(bf16p(x), bf16p_mut(y), N, H, W, C, KH, KW, SH, SW, PT, PL, Ho, Wo,
                                  cur_stream(x), sc, sh, int(post_act)), "maxpool");
  return y;
}

// Depthwise conv (dwconv.hip): x NHWC bf16 (C % 8 == 0), w [KH*KW][C] f32 (BatchNorm
// folded in), bias [C] f32 -> act(conv + bias) as [N][Ho][Wo][C] bf16.  Top /
// left padding and the output size come from the caller (SAME / VALID /
// explicit padding all reduce to them); taps outside the image read zero.
Tensor dwconv2d(const Tensor& x, const Tensor& w, const Tensor& bias, int64_t KH, int64_t KW, int64_t SH, int64_t SW,
                int64_t PT, int64_t PL, int64_t Ho, int64_t Wo, int64_t act, const c10::optional<Tensor>& out,
                int64_t strip) {
  TORCH_CHECK(act == tfsk::kActNone || act == tfsk::kActRelu || act == tfsk::kActRelu6 ||
              act == tfsk::kActHardSwish || act == tfsk::kActSwish,
              "dwconv2d: the activation is none (0), relu (1), relu6 (5), hard_swish (7) or swish (9), got ", act);
  need(x, at::kBFloat16, "x");
  need(w, at::kFloat, "w");
  need(bias, at::kFloat, "bias");
  TORCH_CHECK(x.dim() == 4 && x.size(3) > 0 && x.size(3) % 8 == 0, "dwconv2d: NHWC with C % 8 == 0 (got ",
              x.dim() == 4 ? x.size(3) : -1, " channels)");
  TORCH_CHECK(KH >= 1 && KW >= 1 && KH <= 7 && KW <= 7, "dwconv2d: filters up to 7 x 7 (got ", KH, " x ", KW, ")");
  TORCH_CHECK(SH >= 1 && SW >= 1 && PT >= 0 && PL >= 0 && Ho >= 1 && Wo >= 1, "dwconv2d: bad geometry");
  const int64_t N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  TORCH_CHECK(H >= 1 && W >= 1, "dwconv2d: empty image");
  // the last window must start inside the padded image: no output made of padding alone
  TORCH_CHECK((Ho - 1) * SH - PT < H && (Wo - 1) * SW - PL < W, "dwconv2d: output larger than the input allows");
  TORCH_CHECK(w.numel() == KH * KW * C, "dwconv2d: w must be [KH*KW][C] (channel multiplier 1)");
  TORCH_CHECK(bias.numel() == C, "dwconv2d: bias must have C entries");
  TORCH_CHECK(w.device() == x.device() && bias.device() == x.device(), "dwconv2d: tensors on different devices");
  const bool five = KH == 5 && KW == 5 && SH == SW && (SH == 1 || SH == 2);
  TORCH_CHECK(strip == 0 || strip == tfsk::kDwStripShort || strip == tfsk::kDwStripTall ||
              (five && strip == tfsk::kDwStrip5Tall), "dwconv2d: strip must be 0, ", tfsk::kDwStripShort, " or ",
              tfsk::kDwStripTall, " (or, for a 5 x 5 filter with equal strides 1 or 2, ", tfsk::kDwStrip5Tall,
              "), got ", strip);
  TORCH_CHECK(x.numel() * 2 < 0x7ffffff0LL && N * Ho * Wo * C * 2 < 0x7ffffff0LL, "dwconv2d operands must be < 2 GiB");
  TORCH_CHECK(Wo * (C / 8) <= 65535LL * 256, "dwconv2d: output rows of more than 16 M chunks");
  TORCH_CHECK(!(five && strip != 0 && strip != tfsk::kDwStripTall) || Wo * (C / 4) <= 65535LL * 256,
              "dwconv2d: output rows of more than 8 M half chunks (5 x 5 strips)");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = out.has_value() ? *out : torch::empty({N, Ho, Wo, C}, x.options());
  need(y, at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == N * Ho * Wo * C && y.device() == x.device(), "out has the wrong size");
  TORCH_CHECK(aligned16(x) && aligned16(w) && aligned16(bias) && aligned16(y), "dwconv2d: tensors must be 16-B aligned");
  check(tfsk::dwconv_nhwc_launch(bf16p(x), w.data_ptr<float>(), bias.data_ptr<float>(), bf16p_mut(y), int(N), int(H),
                                 int(W), int(C), int(KH), int(KW), int(SH), int(SW), int(PT), int(PL), int(Ho), int(Wo),
                                 int(act), int(strip), cur_stream(x)), "dwconv2d");
  return y;
}

// Depthwise 7x7 conv + bias + LayerNorm over C in one launch (dwln.hip): x NHWC
// bf16 (C % 8 == 0, 8 <= C <= kDwLnMaxC), w [49][C], bias, gamma, beta [C] f32
// -> (LN_C(conv + bias) * gamma + beta) as [N][Ho][Wo][C] bf16, the conv result
// in fp32 throughout.  Geometry as dwconv2d's; kh, kw, sh, sw are there to be
// checked: the kernel is 7 x 7 / stride 1 only.
Tensor dwconv_ln(const Tensor& x, const Tensor& w, const Tensor& bias, const Tensor& gamma, const Tensor& beta,
                 double eps, int64_t PT, int64_t PL, int64_t Ho, int64_t Wo, const c10::optional<Tensor>& out,
                 int64_t KH, int64_t KW, int64_t SH, int64_t SW) {
  need(x, at::kBFloat16, "x");
  need(w, at::kFloat, "w");
  need(bias, at::kFloat, "bias");
  need(gamma, at::kFloat, "gamma");
  need(beta, at::kFloat, "beta");
  TORCH_CHECK(KH == 7 && KW == 7, "dwconv_ln: the filter is 7 x 7 (got ", KH, " x ", KW, ")");
  TORCH_CHECK(SH == 1 && SW == 1, "dwconv_ln: the stride is 1 (got ", SH, " x ", SW, ")");
  TORCH_CHECK(x.dim() == 4, "dwconv_ln: x must be NHWC");
  const int64_t N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  TORCH_CHECK(C % 8 == 0 && C >= 8 && C <= tfsk::kDwLnMaxC, "dwconv_ln: C % 8 == 0 and 8 <= C <= ", tfsk::kDwLnMaxC,
              " (got ", C, " channels)");
  TORCH_CHECK(PT >= 0 && PL >= 0 && Ho >= 1 && Wo >= 1, "dwconv_ln: bad geometry");
  TORCH_CHECK(H >= 1 && W >= 1, "dwconv_ln: empty image");
  // the last window must start inside the padded image: no output made of padding alone
  TORCH_CHECK(Ho - 1 - PT < H && Wo - 1 - PL < W, "dwconv_ln: output larger than the input allows");
  TORCH_CHECK(w.numel() == 49 * C, "dwconv_ln: w must be [49][C] (a 7 x 7 filter, channel multiplier 1), got ",
              w.numel(), " elements for ", C, " channels");
  TORCH_CHECK(bias.numel() == C, "dwconv_ln: bias must have C entries");
  TORCH_CHECK(gamma.numel() == C && beta.numel() == C, "dwconv_ln: gamma and beta must have C entries (got ",
              gamma.numel(), " and ", beta.numel(), " for ", C, " channels)");
  TORCH_CHECK(eps >= 0.0 && std::isfinite(eps), "dwconv_ln: eps must be finite and >= 0");
  TORCH_CHECK(w.device() == x.device() && bias.device() == x.device() && gamma.device() == x.device() &&
              beta.device() == x.device(), "dwconv_ln: tensors on different devices");
  TORCH_CHECK(x.numel() * 2 < 0x7ffffff0LL && N * Ho * Wo * C * 2 < 0x7ffffff0LL, "dwconv_ln operands must be < 2 GiB");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = out.has_value() ? *out : torch::empty({N, Ho, Wo, C}, x.options());
  need(y, at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == N * Ho * Wo * C && y.device() == x.device(), "out has the wrong size");
  TORCH_CHECK(aligned16(x) && aligned16(w) && aligned16(bias) && aligned16(gamma) && aligned16(beta) && aligned16(y),
              "dwconv_ln: tensors must be 16-B aligned");
  if (y.numel() == 0) return y;
  check(tfsk::dwconv_ln_launch(bf16p(x), w.data_ptr<float>(), bias.data_ptr<float>(), gamma.data_ptr<float>(),
                               beta.data_ptr<float>(), bf16p_mut(y), int(N), int(H), int(W), int(C), int(KH), int(KW),
                               int(SH), int(SW), int(PT), int(PL), int(Ho), int(Wo), float(eps), cur_stream(x)),
        "dwconv_ln");
  return y;
}

// Grouped 3x3 conv (gconv.hip): x NHWC bf16, w the bf16 filter in MFMA fragment
// order (launch.h: gconv_packed_elems(C, cg) elements, graph/fused.py
// pack_grouped_filter), bias [C] f32 -> act(conv + bias) as [N][Ho][Wo][C] bf16.
// cg inputs and cg_out outputs per group (cg_out < 0: cg), strides sh x sw (sw
// < 0: sh), a kh x kw filter.  What the kernel does not take -- launch.h
// gconv_supported, an act other than none / relu -- is the launcher's
// hipErrorInvalidValue, raised here before anything is written.
Tensor gconv2d(const Tensor& x, const Tensor& w, const Tensor& bias, int64_t cg, int64_t SH, int64_t PT, int64_t PL,
               int64_t Ho, int64_t Wo, int64_t act, const c10::optional<Tensor>& out, int64_t cg_out, int64_t SW,
               int64_t KH, int64_t KW) {
  need(x, at::kBFloat16, "x");
  need(w, at::kBFloat16, "w");
  need(bias, at::kFloat, "bias");
  TORCH_CHECK(x.dim() == 4 && x.size(3) > 0, "gconv2d: x must be NHWC");
  if (cg_out < 0) cg_out = cg;
  if (SW < 0) SW = SH;
  const int64_t N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  TORCH_CHECK(H >= 1 && W >= 1 && PT >= 0 && PL >= 0 && Ho >= 1 && Wo >= 1, "gconv2d: bad geometry");
  TORCH_CHECK(cg >= 1 && cg_out >= 1 && cg <= 4096 && cg_out <= 4096 && SH >= 1 && SW >= 1 && SH <= 64 && SW <= 64 &&
              KH >= 1 && KW >= 1 && KH <= 64 && KW <= 64, "gconv2d: bad filter geometry");
  // the last window must start inside the padded image: no output made of padding alone
  TORCH_CHECK((Ho - 1) * SH - PT < H && (Wo - 1) * SW - PL < W, "gconv2d: output larger than the input allows");
  TORCH_CHECK(bias.numel() == C, "gconv2d: bias must have C entries");
  TORCH_CHECK(w.device() == x.device() && bias.device() == x.device(), "gconv2d: tensors on different devices");
  const bool ok = tfsk::gconv_supported(int(C), int(cg), int(cg_out), int(KH), int(KW), int(SH), int(SW));
  TORCH_CHECK(!ok || w.numel() == tfsk::gconv_packed_elems(int(C), int(cg)), "gconv2d: w must hold ",
              ok ? tfsk::gconv_packed_elems(int(C), int(cg)) : 0, " packed elements, got ", w.numel());
  TORCH_CHECK(x.numel() * 2 < 0x7ffffff0LL && N * Ho * Wo * C * 2 < 0x7ffffff0LL, "gconv2d operands must be < 2 GiB");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = out.has_value() ? *out : torch::empty({N, Ho, Wo, C}, x.options());
  need(y, at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == N * Ho * Wo * C && y.device() == x.device(), "out has the wrong size");
  TORCH_CHECK(aligned16(x) && aligned16(w) && aligned16(bias) && aligned16(y), "gconv2d: tensors must be 16-B aligned");
  check(tfsk::gconv_nhwc_launch(bf16p(x), bf16p(w), bias.data_ptr<float>(), bf16p_mut(y), int(N), int(H), int(W), int(C),
                                int(cg), int(cg_out), int(KH), int(KW), int(SH), int(SW), int(PT), int(PL), int(Ho),
                                int(Wo), int(act), cur_stream(x)), "gconv2d");
  return y;
}

// Squeeze-and-excite gate (se.hip): x NHWC bf16, w1 [C][Cr], b1 [Cr], w2 [Cr][C],
// b2 [C] f32 (the TF 1x1 filters reshaped [Cin][Cout]) -> gate [B][C] f32 =
// gate_act(act1(mean_hw(x) w1 + b1) w2 + b2).
Tensor se_gate(const Tensor& x, const Tensor& w1, const Tensor& b1, const Tensor& w2, const Tensor& b2, int64_t act1,
               int64_t gate_act, const c10::optional<Tensor>& out) {
  TORCH_CHECK(act1 == tfsk::kActNone || act1 == tfsk::kActRelu || act1 == tfsk::kActSwish,
              "se_gate: act1 is none (0), relu (1) or swish (9), got ", act1);
  TORCH_CHECK(gate_act == tfsk::kActHardSigmoid || gate_act == tfsk::kActSigmoid,
              "se_gate: gate_act is hard_sigmoid (6) or sigmoid (8), got ", gate_act);
  need(x, at::kBFloat16, "x");
  need(w1, at::kFloat, "w1");
  need(b1, at::kFloat, "b1");
  need(w2, at::kFloat, "w2");
  need(b2, at::kFloat, "b2");
  TORCH_CHECK(x.dim() == 4, "se_gate: x must be NHWC");
  const int64_t B = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
  TORCH_CHECK(C % 8 == 0 && C >= 8 && C <= tfsk::kSeMaxC, "se_gate: C % 8 == 0 and 8 <= C <= ", tfsk::kSeMaxC,
              " (got ", C, " channels)");
  TORCH_CHECK(w1.dim() == 2 && w1.size(0) == C, "se_gate: w1 must be [C][Cr]");
  const int64_t Cr = w1.size(1);
  TORCH_CHECK(Cr >= 1 && Cr <= tfsk::kSeMaxCr, "se_gate: 1 <= Cr <= ", tfsk::kSeMaxCr, " (got ", Cr, ")");
  TORCH_CHECK(HW >= 1, "se_gate: H * W >= 1 (empty image)");
  TORCH_CHECK(b1.dim() == 1 && b1.size(0) == Cr, "se_gate: b1 must be [Cr]");
  TORCH_CHECK(w2.dim() == 2 && w2.size(0) == Cr && w2.size(1) == C, "se_gate: w2 must be [Cr][C]");
  TORCH_CHECK(b2.dim() == 1 && b2.size(0) == C, "se_gate: b2 must be [C]");
  TORCH_CHECK(x.numel() * 2 < 0x7ffffff0LL, "se_gate: x must be < 2 GiB");
  TORCH_CHECK(w1.device() == x.device() && b1.device() == x.device() && w2.device() == x.device() &&
              b2.device() == x.device(), "se_gate: tensors on different devices");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor g = out.has_value() ? *out : torch::empty({B, C}, x.options().dtype(at::kFloat));
  need(g, at::kFloat, "out");
  TORCH_CHECK(g.numel() == B * C && g.device() == x.device(), "out has the wrong size");
  TORCH_CHECK(aligned16(x) && aligned16(w1) && aligned16(b1) && aligned16(w2) && aligned16(b2) && aligned16(g),
              "se_gate: tensors must be 16-B aligned");
  check(tfsk::se_gate_launch(bf16p(x), w1.data_ptr<float>(), b1.data_ptr<float>(), w2.data_ptr<float>(),
                             b2.data_ptr<float>(), g.data_ptr<float>(), int(B), int(HW), int(C), int(Cr), int(act1),
                             int(gate_act), cur_stream(x)), "se_gate");
  return g;
}

// y = bf16(x * gate[b][c]): x NHWC bf16 (C % 8 == 0), gate [B][C] f32.
Tensor se_scale(const Tensor& x, const Tensor& gate, const c10::optional<Tensor>& out) {
  need(x, at::kBFloat16, "x");
  need(gate, at::kFloat, "gate");
  TORCH_CHECK(x.dim() == 4 && x.size(3) >= 8 && x.size(3) % 8 == 0, "se_scale: NHWC with C % 8 == 0 (got ",
              x.dim() == 4 ? x.size(3) : -1, " channels)");
  const int64_t B = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
  TORCH_CHECK(HW >= 1, "se_scale: H * W >= 1 (empty image)");
  TORCH_CHECK(gate.numel() == B * C && gate.device() == x.device(), "se_scale: gate must be [B][C]");
  TORCH_CHECK(x.numel() * 2 < 0x7ffffff0LL, "se_scale: x must be < 2 GiB");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = out.has_value() ? *out : torch::empty_like(x);
  need(y, at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == x.numel() && y.device() == x.device(), "out has the wrong size");
  TORCH_CHECK(aligned16(x) && aligned16(gate) && aligned16(y), "se_scale: tensors must be 16-B aligned");
  check(tfsk::se_scale_launch(bf16p(x), gate.data_ptr<float>(), bf16p_mut(y), int(B), int(HW), int(C), cur_stream(x)),
        "se_scale");
  return y;
}

// ResNet stem: conv 7x7/2 (+bias, act) -> max pool 3x3/2 (+post) in one kernel
// (stem.hip).  x: fp32 NHWC request with C <= 4 (or that request converted to
// bf16 on ingest, csrc/ingest.h); w: [cout][ldw] bf16 in the padded-RGBA order
// of the c4 stem ([kh][8 taps][4 ch]).
Tensor stem_pool(const Tensor& x, const Tensor& w, const Tensor& bias, int64_t PT, int64_t PB, int64_t PL, int64_t PR,
                 int64_t act, int64_t PPT, int64_t PPB, int64_t PPL, int64_t PPR,
                 const c10::optional<Tensor>& post_scale, const c10::optional<Tensor>& post_shift, int64_t post_act) {
  const bool xb16 = x.scalar_type() == at::kBFloat16;
  need(x, xb16 ? at::kBFloat16 : at::kFloat, "x");
  need(w, at::kBFloat16, "w");
  need(bias, at::kFloat, "bias");
  TORCH_CHECK(x.dim() == 4 && x.size(3) >= 1 && x.size(3) <= 4, "stem_pool: x must be NHWC with C <= 4");
  TORCH_CHECK(w.dim() == 2 && w.size(0) % 16 == 0 && w.size(0) >= 16 && w.size(0) <= 64 && w.size(1) >= 224 &&
              w.size(1) % 8 == 0, "stem_pool: w must be [cout in 16..64 step 16][>= 224, % 8]");
  TORCH_CHECK(bias.numel() == w.size(0), "stem_pool: bias must have cout entries");
  TORCH_CHECK(PT >= 0 && PB >= 0 && PL >= 0 && PR >= 0 && PPT >= 0 && PPT <= 2 && PPL >= 0 && PPL <= 2 &&
              PPB >= 0 && PPR >= 0, "stem_pool: bad padding");
  TORCH_CHECK(w.device() == x.device() && bias.device() == x.device(), "stem_pool: tensors on different devices");
  Tensor xin = x;
  if (xb16 && x.numel() % 2) {
    // the bf16 path reads whole aligned dwords: an odd element count's last
    // pixel reads 2 B past the tensor, which must still lie in its storage;
    // otherwise the kernel reads a copy with one element of padding (the
    // serving path's ingest buffers are padded, so it never copies)
    const int64_t avail = int64_t(x.storage().nbytes()) - int64_t(x.storage_offset()) * 2;
    if (avail < x.numel() * 2 + 2 || !x.is_contiguous()) {
      Tensor padded = torch::zeros({x.numel() + 1}, x.options());
      padded.narrow(0, 0, x.numel()).copy_(x.reshape({-1}));
      xin = padded.narrow(0, 0, x.numel()).view(x.sizes());
    }
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3), cout = w.size(0);
  const int Hc = (H + PT + PB - 7) / 2 + 1, Wc = (W + PL + PR - 7) / 2 + 1;
  TORCH_CHECK(Hc >= 1 && Wc >= 1, "stem_pool: input smaller than the filter");
  const int Hp = (Hc + PPT + PPB - 3) / 2 + 1, Wp = (Wc + PPL + PPR - 3) / 2 + 1;
  TORCH_CHECK(Hp >= 1 && Wp >= 1, "stem_pool: conv output smaller than the pool window");
  Tensor y = torch::empty({N, Hp, Wp, cout}, x.options().dtype(at::kBFloat16));
  const float* sc = nullptr;
  const float* sh = nullptr;
  if (post_scale.has_value()) {
    TORCH_CHECK(post_shift.has_value(), "post_scale needs post_shift");
    need(*post_scale, at::kFloat, "post_scale");
    need(*post_shift, at::kFloat, "post_shift");
    TORCH_CHECK(post_scale->numel() == cout && post_shift->numel() == cout, "post scale / shift must have cout entries");
    sc = post_scale->data_ptr<float>();
    sh = post_shift->data_ptr<float>();
  }
  check(tfsk::stem_pool_launch(xin.data_ptr(), xb16, bf16p(w), int(w.size(1)), bias.data_ptr<float>(), bf16p_mut(y), N,
                               H, W, C, cout, int(PT), int(PL), Hc, Wc, int(PPT), int(PPL), Hp, Wp, int(act), sc, sh,
                               int(post_act), cur_stream(x)), "stem_pool");
  return y;
}

// A bottleneck's expand 1x1 (+ shortcut, act) and the next bottleneck's
// reduce 1x1 (+ act) as one kernel (chain.hip): returns (y1, y2), NHWC bf16.
// With x2 (same n, h, w as x) the expand reads the rows [x | x2] against the
// K-concatenated w1: the dual conv of a projecting block with stride 1.
std::vector<Tensor> conv_chain(const Tensor& x, const Tensor& w1, const Tensor& b1,
                               const c10::optional<Tensor>& residual, int64_t act1, const Tensor& w2,
                               const Tensor& b2, int64_t act2, const c10::optional<Tensor>& x2) {
  need(x, at::kBFloat16, "x");
  need(w1, at::kBFloat16, "w1");
  need(w2, at::kBFloat16, "w2");
  need(b1, at::kFloat, "b1");
  need(b2, at::kFloat, "b2");
  TORCH_CHECK(x.dim() == 4, "conv_chain: x must be NHWC");
  const bool dual = x2.has_value();
  const int Ka = x.size(3);
  const uint16_t* x2p = nullptr;
  if (dual) {
    need(*x2, at::kBFloat16, "x2");
    TORCH_CHECK(x2->dim() == 4 && x2->size(0) == x.size(0) && x2->size(1) == x.size(1) && x2->size(2) == x.size(2),
                "conv_chain: x2 must have x's n, h, w");
    TORCH_CHECK(Ka % 64 == 0 && x2->size(3) % 64 == 0 && x2->size(3) > 0,
                "conv_chain: both sources' channels must be multiples of 64");
    TORCH_CHECK(x2->device() == x.device(), "conv_chain: tensors on different devices");
    x2p = bf16p(*x2);
  }
  const int K1 = Ka + (dual ? int(x2->size(3)) : 0), N1 = w1.size(0), N2 = w2.size(0);
  TORCH_CHECK(w1.dim() == 2 && w2.dim() == 2 && w1.size(1) >= K1 && w2.size(1) >= N1 && w1.size(1) % 8 == 0 &&
                  w2.size(1) % 8 == 0, "conv_chain: w1 [N1][>= K1], w2 [N2][>= N1]");
  TORCH_CHECK(tfsk::conv_chain_supported(K1, N1, N2, dual), "conv_chain: unsupported shape K1=", K1, " N1=", N1,
              " N2=", N2, dual ? " (dual)" : "");
  TORCH_CHECK(b1.numel() == N1 && b2.numel() == N2, "conv_chain: bias sizes");
  TORCH_CHECK(w1.device() == x.device() && w2.device() == x.device() && b1.device() == x.device() &&
                  b2.device() == x.device(), "conv_chain: tensors on different devices");
  const uint16_t* rp = nullptr;
  if (residual.has_value()) {
    need(*residual, at::kBFloat16, "residual");
    TORCH_CHECK(residual->dim() == 4 && residual->size(0) == x.size(0) && residual->size(1) == x.size(1) &&
                    residual->size(2) == x.size(2) && residual->size(3) == N1, "conv_chain: residual [n][h][w][N1]");
    rp = bf16p(*residual);
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  const int M = x.size(0) * x.size(1) * x.size(2);
  Tensor y1 = torch::empty({x.size(0), x.size(1), x.size(2), N1}, x.options());
  Tensor y2 = torch::empty({x.size(0), x.size(1), x.size(2), N2}, x.options());
  check(tfsk::conv_chain_launch(bf16p(x), bf16p(w1), int(w1.size(1)), b1.data_ptr<float>(), rp, bf16p_mut(y1),
                                bf16p(w2), int(w2.size(1)), b2.data_ptr<float>(), bf16p_mut(y2), M, K1, N1, N2,
                                int(act1), int(act2), cur_stream(x), x2p, Ka),
        "conv_chain");
  return {y1, y2};
}

// A wide 1x1 conv (+ shortcut, act) on the row-panel kernel (panel.hip): a
// workgroup owns bm rows x cout / nsplit columns and reads its rows of x once.
Tensor conv1x1_panel(const Tensor& x, const Tensor& w, const Tensor& bias, const c10::optional<Tensor>& residual,
                     int64_t act, int64_t bm, int64_t nsplit, const c10::optional<Tensor>& out) {
  need(x, at::kBFloat16, "x");
  need(w, at::kBFloat16, "w");
  need(bias, at::kFloat, "bias");
  TORCH_CHECK(x.dim() == 4, "conv1x1_panel: x must be NHWC");
  const int64_t M64 = x.size(0) * x.size(1) * x.size(2);
  const int K = x.size(3), N = w.size(0);
  TORCH_CHECK(w.dim() == 2 && w.size(1) >= K && w.size(1) % 8 == 0, "conv1x1_panel: w [N][>= K, a multiple of 8]");
  TORCH_CHECK(M64 < (int64_t(1) << 31) && tfsk::conv1x1_panel_supported(int(M64), N, K, int(bm), int(nsplit)),
              "conv1x1_panel: unsupported shape M=", M64, " N=", N, " K=", K, " bm=", bm, " nsplit=", nsplit);
  TORCH_CHECK(act == tfsk::kActNone || act == tfsk::kActRelu, "conv1x1_panel: act must be none or relu");
  TORCH_CHECK(bias.numel() == N, "conv1x1_panel: bias size");
  TORCH_CHECK(w.device() == x.device() && bias.device() == x.device(), "conv1x1_panel: tensors on different devices");
  const uint16_t* rp = nullptr;
  if (residual.has_value()) {
    need(*residual, at::kBFloat16, "residual");
    TORCH_CHECK(residual->dim() == 4 && residual->size(0) == x.size(0) && residual->size(1) == x.size(1) &&
                    residual->size(2) == x.size(2) && residual->size(3) == N && residual->device() == x.device(),
                "conv1x1_panel: residual [n][h][w][N]");
    rp = bf16p(*residual);
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = out.has_value() ? *out : torch::empty({x.size(0), x.size(1), x.size(2), N}, x.options());
  need(y, at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == M64 * N && y.device() == x.device(), "conv1x1_panel: out [n][h][w][N]");
  TORCH_CHECK(aligned16(x) && aligned16(w) && aligned16(bias) && aligned16(y) && (!rp || aligned16(*residual)),
              "conv1x1_panel: operands must be 16-byte aligned");
  check(tfsk::conv1x1_panel_launch(bf16p(x), bf16p(w), int(w.size(1)), bias.data_ptr<float>(), rp, bf16p_mut(y),
                                   int(M64), N, K, int(bm), int(nsplit), int(act), cur_stream(x)),
        "conv1x1_panel");
  return y;
}

Tensor global_avgpool(const Tensor& x, const c10::optional<Tensor>& out) {
  need(x, at::kBFloat16, "x");
  TORCH_CHECK(x.dim() == 4 && x.size(3) % 8 == 0, "global_avgpool: NHWC with C % 8 == 0");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  const int N = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
  Tensor y = out.has_value() ? *out : torch::empty({N, C}, x.options());
  need(y, at::kBFloat16, "out");
  check(tfsk::global_avgpool_nhwc_launch(bf16p(x), bf16p_mut(y), N, HW, C, cur_stream(x)), "gap");
  return y;
}

std::vector<Tensor> softmax_argmax(const Tensor& logits, bool want_probs, bool want_classes,
                                   const c10::optional<Tensor>& probs_out,
                                   const c10::optional<Tensor>& classes_out) {
  // rows may be strided (a [M, N] view of a GEMM output padded to ldc > N)
  TORCH_CHECK(logits.is_cuda() && logits.dim() >= 1 && logits.stride(-1) == 1 &&
                  (logits.is_contiguous() || logits.dim() == 2),
              "logits must be a GPU tensor with unit column stride (contiguous, or 2-D with a row stride)");
  const bool bf = logits.scalar_type() == at::kBFloat16;
  TORCH_CHECK(bf || logits.scalar_type() == at::kFloat, "logits must be f32 or bf16");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
  const int cols = logits.size(-1);
  const int rows = logits.numel() / cols;
  const long ld = logits.dim() == 2 ? long(logits.stride(0)) : long(cols);
  TORCH_CHECK(ld >= cols, "logits row stride");
  Tensor probs, classes;
  if (want_probs) {
    probs = probs_out.has_value() ? *probs_out : torch::empty(logits.sizes(), logits.options().dtype(at::kFloat));
    need(probs, at::kFloat, "probs");
  }
  if (want_classes) {
    auto sz = logits.sizes().vec();
    sz.pop_back();
    classes = classes_out.has_value() ? *classes_out : torch::empty(sz, logits.options().dtype(at::kLong));
    need(classes, at::kLong, "classes");
  }
  check(tfsk::softmax_argmax_launch(logits.data_ptr(), bf, want_probs ? probs.data_ptr<float>() : nullptr,
                                    want_classes ? classes.data_ptr<int64_t>() : nullptr, rows, cols, ld,
                                    cur_stream(logits)), "softmax_argmax");
  return {probs, classes};
}

// ResNet-style head: probs, classes = softmax/argmax(mean_hw(x) @ w^T + bias)[:, :n]
// With `probs_host` / `classes_host` (pinned host addresses of >= M rows, 0:
// none) the one-launch head also stores its rows there; the returned flag
// says whether it did (only the one-launch path can).
std::tuple<Tensor, Tensor, bool> classifier_head_impl(const Tensor& x, const Tensor& w, const Tensor& bias, int64_t n,
                                                      int64_t probs_host, int64_t classes_host);

std::vector<Tensor> classifier_head(const Tensor& x, const Tensor& w, const Tensor& bias, int64_t n) {
  auto r = classifier_head_impl(x, w, bias, n, 0, 0);
  return {std::get<0>(r), std::get<1>(r)};
}

std::tuple<Tensor, Tensor, bool> classifier_head_impl(const Tensor& x, const Tensor& w, const Tensor& bias, int64_t n,
                                                      int64_t probs_host, int64_t classes_host) {
  need(x, at::kBFloat16, "x");
  need(w, at::kBFloat16, "w");
  need(bias, at::kFloat, "bias");
  TORCH_CHECK(x.dim() == 4, "classifier_head: x must be NHWC");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  const int M = x.size(0), HW = x.size(1) * x.size(2), K = x.size(3);
  TORCH_CHECK(w.dim() == 2 && w.size(1) == K && (K == 512 || K == 1024 || K == 2048 || K == 4096),
              "classifier_head: w [Np][K] with K in {512, 1024, 2048, 4096}");
  const int Np = w.size(0);
  TORCH_CHECK(bias.numel() == Np && n >= 1 && n <= Np, "classifier_head: bias [Np], 1 <= n <= Np");
  Tensor part = torch::empty({int64_t(tfsk::classifier_head_ws_floats(M, K, Np))}, x.options().dtype(at::kFloat));
  Tensor probs = torch::empty({M, n}, x.options().dtype(at::kFloat));
  Tensor classes = torch::empty({M}, x.options().dtype(at::kLong));
  // small batches: one launch that hands off through an arrival counter (its
  // last workgroup runs the softmax rows serially, so only up to
  // TFSERVE_HEAD_FUSED rows, default 4, at most 16; 0 keeps three launches)
  int* counter = nullptr;
  const char* hf = std::getenv("TFSERVE_HEAD_FUSED");
  const int fused_max = hf && hf[0] ? std::min(16, std::atoi(hf)) : 4;
  if (M <= fused_max) {
    tfsk::splitk_counters_prepare(cur_stream(x));
    counter = tfsk::splitk_counters(1, cur_stream(x));
  }
  // host rows only where the one-launch path runs (same conditions as the launcher)
  const bool to_host = counter != nullptr && (probs_host != 0 || classes_host != 0) &&
                       tfsk::classifier_head_one_launch(M, HW, K, Np, int(n));
  check(tfsk::classifier_head_launch(bf16p(x), bf16p(w), bias.data_ptr<float>(), part.data_ptr<float>(),
                                     probs.data_ptr<float>(), classes.data_ptr<int64_t>(), M, HW, K, Np, int(n),
                                     cur_stream(x), counter,
                                     to_host ? reinterpret_cast<float*>(probs_host) : nullptr,
                                     to_host ? reinterpret_cast<int64_t*>(classes_host) : nullptr),
        "classifier_head");
  return {probs, classes, to_host};
}

Tensor ingest_c4(const Tensor& x, const c10::optional<Tensor>& out) {
  need(x, at::kFloat, "x");
  TORCH_CHECK(x.dim() == 4 && x.size(3) <= 4, "ingest_c4: NHWC with C <= 4");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = out.has_value() ? *out : torch::empty({x.size(0), x.size(1), x.size(2), 4}, x.options().dtype(at::kBFloat16));
  need(y, at::kBFloat16, "out");
  check(tfsk::ingest_c4_launch(x.data_ptr<float>(), bf16p_mut(y), x.numel() / x.size(3), x.size(3), cur_stream(x)),
        "ingest_c4");
  return y;
}

// Zero-copy ingest: the kernel reads fp32 rows straight out of a *pinned host*
// tensor (device-accessible; e.g. a lane's request staging buffer) over PCIe,
// instead of an SDMA copy followed by a device pass.
void need_pinned_f32(const Tensor& x, const char* name) {
  TORCH_CHECK(x.device().is_cpu() && x.is_pinned(), name, " must be a pinned host tensor");
  TORCH_CHECK(x.scalar_type() == at::kFloat && x.is_contiguous(), name, " must be contiguous float32");
}

void ingest_c4_from_host(const Tensor& x, const Tensor& out) {
  need_pinned_f32(x, "x");
  need(out, at::kBFloat16, "out");
  TORCH_CHECK(x.dim() == 4 && x.size(3) >= 1 && x.size(3) <= 4, "ingest_c4_from_host: x must be NHWC with C <= 4");
  const int64_t pixels = x.numel() / x.size(3);
  TORCH_CHECK(out.numel() == pixels * 4, "ingest_c4_from_host: out must hold pixels x 4 channels");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(out.device());
  check(tfsk::ingest_c4_launch(x.data_ptr<float>(), bf16p_mut(out), pixels, int(x.size(3)), cur_stream(out)),
        "ingest_c4_from_host");
}

Tensor ingest_c4_padded(const Tensor& x, int64_t Hp, int64_t Wp, int64_t pt, int64_t pl) {
  need(x, at::kFloat, "x");
  TORCH_CHECK(x.dim() == 4 && x.size(3) >= 1 && x.size(3) <= 4, "ingest_c4_padded: NHWC with C <= 4");
  TORCH_CHECK(pt >= 0 && pl >= 0 && Hp >= pt + x.size(1) && Wp >= pl + x.size(2), "ingest_c4_padded: padding");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = torch::empty({x.size(0), Hp, Wp, 4}, x.options().dtype(at::kBFloat16));
  check(tfsk::ingest_c4_pad_launch(x.data_ptr<float>(), bf16p_mut(y), x.size(0), x.size(1), x.size(2), x.size(3),
                                   Hp, Wp, pt, pl, cur_stream(x)),
        "ingest_c4_padded");
  return y;
}

void cast_bf16_from_host(const Tensor& x, const Tensor& out) {
  need_pinned_f32(x, "x");
  need(out, at::kBFloat16, "out");
  TORCH_CHECK(out.numel() == x.numel(), "cast_bf16_from_host: size mismatch");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(out.device());
  check(tfsk::cast_f32_bf16_launch(x.data_ptr<float>(), bf16p_mut(out), x.numel(), cur_stream(out)),
        "cast_bf16_from_host");
}

void h2d_rows(const Tensor& host, const Tensor& dev) {
  TORCH_CHECK(host.device().is_cpu() && host.is_pinned() && host.is_contiguous(), "h2d_rows: host must be a "
              "contiguous pinned CPU tensor");
  TORCH_CHECK(dev.is_cuda() && dev.is_contiguous(), "h2d_rows: dev must be a contiguous device tensor");
  const int64_t bytes = host.numel() * host.element_size();
  TORCH_CHECK(bytes == dev.numel() * dev.element_size(), "h2d_rows: size mismatch");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(dev.device());
  check(tfsk::h2d_rows_launch(host.data_ptr(), dev.data_ptr(), bytes, cur_stream(dev)), "h2d_rows");
}

Tensor cast_bf16(const Tensor& x, const c10::optional<Tensor>& out) {
  need(x, at::kFloat, "x");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = out.has_value() ? *out : torch::empty(x.sizes(), x.options().dtype(at::kBFloat16));
  need(y, at::kBFloat16, "out");
  check(tfsk::cast_f32_bf16_launch(x.data_ptr<float>(), bf16p_mut(y), x.numel(), cur_stream(x)), "cast");
  return y;
}

// y = LN(x @ w^T + bias + residual) * gamma + beta in one launch (lngemm.hip);
// x [.., K] contiguous bf16, w_frag = w [N][K] bf16 pre-shuffled fragment-major
// ([N/16][K/32][4][16][8]: graph/fused.py ln_weight_frags), bias / gamma / beta f32 [N]
Tensor linear_ln(const Tensor& x, const Tensor& w, const c10::optional<Tensor>& bias,
                 const c10::optional<Tensor>& residual, const Tensor& gamma, const Tensor& beta, double eps,
                 int64_t bm, const c10::optional<Tensor>& out) {
  need(x, at::kBFloat16, "x");
  need(w, at::kBFloat16, "w");
  need(gamma, at::kFloat, "gamma");
  need(beta, at::kFloat, "beta");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  const int K = x.size(-1), M = x.numel() / K, N = w.size(0);
  TORCH_CHECK(w.is_contiguous() && w.numel() == int64_t(N) * K, "linear_ln: w_frag must be a contiguous [N][K]");
  TORCH_CHECK(tfsk::lngemm_supported(M, N, K, int(bm)), "linear_ln: unsupported shape M=", M, " N=", N, " K=", K,
              " bm=", bm);
  TORCH_CHECK(gamma.numel() == N && beta.numel() == N, "linear_ln: gamma / beta size");
  auto sizes = x.sizes().vec();
  sizes.back() = N;
  Tensor y = out.has_value() ? *out : torch::empty(sizes, x.options());
  need(y, at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == int64_t(M) * N, "linear_ln: out has the wrong size");
  tfsk::LnGemmArgs a;
  a.x = bf16p(x); a.w = bf16p(w); a.gamma = gamma.data_ptr<float>(); a.beta = beta.data_ptr<float>();
  a.y = bf16p_mut(y); a.M = M; a.N = N; a.K = K; a.ldx = K; a.eps = float(eps);
  if (bias.has_value()) {
    need(*bias, at::kFloat, "bias");
    TORCH_CHECK(bias->numel() == N, "linear_ln: bias size");
    a.bias = bias->data_ptr<float>();
  }
  if (residual.has_value()) {
    need(*residual, at::kBFloat16, "residual");
    TORCH_CHECK(residual->numel() == y.numel(), "linear_ln: residual shape must match the output");
    a.r = bf16p(*residual);
  }
  check(tfsk::lngemm_launch(a, int(bm), cur_stream(x)), "linear_ln");
  return y;
}

Tensor layernorm(const Tensor& x, const c10::optional<Tensor>& residual, const Tensor& gamma, const Tensor& beta,
                 double eps, const c10::optional<Tensor>& out) {
  need(x, at::kBFloat16, "x");
  need(gamma, at::kFloat, "gamma");
  need(beta, at::kFloat, "beta");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  const int cols = x.size(-1);
  TORCH_CHECK(cols % 8 == 0 && gamma.numel() == cols && beta.numel() == cols, "layernorm shapes");
  TORCH_CHECK(aligned16(gamma) && aligned16(beta), "layernorm: gamma / beta must be 16-B aligned");
  const int rows = x.numel() / cols;
  const uint16_t* r = nullptr;
  if (residual.has_value()) {
    need(*residual, at::kBFloat16, "residual");
    TORCH_CHECK(residual->numel() == x.numel(), "residual shape");
    r = bf16p(*residual);
  }
  Tensor y = out.has_value() ? *out : torch::empty_like(x);
  need(y, at::kBFloat16, "out");
  check(tfsk::layernorm_launch(bf16p(x), r, gamma.data_ptr<float>(), beta.data_ptr<float>(), bf16p_mut(y), rows,
                               cols, float(eps), cur_stream(x)), "layernorm");
  return y;
}

// ids / type_ids: int32, any shape, flattened to tokens; pos: [>= seq, Hd] rows
// indexed by token % seq. Returns ids.shape + [Hd].
Tensor embed_ln(const Tensor& ids, const c10::optional<Tensor>& type_ids, const Tensor& word,
                const c10::optional<Tensor>& pos, const c10::optional<Tensor>& type, const Tensor& gamma,
                const Tensor& beta, double eps, int64_t seq) {
  need(ids, at::kInt, "ids");
  need(word, at::kBFloat16, "word");
  need(gamma, at::kFloat, "gamma");
  need(beta, at::kFloat, "beta");
  TORCH_CHECK(word.dim() == 2, "word table must be 2-D");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(ids.device());
  const int64_t tokens = ids.numel(), Hd = word.size(1);
  TORCH_CHECK(Hd % 8 == 0 && Hd <= 2048, "embed_ln: hidden must be a multiple of 8 and <= 2048");
  TORCH_CHECK(gamma.numel() == Hd && beta.numel() == Hd, "embed_ln: LN params shape");
  TORCH_CHECK(aligned16(gamma) && aligned16(beta), "embed_ln: gamma / beta must be 16-B aligned");
  TORCH_CHECK(seq > 0 && tokens % seq == 0 && tokens < (int64_t(1) << 31), "embed_ln: tokens must be batch * seq");
  const int* tt = nullptr;
  const uint16_t *pp = nullptr, *tp = nullptr;
  int ntypes = 0;
  if (type_ids.has_value()) {
    TORCH_CHECK(type.has_value(), "embed_ln: type_ids without a type table");
    need(*type_ids, at::kInt, "type_ids");
    need(*type, at::kBFloat16, "type");
    TORCH_CHECK(type_ids->numel() == tokens && type->dim() == 2 && type->size(1) == Hd, "embed_ln: type shapes");
    tt = type_ids->data_ptr<int>();
    tp = bf16p(*type);
    ntypes = type->size(0);
  }
  if (pos.has_value()) {
    need(*pos, at::kBFloat16, "pos");
    TORCH_CHECK(pos->dim() == 2 && pos->size(1) == Hd && pos->size(0) >= seq, "embed_ln: pos shape");
    pp = bf16p(*pos);
  }
  auto shape = ids.sizes().vec();
  shape.push_back(Hd);
  Tensor y = torch::empty(shape, word.options());
  check(tfsk::embed_ln_launch(ids.data_ptr<int>(), tt, bf16p(word), pp, tp, gamma.data_ptr<float>(),
                              beta.data_ptr<float>(), bf16p_mut(y), tokens, seq, Hd, word.size(0), ntypes,
                              float(eps), cur_stream(ids)), "embed_ln");
  return y;
}

Tensor attention(const Tensor& qkv, const c10::optional<Tensor>& mask_bias, int64_t heads, double scale,
                 const c10::optional<Tensor>& out, int64_t mask_bstride, int64_t mask_qstride, int64_t form) {
  need(qkv, at::kBFloat16, "qkv");
  TORCH_CHECK(qkv.dim() == 3, "qkv must be [B, S, 3*H*D]");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(qkv.device());
  const int B = qkv.size(0), S = qkv.size(1), HD3 = qkv.size(2);
  TORCH_CHECK(HD3 % (3 * heads) == 0, "qkv width must be 3*heads*head_dim");
  const int D = HD3 / (3 * heads);
  TORCH_CHECK(D == 64, "attention kernel supports head_dim 64");
  TORCH_CHECK(form == 0 || form == tfsk::kAttnFormRagged, "attention: unknown form ", form, " (0 or 1)");
  TORCH_CHECK(S >= 1 && S <= tfsk::kMaxAttentionSeq, "attention kernel supports 1 <= S <= ", tfsk::kMaxAttentionSeq);
  if (form == tfsk::kAttnFormRagged) {
    TORCH_CHECK(S <= tfsk::kAttnRaggedMaxSeq, "attention form 1 supports 1 <= S <= ", tfsk::kAttnRaggedMaxSeq,
                ", got S = ", S);
    TORCH_CHECK(int64_t(S) * HD3 * 2 < (int64_t(1) << 31), "attention form 1: one image's qkv rows exceed 2 GiB");
    TORCH_CHECK(aligned16(qkv), "attention form 1: qkv must be 16-byte aligned");
  }
  const float* mb = nullptr;
  if (mask_bias.has_value()) {
    need(*mask_bias, at::kFloat, "mask_bias");
    // largest index the kernel reads must be inside the mask tensor
    const int64_t last = int64_t(B - 1) * mask_bstride + int64_t(S - 1) * mask_qstride + (S - 1);
    TORCH_CHECK(mask_bstride >= 0 && mask_qstride >= 0 && last < mask_bias->numel(),
                "mask strides exceed the mask tensor");
    mb = mask_bias->data_ptr<float>();
  }
  Tensor y = out.has_value() ? *out : torch::empty({B, S, heads * D}, qkv.options());
  need(y, at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == int64_t(B) * S * heads * D, "out has the wrong size");
  TORCH_CHECK(form == 0 || aligned16(y), "attention form 1: out must be 16-byte aligned");
  check(tfsk::attention_launch(bf16p(qkv), mb, bf16p_mut(y), B, S, heads, D, float(scale), mask_bstride,
                               mask_qstride, int(form), cur_stream(qkv)),
        "attention");
  return y;
}

// the (Hf, Wf, ws, shift) of a window_attention grid argument, zeros for None
struct WattnGrid { int64_t Hf = 0, Wf = 0, ws = 0, shift = 0; };
WattnGrid wattn_grid(const c10::optional<std::vector<int64_t>>& grid) {
  WattnGrid g;
  if (!grid.has_value()) return g;
  TORCH_CHECK(grid->size() == 4, "window_attention: grid must be (Hf, Wf, ws, shift)");
  g.Hf = (*grid)[0]; g.Wf = (*grid)[1]; g.ws = (*grid)[2]; g.shift = (*grid)[3];
  TORCH_CHECK(g.Hf >= 1 && g.Wf >= 1 && g.ws >= 1, "window_attention: grid sizes must be positive");
  return g;
}

// qkv: [R, 3*H*32] bf16; bias: [H, S, S] f32; mask: [nW, S, S] f32 or None; grid: None or (Hf, Wf, ws, shift)
Tensor window_attention(const Tensor& qkv, const Tensor& bias, const c10::optional<Tensor>& mask, int64_t heads,
                        double scale, const c10::optional<Tensor>& out,
                        const c10::optional<std::vector<int64_t>>& grid) {
  need(qkv, at::kBFloat16, "qkv");
  need(bias, at::kFloat, "bias");
  TORCH_CHECK(qkv.dim() == 2, "window_attention: qkv must be [R, 3*H*D]");
  TORCH_CHECK(heads >= 1 && qkv.size(1) % (3 * heads) == 0, "window_attention: qkv width must be 3*heads*head_dim");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(qkv.device());
  const int64_t R = qkv.size(0), D = qkv.size(1) / (3 * heads);
  TORCH_CHECK(D == tfsk::kWattnHeadDim, "window_attention kernel supports head_dim ", tfsk::kWattnHeadDim, ", got ", D);
  TORCH_CHECK(bias.dim() == 3 && bias.size(1) == bias.size(2), "window_attention: bias must be [H, S, S]");
  const int64_t S = bias.size(1);
  TORCH_CHECK(S >= 1 && S <= tfsk::kWattnMaxSeq, "window_attention kernel supports 1 <= S <= ", tfsk::kWattnMaxSeq,
              ", got S = ", S);
  TORCH_CHECK(bias.size(0) == heads, "window_attention: bias has ", bias.size(0), " heads, expected ", heads);
  int64_t nW = 0;
  const float* mp = nullptr;
  if (mask.has_value()) {
    need(*mask, at::kFloat, "mask");
    TORCH_CHECK(mask->dim() == 3 && mask->size(0) >= 1 && mask->size(1) == S && mask->size(2) == S,
                "window_attention: mask must be [nW, ", S, ", ", S, "]");
    TORCH_CHECK(aligned16(*mask), "window_attention: mask must be 16-byte aligned");
    nW = mask->size(0);
    mp = mask->data_ptr<float>();
  }
  const WattnGrid g = wattn_grid(grid);
  if (g.ws > 0) {
    TORCH_CHECK(g.Hf % g.ws == 0 && g.Wf % g.ws == 0, "window_attention: the ", g.Hf, " x ", g.Wf,
                " map is not a multiple of the window ", g.ws);
    TORCH_CHECK(g.ws * g.ws == S, "window_attention: window ", g.ws, " x ", g.ws, " does not have S = ", S, " tokens");
    TORCH_CHECK(g.shift >= 0 && g.shift < g.ws, "window_attention: shift ", g.shift, " outside [0, ", g.ws, ")");
    TORCH_CHECK(nW == 0 || nW == (g.Hf / g.ws) * (g.Wf / g.ws), "window_attention: mask has ", nW,
                " windows, the map has ", (g.Hf / g.ws) * (g.Wf / g.ws));
    TORCH_CHECK(R % (g.Hf * g.Wf) == 0, "window_attention: ", R, " rows are not whole ", g.Hf, " x ", g.Wf, " maps");
  } else {
    TORCH_CHECK(R % S == 0, "window_attention: ", R, " rows are not whole windows of ", S);
  }
  const int64_t lim = int64_t(1) << 31;
  TORCH_CHECK(qkv.numel() * 2 < lim && bias.numel() * 4 < lim && nW * S * S * 4 < lim,
              "window_attention: operands must be smaller than 2 GiB");
  TORCH_CHECK(aligned16(qkv), "window_attention: qkv must be 16-byte aligned");
  TORCH_CHECK(aligned16(bias), "window_attention: bias must be 16-byte aligned");
  Tensor y = out.has_value() ? *out : torch::empty({R, heads * D}, qkv.options());
  need(y, at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == R * heads * D, "window_attention: out has the wrong size");
  TORCH_CHECK(aligned16(y), "window_attention: out must be 16-byte aligned");
  TORCH_CHECK(tfsk::window_attention_supported(R, S, heads, D, nW, g.Hf, g.Wf, g.ws, g.shift),
              "window_attention: unsupported launch");
  check(tfsk::window_attention_launch(bf16p(qkv), bias.data_ptr<float>(), mp, bf16p_mut(y), R, int(S), int(heads),
                                      int(nW), float(scale), int(g.Hf), int(g.Wf), int(g.ws), int(g.shift),
                                      cur_stream(qkv)),
        "window_attention");
  return y;
}

// y[b, 0, :] = bf16(table[0, :]); y[b, 1 + p, :] = bf16(float(x[b, p, :]) + table[1 + p, :])
// x: [B, P, C] bf16 (any leading shape with B * P * C elements per the arguments), table: [P + 1, C] f32
Tensor patch_tokens(const Tensor& x, const Tensor& table, const c10::optional<Tensor>& out) {
  need(x, at::kBFloat16, "x");
  need(table, at::kFloat, "table");
  TORCH_CHECK(x.dim() == 3, "patch_tokens: x must be [B, P, C]");
  TORCH_CHECK(table.dim() == 2 && table.size(0) == x.size(1) + 1 && table.size(1) == x.size(2),
              "patch_tokens: table must be [P + 1, C]");
  const int64_t B = x.size(0), P = x.size(1), C = x.size(2);
  TORCH_CHECK(C % 8 == 0, "patch_tokens: C % 8 != 0 (C = ", C, ")");
  TORCH_CHECK(aligned16(x), "patch_tokens: x must be 16-byte aligned");
  TORCH_CHECK(aligned16(table), "patch_tokens: table must be 16-byte aligned");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  Tensor y = out.has_value() ? *out : torch::empty({B, P + 1, C}, x.options());
  need(y, at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == B * (P + 1) * C, "patch_tokens: out has the wrong size");
  TORCH_CHECK(aligned16(y), "patch_tokens: out must be 16-byte aligned");
  TORCH_CHECK(tfsk::patch_tokens_supported(B, P, C), "patch_tokens: operands must be smaller than 2 GiB");
  check(tfsk::patch_tokens_launch(bf16p(x), table.data_ptr<float>(), bf16p_mut(y), B, P, C, cur_stream(x)),
        "patch_tokens");
  return y;
}

// out[b, F0 + f, :] = bf16(sum_l table_f[ids[b, first_f + l], :]); out[b, 0, :] = dense[b, :] when dense is given
// ids: [B, T] int32 / int64, blob: [rows, D] bf16, feat: [F, 4] int64 on the device, features: the same F x 4
// values on the host (checked here; the op builds both from one list), dense: [B, D] bf16
Tensor embedding_bag(const Tensor& ids, const Tensor& blob, const Tensor& feat, const std::vector<int64_t>& features,
                     const c10::optional<Tensor>& dense, const c10::optional<Tensor>& out) {
  TORCH_CHECK(ids.scalar_type() == at::kInt || ids.scalar_type() == at::kLong, "embedding_bag: ids has dtype ",
              ids.scalar_type(), ", expected int32 or int64");
  need(ids, ids.scalar_type(), "ids");
  need(blob, at::kBFloat16, "blob");
  need(feat, at::kLong, "feat");
  TORCH_CHECK(ids.dim() == 2, "embedding_bag: ids must be [B, T]");
  TORCH_CHECK(blob.dim() == 2, "embedding_bag: blob must be [rows, D]");
  const int64_t B = ids.size(0), T = ids.size(1), rows = blob.size(0), D = blob.size(1);
  TORCH_CHECK(feat.dim() == 2 && feat.size(0) >= 1 && feat.size(1) == 4, "embedding_bag: feat must be [F, 4]");
  const int64_t F = feat.size(0);
  TORCH_CHECK(int64_t(features.size()) == F * 4, "embedding_bag: features has ", features.size(),
              " values, feat has ", F * 4);
  TORCH_CHECK(D % 8 == 0 && D >= tfsk::kEmbagMinD && D <= tfsk::kEmbagMaxD, "embedding_bag: D must be a multiple of 8 in [",
              tfsk::kEmbagMinD, ", ", tfsk::kEmbagMaxD, "], got ", D);
  TORCH_CHECK(T >= 1, "embedding_bag: ids has no columns");
  for (int64_t f = 0; f < F; ++f) {
    const int64_t* p = features.data() + f * 4;
    TORCH_CHECK(p[3] >= 1 && p[3] <= tfsk::kEmbagMaxHot, "embedding_bag: feature ", f, " has hotness ", p[3],
                ", supported 1 .. ", tfsk::kEmbagMaxHot);
    TORCH_CHECK(tfsk::embedding_bag_feature_ok(p[0], p[1], p[2], p[3], rows, T, D), "embedding_bag: feature ", f,
                " (row base ", p[0], ", rows ", p[1], ", first slot ", p[2], ", hotness ", p[3],
                ") does not fit the blob [", rows, ", ", D, "] / ids [., ", T, "], or its table is 2 GiB or more");
    TORCH_CHECK((p[0] * D * 2) % 16 == 0, "embedding_bag: table ", f, " must be 16-byte aligned");
  }
  TORCH_CHECK(aligned16(ids), "embedding_bag: ids must be 16-byte aligned");
  TORCH_CHECK(aligned16(blob), "embedding_bag: blob must be 16-byte aligned");
  const uint16_t* dp = nullptr;
  if (dense.has_value()) {
    need(*dense, at::kBFloat16, "dense");
    TORCH_CHECK(dense->dim() == 2 && dense->size(0) == B && dense->size(1) == D, "embedding_bag: dense must be [", B,
                ", ", D, "]");
    TORCH_CHECK(aligned16(*dense), "embedding_bag: dense must be 16-byte aligned");
    dp = bf16p(*dense);
  }
  const int64_t F0 = dp != nullptr ? 1 : 0;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(ids.device());
  Tensor y = out.has_value() ? *out : torch::empty({B, F0 + F, D}, blob.options());
  need(y, at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == B * (F0 + F) * D, "embedding_bag: out has the wrong size");
  TORCH_CHECK(aligned16(y), "embedding_bag: out must be 16-byte aligned");
  const bool i64 = ids.scalar_type() == at::kLong;
  TORCH_CHECK(tfsk::embedding_bag_supported(B, T, D, F, F0, i64),
              "embedding_bag: ids, dense and out must be smaller than 2 GiB, with at most 65535 rows per sample");
  check(tfsk::embedding_bag_launch(ids.data_ptr(), i64, bf16p(blob), feat.data_ptr<int64_t>(), dp, bf16p_mut(y), B, T,
                                   D, F, cur_stream(ids)),
        "embedding_bag");
  return y;
}

// out[b] = [dense[b] | z_i . z_j in tril order | zeros], out: [B, ceil8(Dd + pairs + pad)]
Tensor dot_interaction(const Tensor& z, const c10::optional<Tensor>& dense, bool self_interaction, int64_t pad,
                       const c10::optional<Tensor>& out) {
  need(z, at::kBFloat16, "z");
  TORCH_CHECK(z.dim() == 3, "dot_interaction: z must be [B, F, D]");
  const int64_t B = z.size(0), F = z.size(1), D = z.size(2);
  TORCH_CHECK(F >= 2 && F <= tfsk::kInteractMaxF, "dot_interaction: supports 2 <= F <= ", tfsk::kInteractMaxF,
              ", got F = ", F);
  TORCH_CHECK(D % 32 == 0 && D >= 32 && D <= tfsk::kInteractMaxD, "dot_interaction: D must be a multiple of 32 in [32, ",
              tfsk::kInteractMaxD, "], got ", D);
  TORCH_CHECK(pad >= 0, "dot_interaction: pad must be >= 0, got ", pad);
  TORCH_CHECK(aligned16(z), "dot_interaction: z must be 16-byte aligned");
  int64_t Dd = 0;
  const uint16_t* dp = nullptr;
  if (dense.has_value()) {
    need(*dense, at::kBFloat16, "dense");
    TORCH_CHECK(dense->dim() == 2 && dense->size(0) == B, "dot_interaction: dense must be [", B, ", Dd]");
    Dd = dense->size(1);
    TORCH_CHECK(Dd >= 8 && Dd % 8 == 0, "dot_interaction: Dd % 8 != 0 (Dd = ", Dd, ")");
    TORCH_CHECK(aligned16(*dense), "dot_interaction: dense must be 16-byte aligned");
    dp = bf16p(*dense);
  }
  const int64_t Wp = tfsk::dot_interaction_width(F, Dd, pad, self_interaction);
  TORCH_CHECK(Wp - Dd <= tfsk::kInteractMaxTail, "dot_interaction: pairs + pad exceed ", tfsk::kInteractMaxTail,
              " columns");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(z.device());
  Tensor y = out.has_value() ? *out : torch::empty({B, Wp}, z.options());
  need(y, at::kBFloat16, "out");
  TORCH_CHECK(y.numel() == B * Wp, "dot_interaction: out has the wrong size (expected [", B, ", ", Wp, "])");
  TORCH_CHECK(aligned16(y), "dot_interaction: out must be 16-byte aligned");
  TORCH_CHECK(tfsk::dot_interaction_supported(B, F, D, Dd, pad, self_interaction),
              "dot_interaction: operands must be smaller than 2 GiB");
  check(tfsk::dot_interaction_launch(bf16p(z), dp, bf16p_mut(y), B, F, D, Dd, pad, self_interaction, cur_stream(z)),
        "dot_interaction");
  return y;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 HIP kernels (MFMA implicit-GEMM conv/GEMM, attention, norms, pooling)";
  m.def("conv2d", &conv2d, "NHWC implicit-GEMM conv (+bias +residual +act)", py::arg("x"), py::arg("w"),
        py::arg("bias"), py::arg("residual"), py::arg("kh"), py::arg("kw"), py::arg("sh"), py::arg("sw"),
        py::arg("pt"), py::arg("pb"), py::arg("pl"), py::arg("pr"), py::arg("act") = 0, py::arg("cfg") = 0,
        py::arg("out") = py::none(), py::arg("out_f32") = false, py::arg("splits") = 1,
        py::arg("post_scale") = py::none(), py::arg("post_shift") = py::none(), py::arg("post_act") = 0,
        py::arg("out2") = py::none(), py::arg("post_only") = false);
  m.def("conv_chain", &conv_chain, "expand 1x1 (+residual, act) -> next reduce 1x1 (+act) in one kernel",
        py::arg("x"), py::arg("w1"), py::arg("b1"), py::arg("residual"), py::arg("act1"), py::arg("w2"),
        py::arg("b2"), py::arg("act2"), py::arg("x2") = py::none());
  m.def("conv_chain_supported", [](int64_t k1, int64_t n1, int64_t n2, bool dual) {
    return tfsk::conv_chain_supported(int(k1), int(n1), int(n2), dual);
  }, py::arg("k1"), py::arg("n1"), py::arg("n2"), py::arg("dual") = false);
  m.def("conv1x1_panel", &conv1x1_panel, "wide 1x1 conv (+residual, act) on the row-panel kernel: A read once",
        py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("residual"), py::arg("act"), py::arg("bm"),
        py::arg("nsplit"), py::arg("out") = py::none());
  m.def("conv1x1_panel_supported", [](int64_t m, int64_t n, int64_t k, int64_t bm, int64_t nsplit, int64_t act,
                                      const c10::optional<int64_t>& res_stride) {
    // act / res_stride: what the launch would be given (a residual's row stride must be n)
    return m < (int64_t(1) << 31) && n < (int64_t(1) << 31) &&
           tfsk::conv1x1_panel_supported(int(m), int(n), int(k), int(bm), int(nsplit)) &&
           (act == tfsk::kActNone || act == tfsk::kActRelu) && (!res_stride.has_value() || *res_stride == n);
  }, py::arg("m"), py::arg("n"), py::arg("k"), py::arg("bm"), py::arg("nsplit"), py::arg("act") = 0,
        py::arg("res_stride") = py::none());
  m.def("conv1x1_panel_forms", [](int64_t m, int64_t n, int64_t k) {
    int bm[tfsk::kPanelMaxForms], ns[tfsk::kPanelMaxForms];
    std::vector<std::pair<int64_t, int64_t>> forms;
    if (m >= (int64_t(1) << 31) || n >= (int64_t(1) << 31)) return forms;
    const int c = tfsk::conv1x1_panel_forms(int(m), int(n), int(k), bm, ns);
    for (int i = 0; i < c; ++i) forms.emplace_back(bm[i], ns[i]);
    return forms;
  }, "the (bm, nsplit) forms of conv1x1_panel worth timing for an M x N x K conv (none: unsupported)");
  m.def("conv2d_dual", &conv2d_dual, "act(conv1x1(h) + conv1x1_stride(x) + bias) as one K-concatenated GEMM",
        py::arg("h"), py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("sh"), py::arg("sw"), py::arg("act") = 0,
        py::arg("cfg") = 36, py::arg("out") = py::none(), py::arg("splits") = 1,
        py::arg("post_scale") = py::none(), py::arg("post_shift") = py::none(), py::arg("post_act") = 0,
        py::arg("out2") = py::none(), py::arg("post_only") = false);
  m.def("linear_lnx", &linear_lnx,
        "GEMM whose A / residual rows are LayerNorm inputs (statistics as partials), optionally "
        "returning its own rows' partials: {y, partials}",
        py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("residual"), py::arg("act"), py::arg("cfg"),
        py::arg("out_f32") = false, py::arg("out") = py::none(), py::arg("a_st") = py::none(),
        py::arg("a_colsum") = py::none(), py::arg("a_eps") = 1e-12, py::arg("r_st") = py::none(),
        py::arg("r_gamma") = py::none(), py::arg("r_beta") = py::none(), py::arg("r_eps") = 1e-12,
        py::arg("stats") = false);
  m.def("linear", &linear,"x @ w^T (+bias +residual +act)", py::arg("x"), py::arg("w"), py::arg("bias"),
        py::arg("residual") = py::none(), py::arg("act") = 0, py::arg("cfg") = 0, py::arg("out_f32") = false,
        py::arg("alpha") = 1.0, py::arg("out") = py::none(), py::arg("splits") = 1);
  m.def("stem_pool", &stem_pool, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("pt"), py::arg("pb"),
        py::arg("pl"), py::arg("pr"), py::arg("act"), py::arg("ppt"), py::arg("ppb"), py::arg("ppl"), py::arg("ppr"),
        py::arg("post_scale") = py::none(), py::arg("post_shift") = py::none(), py::arg("post_act") = 0);
  m.def("maxpool", &maxpool, py::arg("x"), py::arg("kh"), py::arg("kw"), py::arg("sh"), py::arg("sw"),
        py::arg("pt"), py::arg("pb"), py::arg("pl"), py::arg("pr"), py::arg("out") = py::none(),
        py::arg("post_scale") = py::none(), py::arg("post_shift") = py::none(), py::arg("post_act") = 0);
  m.def("dwconv2d", &dwconv2d, "depthwise conv: act(conv(x, w [KH*KW][C] f32) + bias), NHWC bf16", py::arg("x"),
        py::arg("w"), py::arg("bias"), py::arg("kh"), py::arg("kw"), py::arg("sh"), py::arg("sw"), py::arg("pt"),
        py::arg("pl"), py::arg("ho"), py::arg("wo"), py::arg("act") = 0, py::arg("out") = py::none(),
        py::arg("strip") = 0);
  m.def("dwconv_strip", [](int64_t n, int64_t ho, int64_t wo, int64_t c, int64_t kh, int64_t kw, int64_t sh,
                           int64_t sw) {
    return tfsk::dwconv_strip(int(n), int(ho), int(wo), int(c), int(kh), int(kw), int(sh), int(sw));
  }, "output rows per thread dwconv2d picks by itself (0: the generic kernel, which has no strips)");
  m.def("dwconv_forms", [](int64_t n, int64_t ho, int64_t wo, int64_t c, int64_t kh, int64_t kw, int64_t sh,
                           int64_t sw) {
    int forms[tfsk::kDwMaxForms];
    const int k = tfsk::dwconv_forms(int(n), int(ho), int(wo), int(c), int(kh), int(kw), int(sh), int(sw), forms);
    return std::vector<int64_t>(forms, forms + k);
  }, "the strip values dwconv2d takes for the shape: [0], [0, 2, 8] (3 x 3 strips) or [0, 2, 4] (5 x 5 strips)");
  m.def("dwconv_ln", &dwconv_ln, "depthwise 7x7 conv + bias + LayerNorm over C in one launch, NHWC bf16",
        py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("gamma"), py::arg("beta"), py::arg("eps"), py::arg("pt"),
        py::arg("pl"), py::arg("ho"), py::arg("wo"), py::arg("out") = py::none(), py::arg("kh") = 7,
        py::arg("kw") = 7, py::arg("sh") = 1, py::arg("sw") = 1);
  m.def("dwconv_ln_supported", [](int64_t n, int64_t ho, int64_t wo, int64_t c, int64_t kh, int64_t kw, int64_t sh,
                                  int64_t sw) {
    return tfsk::dwconv_ln_supported(n, ho, wo, c, int(kh), int(kw), int(sh), int(sw));
  }, "whether dwconv_ln takes the shape: 7 x 7, stride 1, C % 8 == 0, 8 <= C <= dwconv_ln_max_c");
  m.def("dwconv_ln_grid", [](int64_t n, int64_t ho, int64_t wo, int64_t c) {
    return int64_t(tfsk::dwconv_ln_grid(n, ho, wo, c));
  }, "workgroups of the dwconv_ln launch for the shape (0: nothing to launch or unsupported)");
  m.attr("dwconv_ln_max_c") = int64_t(tfsk::kDwLnMaxC);
  m.def("gconv2d", &gconv2d, "grouped 3x3 conv on MFMA: act(conv(x, w packed bf16) + bias), NHWC bf16", py::arg("x"),
        py::arg("w"), py::arg("bias"), py::arg("cg"), py::arg("sh"), py::arg("pt"), py::arg("pl"), py::arg("ho"),
        py::arg("wo"), py::arg("act") = 0, py::arg("out") = py::none(), py::arg("cg_out") = -1, py::arg("sw") = -1,
        py::arg("kh") = 3, py::arg("kw") = 3);
  m.def("gconv_supported", [](int64_t c, int64_t cg_in, int64_t cg_out, int64_t kh, int64_t kw, int64_t sh,
                              int64_t sw) {
    return tfsk::gconv_supported(int(c), int(cg_in), int(cg_out), int(kh), int(kw), int(sh), int(sw));
  }, "whether gconv2d takes C channels in groups of cg_in inputs / cg_out outputs, a kh x kw filter, strides sh x sw");
  m.def("gconv_ksteps", [](int64_t cg) { return tfsk::gconv_ksteps(int(cg)); },
        "32-deep MFMA k-steps gconv2d sums per output (zero-filled padding slots included)");
  m.def("se_gate", &se_gate, "squeeze-excite gate [B][C] f32: gate_act(act1(mean_hw(x) w1 + b1) w2 + b2)",
        py::arg("x"), py::arg("w1"), py::arg("b1"), py::arg("w2"), py::arg("b2"), py::arg("act1") = 1,
        py::arg("gate_act") = 6, py::arg("out") = py::none());
  m.def("se_scale", &se_scale, "bf16(x * gate[b][c]), NHWC bf16 x, [B][C] f32 gate", py::arg("x"), py::arg("gate"),
        py::arg("out") = py::none());
  m.def("se_gate_supported", [](int64_t b, int64_t hw, int64_t c, int64_t cr) {
    return tfsk::se_gate_supported(b, hw, c, cr);
  }, "whether se_gate takes B images of HW pixels, C channels and Cr hidden units");
  m.def("global_avgpool", &global_avgpool, py::arg("x"), py::arg("out") = py::none());
  m.def("classifier_head", &classifier_head, "softmax/argmax(mean_hw(x) @ w^T + bias)[:, :n]", py::arg("x"),
        py::arg("w"), py::arg("bias"), py::arg("n"));
  m.def("softmax_argmax", &softmax_argmax, py::arg("logits"), py::arg("want_probs") = true,
        py::arg("want_classes") = true, py::arg("probs_out") = py::none(), py::arg("classes_out") = py::none());
  m.def("dense_softmax", &dense_softmax, "softmax(x @ w[:n]^T + bias[:n]) for n <= 16 labels (x f32)",
        py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("n"));
  m.def("key_mask_adder", &key_mask_adder, "(one - m) * scale as f32", py::arg("m"), py::arg("one"),
        py::arg("scale"));
  m.def("cast_bf16", &cast_bf16, py::arg("x"), py::arg("out") = py::none());
  m.def("ingest_c4", &ingest_c4, "fp32 NHWC (C<=4) -> bf16 NHWC C=4", py::arg("x"), py::arg("out") = py::none());
  m.def("ingest_c4_padded", &ingest_c4_padded, "fp32 NHWC (C<=4) -> zero-bordered bf16 RGBA [N][Hp][Wp][4]",
        py::arg("x"), py::arg("hp"), py::arg("wp"), py::arg("pt"), py::arg("pl"));
  m.def("ingest_c4_from_host", &ingest_c4_from_host, "ingest_c4 reading a pinned host tensor (zero-copy)",
        py::arg("x"), py::arg("out"));
  m.def("h2d_rows", &h2d_rows, py::arg("host"), py::arg("dev"),
        "copy a pinned host tensor into a device tensor with a kernel (system-scope loads; capturable)");
  m.def("cast_bf16_from_host", &cast_bf16_from_host, "fp32 pinned host tensor -> bf16 device tensor",
        py::arg("x"), py::arg("out"));
  m.def("linear_ln", &linear_ln, "LN(x @ w^T + bias + residual) * gamma + beta, whole rows per workgroup",
        py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("residual"), py::arg("gamma"), py::arg("beta"),
        py::arg("eps"), py::arg("bm") = 32, py::arg("out") = py::none());
  m.def("linear_ln_supported", [](int64_t M, int64_t N, int64_t K, int64_t bm) {
    return tfsk::lngemm_supported(int(M), int(N), int(K), int(bm));
  });
  m.def("layernorm", &layernorm, py::arg("x"), py::arg("residual"), py::arg("gamma"), py::arg("beta"),
        py::arg("eps"), py::arg("out") = py::none());
  m.def("embed_ln", &embed_ln, py::arg("ids"), py::arg("type_ids"), py::arg("word"), py::arg("pos"),
        py::arg("type"), py::arg("gamma"), py::arg("beta"), py::arg("eps"), py::arg("seq"));
  m.def("classifier_head_to_host", &classifier_head_impl, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("n"),
        py::arg("probs_host"), py::arg("classes_host"),
        "classifier_head that also stores its rows into pinned host memory when it runs as one launch: "
        "(probs, classes, wrote_host)");
  m.def("attention", &attention, py::arg("qkv"), py::arg("mask_bias"), py::arg("heads"), py::arg("scale"),
        py::arg("out") = py::none(), py::arg("mask_bstride") = 0, py::arg("mask_qstride") = 0, py::arg("form") = 0,
        "form 0: the fixed-S / KV-block kernels; form 1: the register kernel for any 1 <= S <= 256");
  m.def("attention_forms", [](int64_t S) {
    int forms[2];
    const int k = tfsk::attention_forms(int(std::min<int64_t>(std::max<int64_t>(S, 0), 1 << 30)), forms);
    return std::vector<int64_t>(forms, forms + k);
  }, "the forms attention takes at length S: [0], or [0, 1] where the ragged register kernel applies");
  m.def("window_attention", &window_attention, py::arg("qkv"), py::arg("bias"), py::arg("mask"), py::arg("heads"),
        py::arg("scale"), py::arg("out") = py::none(), py::arg("grid") = py::none(),
        "windowed attention (Swin): S <= 64 tokens per window, 32-wide heads, per-head bias [H, S, S], optional "
        "shift mask [nW, S, S]; grid = (Hf, Wf, ws, shift) addresses the windows in an image-order buffer");
  m.def("window_attention_supported",
        [](int64_t R, int64_t S, int64_t H, int64_t D, int64_t nW, const c10::optional<std::vector<int64_t>>& grid) {
          if (grid.has_value() && grid->size() != 4) return false;
          const bool on = grid.has_value();
          const int64_t Hf = on ? (*grid)[0] : 0, Wf = on ? (*grid)[1] : 0, ws = on ? (*grid)[2] : 0,
                        shift = on ? (*grid)[3] : 0;
          if (on && (Hf < 1 || Wf < 1 || ws < 1)) return false;
          return tfsk::window_attention_supported(R, S, H, D, nW, Hf, Wf, ws, shift);
        },
        py::arg("R"), py::arg("S"), py::arg("H"), py::arg("D"), py::arg("nW") = 0, py::arg("grid") = py::none(),
        "whether window_attention takes R rows of H heads of width D in windows of S (nW mask windows, 0: no mask)");
  m.def("patch_tokens", &patch_tokens, "class token + patches + position embedding in one launch",
        py::arg("x"), py::arg("table"), py::arg("out") = py::none());
  m.def("patch_tokens_supported", [](int64_t b, int64_t p, int64_t c) { return tfsk::patch_tokens_supported(b, p, c); },
        "whether patch_tokens takes [B, P, C]: C % 8 == 0 and every operand below 2 GiB");
  m.def("embedding_bag", &embedding_bag, "pooled row gathers of every sparse feature (+ the dense row) in one launch",
        py::arg("ids"), py::arg("blob"), py::arg("feat"), py::arg("features"), py::arg("dense") = py::none(),
        py::arg("out") = py::none());
  m.def("embedding_bag_supported",
        [](int64_t b, int64_t t, int64_t d, const std::vector<int64_t>& features, int64_t rows, bool dense, bool ids64) {
          if (features.empty() || features.size() % 4 != 0) return false;
          const int64_t F = int64_t(features.size() / 4);
          if (!tfsk::embedding_bag_supported(b, t, d, F, dense ? 1 : 0, ids64)) return false;
          for (int64_t f = 0; f < F; ++f) {
            const int64_t* p = features.data() + f * 4;
            if (!tfsk::embedding_bag_feature_ok(p[0], p[1], p[2], p[3], rows, t, d)) return false;
          }
          return true;
        },
        py::arg("B"), py::arg("T"), py::arg("D"), py::arg("features"), py::arg("rows"), py::arg("dense") = false,
        py::arg("ids64") = true,
        "whether embedding_bag takes ids [B, T] and a blob [rows, D] with the flat (row base, V, first slot, hotness) "
        "features: D % 8 == 0 in [8, 1024], hotness 1 .. 64, every table and operand below 2 GiB");
  m.def("dot_interaction", &dot_interaction, "dense | pairwise dots in tril order | zero tail, one launch",
        py::arg("z"), py::arg("dense") = py::none(), py::arg("self_interaction") = false, py::arg("pad") = 0,
        py::arg("out") = py::none());
  m.def("dot_interaction_supported",
        [](int64_t b, int64_t f, int64_t d, int64_t dd, int64_t pad, bool self_interaction) {
          return tfsk::dot_interaction_supported(b, f, d, dd, pad, self_interaction);
        },
        py::arg("B"), py::arg("F"), py::arg("D"), py::arg("Dd") = 0, py::arg("pad") = 0,
        py::arg("self_interaction") = false,
        "whether dot_interaction takes Z [B, F, D] with Dd dense columns: 2 <= F <= 32, D % 32 == 0 in [32, 256], "
        "Dd % 8 == 0");
  m.def("dot_interaction_width",
        [](int64_t f, int64_t dd, int64_t pad, bool self_interaction) {
          return tfsk::dot_interaction_width(f, dd, pad, self_interaction);
        },
        py::arg("F"), py::arg("Dd") = 0, py::arg("pad") = 0, py::arg("self_interaction") = false,
        "row stride of dot_interaction's output: ceil8(Dd + pairs + pad)");
  m.def("splitk_counters_set_owner", [](int64_t owner) { tfsk::splitk_counters_set_owner(owner); },
        "tag the split-K counter slices this thread's captures take (0 = none)");
  m.def("splitk_counters_release", [](int64_t owner) { return tfsk::splitk_counters_release(owner); },
        "return an owner's captured split-K counter slices to the pool");
  m.def("splitk_counters_captured_in_use", []() { return tfsk::splitk_counters_captured_in_use(); });
  m.def("splitk_counters_reclaim", []() { return tfsk::splitk_counters_reclaim(); },
        "advance released captured slices (fence on their replay streams -> zero on the lane's stream -> free); "
        "never blocks; call outside any capture on this thread; returns the ints made reusable");
  m.def("splitk_counters_add_stream", [](int64_t owner, int64_t stream) {
          tfsk::splitk_counters_add_stream(owner, reinterpret_cast<hipStream_t>(stream));
        }, py::arg("owner"), py::arg("stream"),
        "another stream the owner's graph replays on (its fence must complete before the slices are reused)");
  m.def("splitk_counters_pending", []() { return tfsk::splitk_counters_pending(); });
  m.def("set_wg_trace", [](const c10::optional<Tensor>& t) {
    if (!t.has_value()) {
      g_trace = nullptr;
      g_trace_cap = 0;
      tfsk::attention_set_trace(nullptr, 0);
      return;
    }
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kLong && t->is_contiguous(), "trace: int64 device tensor");
    g_trace = reinterpret_cast<long long*>(t->data_ptr<int64_t>());
    g_trace_cap = int(std::min<int64_t>(t->numel() / 8, 1 << 30));
    tfsk::attention_set_trace(g_trace, g_trace_cap);
  }, "per-workgroup wall-clock stamps of the following GEMM / conv launches (None: off)");
  m.def("set_attention_plds", [](int64_t mode) { return tfsk::attention_set_plds(int(mode)); },
        "fixed-S attention: 1 = the P-through-LDS kernel, 0 = P in registers (default), -1 = env; returns the "
        "previous mode (process-wide; set it outside captures)");
  m.def("set_splitk_fixup", [](int64_t mode) {
    const int prev = g_fixup_override;
    g_fixup_override = mode < 0 ? -1 : (mode ? 1 : 0);
    return prev;
  }, "in-kernel split-K for this thread's following launches: 1 on, 0 off, -1 default (env, else small "
     "launches); returns the previous mode (restore it when done)");
  m.def("get_splitk_fixup", []() { return g_fixup_override; });
  m.def("classifier_head_one_launch", [](int64_t M, int64_t HW, int64_t K, int64_t Np, int64_t n) {
    return tfsk::classifier_head_one_launch(int(M), int(HW), int(K), int(Np), int(n));
  });
  m.def("relu6_config", [](int64_t cfg) { return relu6_cfg(cfg); },
        "whether the tile config's kernels implement activation relu6 (the igemm ones do)");
  m.def("num_configs", []() { return tfsk::kNumIGemmConfigs; });
  // (in the order of the rows of tile_configs.h; the GPU tests parametrize over them)
  auto ids_where = [](bool (*in_family)(tfsk::TileFamily)) {
    std::vector<int> v;
    for (int i = 0; i < tfsk::kTileTable.n; ++i)
      if (in_family(tfsk::kTileTable.rows[i].family)) v.push_back(tfsk::kTileTable.rows[i].id);
    return v;
  };
  m.def("cgemm_configs", [ids_where]() { return ids_where(tfsk::cgemm_family); });
  m.def("halo_configs", [ids_where]() { return ids_where(tfsk::halo_family); });
  m.def("halo_persist_tiles", [](int64_t n, int64_t ho, int64_t wo) {
    long tiles = 0;
    int th = 0, tw = 0, ti = 0;
    TORCH_CHECK(n > 0 && ho > 0 && wo > 0 && n * ho * wo < (int64_t(1) << 23) &&
                    tfsk::halo_persist_tiles(int(n), int(ho), int(wo), tiles, th, tw, ti),
                "halo_persist_tiles: no persistent launch for ", n, " x ", ho, " x ", wo);
    return std::make_tuple(int64_t(tiles), th, tw, ti);
  }, py::arg("n"), py::arg("ho"), py::arg("wo"),
     "(tiles, TH, TW, TI) of config 146's launch for n images of ho x wo outputs (host only; launches nothing)");
  m.def("config_tile", [](int64_t cfg) {
    const tfsk::TileConfig* c = config_of(cfg);
    TORCH_CHECK(c != nullptr, "bad tile config ", cfg);
    return std::make_pair(c->bm, c->bn);
  }, "(BM, BN) of a tile config; raises for an id that is not one");
}
