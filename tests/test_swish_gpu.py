"""Swish (activation code 9) where hard-swish is built in: the depthwise kernels
(every form dwconv_forms offers, the 5x5 strips included), the igemm family and
the split-K reduce, each under the elementwise bound of swish_bounds.py
(Lipschitz 1.1, own error |x| sigma ((1 - sigma)(1 + 1.5 |x|) + 4) E;
docs/numerics.md "Swish and sigmoid").  EVERY output element is checked, every
output buffer is pre-filled with NaN.  Pre-activations are ~ N(0, 3^2): asserted
on the reference, 10-25 % lie below -3 and 10-25 % above +3, so both tails and
the curved part are hit (and hard-swish in swish's place, up to 0.142 away,
cannot pass).  cgemm, bgemm, halo, the dual conv and the deferred-LayerNorm GEMM
are left without it and say so; sigmoid (code 8) is a gate activation and no
GEMM / conv / depthwise epilogue takes it.  Each test prints its worst
error / bound."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import dwconv_bounds as db  # noqa: E402
import kernel_bounds as kb  # noqa: E402
import swish_bounds as wb  # noqa: E402
from kernel_bounds import BF, rnd  # noqa: E402
from rust_tensorflow_serving2_amd import ops  # noqa: E402
from rust_tensorflow_serving2_amd.graph.ops import tf_same_pads  # noqa: E402
from rust_tensorflow_serving2_amd.ops import ACT, BGEMM, HALO_PERSIST, hip  # noqa: E402

DEV = torch.device("cuda:0")
SWISH = ACT["swish"]
SPREAD = 3.0

# (n, h, w, c), (kh, kw), (sh, sw), padding -- test_hard_swish_gpu.DW_CASES
DW_CASES = {
    "centre_tap_only": ((1, 1, 1, 8), (3, 3), (1, 1), "SAME"),
    "h_ne_w_3_chunks": ((2, 7, 5, 24), (3, 3), (1, 1), "SAME"),
    "s2_same_odd_even": ((1, 9, 12, 8), (3, 3), (2, 2), "SAME"),
    "explicit": ((1, 6, 6, 8), (3, 3), (1, 1), (2, 0, 0, 2)),
    "generic_5x5": ((1, 9, 9, 8), (5, 5), (1, 1), "SAME"),
    "partial_wave_s2": ((2, 33, 33, 136), (3, 3), (2, 2), "SAME"),
    "generic_5x5_s2_explicit": ((1, 9, 11, 16), (5, 5), (2, 2), (2, 2, 2, 2)),
}
IGEMM_CFGS = list(range(hip().num_configs()))
CGEMM_CFG = 36
BGEMM_CFG = sorted(BGEMM)[0]
HALO_CFG = next(c for c in hip().halo_configs() if c != HALO_PERSIST)


def dev(t):
    return None if t is None else t.to(DEV)


def both_tails_and_the_curve(pre):
    lo, hi = (pre < -3).double().mean().item(), (pre > 3).double().mean().item()
    assert 0.10 < lo < 0.25 and 0.10 < hi < 0.25, (lo, hi)


def test_codes_match_the_kernels():
    assert ACT == {"none": 0, "relu": 1, "gelu_tanh": 2, "gelu_erf": 3, "tanh": 4, "relu6": 5, "hard_sigmoid": 6,
                   "hard_swish": 7, "sigmoid": 8, "swish": 9}
    assert ops.IGEMM_ONLY_ACTS == ("relu6", "hard_swish", "swish")


# ---------------------------------------------------------------- depthwise
def geometry(shape, k, s, padding):
    _n, h, w, _c = shape
    if padding == "SAME":
        pads = tf_same_pads(h, k[0], s[0]) + tf_same_pads(w, k[1], s[1])
    else:
        pads = tuple(padding)
    ho = (h + pads[0] + pads[1] - k[0]) // s[0] + 1
    wo = (w + pads[2] + pads[3] - k[1]) // s[1] + 1
    return pads, ho, wo


@functools.lru_cache(maxsize=None)
def dw_case(name):
    shape, k, s, padding = DW_CASES[name]
    pads, ho, wo = geometry(shape, k, s, padding)
    c = shape[3]
    seed = sorted(DW_CASES).index(name) * 10 + 500
    x = rnd(*shape, seed=seed + 1).to(BF)
    w = rnd(k[0], k[1], c, scale=SPREAD / math.sqrt(k[0] * k[1]), seed=seed + 2)
    b = rnd(c, scale=0.3, seed=seed + 3)
    # windows on the border see fewer taps: the filter is rescaled by the reference's own spread,
    # so that the pre-activations have standard deviation 3 over the whole output
    w = w * (SPREAD / max(db.dw_parts(x, w, 0 * b, s, pads)[0].std().item(), 1e-3)) if shape[1] * shape[2] > 1 else w
    pre, mag = db.dw_parts(x, w, b, s, pads)
    assert pre.shape == (shape[0], ho, wo, c)
    return (x.to(DEV), w.reshape(k[0] * k[1], c).contiguous().to(DEV), b.to(DEV)), (pre, mag), (pads, ho, wo)


def forms_of(name):
    shape, k, s, _padding = DW_CASES[name]
    _pads, ho, wo = dw_case(name)[2]
    return tuple(hip().dwconv_forms(shape[0], ho, wo, shape[3], k[0], k[1], s[0], s[1]))


@pytest.mark.parametrize("name", sorted(DW_CASES))
def test_dwconv_swish_within_bound(name):
    shape, k, s, _padding = DW_CASES[name]
    (x, w, b), (pre, mag), (pads, ho, wo) = dw_case(name)
    if pre.numel() >= 500:
        # (SAME borders see fewer taps, so the tails are a little lighter than N(0, 3^2)'s 16 %)
        both_tails_and_the_curve(pre)
    ref, bound = wb.swish_dw(pre, mag, k[0] * k[1])
    for strip in forms_of(name):
        out = torch.full((shape[0], ho, wo, shape[3]), float("nan"), dtype=BF, device=DEV)
        y = hip().dwconv2d(x, w, b, k[0], k[1], s[0], s[1], pads[0], pads[2], ho, wo, SWISH, out, strip)
        assert y.data_ptr() == out.data_ptr()
        worst = kb.assert_within(y, ref, bound, f"dwconv swish {name} strip={strip}")
        print(f"dwconv swish {name} strip={strip}: worst err / bound = {worst:.3f}")


def test_dw_cases_reach_every_kernel():
    assert forms_of("generic_5x5") == (0, 2, 4) and forms_of("generic_5x5_s2_explicit") == (0, 2, 4)
    assert forms_of("partial_wave_s2") == (0, 2, 8) and forms_of("h_ne_w_3_chunks") == (0, 2, 8)


# ---------------------------------------------------------------- GEMM / conv
@pytest.mark.parametrize("cfg", IGEMM_CFGS)
def test_linear_swish_within_bound(cfg):
    """One full tile plus a partial one; N % 8 != 0 on the 64-wide tiles' case
    (N = 68: the scalar tail of the epilogue and of the split-K reduce)."""
    m, n = kb.tile_shape(*hip().config_tile(cfg))
    k = 128
    worst = 0.0
    for n_, with_res in ((n, False), (n - 4, False), (n, True)):
        x = rnd(m, k, seed=1).to(BF)
        w = rnd(n_, k, scale=SPREAD / math.sqrt(k), seed=2).to(BF)
        b = rnd(n_, scale=0.3, seed=3)
        res = rnd(m, n_, scale=0.5, seed=4).to(BF) if with_res else None
        pre, mag = kb.gemm_parts(x, w, b, res)
        both_tails_and_the_curve(pre)
        for splits in (1, 2):
            for out_f32 in (False, True):
                out = torch.full((m, n_), float("nan"), device=DEV, dtype=torch.float32 if out_f32 else BF)
                y = hip().linear(dev(x), dev(w), dev(b), dev(res), SWISH, cfg, out_f32, 1.0, out, splits)
                ref, bound = wb.swish_epilogue(pre, mag, k, splits, out_f32)
                worst = max(worst, kb.assert_within(y, ref, bound, f"linear swish cfg {cfg} n={n_} res={with_res} "
                                                                   f"splits={splits} f32={out_f32}"))
    print(f"linear swish cfg {cfg}: worst err / bound = {worst:.3f}")


def pack_w(w_hwio):
    kh, kw, cin, cout = w_hwio.shape
    k = kh * kw * cin
    kp = -(-k // 64) * 64
    w = w_hwio.permute(3, 0, 1, 2).reshape(cout, k)
    return torch.cat([w, torch.zeros(cout, kp - k)], 1).to(BF).contiguous().to(DEV)


CONV_GEOMS = [("1x1 dense", 1, 1, (0, 0, 0, 0)), ("1x1 stride 2", 1, 2, (0, 0, 0, 0)),
              ("3x3 stride 1", 3, 1, (1, 1, 1, 1)), ("3x3 stride 2", 3, 2, (0, 1, 0, 1))]


@functools.lru_cache(maxsize=None)
def conv_case(k, s, pads, with_res):
    n, h, w, cin, cout = 5, 7, 9, 64, 72
    x = rnd(n, h, w, cin, seed=11).to(BF)
    wt = rnd(k, k, cin, cout, scale=SPREAD / math.sqrt(k * k * cin), seed=12).to(BF).float()
    b = rnd(cout, scale=0.3, seed=13)
    ho, wo = (h + pads[0] + pads[1] - k) // s + 1, (w + pads[2] + pads[3] - k) // s + 1
    res = rnd(n, ho, wo, cout, scale=0.5, seed=14).to(BF) if with_res else None
    pre, mag = kb.conv_parts(x, wt, b, s, pads, res)
    return dev(x), pack_w(wt), dev(b), dev(res), pre, mag


@pytest.mark.parametrize("cfg", IGEMM_CFGS)
def test_conv_swish_within_bound(cfg):
    """The shapes of test_relu6_gpu.py (5 x 7 x 9 x 64 -> 72 channels: a partial
    tile in M and an 8-column tail in N) on every igemm config."""
    worst = 0.0
    for what, k, s, pads in CONV_GEOMS:
        for with_res in ((False, True) if k == 1 and s == 1 else (False,)):
            x, w, b, res, pre, mag = conv_case(k, s, pads, with_res)
            if pre.numel() >= 500:
                both_tails_and_the_curve(pre)
            for splits in (1, 2):
                out = torch.full(tuple(pre.shape), float("nan"), device=DEV, dtype=BF)
                y = hip().conv2d(x, w, b, res, k, k, s, s, *pads, act=SWISH, cfg=cfg, out=out, splits=splits)
                ref, bound = wb.swish_epilogue(pre, mag, k * k * 64, splits)
                worst = max(worst, kb.assert_within(y, ref, bound, f"conv swish {what} cfg {cfg} res={with_res} "
                                                                   f"splits={splits}"))
    print(f"conv swish cfg {cfg}: worst err / bound = {worst:.3f}")


# ---------------------------------------------------------------- rejections
def test_other_families_are_left_without_swish():
    igemm_ids = set(IGEMM_CFGS)
    other_ids = set(hip().cgemm_configs()) | set(hip().halo_configs())
    assert all(hip().relu6_config(c) for c in igemm_ids) and not any(hip().relu6_config(c) for c in other_ids)
    x = torch.zeros(256, 64, dtype=BF, device=DEV)
    w = torch.zeros(64, 64, dtype=BF, device=DEV)
    w9 = torch.zeros(64, 576, dtype=BF, device=DEV)
    wd = torch.zeros(64, 128, dtype=BF, device=DEV)
    b = torch.zeros(64, device=DEV)
    x4 = x.reshape(1, 16, 16, 64)
    launches = [lambda act, cfg=cfg: hip().linear(x, w, b, None, act, cfg) for cfg in (CGEMM_CFG, BGEMM_CFG)]
    launches += [lambda act, cfg=cfg: hip().conv2d(x4, w9, b, None, 3, 3, 1, 1, 1, 1, 1, 1, act=act, cfg=cfg)
                 for cfg in (HALO_CFG, HALO_PERSIST)]
    launches += [lambda act: hip().conv2d_dual(x4, x4, wd, b, 1, 1, act, CGEMM_CFG),
                 lambda act: hip().linear_lnx(x, w, b, None, act, CGEMM_CFG)]
    for launch in launches:
        with pytest.raises(RuntimeError, match=r"(?<!hard_)swish"):
            launch(SWISH)
        out = launch(ACT["relu"])                 # it is the activation that is refused
        assert (out[0] if isinstance(out, (list, tuple)) else out).numel() == 256 * 64
    for m, n, k, flags in ((2048, 256, 256, dict(aligned64=True)), (1024, 64, 576, dict(aligned64=True, halo=True)),
                           (96, 1280, 320, dict(aligned64=True)), (4096, 32, 128, dict(aligned64=True, stem=True))):
        default = ops.candidates(m, n, k, **flags)
        only = ops.candidates(m, n, k, igemm_act=True, **flags)
        assert only and only == [cs for cs in default if cs[0] not in other_ids]


def test_sigmoid_is_no_epilogue_anywhere():
    x = torch.zeros(64, 64, dtype=BF, device=DEV)
    w = torch.zeros(64, 64, dtype=BF, device=DEV)
    b = torch.zeros(64, device=DEV)
    x4 = x.reshape(1, 8, 8, 64)
    for cfg in (3, CGEMM_CFG):
        with pytest.raises(RuntimeError, match="unknown activation"):
            hip().linear(x, w, b, None, 8, cfg)
        with pytest.raises(RuntimeError, match="activation"):
            hip().conv2d(x4, w, b, None, 1, 1, 1, 1, 0, 0, 0, 0, act=8, cfg=cfg)
    with pytest.raises(RuntimeError, match="unknown activation"):
        hip().linear_lnx(x, w, b, None, 8, CGEMM_CFG)
    with pytest.raises(RuntimeError, match="activation"):
        hip().dwconv2d(x4, torch.zeros(9, 64, device=DEV), b, 3, 3, 1, 1, 1, 1, 8, 8, 8)
    y = hip().dwconv2d(x4, torch.zeros(9, 64, device=DEV), b, 3, 3, 1, 1, 1, 1, 8, 8, SWISH)
    assert y.shape == (1, 8, 8, 64) and (y == 0).all()
