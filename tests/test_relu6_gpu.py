"""ReLU6 as an epilogue of the GEMM / conv kernels (activation code 5).

ReLU6 is built into the igemm family (which takes every shape and operand
mode) and the split-K reduce; each is held to the elementwise bound of
dwconv_bounds.relu6_epilogue (the clamp is exact and 1-Lipschitz, so the ReLU
bound holds; docs/numerics.md).  cgemm was left without it because the extra
case cost 61 of its kernels registers, bgemm and halo to keep the ResNet / BERT
kernels byte-identical (profiles/dwconv/resources_before_after.txt,
docs/benchmarks.md "MobileNet"): their bindings raise for relu6 and
ops.candidates(relu6=True) offers none of their configs.  The smallest M / N
that fill one tile plus a partial one; pre-activations ~ N(3, 4.45^2), so about
a quarter of the outputs is clamped on each side -- asserted on the reference.
The bindings reject activation codes their kernels do not implement instead of
running them as "none"."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import dwconv_bounds as db  # noqa: E402
import kernel_bounds as kb  # noqa: E402
from kernel_bounds import BF, rnd  # noqa: E402
from rust_tensorflow_serving2_amd import ops  # noqa: E402
from rust_tensorflow_serving2_amd.ops import ACT, BGEMM, HALO_PERSIST, hip  # noqa: E402

DEV = torch.device("cuda:0")
RELU6 = ACT["relu6"]
SPREAD = 4.45            # 0.6745 * 4.45 = 3: quartiles of N(3, 4.45^2) at 0 and 6

IGEMM_CFG = 3            # 64 x 64: N = 72 is one tile plus an 8-column tail
CGEMM_CFG = 36
BGEMM_CFG = sorted(BGEMM)[0]
HALO_CFG = next(c for c in hip().halo_configs() if c != HALO_PERSIST)


def dev(t):
    return None if t is None else t.to(DEV)


def clamped_both_sides(pre):
    lo, hi = (pre < 0).double().mean().item(), (pre > 6).double().mean().item()
    assert 0.12 < lo < 0.38 and 0.12 < hi < 0.38, (lo, hi)


def test_relu6_code_matches_the_kernels():
    assert RELU6 == 5


@pytest.mark.parametrize("cfg", [IGEMM_CFG, 0, 12])
def test_linear_relu6_within_bound(cfg):
    m, n = kb.tile_shape(*hip().config_tile(cfg))
    assert cfg != IGEMM_CFG or n == 72
    k = 128
    x = rnd(m, k, seed=1).to(BF)
    w = rnd(n, k, scale=SPREAD / math.sqrt(k), seed=2).to(BF)
    b = 3.0 + rnd(n, scale=0.3, seed=3)
    pre, mag = kb.gemm_parts(x, w, b)
    clamped_both_sides(pre)
    for splits in (1, 2):
        for out_f32 in (False, True):
            out = torch.full((m, n), float("nan"), device=DEV, dtype=torch.float32 if out_f32 else BF)
            y = hip().linear(dev(x), dev(w), dev(b), None, RELU6, cfg, out_f32, 1.0, out, splits)
            ref, bound = db.relu6_epilogue(pre, mag, k, splits, out_f32)
            kb.assert_within(y, ref, bound, f"linear relu6 cfg {cfg} splits={splits} f32={out_f32}")
            assert (y.float() == 6.0).any() and (y.float() == 0.0).any()


def pack_w(w_hwio):
    kh, kw, cin, cout = w_hwio.shape
    k = kh * kw * cin
    kp = -(-k // 64) * 64
    w = w_hwio.permute(3, 0, 1, 2).reshape(cout, k)
    return torch.cat([w, torch.zeros(cout, kp - k)], 1).to(BF).contiguous().to(DEV)


@pytest.mark.parametrize("what,cfg,k,s,pads", [("1x1 dense", IGEMM_CFG, 1, 1, (0, 0, 0, 0)),
                                               ("1x1 stride 2", IGEMM_CFG, 1, 2, (0, 0, 0, 0)),
                                               ("3x3 stride 1", 1, 3, 1, (1, 1, 1, 1)),
                                               ("3x3 stride 2", IGEMM_CFG, 3, 2, (0, 1, 0, 1))])
def test_conv_relu6_within_bound(what, cfg, k, s, pads):
    n, h, w, cin, cout = 5, 7, 9, 64, 72
    x = rnd(n, h, w, cin, seed=11).to(BF)
    wt = rnd(k, k, cin, cout, scale=SPREAD / math.sqrt(k * k * cin), seed=12).to(BF).float()
    b = 3.0 + rnd(cout, scale=0.3, seed=13)
    pre, mag = kb.conv_parts(x, wt, b, s, pads)
    clamped_both_sides(pre)
    for splits in (1, 2):
        out = torch.full(tuple(pre.shape), float("nan"), device=DEV, dtype=BF)
        y = hip().conv2d(dev(x), pack_w(wt), dev(b), None, k, k, s, s, *pads, act=RELU6, cfg=cfg, out=out,
                         splits=splits)
        ref, bound = db.relu6_epilogue(pre, mag, k * k * cin, splits)
        kb.assert_within(y, ref, bound, f"conv relu6 {what} cfg {cfg} splits={splits}")
        assert (y.float() == 6.0).any() and (y.float() == 0.0).any()


@pytest.mark.parametrize("cfg", [IGEMM_CFG, 1])
def test_padded_rgba_stem_relu6_within_bound(cfg):
    """MobileNet's first layer: 3x3 / 2 on RGB through the padded-RGBA operand
    mode (zero-bordered bf16 RGBA, filter rows padded to 4 x 8 taps x 4 ch)."""
    n, h, w, c, cout, k, s = 2, 19, 17, 3, 72, 3, 2
    x = (rnd(n, h, w, c, seed=21)).to(BF).float()          # the ingest rounds to bf16: start there
    wt = rnd(k, k, c, cout, scale=SPREAD / math.sqrt(k * k * c), seed=22).to(BF).float()
    b = 3.0 + rnd(cout, scale=0.3, seed=23)
    pads = (0, 1, 0, 1)
    ho, wo = (h + pads[0] + pads[1] - k) // s + 1, (w + pads[2] + pads[3] - k) // s + 1
    khp = k + k % 2
    w4 = torch.zeros(khp, 8, 4, cout)
    w4[:k, :k, :c, :] = wt
    wp = w4.permute(3, 0, 1, 2).reshape(cout, khp * 32).to(BF).contiguous().to(DEV)
    pre, mag = kb.conv_parts(x, wt, b, s, pads)
    clamped_both_sides(pre)
    xp = hip().ingest_c4_padded(dev(x), (ho - 1) * s + khp, (wo - 1) * s + 8, pads[0], pads[2])
    out = torch.full((n, ho, wo, cout), float("nan"), device=DEV, dtype=BF)
    y = hip().conv2d(xp, wp, dev(b), None, khp, 8, s, s, 0, 0, 0, 0, act=RELU6, cfg=cfg, out=out)
    ref, bound = db.relu6_epilogue(pre, mag, khp * 32, 1)
    kb.assert_within(y, ref, bound, f"padded RGBA stem relu6 cfg {cfg}")
    assert (y.float() == 6.0).any() and (y.float() == 0.0).any()


def test_cgemm_bgemm_and_halo_are_left_without_relu6():
    """Only the igemm kernels have the ReLU6 case: the bindings say so for every
    other family instead of running "none" (conv2d_dual runs on cgemm alone),
    and the tuner never offers their configs to a relu6 launch -- while it
    still offers them without."""
    igemm_ids = set(range(hip().num_configs()))
    other_ids = set(hip().cgemm_configs()) | set(hip().halo_configs())
    assert {CGEMM_CFG, BGEMM_CFG, HALO_CFG, HALO_PERSIST} <= other_ids and not (igemm_ids & other_ids)
    assert all(hip().relu6_config(c) for c in igemm_ids) and not any(hip().relu6_config(c) for c in other_ids)
    x = torch.zeros(256, 64, dtype=BF, device=DEV)
    w = torch.zeros(64, 64, dtype=BF, device=DEV)
    w9 = torch.zeros(64, 576, dtype=BF, device=DEV)
    b = torch.zeros(64, device=DEV)
    x4 = x.reshape(1, 16, 16, 64)
    for splits in (1, 2):
        for cfg in (CGEMM_CFG, BGEMM_CFG):
            with pytest.raises(RuntimeError, match="relu6"):
                hip().linear(x, w, b, None, RELU6, cfg, splits=splits)
            with pytest.raises(RuntimeError, match="relu6"):
                hip().conv2d(x4, w, b, None, 1, 1, 1, 1, 0, 0, 0, 0, act=RELU6, cfg=cfg, splits=splits)
        for cfg in (HALO_CFG, HALO_PERSIST):
            with pytest.raises(RuntimeError, match="relu6"):
                hip().conv2d(x4, w9, b, None, 3, 3, 1, 1, 1, 1, 1, 1, act=RELU6, cfg=cfg, splits=splits)
        with pytest.raises(RuntimeError, match="relu6"):
            hip().conv2d_dual(x4, x4, torch.zeros(64, 128, dtype=BF, device=DEV), b, 1, 1, RELU6, CGEMM_CFG, None,
                              splits)
    # the same launches with relu are fine: it is the activation that is refused
    assert hip().conv2d(x4, w9, b, None, 3, 3, 1, 1, 1, 1, 1, 1, act=ACT["relu"], cfg=HALO_CFG).shape == (1, 16, 16, 64)
    for m, n, k, flags in ((2048, 256, 256, dict(aligned64=True)), (1024, 64, 576, dict(aligned64=True, halo=True)),
                           (96, 1280, 320, dict(aligned64=True)), (4096, 32, 128, dict(aligned64=True, stem=True))):
        with6 = {c for c, _s in ops.candidates(m, n, k, relu6=True, **flags)}
        without = {c for c, _s in ops.candidates(m, n, k, **flags)}
        assert with6 and with6 <= igemm_ids, (m, n, k, sorted(with6 - igemm_ids))
        assert without & other_ids and with6 == without - other_ids      # the default is today's list


def test_bindings_reject_unknown_activation_codes():
    x = torch.zeros(64, 64, dtype=BF, device=DEV)
    w = torch.zeros(64, 64, dtype=BF, device=DEV)
    b = torch.zeros(64, device=DEV)
    x4 = x.reshape(1, 8, 8, 64)
    for act in (6, -1, 99):
        for cfg in (IGEMM_CFG, CGEMM_CFG, BGEMM_CFG):
            with pytest.raises(RuntimeError, match="unknown activation"):
                hip().linear(x, w, b, None, act, cfg)
        for cfg in (IGEMM_CFG, CGEMM_CFG):
            with pytest.raises(RuntimeError, match="activation"):
                hip().conv2d(x4, w, b, None, 1, 1, 1, 1, 0, 0, 0, 0, act=act, cfg=cfg)
        with pytest.raises(RuntimeError, match="activation"):
            hip().conv2d_dual(x4, x4, torch.zeros(64, 128, dtype=BF, device=DEV), b, 1, 1, act, CGEMM_CFG)
    # the deferred-LayerNorm epilogue and the post-activation outputs have no ReLU6
    with pytest.raises(RuntimeError, match="activation"):
        hip().linear_lnx(x, w, b, None, RELU6, CGEMM_CFG)
    with pytest.raises(RuntimeError, match="post activation"):
        hip().conv2d(x4, w, b, None, 1, 1, 1, 1, 0, 0, 0, 0, act=0, cfg=CGEMM_CFG, post_scale=b, post_shift=b,
                     post_act=RELU6, post_only=True)
    with pytest.raises(RuntimeError, match="post activation"):
        hip().maxpool(x4, 3, 3, 2, 2, 0, 1, 0, 1, post_scale=b, post_shift=b, post_act=RELU6)
