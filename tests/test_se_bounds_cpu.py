"""The checker of the hard-swish and squeeze-excite bounds (se_bounds.py) tested
on the CPU, as test_kernel_bounds_cpu.py tests kernel_bounds: an fp32 torch
emulation of each kernel passes its bound, and each plausible mistake -- a sum
for a mean, a dropped bias, the wrong activation, the wrong scale, a gate from
the neighbouring image, weights rounded to bf16 -- fails it."""
import math

import pytest
import torch
import torch.nn.functional as F

import dwconv_bounds as db
import kernel_bounds as kb
import se_bounds as sb
from kernel_bounds import BF, rnd

SHAPE = (3, 7, 5, 24, 8)        # B, H, W, C, Cr


def hsig32(x):
    return torch.clamp(x + 3.0, 0.0, 6.0) * (1.0 / 6.0)


def gate32(x, w1, b1, w2, b2, act1="relu", mean=True, use_b1=True, use_b2=True, relu6=False, bf16_weights=False):
    """se_gate in fp32 torch, with the mistakes as switches."""
    if bf16_weights:
        w1, w2 = w1.to(BF).float(), w2.to(BF).float()
    xf = x.float()
    p = xf.mean(dim=(1, 2)) if mean else xf.sum(dim=(1, 2))
    pre1 = p @ w1 + (b1 if use_b1 else 0.0)
    h = torch.clamp(pre1, 0.0, 6.0) if relu6 else (torch.relu(pre1) if act1 == "relu" else pre1)
    return hsig32(h @ w2 + (b2 if use_b2 else 0.0))


def scale32(x, gate):
    return (x.float() * gate[:, None, None, :]).to(BF)


@pytest.fixture(scope="module")
def se_case():
    ins = sb.se_inputs(*SHAPE, act1="relu", seed=100)
    ref, bound, pre2 = sb.se_gate_parts(*ins, "relu")
    return ins, ref, bound, pre2


def test_inputs_reach_both_clamps_and_the_relu6_knee(se_case):
    ins, _ref, _bound, pre2 = se_case
    x, w1, b1, _w2, _b2 = ins
    assert (pre2 < -3).any() and (pre2 > 3).any() and ((pre2 > -3) & (pre2 < 3)).double().mean() > 0.4
    pre1 = kb.d(x).mean(dim=(1, 2)) @ kb.d(w1) + kb.d(b1)
    assert (pre1 > 6).any() and (pre1 < 0).any()


@pytest.mark.parametrize("act1", ["relu", "none"])
def test_gate_emulation_within_bound(act1):
    ins = sb.se_inputs(*SHAPE, act1=act1, seed=100)
    ref, bound = sb.se_gate_ref(*ins, act1)
    worst = kb.assert_within(gate32(*ins, act1=act1), ref, bound, f"se_gate emulation {act1}")
    assert worst < 0.5         # fp32 torch rounds to nearest: half of E per operation at the most


@pytest.mark.parametrize("mistake", [dict(mean=False), dict(use_b1=False), dict(use_b2=False), dict(relu6=True),
                                     dict(bf16_weights=True)])
def test_gate_mistakes_fail(se_case, mistake):
    ins, ref, bound, _pre2 = se_case
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within(gate32(*ins, **mistake), ref, bound, str(mistake))


def test_gate_from_the_neighbouring_image_fails(se_case):
    ins, ref, bound, _pre2 = se_case
    g = gate32(*ins)
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within(g.roll(1, 0), ref, bound, "rolled gate")
    x = ins[0]
    sref, sbound = sb.se_scale_ref(x, g)
    kb.assert_within(scale32(x, g), sref, sbound, "se_scale emulation")
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within(scale32(x, g.roll(1, 0)), sref, sbound, "se_scale with the neighbour's gate")
    # a truncating store (2^-7) instead of round-to-nearest-even (2^-8) fails too
    trunc = ((x.float() * g[:, None, None, :]).view(torch.int32) & -65536).view(torch.float32)
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within(trunc, sref, sbound, "truncated se_scale")


def test_op_emulation_within_bound(se_case):
    ins, _ref, _bound, _pre2 = se_case
    ref, bound = sb.se_op_ref(*ins, "relu")
    kb.assert_within(scale32(ins[0], gate32(*ins)), ref, bound, "se op emulation")
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within(scale32(ins[0], gate32(*ins, bf16_weights=True)), ref, bound, "se op, bf16 weights")


def test_hard_sigmoid_scale_of_slim_is_outside_the_kernel_bound_but_far_inside_bf16():
    """0.16667 for 1/6 is 2e-5 off: more than the 3 E of the fp32 gate, so the
    kernels use 1/6 itself; next to a bf16 store (2^-9) it is nothing."""
    assert 3 * kb.E < abs(0.16667 - 1 / 6) < 1e-4 / 6 < 2.0 ** -9 / 6


# ---------------------------------------------------------------- hard-swish
def hswish32(x, upper=True, scale=1.0 / 6.0):
    t = torch.clamp(x + 3.0, 0.0, 6.0) if upper else torch.relu(x + 3.0)
    return x * (t * scale)


@pytest.fixture(scope="module")
def dw_case():
    x = rnd(2, 9, 11, 16, seed=1).to(BF)
    w = rnd(5, 5, 16, scale=3.0 / 5.0, seed=2)
    b = rnd(16, scale=0.3, seed=3)
    pads = (2, 2, 2, 2)
    pre, mag = db.dw_parts(x, w, b, 2, pads)
    wt = w.permute(2, 0, 1).reshape(16, 1, 5, 5)
    y = F.conv2d(F.pad(x.float().permute(0, 3, 1, 2), [2, 2, 2, 2]), wt, stride=2, groups=16).permute(0, 2, 3, 1) + b
    return pre, mag, y


def test_hard_swish_inputs_cover_both_clamps_and_the_curve(dw_case):
    pre, _mag, _y = dw_case
    lo, hi = (pre < -3).double().mean().item(), (pre > 3).double().mean().item()
    assert 0.10 < lo < 0.25 and 0.10 < hi < 0.25, (lo, hi)


def test_hard_swish_depthwise_emulation_within_bound(dw_case):
    pre, mag, y = dw_case
    ref, bound = sb.hard_swish_dw(pre, mag, 25)
    kb.assert_within(hswish32(y).to(BF), ref, bound, "dwconv hard-swish emulation")


@pytest.mark.parametrize("mistake", [dict(upper=False), dict(scale=0.2)])
def test_hard_swish_mistakes_fail(dw_case, mistake):
    pre, mag, y = dw_case
    ref, bound = sb.hard_swish_dw(pre, mag, 25)
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within(hswish32(y, **mistake).to(BF), ref, bound, str(mistake))


def test_hard_swish_gemm_emulation_within_bound():
    m, n, k = 70, 72, 128
    x = rnd(m, k, seed=1).to(BF)
    w = rnd(n, k, scale=3.0 / math.sqrt(k), seed=2).to(BF)
    b = rnd(n, scale=0.3, seed=3)
    pre, mag = kb.gemm_parts(x, w, b)
    y = x.float() @ w.float().t() + b
    for out_f32 in (False, True):
        ref, bound = sb.hard_swish_epilogue(pre, mag, k, 1, out_f32)
        out = hswish32(y) if out_f32 else hswish32(y).to(BF)
        kb.assert_within(out, ref, bound, f"gemm hard-swish emulation f32={out_f32}")
        with pytest.raises(AssertionError, match="outside the bound"):
            kb.assert_within(torch.clamp(y, 0.0, 6.0) if out_f32 else torch.clamp(y, 0.0, 6.0).to(BF), ref, bound,
                             "relu6 for hard-swish")


def test_hard_sigmoid_reference():
    x = torch.tensor([-4.0, -3.0, 0.0, 1.5, 3.0, 5.0], dtype=torch.float64)
    assert torch.equal(sb.hard_sigmoid64(x), torch.tensor([0.0, 0.0, 0.5, 0.75, 1.0, 1.0], dtype=torch.float64))
    assert torch.allclose(sb.hard_swish64(x), x * sb.hard_sigmoid64(x))
