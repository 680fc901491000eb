"""The checker of the swish and sigmoid-gate bounds (swish_bounds.py) tested on
the CPU, as test_se_bounds_cpu.py tests se_bounds: the Lipschitz constants hold
on an fp64 grid, an fp32 torch emulation of each kernel (the operation sequence
of kernels/common.h: product, exp2, add, reciprocal, product) passes its bound,
and each plausible mistake -- hard-swish for swish, the sigmoid alone, x
sigma(2x), ReLU for swish in act1, a hard-sigmoid gate, FC weights rounded to
bf16, a gate from the neighbouring image -- fails it."""
import math

import pytest
import torch
import torch.nn.functional as F

import dwconv_bounds as db
import kernel_bounds as kb
import se_bounds as sb
import swish_bounds as wb
from kernel_bounds import BF, rnd

SHAPE = (3, 7, 5, 24, 8)        # B, H, W, C, Cr


def test_lipschitz_constants_on_a_grid():
    x = torch.linspace(-40.0, 40.0, 800001, dtype=torch.float64)
    s = torch.sigmoid(x)
    dswish = s * (1.0 + x * (1.0 - s))
    i = int(dswish.abs().argmax())
    assert abs(dswish[i].item() - 1.09984) < 1e-5 and abs(x[i].item() - 2.3994) < 1e-3
    assert dswish.abs().max().item() < wb.L_SWISH
    assert (s * (1.0 - s)).max().item() <= wb.L_SIGMOID
    # finite differences agree: the constants bound the functions wb.swish64 / wb.sigmoid64 themselves
    step = (x[1] - x[0]).item()
    assert (wb.swish64(x)[1:] - wb.swish64(x)[:-1]).abs().max().item() <= wb.L_SWISH * step
    assert (wb.sigmoid64(x)[1:] - wb.sigmoid64(x)[:-1]).abs().max().item() <= wb.L_SIGMOID * step * (1 + 1e-9)
    # swish and hard-swish differ by up to 0.142 (where a test must tell them apart)
    gap = (wb.swish64(x) - sb.hard_swish64(x)).abs().max().item()
    assert 0.13 < gap < 0.15, gap


def test_own_error_of_the_fp32_sequence_on_a_grid():
    """Every fp32 x of a dense grid over [-100, 100], and the tails: the
    emulated sequence is inside swish_own / sigmoid_own alone (no accumulation
    error, no output rounding)."""
    x = torch.cat([torch.linspace(-100.0, 100.0, 400001), torch.tensor([-1e4, -200.0, -88.0, -87.0, 0.0, 88.0, 1e4])])
    x64 = x.double()
    worst = kb.assert_within(wb.swish_f32(x), wb.swish64(x64), wb.swish_own(x64), "swish own error")
    assert worst < 0.75, worst
    worst = kb.assert_within(wb.sigmoid_f32(x), wb.sigmoid64(x64), wb.sigmoid_own(x64), "sigmoid own error")
    assert worst < 0.75, worst
    # the limits without special cases
    assert wb.swish_f32(torch.tensor([-1e4]))[0].item() == 0.0 and wb.swish_f32(torch.tensor([1e4]))[0].item() == 1e4
    assert wb.sigmoid_f32(torch.tensor([-1e4, 1e4])).tolist() == [0.0, 1.0]


# ---------------------------------------------------------------- epilogues
MISTAKES = {
    "hard_swish": lambda y: y * (torch.clamp(y + 3.0, 0.0, 6.0) * (1.0 / 6.0)),
    "sigmoid_alone": lambda y: torch.sigmoid(y),
    "x_sigmoid_2x": lambda y: y * torch.sigmoid(2.0 * y),
}


@pytest.fixture(scope="module")
def dw_case():
    x = rnd(2, 9, 11, 16, seed=1).to(BF)
    w = rnd(5, 5, 16, scale=3.0 / 5.0, seed=2)
    b = rnd(16, scale=0.3, seed=3)
    pre, mag = db.dw_parts(x, w, b, 2, (2, 2, 2, 2))
    wt = w.permute(2, 0, 1).reshape(16, 1, 5, 5)
    y = F.conv2d(F.pad(x.float().permute(0, 3, 1, 2), [2, 2, 2, 2]), wt, stride=2, groups=16).permute(0, 2, 3, 1) + b
    return pre, mag, y


def test_swish_inputs_cover_both_tails(dw_case):
    pre, _mag, _y = dw_case
    lo, hi = (pre < -3).double().mean().item(), (pre > 3).double().mean().item()
    assert 0.10 < lo < 0.25 and 0.10 < hi < 0.25, (lo, hi)


def test_swish_depthwise_emulation_within_bound(dw_case):
    pre, mag, y = dw_case
    ref, bound = wb.swish_dw(pre, mag, 25)
    kb.assert_within(wb.swish_f32(y).to(BF), ref, bound, "dwconv swish emulation")


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_swish_depthwise_mistakes_fail(dw_case, mistake):
    pre, mag, y = dw_case
    ref, bound = wb.swish_dw(pre, mag, 25)
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within(MISTAKES[mistake](y).to(BF), ref, bound, mistake)


def test_swish_gemm_emulation_within_bound():
    m, n, k = 70, 72, 128
    x = rnd(m, k, seed=1).to(BF)
    w = rnd(n, k, scale=3.0 / math.sqrt(k), seed=2).to(BF)
    b = rnd(n, scale=0.3, seed=3)
    pre, mag = kb.gemm_parts(x, w, b)
    y = x.float() @ w.float().t() + b
    for out_f32 in (False, True):
        ref, bound = wb.swish_epilogue(pre, mag, k, 1, out_f32)
        out = wb.swish_f32(y)
        kb.assert_within(out if out_f32 else out.to(BF), ref, bound, f"gemm swish emulation f32={out_f32}")
        for name, wrong in MISTAKES.items():
            with pytest.raises(AssertionError, match="outside the bound"):
                kb.assert_within(wrong(y) if out_f32 else wrong(y).to(BF), ref, bound, name)


# ---------------------------------------------------------------- se_gate
def gate32(x, w1, b1, w2, b2, act1="swish", gate="sigmoid", bf16_weights=False):
    """se_gate in fp32 torch, with the mistakes as switches."""
    if bf16_weights:
        w1, w2 = w1.to(BF).float(), w2.to(BF).float()
    pre1 = x.float().mean(dim=(1, 2)) @ w1 + b1
    h = {"swish": wb.swish_f32, "relu": torch.relu, "none": lambda t: t}[act1](pre1)
    pre2 = h @ w2 + b2
    return wb.sigmoid_f32(pre2) if gate == "sigmoid" else torch.clamp(pre2 + 3.0, 0.0, 6.0) * (1.0 / 6.0)


@pytest.fixture(scope="module")
def se_case():
    ins = wb.se_inputs(*SHAPE, act1="swish", seed=100)
    ref, bound, pre2 = wb.se_gate_parts(*ins, "swish", "sigmoid")
    return ins, ref, bound, pre2


def test_gate_inputs_reach_both_tails(se_case):
    _ins, ref, _bound, pre2 = se_case
    assert (pre2 < -3).any() and (pre2 > 3).any() and ((pre2 > -3) & (pre2 < 3)).double().mean() > 0.4
    assert ref.min() < 0.05 and ref.max() > 0.95


@pytest.mark.parametrize("act1,gate", [("swish", "sigmoid"), ("relu", "sigmoid"), ("none", "sigmoid"),
                                       ("swish", "hard_sigmoid")])
def test_gate_emulation_within_bound(act1, gate):
    ins = wb.se_inputs(*SHAPE, act1=act1, seed=100)
    ref, bound, _pre2 = wb.se_gate_parts(*ins, act1, gate)
    worst = kb.assert_within(gate32(*ins, act1=act1, gate=gate), ref, bound, f"se_gate emulation {act1} {gate}")
    assert worst < 0.5         # fp32 torch rounds to nearest: half of E per operation at the most


def test_reference_agrees_with_se_bounds_where_both_apply():
    ins = sb.se_inputs(*SHAPE, act1="relu", seed=100)
    a, b = sb.se_gate_parts(*ins, "relu"), wb.se_gate_parts(*ins, "relu", "hard_sigmoid")
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("mistake", [dict(act1="relu"), dict(gate="hard_sigmoid"), dict(bf16_weights=True)],
                         ids=lambda m: "-".join(f"{k}={v}" for k, v in m.items()))
def test_gate_mistakes_fail(se_case, mistake):
    ins, ref, bound, _pre2 = se_case
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within(gate32(*ins, **mistake), ref, bound, str(mistake))


def test_gate_from_the_neighbouring_image_fails(se_case):
    ins, ref, bound, _pre2 = se_case
    g = gate32(*ins)
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within(g.roll(1, 0), ref, bound, "rolled gate")
    oref, obound = wb.se_op_ref(*ins, "swish", "sigmoid")
    x = ins[0]
    kb.assert_within((x.float() * g[:, None, None, :]).to(BF), oref, obound, "se op emulation")
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within((x.float() * g.roll(1, 0)[:, None, None, :]).to(BF), oref, obound, "op, neighbour's gate")
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within((x.float() * gate32(*ins, bf16_weights=True)[:, None, None, :]).to(BF), oref, obound,
                         "op, bf16 weights")
