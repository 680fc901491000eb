"""The bound of dwln_bounds is met by the fused arithmetic and violated by the
unfused one, on the CPU: so test_dwln_gpu.py cannot pass on a kernel that
rounds the conv result to bf16 before the LayerNorm.

1. An fp32 torch emulation of kernels/dwln.hip (fp32 conv + bias,
   F.layer_norm, one bf16 store) is inside the bound at EVERY element.
2. The unfused pair (conv result rounded to bf16, then the LayerNorm) violates
   it at 1 % of the elements or more.

Inputs: x ~ randn (bf16), w ~ randn / 7, bias ~ 0.3 randn, gamma ~ 1 + 0.2
randn, beta ~ 0.2 randn.  Measured with these seeds: the fp32 emulation's worst
err / bound is 0.93 to 0.97 (the bound is tight in the output-rounding term);
of the unfused pair's elements 9 % to 20 % are outside, the worst 10 x to 47 x
the bound."""
import functools

import pytest
import torch.nn.functional as F

import dwln_bounds as lb
import kernel_bounds as kb
from kernel_bounds import BF, rnd

# (n, h, w, c), pads, eps
CASES = {
    "c96_9x11": ((2, 9, 11, 96), lb.SAME, 1e-6),
    "c768_7x7": ((1, 7, 7, 768), lb.SAME, 1e-6),
    "c8_3x5": ((2, 3, 5, 8), lb.SAME, 1e-6),
    "c384_14x14_eps1e-3": ((1, 14, 14, 384), lb.SAME, 1e-3),
    "c40_valid": ((2, 10, 9, 40), lb.VALID, 1e-6),
}


@functools.lru_cache(maxsize=None)
def case(name):
    shape, pads, eps = CASES[name]
    c = shape[3]
    seed = sorted(CASES).index(name) * 10 + 1300
    x = rnd(*shape, seed=seed + 1).to(BF)
    w = rnd(7, 7, c, scale=1.0 / 7.0, seed=seed + 2)
    b = rnd(c, scale=0.3, seed=seed + 3)
    gamma = 1.0 + rnd(c, scale=0.2, seed=seed + 4)
    beta = rnd(c, scale=0.2, seed=seed + 5)
    ref, bound = lb.dwln_ref(x, w, b, gamma, beta, eps, pads)
    return (x, w, b, gamma, beta), (ref, bound)


def conv32(x, w, b, pads):
    pt, pb, pl, pr = pads
    c = w.shape[2]
    wt = w.permute(2, 0, 1).reshape(c, 1, 7, 7)
    y = F.conv2d(F.pad(x.float().permute(0, 3, 1, 2), [pl, pr, pt, pb]), wt, groups=c)
    return y.permute(0, 2, 3, 1) + b


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_arithmetic_is_inside_the_bound_everywhere(name):
    shape, pads, eps = CASES[name]
    (x, w, b, gamma, beta), (ref, bound) = case(name)
    y = F.layer_norm(conv32(x, w, b, pads), (shape[3],), gamma, beta, eps).to(BF)
    worst = kb.assert_within(y, ref, bound, f"dwln fp32 emulation {name}")
    print(f"dwln fp32 emulation {name}: worst err / bound = {worst:.3f}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_unfused_arithmetic_violates_the_bound(name):
    shape, pads, eps = CASES[name]
    (x, w, b, gamma, beta), (ref, bound) = case(name)
    mid = conv32(x, w, b, pads).to(BF)                      # dwconv2d's output
    y = F.layer_norm(mid.float(), (shape[3],), gamma, beta, eps).to(BF)
    ratio = (y.double() - ref).abs() / bound
    frac = (ratio > 1.0).double().mean().item()
    print(f"dwln unfused {name}: {int((ratio > 1.0).sum())} of {ratio.numel()} elements outside, "
          f"worst err / bound = {ratio.max().item():.1f}")
    assert frac >= 0.01, f"{name}: only {frac:.4f} of the elements violate the bound"
