"""The scheme of attention_ragged_kernel (kernels/attention.hip, form 1),
emulated in torch on the CPU, against kernel_bounds.attention_ref:

* K, V and Q padded with zero rows to SP = max(64, ceil32(S)) keys (what the
  buffer descriptors return past the image);
* scores in fp32, s = (q . k) scale + mask, then keys >= S closed by a SELECT
  to -inf before the row maximum;
* p = exp(s - max) in fp32, summed unrounded in fp32, rounded to bf16 for P V;
* P V accumulated in fp32, divided by the sum, stored as bf16.

It must meet the bound at every length, and the two ways of getting the
padding wrong must violate it -- so the bound is shown to see them:

1. padded keys left at score 0 (no select): their p = exp(0 - max) joins the
   sum;
2. padded keys "masked" by adding -10000 to their zero score: harmless while
   the live scores are near 0, wrong on a row whose live scores are far below
   -10000 (a mask adder of -30000 on every live key: the softmax over the live
   keys does not change, but the padded keys at -10000 now win the maximum).

Both show on rows of very negative live scores, which is the input used.
"""
import pytest
import torch

import kernel_bounds as kb

BF = torch.bfloat16
LENGTHS = (1, 5, 33, 50, 65, 197, 255)
LOW = -30000.0


def padded_length(s):
    return max(64, (s + 31) // 32 * 32)


def emulate(qkv, heads, scale, mask, padding="select"):
    """qkv [B, S, 3 H 64] bf16, mask None or a [B, S] key adder -> [B, S, H 64] bf16."""
    b, s, hd3 = qkv.shape
    d = hd3 // (3 * heads)
    sp = padded_length(s)
    q, k, v = qkv.float().reshape(b, s, 3, heads, d).permute(2, 0, 3, 1, 4)         # [B, H, S, D] each
    zeros = torch.zeros(b, heads, sp - s, d)
    k, v = torch.cat([k, zeros], 2), torch.cat([v, zeros], 2)
    sc = (q @ k.transpose(-1, -2)) * scale                                           # padded keys: exactly 0
    m = torch.zeros(b, sp)
    if mask is not None:
        m[:, :s] = mask
    sc = sc + m[:, None, None, :]
    dead = torch.arange(sp) >= s
    if padding == "select":
        sc = torch.where(dead, torch.full_like(sc, float("-inf")), sc)
    elif padding == "add -10000":
        sc = sc + torch.where(dead, -10000.0, 0.0)
    else:
        assert padding == "left at 0"
    p = torch.exp(sc - sc.amax(-1, keepdim=True))
    total = p.sum(-1, keepdim=True)
    o = (p.to(BF).float() @ v) / total
    return o.to(BF).permute(0, 2, 1, 3).reshape(b, s, heads * d)


def case(s):
    b, h = 2, 2
    qkv = kb.rnd(b, s, 3 * h * 64, seed=500 + s).to(BF)
    low = torch.full((b, s), LOW)
    return qkv, h, low


@pytest.mark.parametrize("s", LENGTHS)
def test_scheme_meets_the_bound(s):
    qkv, h, low = case(s)
    part = torch.zeros_like(low)
    part[1, s // 2:] = -10000.0
    part[1, 0] = 0.0
    for name, mask in (("none", None), ("key", part), ("all keys -30000", low)):
        ref, bound = kb.attention_ref(qkv, h, 1 / 8, mask)
        worst = kb.assert_within(emulate(qkv, h, 1 / 8, mask), ref, bound, f"ragged scheme S={s} mask {name}")
        print(f"S={s} SP={padded_length(s)} mask {name}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("padding", ["left at 0", "add -10000"])
@pytest.mark.parametrize("s", LENGTHS)
def test_wrong_padding_violates_the_bound(s, padding):
    qkv, h, low = case(s)
    ref, bound = kb.attention_ref(qkv, h, 1 / 8, low)
    y = emulate(qkv, h, 1 / 8, low, padding)
    assert padded_length(s) > s
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within(y, ref, bound, f"S={s} padded keys {padding}")


def test_padded_length_table():
    assert [padded_length(s) for s in (1, 50, 64, 65, 96, 97, 197, 224, 225, 255, 256)] == \
        [64, 64, 64, 96, 96, 128, 224, 224, 256, 256, 256]


def test_attention_forms_table():
    from rust_tensorflow_serving2_amd.ops import hip
    forms = hip().attention_forms
    for s in (64, 128, 192, 256):
        assert forms(s) == [0], s
    for s in (257, 384, 512, 577, 4096):
        assert forms(s) == [0], s
    for s in (1, 5, 50, 63, 65, 100, 127, 129, 191, 193, 197, 255):
        assert forms(s) == [0, 1], s
