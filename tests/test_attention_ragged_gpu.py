"""attention(form=1): the register-resident kernel for any 1 <= S <= 256.

Every case runs form 1 against kernel_bounds.attention_ref (fp64 reference,
elementwise bound) through kb.assert_within.  The lengths cover every padded
instantiation (64 ... 256 in steps of 32), both sides of each 32 and 64
boundary, a last query block with one live row (65, 129, 193) and fully dead
waves (1, 5, 65: rows 16.. of the last block).  The guard-band, isolation and
many-workgroup cases are what catches a dead query row stored into the next
image, a K / V row read past the image, and stale LDS meeting a closed key.
"""
import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LENGTHS = (1, 5, 31, 33, 50, 63, 65, 100, 127, 129, 191, 193, 197, 223, 225, 255)
NAN = float("nan")


def hip():
    from rust_tensorflow_serving2_amd.ops import hip as _hip
    return _hip()


def dev(t):
    return None if t is None else t.cuda()


def masks_for(b, s):
    """(name, mask for the reference, mask tensor for the kernel, bstride, qstride)."""
    key = torch.zeros(b, s)
    key[b - 1, s // 2:] = -10000.0
    key[b - 1, 0] = 0.0                                       # S = 1: keep the one key open
    full = torch.triu(torch.full((s, s), -10000.0), 1).expand(b, 1, s, s).contiguous()
    out = [("none", None, 0, 0), ("key", key, s, 0), ("per-query", full, s * s, s)]
    if s > 64:
        for name, fill in (("-10000", -10000.0), ("-inf", float("-inf")), ("f32 min", torch.finfo(torch.float32).min)):
            m = torch.zeros(b, s)
            m[:, :64] = fill
            out.append((f"first 64 keys {name}", m, s, 0))
    return out


_REF = {}


def reference(qkv, h, scale, mask, tag):
    """attention_ref computed once per input (tag names it) and never modified."""
    if tag not in _REF:
        _REF[tag] = kb.attention_ref(qkv, h, scale, mask)
    return _REF[tag]


def inputs(b, s, h):
    return kb.rnd(b, s, 3 * h * 64, seed=1000 + 7 * s + b).to(BF)


@pytest.mark.parametrize("b,h", [(1, 1), (2, 3)])
@pytest.mark.parametrize("s", LENGTHS)
def test_ragged_within_bound(s, b, h):
    scale = 1 / 8
    qkv = inputs(b, s, h)
    x = dev(qkv)
    for name, mask, bstride, qstride in masks_for(b, s):
        y = hip().attention(x, dev(mask), h, scale, None, bstride, qstride, form=1)
        ref, bound = reference(qkv, h, scale, mask, (s, b, h, name))
        assert torch.isfinite(y).all(), f"S={s} {name}: non-finite output"
        worst = kb.assert_within(y, ref, bound, f"attention form 1 S={s} b={b} h={h} mask {name}")
        print(f"attention form 1 S={s} b={b} h={h} mask {name}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("s", (1, 50, 65, 197, 255))
def test_ragged_guard_bands(s):
    """qkv and out are views into larger NaN-filled buffers: nothing past the
    last image is read into a live result, nothing outside out is written."""
    b, h, scale = 2, 2, 1 / 8
    qkv = inputs(b, s, h)
    n_in, n_out, guard = qkv.numel(), b * s * h * 64, 4096          # guard: elements, a 16-B multiple
    big_in = torch.full((guard + n_in + guard,), NAN, dtype=BF, device="cuda")
    big_in[guard:guard + n_in] = dev(qkv).reshape(-1)
    big_out = torch.full((guard + n_out + guard,), NAN, dtype=BF, device="cuda")
    x = big_in[guard:guard + n_in].view(b, s, 3 * h * 64)
    out = big_out[guard:guard + n_out].view(b, s, h * 64)
    key = torch.zeros(b, s)
    key[0, s // 2 + 1:] = -10000.0
    for name, mask, bstride in (("none", None, 0), ("key", key, s)):
        big_out[guard:guard + n_out] = NAN
        y = hip().attention(x, dev(mask), h, scale, out, bstride, 0, form=1)
        assert y.data_ptr() == out.data_ptr()
        ref, bound = reference(qkv, h, scale, mask, ("guard", s, name))
        assert torch.isfinite(y).all(), f"S={s} {name}: non-finite output (a row past the image was read?)"
        kb.assert_within(y, ref, bound, f"guarded attention form 1 S={s} mask {name}")
        assert torch.isnan(big_out[:guard]).all() and torch.isnan(big_out[guard + n_out:]).all(), \
            f"S={s} {name}: a guard element of the output buffer was written"
    assert torch.isnan(big_in[:guard]).all() and torch.isnan(big_in[guard + n_in:]).all()


@pytest.mark.parametrize("bad", (0, 1))
@pytest.mark.parametrize("s", (5, 65, 197))
def test_ragged_image_isolation(s, bad):
    """One image all NaN: the other image's rows are within bound."""
    h, scale = 2, 1 / 8
    qkv = inputs(2, s, h)
    good = 1 - bad
    ref, bound = reference(qkv, h, scale, None, ("iso", s))
    poisoned = qkv.clone()
    poisoned[bad] = NAN
    y = hip().attention(dev(poisoned), None, h, scale, None, 0, 0, form=1)
    kb.assert_within(y[good], ref[good], bound[good], f"S={s}: image {good} beside a NaN image {bad}")


@pytest.mark.parametrize("bad", (0, 1))
@pytest.mark.parametrize("s", (5, 65, 197))
def test_ragged_head_isolation(s, bad):
    """One head's Q, K and V columns NaN: the other head is within bound."""
    h, scale = 2, 1 / 8
    qkv = inputs(2, s, h)
    good = 1 - bad
    ref, bound = reference(qkv, h, scale, None, ("iso", s))
    poisoned = qkv.clone().reshape(2, s, 3, h, 64)
    poisoned[:, :, :, bad] = NAN
    y = hip().attention(dev(poisoned.reshape(2, s, 3 * h * 64)), None, h, scale, None, 0, 0, form=1)
    cols = slice(good * 64, good * 64 + 64)
    kb.assert_within(y[..., cols], ref[..., cols], bound[..., cols], f"S={s}: head {good} beside a NaN head {bad}")


@pytest.mark.parametrize("s", (33, 197))
def test_ragged_reruns_bit_equal(s):
    b, h = 2, 3
    x = dev(inputs(b, s, h))
    key = torch.zeros(b, s)
    key[1, s // 2:] = -10000.0
    m = dev(key)
    first = hip().attention(x, m, h, 1 / 8, None, s, 0, form=1).clone()
    # another launch in between leaves other values in LDS
    hip().attention(dev(inputs(b, 255, h)), None, h, 1 / 8, None, 0, 0, form=1)
    for _ in range(3):
        assert torch.equal(hip().attention(x, m, h, 1 / 8, None, s, 0, form=1), first)


def test_ragged_more_workgroups_than_cus():
    """One launch of 11 * 12 * 4 = 528 workgroups (S = 197: four query blocks)."""
    b, s, h = 11, 197, 12
    qkv = inputs(b, s, h)
    y = hip().attention(dev(qkv), None, h, 1 / 8, None, 0, 0, form=1)
    ref, bound = kb.attention_ref(qkv, h, 1 / 8, None)
    kb.assert_within(y, ref, bound, "attention form 1, 528 workgroups")


@pytest.mark.parametrize("s", (50, 197))
def test_both_forms_within_bound_of_the_reference(s):
    b, h = 2, 3
    qkv = inputs(b, s, h)
    key = torch.zeros(b, s)
    key[1, s // 2:] = -10000.0
    ref, bound = kb.attention_ref(qkv, h, 1 / 8, key)
    for form in (0, 1):
        y = hip().attention(dev(qkv), dev(key), h, 1 / 8, None, s, 0, form=form)
        kb.assert_within(y, ref, bound, f"attention form {form} S={s}")


def test_attention_forms_binding():
    f = hip().attention_forms
    assert [f(s) for s in (64, 128, 192, 256, 257, 577)] == [[0]] * 6
    assert [f(s) for s in (1, 50, 65, 197, 255)] == [[0, 1]] * 5


def test_binding_rejections():
    H = hip()
    with pytest.raises(RuntimeError, match="1 <= S"):
        H.attention(torch.zeros(1, 0, 192, dtype=BF, device="cuda"), None, 1, 0.125, form=1)
    with pytest.raises(RuntimeError, match="form 1 supports 1 <= S <= 256"):
        H.attention(torch.zeros(1, 257, 192, dtype=BF, device="cuda"), None, 1, 0.125, form=1)
    with pytest.raises(RuntimeError, match="head_dim 64"):
        H.attention(torch.zeros(1, 50, 96, dtype=BF, device="cuda"), None, 1, 0.125, form=1)
    with pytest.raises(RuntimeError, match="unknown form"):
        H.attention(torch.zeros(1, 50, 192, dtype=BF, device="cuda"), None, 1, 0.125, form=2)
