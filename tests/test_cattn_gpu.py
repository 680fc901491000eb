"""causal_attention (kernels/cattn.hip) against kernel_bounds.attention_ref, the
fp64 reference with its elementwise bound, given the -inf upper triangle (plus
the key adder) as a [B, 1, S, S] mask.

The lengths lie on both sides of the 64-key block and of either query-block
height (64 / 128 rows, both forced through ``qb``), leave a ragged last block,
and reach five key blocks so that the two-deep K / V buffer wraps twice.
Causality and isolation are checked bit for bit: a row's result may not depend
on a later token, another image or another head."""
import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")
LENGTHS = (1, 17, 63, 64, 65, 127, 128, 129, 200, 320)
SCALE = 1 / 8
_REF = {}


def hip():
    from rust_tensorflow_serving2_amd.ops import hip as _hip
    return _hip()


def inputs(b, s, h):
    return kb.rnd(b, s, 3 * h * 64, seed=2000 + 7 * s + b).to(BF)


def padding_adder(b, s):
    a = torch.zeros(b, s)
    a[:, s - s // 4:] = -10000.0
    return a


def reference(qkv, h, adder, tag):
    """(ref, bound) of the causal attention, computed once per input (tag names it)."""
    if tag not in _REF:
        b, s, _ = qkv.shape
        mask = torch.triu(torch.full((s, s), float("-inf")), 1).expand(b, 1, s, s).clone()
        if adder is not None:
            mask = mask + adder[:, None, None, :]
        _REF[tag] = kb.attention_ref(qkv, h, SCALE, mask)
    return _REF[tag]


@pytest.mark.parametrize("qb", [64, 128])
@pytest.mark.parametrize("padded", [False, True], ids=["no-adder", "right-padded"])
@pytest.mark.parametrize("s", LENGTHS)
def test_within_bound_inside_guard_bands(s, padded, qb):
    """qkv and out are views into NaN-filled buffers: nothing outside qkv reaches a result, nothing outside out is
    written."""
    b, h = 2, 2
    qkv = inputs(b, s, h)
    adder = padding_adder(b, s) if padded else None
    n_in, n_out, guard = qkv.numel(), b * s * h * 64, 4096          # guard: elements, a 16-B multiple
    big_in = torch.full((guard + n_in + guard,), NAN, dtype=BF, device="cuda")
    big_in[guard:guard + n_in] = qkv.cuda().reshape(-1)
    big_out = torch.full((guard + n_out + guard,), NAN, dtype=BF, device="cuda")
    out = big_out[guard:guard + n_out].view(b, s, h * 64)
    y = hip().causal_attention(big_in[guard:guard + n_in].view(b, s, 3 * h * 64), None if adder is None else adder.cuda(),
                               h, SCALE, out, qb)
    assert y.data_ptr() == out.data_ptr()
    ref, bound = reference(qkv, h, adder, (s, padded))
    worst = kb.assert_within(y, ref, bound, f"causal attention S={s} padded={padded} qb={qb}")
    print(f"causal attention S={s} padded={padded} qb={qb}: worst err/bound {worst:.3f}")
    assert torch.isnan(big_out[:guard]).all() and torch.isnan(big_out[guard + n_out:]).all(), "a guard element was written"
    assert torch.isnan(big_in[:guard]).all() and torch.isnan(big_in[guard + n_in:]).all()


@pytest.mark.parametrize("qb", [64, 128])
@pytest.mark.parametrize("cut", [0, 63, 64, 130])
def test_rows_do_not_see_later_tokens(cut, qb):
    """Tokens > cut overwritten with +-3e4 (finite: a closed key's 0 x Inf is NaN in the reference graph too):
    rows <= cut are bit-equal.  An off-by-one on the diagonal or a stale LDS buffer shows here."""
    b, s, h = 2, 200, 2
    qkv = inputs(b, s, h)
    first = hip().causal_attention(qkv.cuda(), None, h, SCALE, None, qb)
    later = qkv.clone()
    later[:, cut + 1:] = torch.where(kb.rnd(b, s - cut - 1, 3 * h * 64, seed=5) > 0, 3e4, -3e4).to(BF)
    second = hip().causal_attention(later.cuda(), None, h, SCALE, None, qb)
    assert torch.isfinite(second[:, :cut + 1]).all()
    assert torch.equal(first[:, :cut + 1], second[:, :cut + 1])


@pytest.mark.parametrize("what", ["image", "head"])
@pytest.mark.parametrize("bad", [0, 1])
def test_nan_neighbour_leaves_the_clean_one_bit_equal(bad, what):
    s, h, good = 129, 2, 1 - bad
    qkv = inputs(2, s, h).reshape(2, s, 3, h, 64)
    if what == "image":
        solo = hip().causal_attention(qkv[good:good + 1].reshape(1, s, -1).contiguous().cuda(), None, h, SCALE)[0]
        qkv[bad] = NAN
        both = hip().causal_attention(qkv.reshape(2, s, -1).cuda(), None, h, SCALE)[good]
    else:
        solo = hip().causal_attention(qkv[:, :, :, good].reshape(2, s, -1).contiguous().cuda(), None, 1, SCALE)
        qkv[:, :, :, bad] = NAN
        both = hip().causal_attention(qkv.reshape(2, s, -1).cuda(), None, h, SCALE)[..., good * 64:good * 64 + 64]
    assert torch.equal(solo, both)


def test_rerun_is_bit_equal():
    b, s, h = 2, 200, 3
    x, a = inputs(b, s, h).cuda(), padding_adder(b, s).cuda()
    first = hip().causal_attention(x, a, h, SCALE).clone()
    hip().causal_attention(inputs(b, 320, h).cuda(), None, h, SCALE)      # leaves other values in LDS
    assert torch.equal(hip().causal_attention(x, a, h, SCALE), first)


@pytest.mark.parametrize("b,s,h,qb", [(64, 128, 8, 0), (128, 128, 8, 128), (1, 1024, 2, 0), (1, 1024, 2, 128)],
                         ids=["1024-workgroups", "1024-workgroups-qb128", "S1024", "S1024-qb128"])
def test_launch_geometries(b, s, h, qb):
    """More workgroups than the machine has CUs, and GPT-2's real length once."""
    qkv = inputs(b, s, h)
    y = hip().causal_attention(qkv.cuda(), None, h, SCALE, None, qb)
    ref, bound = reference(qkv, h, None, ("geometry", b, s, h))
    kb.assert_within(y, ref, bound, f"causal attention {b} x {s} x {h} qb={qb}")


def test_rejections():
    H = hip()

    def z(*shape):
        return torch.zeros(*shape, dtype=BF, device="cuda")
    assert H.causal_attention_supported(1, 64) and H.causal_attention_supported(4096, 64)
    assert not H.causal_attention_supported(0, 64) and not H.causal_attention_supported(4097, 64)
    assert not H.causal_attention_supported(128, 32)
    with pytest.raises(RuntimeError, match="head_dim 64"):
        H.causal_attention(z(1, 50, 96), None, 1, SCALE)
    with pytest.raises(RuntimeError, match="1 <= S"):
        H.causal_attention(z(1, 0, 192), None, 1, SCALE)
    with pytest.raises(RuntimeError, match="1 <= S"):
        H.causal_attention(z(1, 4097, 192), None, 1, SCALE)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        H.causal_attention(z(1 * 50 * 192 + 8)[4:-4].view(1, 50, 192), None, 1, SCALE)
    for adder in (torch.zeros(2, 49), torch.zeros(3, 50), torch.zeros(50)):
        with pytest.raises(RuntimeError, match="key_adder must be"):
            H.causal_attention(z(2, 50, 192), adder.cuda(), 1, SCALE)
    with pytest.raises(RuntimeError, match="dtype"):
        H.causal_attention(z(2, 50, 192), torch.zeros(2, 50, dtype=torch.float64, device="cuda"), 1, SCALE)
    with pytest.raises(RuntimeError, match="wrong size"):
        H.causal_attention(z(2, 50, 192), None, 1, SCALE, z(2, 50, 128))
    with pytest.raises(RuntimeError, match="out must be 16-byte aligned"):
        H.causal_attention(z(1, 50, 192), None, 1, SCALE, z(50 * 64 + 8)[4:-4].view(1, 50, 64))
