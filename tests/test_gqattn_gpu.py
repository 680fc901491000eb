"""rope_gqa_attention (kernels/gqattn.hip) against gqattn_bounds.rope_gqa_ref, the
fp64 reference (rotation in fp64 from the bf16 inputs, K / V heads expanded, the
-inf triangle plus the adder) with its elementwise bound.

The lengths lie on both sides of the 64-key block and of every query-block
height (16 / 32 / 64 rows for G = 4, 8 / 2 / 1), leave a ragged last block and
reach four key blocks, so the two-deep K / V buffer wraps.  The head counts take
every tile mapping: G = 1, 2, 4, 8.  Causality and isolation are bit for bit."""
import pytest
import torch

import gqattn_bounds as gb
import kernel_bounds as kb

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")
SCALE = 1 / 8
HEADS = [(2, 2), (4, 2), (8, 2), (8, 1)]
_REF = {}


def hip():
    from rust_tensorflow_serving2_amd.ops import hip as _hip
    return _hip()


def inputs(b, s, h, k):
    return kb.rnd(b, s, (h + 2 * k) * 64, seed=3000 + 7 * s + b + h).to(BF)


def tables(s, first=0):
    """Llama's tables (theta 10000), rows first .. first + s - 1, one half: (cos, sin) [s, 32] f32."""
    from rust_tensorflow_serving2_amd.models import llama
    cos, sin = llama.rope_tables(first + s)
    return torch.from_numpy(cos[0, 0, first:, :32].copy()), torch.from_numpy(sin[0, 0, first:, :32].copy())


def padding_adder(b, s):
    a = torch.zeros(b, s)
    a[:, s - s // 4:] = -10000.0
    return a


def run(qkv, tab, adder, h, k, out=None):
    return hip().rope_gqa_attention(qkv.cuda(), tab[0].cuda(), tab[1].cuda(), None if adder is None else adder.cuda(),
                                    h, k, SCALE, out)


def reference(qkv, tab, h, k, adder, tag):
    if tag not in _REF:
        _REF[tag] = gb.rope_gqa_ref(qkv, tab[0], tab[1], h, k, SCALE, adder)
    return _REF[tag]


@pytest.mark.parametrize("padded", [False, True], ids=["no-adder", "right-padded"])
@pytest.mark.parametrize("h,k", HEADS)
@pytest.mark.parametrize("s", [1, 17, 64, 65, 129, 200])
def test_within_bound_inside_guard_bands(s, h, k, padded):
    """qkv and out are views into NaN-filled buffers: nothing outside qkv reaches a result, nothing outside out is
    written."""
    b = 2
    qkv, tab = inputs(b, s, h, k), tables(s)
    adder = padding_adder(b, s) if padded else None
    n_in, n_out, guard = qkv.numel(), b * s * h * 64, 4096          # guard: elements, a 16-B multiple
    big_in = torch.full((guard + n_in + guard,), NAN, dtype=BF, device="cuda")
    big_in[guard:guard + n_in] = qkv.cuda().reshape(-1)
    big_out = torch.full((guard + n_out + guard,), NAN, dtype=BF, device="cuda")
    out = big_out[guard:guard + n_out].view(b, s, h * 64)
    y = run(big_in[guard:guard + n_in].view(b, s, -1), tab, adder, h, k, out)
    assert y.data_ptr() == out.data_ptr()
    ref, bound = reference(qkv, tab, h, k, adder, (s, h, k, padded))
    worst = kb.assert_within(y, ref, bound, f"rope gqa attention S={s} H={h}/{k} padded={padded}")
    print(f"rope gqa attention S={s} H={h}/{k} padded={padded}: worst err/bound {worst:.3f}")
    assert torch.isnan(big_out[:guard]).all() and torch.isnan(big_out[guard + n_out:]).all(), "a guard element was written"
    assert torch.isnan(big_in[:guard]).all() and torch.isnan(big_in[guard + n_in:]).all()


@pytest.mark.parametrize("h,k", [(4, 2), (8, 1)])
@pytest.mark.parametrize("cut", [0, 63, 64, 130])
def test_rows_do_not_see_later_tokens(cut, h, k):
    """Tokens > cut overwritten with +-3e4 (finite): rows <= cut are bit-equal."""
    b, s = 2, 200
    qkv, tab = inputs(b, s, h, k), tables(s)
    first = run(qkv, tab, None, h, k)
    later = qkv.clone()
    later[:, cut + 1:] = torch.where(kb.rnd(b, s - cut - 1, qkv.shape[2], seed=5) > 0, 3e4, -3e4).to(BF)
    second = run(later, tab, None, h, k)
    assert torch.isfinite(second[:, :cut + 1]).all()
    assert torch.equal(first[:, :cut + 1], second[:, :cut + 1])


@pytest.mark.parametrize("what", ["group", "query-head"])
@pytest.mark.parametrize("bad", [0, 1])
def test_nan_neighbour_leaves_the_clean_one_bit_equal(bad, what):
    s, h, k, good = 129, 4, 2, 1 - bad
    qkv, tab = inputs(2, s, h, k), tables(s)
    q, kv = qkv[..., :h * 64].reshape(2, s, h, 64).clone(), qkv[..., h * 64:].reshape(2, s, 2, k, 64).clone()
    if what == "group":                # the other K / V head and its two query heads: a run of the clean group alone
        solo = run(torch.cat([q[:, :, 2 * good:2 * good + 2].reshape(2, s, -1),
                              kv[:, :, :, good].reshape(2, s, -1)], -1).contiguous(), tab, None, 2, 1)
        q[:, :, 2 * bad:2 * bad + 2], kv[:, :, :, bad] = NAN, NAN
        both = run(torch.cat([q.reshape(2, s, -1), kv.reshape(2, s, -1)], -1), tab, None, h, k)
        assert torch.equal(solo, both[..., good * 128:good * 128 + 128])
    else:                              # one query head of group 0: the other three heads as in the clean run
        clean = run(qkv, tab, None, h, k)
        q[:, :, bad] = NAN
        both = run(torch.cat([q.reshape(2, s, -1), kv.reshape(2, s, -1)], -1), tab, None, h, k)
        keep = [i for i in range(h * 64) if i // 64 != bad]
        assert torch.equal(clean[..., keep], both[..., keep])


def test_rerun_is_bit_equal():
    b, s, h, k = 2, 200, 8, 2
    x, tab, a = inputs(b, s, h, k), tables(s), padding_adder(b, s)
    first = run(x, tab, a, h, k).clone()
    run(inputs(b, 320, 4, 2), tables(320), None, 4, 2)                    # leaves other values in LDS
    assert torch.equal(run(x, tab, a, h, k), first)


@pytest.mark.parametrize("h,k", [(4, 2), (8, 1)])
def test_position_matters(h, k):
    """Random angles per (row, pair), so that a shift of the table by one row is no uniform rotation (which would
    leave every q . k as it was): the shifted result lies outside the unshifted reference's bound, the unshifted
    one inside.  A kernel that does not rotate k, or rotates it with the query's row, fails the second."""
    b, s = 2, 129
    qkv = inputs(b, s, h, k)
    ang = kb.rnd(s + 1, 32, scale=2.0, seed=11)
    tab, shifted = (ang[:s].cos(), ang[:s].sin()), (ang[1:].cos(), ang[1:].sin())
    ref, bound = gb.rope_gqa_ref(qkv, tab[0], tab[1], h, k, SCALE)
    kb.assert_within(run(qkv, tab, None, h, k), ref, bound, f"random tables H={h}/{k}")
    off = (kb.d(run(qkv, shifted, None, h, k)) - ref).abs() > bound
    assert off[:, 1:].double().mean() > 0.5, "the table's rows do not reach the result"


@pytest.mark.parametrize("b,s,h,k", [(32, 128, 8, 2), (1, 1024, 8, 2)], ids=["512-workgroups", "S1024"])
def test_launch_geometries(b, s, h, k):
    """More workgroups than the machine has CUs, and Llama's real length once."""
    qkv, tab = inputs(b, s, h, k), tables(s)
    ref, bound = gb.rope_gqa_ref(qkv, tab[0], tab[1], h, k, SCALE)
    kb.assert_within(run(qkv, tab, None, h, k), ref, bound, f"rope gqa attention {b} x {s} x {h}/{k}")


def test_rejections():
    H = hip()

    def z(*shape, dtype=BF):
        return torch.zeros(*shape, dtype=dtype, device="cuda")

    def t(s, n=32, dtype=torch.float32):
        return z(s, n, dtype=dtype)
    assert H.rope_gqa_attention_supported(1, 64, 8, 1) and H.rope_gqa_attention_supported(4096, 64, 32, 8)
    assert not H.rope_gqa_attention_supported(0, 64, 4, 2) and not H.rope_gqa_attention_supported(4097, 64, 4, 2)
    assert not H.rope_gqa_attention_supported(128, 32, 4, 2) and not H.rope_gqa_attention_supported(128, 64, 6, 2)
    assert not H.rope_gqa_attention_supported(128, 64, 16, 1) and not H.rope_gqa_attention_supported(128, 64, 4, 3)
    with pytest.raises(RuntimeError, match="head_dim 64"):
        H.rope_gqa_attention(z(1, 50, 4 * 32), t(50, 16), t(50, 16), None, 2, 1, SCALE)
    with pytest.raises(RuntimeError, match="1, 2, 4 or 8"):
        H.rope_gqa_attention(z(1, 50, 8 * 64), t(50), t(50), None, 6, 1, SCALE)
    for s in (0, 4097):
        with pytest.raises(RuntimeError, match="1 <= S"):
            H.rope_gqa_attention(z(1, s, 256), t(s), t(s), None, 2, 1, SCALE)
    with pytest.raises(RuntimeError, match="qkv must be 16-byte aligned"):
        H.rope_gqa_attention(z(50 * 256 + 8)[4:-4].view(1, 50, 256), t(50), t(50), None, 2, 1, SCALE)
    for cos, sin in ((t(49), t(50)), (t(50), t(50, 64)), (z(50 * 32, dtype=torch.float32), t(50))):
        with pytest.raises(RuntimeError, match=r"cos / sin must be \[S, 32\]"):
            H.rope_gqa_attention(z(2, 50, 256), cos, sin, None, 2, 1, SCALE)
    with pytest.raises(RuntimeError, match="dtype"):
        H.rope_gqa_attention(z(2, 50, 256), t(50, dtype=torch.float64), t(50), None, 2, 1, SCALE)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        H.rope_gqa_attention(z(2, 50, 256), t(50).cpu(), t(50), None, 2, 1, SCALE)
    with pytest.raises(RuntimeError, match="cos / sin must be 16-byte aligned"):
        H.rope_gqa_attention(z(2, 50, 256), z(50 * 32 + 4, dtype=torch.float32)[2:-2].view(50, 32), t(50), None, 2, 1, SCALE)
    for adder in (torch.zeros(2, 49), torch.zeros(3, 50), torch.zeros(50)):
        with pytest.raises(RuntimeError, match="key_adder must be"):
            H.rope_gqa_attention(z(2, 50, 256), t(50), t(50), adder.cuda(), 2, 1, SCALE)
    with pytest.raises(RuntimeError, match="wrong size"):
        H.rope_gqa_attention(z(2, 50, 256), t(50), t(50), None, 2, 1, SCALE, z(2, 50, 64))
    with pytest.raises(RuntimeError, match="out must be 16-byte aligned"):
        H.rope_gqa_attention(z(1, 50, 256), t(50), t(50), None, 2, 1, SCALE, z(50 * 128 + 8)[4:-4].view(1, 50, 128))
    with pytest.raises(RuntimeError, match="exceed 2 GiB"):
        H.rope_gqa_attention(torch.empty(0, 4096, 4096 * 64, dtype=BF, device="cuda"), t(4096), t(4096), None, 2048,
                             1024, SCALE)
