"""rope_gqa_attention with 128-wide heads (kernels/gqattn128.hip) against
gqattn_bounds.rope_gqa_ref, whose head width is bound to 128 for this module's
calls: the bound's only D-dependent term, (D + 4) E, is the dot-product depth.

The cases are the D = 64 file's: lengths on both sides of the 64-key block and
of every query-block height (16 / 32 / 64 rows), a ragged last block, four key
blocks so the two-deep K / V buffer wraps; G = 1, 2, 4 (256 threads) and 8 (512
threads).  Causality, isolation and reruns are bit for bit."""
import pytest
import torch

import gqattn_bounds as gb
import kernel_bounds as kb

from test_gqattn_gpu import BF, HEADS, NAN, hip, padding_adder

pytestmark = pytest.mark.gpu
D = 128
SCALE = D ** -0.5
_REF = {}


@pytest.fixture(autouse=True)
def wide_heads(monkeypatch):
    monkeypatch.setattr(gb, "D", D)


def inputs(b, s, h, k):
    return kb.rnd(b, s, (h + 2 * k) * D, seed=4000 + 7 * s + b + h).to(BF)


def tables(s):
    """Llama's tables for 128-wide heads, one half: (cos, sin) [s, 64] f32."""
    from rust_tensorflow_serving2_amd.models import llama
    cos, sin = llama.rope_tables(s, dim=D)
    return torch.from_numpy(cos[0, 0, :, :D // 2].copy()), torch.from_numpy(sin[0, 0, :, :D // 2].copy())


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
    """qkv and out are views into NaN-filled buffers."""
    b = 2
    qkv, tab = inputs(b, s, h, k), tables(s)
    adder = padding_adder(b, s) if padded else None
    n_in, n_out, guard = qkv.numel(), b * s * h * D, 4096          # guard: elements, a 16-B multiple
    big_in = torch.full((guard + n_in + guard,), NAN, dtype=BF, device="cuda")
    big_in[guard:guard + n_in] = qkv.cuda().reshape(-1)
    big_out = torch.full((guard + n_out + guard,), NAN, dtype=BF, device="cuda")
    out = big_out[guard:guard + n_out].view(b, s, h * D)
    y = run(big_in[guard:guard + n_in].view(b, s, -1), tab, adder, h, k, out)
    assert y.data_ptr() == out.data_ptr()
    ref, bound = reference(qkv, tab, h, k, adder, (s, h, k, padded))
    worst = kb.assert_within(y, ref, bound, f"rope gqa attention D=128 S={s} H={h}/{k} padded={padded}")
    print(f"rope gqa attention D=128 S={s} H={h}/{k} padded={padded}: worst err/bound {worst:.3f}")
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
    q, kv = qkv[..., :h * D].reshape(2, s, h, D).clone(), qkv[..., h * D:].reshape(2, s, 2, k, D).clone()
    if what == "group":                # the other K / V head and its two query heads: a run of the clean group alone
        solo = run(torch.cat([q[:, :, 2 * good:2 * good + 2].reshape(2, s, -1),
                              kv[:, :, :, good].reshape(2, s, -1)], -1).contiguous(), tab, None, 2, 1)
        q[:, :, 2 * bad:2 * bad + 2], kv[:, :, :, bad] = NAN, NAN
        both = run(torch.cat([q.reshape(2, s, -1), kv.reshape(2, s, -1)], -1), tab, None, h, k)
        assert torch.equal(solo, both[..., good * 2 * D:(good + 1) * 2 * D])
    else:                              # one query head of group 0: the other three heads as in the clean run
        clean = run(qkv, tab, None, h, k)
        q[:, :, bad] = NAN
        both = run(torch.cat([q.reshape(2, s, -1), kv.reshape(2, s, -1)], -1), tab, None, h, k)
        keep = [i for i in range(h * D) if i // D != bad]
        assert torch.equal(clean[..., keep], both[..., keep])


def test_rerun_is_bit_equal():
    b, s, h, k = 2, 200, 8, 2
    x, tab, a = inputs(b, s, h, k), tables(s), padding_adder(b, s)
    first = run(x, tab, a, h, k).clone()
    run(inputs(b, 320, 8, 1), tables(320), None, 8, 1)                    # leaves other values in LDS
    assert torch.equal(run(x, tab, a, h, k), first)


@pytest.mark.parametrize("b,s,h,k", [(32, 128, 8, 2), (1, 1024, 8, 2)], ids=["512-workgroups", "S1024"])
def test_launch_geometries(b, s, h, k):
    """More workgroups than the machine has CUs, and the served length once."""
    qkv, tab = inputs(b, s, h, k), tables(s)
    ref, bound = gb.rope_gqa_ref(qkv, tab[0], tab[1], h, k, SCALE)
    worst = kb.assert_within(run(qkv, tab, None, h, k), ref, bound, f"rope gqa attention D=128 {b} x {s} x {h}/{k}")
    print(f"rope gqa attention D=128 {b} x {s} x {h}/{k}: worst err/bound {worst:.3f}")


def test_interface():
    H = hip()

    def z(*shape, dtype=BF):
        return torch.zeros(*shape, dtype=dtype, device="cuda")
    for s in (1, 4096):
        for h, k in ((8, 8), (8, 4), (8, 2), (8, 1)):
            assert H.rope_gqa_attention_supported(s, D, h, k)
    assert not H.rope_gqa_attention_supported(0, D, 4, 2) and not H.rope_gqa_attention_supported(4097, D, 4, 2)
    for width in (96, 256):
        assert not H.rope_gqa_attention_supported(50, width, 2, 1)
        with pytest.raises(RuntimeError, match="head_dim 64 or 128"):
            H.rope_gqa_attention(z(1, 50, 4 * width), z(50, width // 2, dtype=torch.float32),
                                 z(50, width // 2, dtype=torch.float32), None, 2, 1, SCALE)
    with pytest.raises(RuntimeError, match=r"cos / sin must be \[S, 64\]"):
        H.rope_gqa_attention(z(1, 50, 4 * D), z(50, 32, dtype=torch.float32), z(50, 32, dtype=torch.float32), None, 2, 1,
                             SCALE)
    with pytest.raises(RuntimeError, match="cos / sin must be 16-byte aligned"):
        H.rope_gqa_attention(z(1, 50, 4 * D), z(50 * 64 + 4, dtype=torch.float32)[2:-2].view(50, 64),
                             z(50, 64, dtype=torch.float32), None, 2, 1, SCALE)


def test_op_reaches_the_kernel():
    """RopeGQAttentionOp on the device is the kernel's launch bit for bit; its torch path lies within the bound too."""
    from rust_tensorflow_serving2_amd.graph.patterns import RopeGQAttentionOp
    b, s, h, k = 2, 129, 4, 2
    qkv, tab, adder = inputs(b, s, h, k), tables(s), padding_adder(b, s)
    ref, bound = gb.rope_gqa_ref(qkv, tab[0], tab[1], h, k, SCALE, adder)
    direct = run(qkv, tab, adder, h, k)
    for use_hip in (True, False):
        op = RopeGQAttentionOp(h, k, D, s, SCALE, -10000.0, tab[0], tab[1], torch.device("cuda"), use_hip)
        (y,) = op(None, None, [qkv.cuda().reshape(b * s, -1), adder.cuda().reshape(b, 1, 1, s)])
        assert y.dtype == BF and y.shape == (b * s, h * D)
        if use_hip:
            assert torch.equal(y.reshape(b, s, -1), direct)
        worst = kb.assert_within(y.reshape(b, s, -1), ref, bound, f"RopeGQAttentionOp D=128 use_hip={use_hip}")
        print(f"RopeGQAttentionOp D=128 use_hip={use_hip}: worst err/bound {worst:.3f}")
