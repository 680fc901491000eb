"""bias_attention (kernels/battn.hip) against battn_bounds.bias_attention_ref.  The
lengths lie on both sides of the 64-key / 64-row block, leave a ragged last block
and reach six key blocks; the table is random, asymmetric in j - i and different per
head, so i - j for j - i, a head offset or a block base off by one shows.  Isolation
and reruns are bit for bit."""
import pytest
import torch

import battn_bounds as bb
import kernel_bounds as kb

from test_gqattn_gpu import BF, NAN, hip, padding_adder

pytestmark = pytest.mark.gpu
SCALE = 1 / 8


def inputs(b, s, h):
    return kb.rnd(b, s, 3 * h * 64, seed=7000 + 7 * s + b + h).to(BF)


def run(qkv, table, adder, h, out=None, scale=SCALE):
    return hip().bias_attention(qkv.cuda(), table.cuda(), None if adder is None else adder.cuda(), h, scale, out)


@pytest.mark.parametrize("padded", [False, True], ids=["no-adder", "right-padded"])
@pytest.mark.parametrize("s", [1, 17, 64, 65, 129, 200, 330])
def test_within_bound_inside_guard_bands(s, padded):
    """qkv and out are views into NaN-filled buffers.  The adder is finite, so every row has an open key."""
    b, h = 2, 2
    qkv, table = inputs(b, s, h), bb.table_for(h, s)
    adder = padding_adder(b, s) if padded else None
    n_in, n_out, guard = qkv.numel(), b * s * h * 64, 4096          # guard: elements, a 16-B multiple
    big_in = torch.full((guard + n_in + guard,), NAN, dtype=BF, device="cuda")
    big_in[guard:guard + n_in] = qkv.cuda().reshape(-1)
    big_out = torch.full((guard + n_out + guard,), NAN, dtype=BF, device="cuda")
    out = big_out[guard:guard + n_out].view(b, s, h * 64)
    y = run(big_in[guard:guard + n_in].view(b, s, -1), table, adder, h, out)
    assert y.data_ptr() == out.data_ptr()
    ref, bound = bb.bias_attention_ref(qkv, table, h, SCALE, adder)
    worst = kb.assert_within(y, ref, bound, f"bias attention S={s} padded={padded}")
    print(f"bias attention S={s} padded={padded}: worst err/bound {worst:.3f}")
    assert torch.isnan(big_out[:guard]).all() and torch.isnan(big_out[guard + n_out:]).all(), "a guard element was written"
    assert torch.isnan(big_in[:guard]).all() and torch.isnan(big_in[guard + n_in:]).all()


@pytest.mark.parametrize("b,s,h", [(16, 256, 4), (1, 1024, 2), (1, 4096, 1)],
                         ids=["256-workgroups", "S1024", "S4096-longest-table"])
def test_launch_geometries(b, s, h):
    qkv, table = inputs(b, s, h), bb.table_for(h, s)
    ref, bound = bb.bias_attention_ref(qkv, table, h, SCALE)
    worst = kb.assert_within(run(qkv, table, None, h), ref, bound, f"bias attention {b} x {s} x {h}")
    print(f"bias attention {b} x {s} x {h}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("what", ["head", "image"])
@pytest.mark.parametrize("bad", [0, 1])
def test_nan_neighbour_leaves_the_clean_one_bit_equal(bad, what):
    s, h, good = 129, 2, 1 - bad
    qkv, table = inputs(2, s, h), bb.table_for(h, s)
    clean = run(qkv, table, None, h)
    x, t = qkv.clone(), table.clone()
    if what == "head":
        x.view(2, s, 3, h, 64)[:, :, :, bad] = NAN
        t[bad] = NAN                                                   # the bad head's table row too
        both = run(x, t, None, h)
        assert torch.equal(clean[..., good * 64:good * 64 + 64], both[..., good * 64:good * 64 + 64])
    else:
        x[bad] = NAN
        assert torch.equal(clean[good], run(x, table, None, h)[good])


def test_rerun_is_bit_equal():
    b, s, h = 2, 200, 4
    x, table, a = inputs(b, s, h), bb.table_for(h, s), padding_adder(b, s)
    first = run(x, table, a, h).clone()
    run(inputs(b, 330, 2), bb.table_for(2, 330), None, 2)               # leaves other values in LDS
    assert torch.equal(run(x, table, a, h), first)


@pytest.mark.parametrize("s", [65, 200])
def test_a_table_of_zeros_is_plain_attention(s):
    """With the same key adder the result lies within kernel_bounds.attention_ref's own bound: the unbiased model."""
    b, h = 2, 2
    qkv, a = inputs(b, s, h), padding_adder(b, s)
    ref, bound = kb.attention_ref(qkv, h, SCALE, a)
    worst = kb.assert_within(run(qkv, torch.zeros(h, 2 * s - 1), a, h), ref, bound, f"zero table S={s}")
    print(f"bias attention, table of zeros, S={s}: worst err/bound {worst:.3f}")


def test_interface():
    H = hip()

    def z(*shape, dtype=BF):
        return torch.zeros(*shape, dtype=dtype, device="cuda")
    f32 = torch.float32
    assert H.bias_attention_supported(1, 64, 12) and H.bias_attention_supported(4096, 64, 1)
    assert not H.bias_attention_supported(0, 64, 2) and not H.bias_attention_supported(4097, 64, 2)
    for width in (32, 128):
        assert not H.bias_attention_supported(50, width, 2)
        with pytest.raises(RuntimeError, match="head_dim 64"):
            H.bias_attention(z(1, 50, 6 * width), z(2, 99, dtype=f32), None, 2, SCALE)
    with pytest.raises(RuntimeError, match=r"table must be \[heads, 2\*S - 1\]"):
        H.bias_attention(z(1, 50, 384), z(2, 100, dtype=f32), None, 2, SCALE)
    with pytest.raises(RuntimeError, match=r"table must be \[heads, 2\*S - 1\]"):
        H.bias_attention(z(1, 50, 384), z(3, 99, dtype=f32), None, 2, SCALE)
    with pytest.raises(RuntimeError, match="table has dtype"):
        H.bias_attention(z(1, 50, 384), z(2, 99), None, 2, SCALE)
    with pytest.raises(RuntimeError, match="table must be contiguous"):
        H.bias_attention(z(1, 50, 384), z(2, 198, dtype=f32)[:, ::2], None, 2, SCALE)
    with pytest.raises(RuntimeError, match="table must be a GPU tensor"):
        H.bias_attention(z(1, 50, 384), torch.zeros(2, 99), None, 2, SCALE)
    with pytest.raises(RuntimeError, match=r"key_adder must be \[B, S\] or \[1, S\]"):
        H.bias_attention(z(2, 50, 384), z(2, 99, dtype=f32), z(3, 50, dtype=f32), 2, SCALE)
    with pytest.raises(RuntimeError, match="qkv must be 16-byte aligned"):
        H.bias_attention(z(50 * 384 + 8)[4:-4].view(1, 50, 384), z(2, 99, dtype=f32), None, 2, SCALE)
    with pytest.raises(RuntimeError, match="out must be 16-byte aligned"):
        H.bias_attention(z(1, 50, 384), z(2, 99, dtype=f32), None, 2, SCALE, z(50 * 128 + 8)[4:-4].view(1, 50, 128))


def test_op_reaches_the_kernel():
    """The op on the device is the kernel's launch bit for bit; its torch path lies within the bound too."""
    from rust_tensorflow_serving2_amd.graph.patterns import BiasAttentionOp
    b, s, h = 2, 129, 2
    qkv, table, adder = inputs(b, s, h), bb.table_for(h, s), padding_adder(b, s)
    ref, bound = bb.bias_attention_ref(qkv, table, h, SCALE, adder)
    direct = run(qkv, table, adder, h)
    for use_hip in (True, False):
        op = BiasAttentionOp(h, 64, s, SCALE, table, torch.device("cuda"), use_hip)
        (y,) = op(None, None, [qkv.cuda().reshape(b * s, -1), adder.cuda().reshape(b, 1, 1, s)])
        assert y.dtype == BF and y.shape == (b * s, h * 64)
        if use_hip:
            assert torch.equal(y.reshape(b, s, -1), direct)
        worst = kb.assert_within(y.reshape(b, s, -1), ref, bound, f"BiasAttentionOp use_hip={use_hip}")
        print(f"BiasAttentionOp use_hip={use_hip}: worst err/bound {worst:.3f}")
