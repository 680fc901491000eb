"""rope_attention (kernels/rattn.hip) against rattn_bounds.rope_attention_ref.  The
lengths lie on both sides of the 64-key / 64-row block, leave a ragged last block
and reach six key blocks.  The windows: none (-1), the diagonal alone (0), 16 (at
S = 330 a middle query block skips key blocks on both sides), 64 (three blocks)
and 100 (both edges inside blocks).  Locality and isolation are bit for bit."""
import pytest
import torch

import kernel_bounds as kb
import rattn_bounds as rb

from test_gqattn_gpu import BF, NAN, SCALE, hip, padding_adder, tables

pytestmark = pytest.mark.gpu


def inputs(b, s, h):
    return kb.rnd(b, s, 3 * h * 64, seed=6000 + 7 * s + b + h).to(BF)


def run(qkv, tab, adder, h, window, out=None):
    return hip().rope_attention(qkv.cuda(), tab[0].cuda(), tab[1].cuda(), None if adder is None else adder.cuda(), h,
                                SCALE, window, out)


@pytest.mark.parametrize("padded", [False, True], ids=["no-adder", "right-padded"])
@pytest.mark.parametrize("window", [-1, 0, 16, 64, 100])
@pytest.mark.parametrize("s", [1, 17, 64, 65, 129, 200, 330])
def test_within_bound_inside_guard_bands(s, window, padded):
    """qkv and out are views into NaN-filled buffers.  The adder is finite, so every row has an open key."""
    b, h = 2, 2
    qkv, tab = inputs(b, s, h), tables(s)
    adder = padding_adder(b, s) if padded else None
    n_in, n_out, guard = qkv.numel(), b * s * h * 64, 4096          # guard: elements, a 16-B multiple
    big_in = torch.full((guard + n_in + guard,), NAN, dtype=BF, device="cuda")
    big_in[guard:guard + n_in] = qkv.cuda().reshape(-1)
    big_out = torch.full((guard + n_out + guard,), NAN, dtype=BF, device="cuda")
    out = big_out[guard:guard + n_out].view(b, s, h * 64)
    y = run(big_in[guard:guard + n_in].view(b, s, -1), tab, adder, h, window, out)
    assert y.data_ptr() == out.data_ptr()
    ref, bound = rb.rope_attention_ref(qkv, tab[0], tab[1], h, SCALE, window, adder)
    worst = kb.assert_within(y, ref, bound, f"rope attention S={s} w={window} padded={padded}")
    print(f"rope attention S={s} w={window} padded={padded}: worst err/bound {worst:.3f}")
    assert torch.isnan(big_out[:guard]).all() and torch.isnan(big_out[guard + n_out:]).all(), "a guard element was written"
    assert torch.isnan(big_in[:guard]).all() and torch.isnan(big_in[guard + n_in:]).all()


@pytest.mark.parametrize("window", [16, 64])
@pytest.mark.parametrize("lo,hi", [(0, 127), (64, 255), (63, 256), (1, 329), (128, 329), (100, 250)])
def test_rows_see_only_their_window(lo, hi, window):
    """Tokens outside [lo, hi] overwritten with +-3e4 (finite): every row whose window lies inside is bit-equal."""
    b, s, h = 2, 330, 2
    qkv, tab = inputs(b, s, h), tables(s)
    first = run(qkv, tab, None, h, window)
    other = torch.where(kb.rnd(b, s, qkv.shape[2], seed=5) > 0, 3e4, -3e4).to(BF)
    other[:, lo:hi + 1] = qkv[:, lo:hi + 1]
    second = run(other, tab, None, h, window)
    rows = [i for i in range(s) if lo <= max(i - window, 0) and min(i + window, s - 1) <= hi]
    assert rows and torch.isfinite(second[:, rows]).all()
    assert torch.equal(first[:, rows], second[:, rows])


@pytest.mark.parametrize("s", [17, 200])
def test_a_window_that_reaches_every_key_is_the_global_form(s):
    qkv, tab, a = inputs(2, s, 2), tables(s), padding_adder(2, s)
    glob = run(qkv, tab, a, 2, -1)
    for window in (s - 1, s, 1 << 40, -7):
        assert torch.equal(run(qkv, tab, a, 2, window), glob)


@pytest.mark.parametrize("window", [-1, 64])
@pytest.mark.parametrize("what", ["head", "image"])
@pytest.mark.parametrize("bad", [0, 1])
def test_nan_neighbour_leaves_the_clean_one_bit_equal(bad, what, window):
    s, h, good = 129, 2, 1 - bad
    qkv, tab = inputs(2, s, h), tables(s)
    clean = run(qkv, tab, None, h, window)
    x = qkv.clone()
    if what == "head":
        x.view(2, s, 3, h, 64)[:, :, :, bad] = NAN
        both = run(x, tab, None, h, window)
        assert torch.equal(clean[..., good * 64:good * 64 + 64], both[..., good * 64:good * 64 + 64])
    else:
        x[bad] = NAN
        assert torch.equal(clean[good], run(x, tab, None, h, window)[good])


@pytest.mark.parametrize("window", [-1, 64])
def test_rerun_is_bit_equal(window):
    b, s, h = 2, 200, 4
    x, tab, a = inputs(b, s, h), tables(s), padding_adder(b, s)
    first = run(x, tab, a, h, window).clone()
    run(inputs(b, 330, 2), tables(330), None, 2, 16)                    # leaves other values in LDS
    assert torch.equal(run(x, tab, a, h, window), first)


@pytest.mark.parametrize("b,s,h,window", [(16, 256, 4, 64), (1, 1024, 2, 64), (1, 1024, 2, -1)],
                         ids=["256-workgroups", "S1024-local", "S1024-global"])
def test_launch_geometries(b, s, h, window):
    """More workgroups than the machine has CUs, and the served length in both forms."""
    qkv, tab = inputs(b, s, h), tables(s)
    ref, bound = rb.rope_attention_ref(qkv, tab[0], tab[1], h, SCALE, window)
    worst = kb.assert_within(run(qkv, tab, None, h, window), ref, bound, f"rope attention {b} x {s} x {h} w={window}")
    print(f"rope attention {b} x {s} x {h} w={window}: worst err/bound {worst:.3f}")


def test_interface():
    H = hip()

    def z(*shape, dtype=BF):
        return torch.zeros(*shape, dtype=dtype, device="cuda")
    for s in (1, 4096):
        for window in (-1, 0, 64, 1 << 40):
            assert H.rope_attention_supported(s, 64, 12, window)
    assert not H.rope_attention_supported(0, 64, 2) and not H.rope_attention_supported(4097, 64, 2)
    for width in (32, 128):
        assert not H.rope_attention_supported(50, width, 2, 64)
        with pytest.raises(RuntimeError, match="head_dim 64"):
            H.rope_attention(z(1, 50, 6 * width), z(50, width // 2, dtype=torch.float32),
                             z(50, width // 2, dtype=torch.float32), None, 2, SCALE)
    with pytest.raises(RuntimeError, match=r"cos / sin must be \[S, 32\]"):
        H.rope_attention(z(1, 50, 384), z(49, 32, dtype=torch.float32), z(49, 32, dtype=torch.float32), None, 2, SCALE, 64)
    with pytest.raises(RuntimeError, match="cos / sin must be 16-byte aligned"):
        H.rope_attention(z(1, 50, 384), z(50 * 32 + 4, dtype=torch.float32)[2:-2].view(50, 32),
                         z(50, 32, dtype=torch.float32), None, 2, SCALE, 64)


@pytest.mark.parametrize("window", [-1, 64])
def test_op_reaches_the_kernel(window):
    """The op on the device is the kernel's launch bit for bit; its torch path lies within the bound too."""
    from rust_tensorflow_serving2_amd.graph.patterns import RopeAttentionOp
    b, s, h = 2, 129, 2
    qkv, tab, adder = inputs(b, s, h), tables(s), padding_adder(b, s)
    ref, bound = rb.rope_attention_ref(qkv, tab[0], tab[1], h, SCALE, window, adder)
    direct = run(qkv, tab, adder, h, window)
    for use_hip in (True, False):
        op = RopeAttentionOp(h, 64, s, SCALE, window, -10000.0, tab[0], tab[1], torch.device("cuda"), use_hip)
        (y,) = op(None, None, [qkv.cuda().reshape(b * s, -1), adder.cuda().reshape(b, 1, 1, s)])
        assert y.dtype == BF and y.shape == (b * s, h * 64)
        if use_hip:
            assert torch.equal(y.reshape(b, s, -1), direct)
        worst = kb.assert_within(y.reshape(b, s, -1), ref, bound, f"RopeAttentionOp w={window} use_hip={use_hip}")
        print(f"RopeAttentionOp w={window} use_hip={use_hip}: worst err/bound {worst:.3f}")
