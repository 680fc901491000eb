"""rope_gqa_attention256 (kernels/gqattn256.hip: 256-wide heads, sliding window, optional
QK-norm) against gqattn256_bounds.rope_gqa256_ref.

The key block is KB = 32 keys and a workgroup holds 16, 32, 64 or 128 query rows, so the lengths
sit on both sides of 16, 32 and 64, 200 is past 128, and the windows sit on both sides of one key block; S = 321
with window 70 starts its walk past block 0 and wraps the two-deep K / V buffer.  Locality,
the causal build's equality and reruns are bit for bit."""
import pytest
import torch

import gqattn256_bounds as gb
import kernel_bounds as kb

from test_gqattn_gpu import BF, HEADS, hip
from test_llama_kernels_gpu import banded, guards_intact

pytestmark = pytest.mark.gpu
D, KB = 256, 32
SCALE = D ** -0.5
EPS = 1e-6


def inputs(b, s, h, k):
    return kb.rnd(b, s, (h + 2 * k) * D, seed=6000 + 7 * s + b + h).to(BF)


def tables(s):
    """Gemma's local tables, one half: (cos, sin) [s, 128] f32."""
    from rust_tensorflow_serving2_amd.models import llama
    cos, sin = llama.rope_tables(s, dim=D)
    return torch.from_numpy(cos[0, 0, :, :D // 2].copy()), torch.from_numpy(sin[0, 0, :, :D // 2].copy())


def gammas():
    return (1 + 0.25 * kb.rnd(D, seed=61)).float(), (1 + 0.25 * kb.rnd(D, seed=62)).float(), EPS


def one_image_padded(b, s):
    """Image b - 1 is right-padded by a quarter; the others are whole.  The diagonal stays open (finite adder)."""
    a = torch.zeros(b, s)
    a[b - 1, s - s // 4:] = -10000.0
    return a


def run(qkv, tab, adder, h, k, window=-1, norm=None, out=None):
    qn = (None, None, 0.0) if norm is None else (norm[0].cuda(), norm[1].cuda(), norm[2])
    return hip().rope_gqa_attention256(qkv.cuda(), tab[0].cuda(), tab[1].cuda(), None if adder is None else adder.cuda(),
                                       h, k, SCALE, window, out, *qn)


def check(b, s, h, k, window, normed, padded):
    """qkv and out are views into NaN-filled buffers."""
    qkv, tab = inputs(b, s, h, k), tables(s)
    norm = gammas() if normed else None
    adder = one_image_padded(b, s) if padded else None
    (big_in, iv), (big_out, ov) = banded(qkv.numel()), banded(b * s * h * D)
    iv.copy_(qkv.reshape(-1))
    y = run(iv.view(b, s, -1), tab, adder, h, k, window, norm, ov.view(b, s, h * D))
    assert y.data_ptr() == ov.data_ptr()
    ref, bound = gb.rope_gqa256_ref(qkv, tab[0], tab[1], h, k, SCALE, window, norm, adder)
    what = f"rope gqa attention D=256 S={s} H={h}/{k} window={window} norm={normed} padded={padded}"
    print(f"{what}: worst err/bound {kb.assert_within(y, ref, bound, what):.3f}")
    assert guards_intact(big_in) and guards_intact(big_out), "a guard element was written"


@pytest.mark.parametrize("normed", [False, True], ids=["plain", "qk-norm"])
@pytest.mark.parametrize("h,k", HEADS)
@pytest.mark.parametrize("window", [-1, 0, 5, KB - 1, KB, KB + 1, 100])
@pytest.mark.parametrize("s", [1, 15, 17, KB - 1, KB + 1, 2 * KB + 1, 200])
def test_within_bound_inside_guard_bands(s, window, h, k, normed):
    check(2, s, h, k, window, normed, False)


@pytest.mark.parametrize("normed", [False, True], ids=["plain", "qk-norm"])
@pytest.mark.parametrize("h,k", HEADS)
@pytest.mark.parametrize("s,window", [(321, 70), (200, 5), (2 * KB + 1, -1)])
def test_padded_image_and_a_walk_that_starts_past_block_0(s, window, h, k, normed):
    check(2, s, h, k, window, normed, True)


@pytest.mark.parametrize("h,k", [(2, 2), (4, 2), (8, 1)])
@pytest.mark.parametrize("window", [0, 5, KB, 70])
def test_rows_see_their_window_and_nothing_else(window, h, k):
    """Row i depends on tokens i - window .. i only: other tokens overwritten with +-3e4 (finite) leave it
    bit-equal; one key inside the window changes it."""
    b, s, i = 2, 200, 131
    qkv, tab, norm = inputs(b, s, h, k), tables(s), gammas()
    first = run(qkv, tab, None, h, k, window, norm)
    other = qkv.clone()
    noise = torch.where(kb.rnd(b, s, qkv.shape[2], seed=5) > 0, 3e4, -3e4).to(BF)
    other[:, :i - window], other[:, i + 1:] = noise[:, :i - window], noise[:, i + 1:]
    second = run(other, tab, None, h, k, window, norm)
    assert torch.isfinite(second[:, i]).all() and torch.equal(first[:, i], second[:, i])
    inside = qkv.clone()
    inside[:, i - window, (h + k) * D:] += 1.0                               # the V heads of the window's first key
    assert not torch.equal(run(inside, tab, None, h, k, window, norm)[:, i], first[:, i])


@pytest.mark.parametrize("h,k", HEADS)
def test_a_window_that_reaches_every_key_is_the_causal_build(h, k):
    b, s = 2, 130
    qkv, tab, a = inputs(b, s, h, k), tables(s), one_image_padded(b, s)
    causal = run(qkv, tab, a, h, k, -1)
    for window in (s - 1, s, 10 ** 6):
        assert torch.equal(run(qkv, tab, a, h, k, window), causal)
    assert not torch.equal(run(qkv, tab, a, h, k, s - 2), causal)            # the LOCAL build closes key 0 for the last row


def test_rerun_is_bit_equal():
    b, s, h, k = 2, 200, 8, 2
    x, tab, a, norm = inputs(b, s, h, k), tables(s), one_image_padded(b, s), gammas()
    first = run(x, tab, a, h, k, 40, norm).clone()
    run(inputs(b, 321, 8, 1), tables(321), None, 8, 1)                      # leaves other values in LDS
    assert torch.equal(run(x, tab, a, h, k, 40, norm), first)


def test_more_workgroups_than_cus_at_the_served_shape():
    """Gemma-3's local layer, S = 1024 and window 511, with 8 x 4 K / V heads: 512 workgroups.  Image 0 is
    held to the bound; every image's result is its own wherever it sits in the batch."""
    b, s, h, k, window = 8, 1024, 8, 4, 511
    qkv, tab, norm = inputs(b, s, h, k), tables(s), gammas()
    y = run(qkv, tab, None, h, k, window, norm)
    ref, bound = gb.rope_gqa256_ref(qkv[:1], tab[0], tab[1], h, k, SCALE, window, norm)
    what = f"rope gqa attention D=256 {b} x {s} x {h}/{k} window={window}"
    print(f"{what}: worst err/bound {kb.assert_within(y[:1], ref, bound, what):.3f}")
    assert torch.equal(run(qkv.flip(0).contiguous(), tab, None, h, k, window, norm).flip(0), y)


def test_interface():
    """Every rejection here is raised by the binding, which checks all that rope_gqa_attention256_launch checks
    before it calls it; the launcher's own hipErrorInvalidValue returns cannot be reached from Python."""
    H = hip()
    f32 = torch.float32

    def z(*shape, dtype=BF):
        return torch.zeros(*shape, dtype=dtype, device="cuda")
    for s in (1, 4096):
        for h, k in ((8, 8), (8, 4), (8, 2), (8, 1)):
            assert H.rope_gqa_attention256_supported(s, h, k)
    assert not H.rope_gqa_attention256_supported(0, 4, 2) and not H.rope_gqa_attention256_supported(4097, 4, 2)
    assert not H.rope_gqa_attention256_supported(50, 6, 2) and not H.rope_gqa_attention256_supported(50, 2, 4)
    tab = z(50, 128, dtype=f32)
    for width in (64, 128):
        with pytest.raises(RuntimeError, match="head_dim 256"):
            H.rope_gqa_attention256(z(1, 50, 4 * width), tab, tab, None, 2, 1, SCALE)
    with pytest.raises(RuntimeError, match=r"cos / sin must be \[S, 128\]"):
        H.rope_gqa_attention256(z(1, 50, 4 * D), z(50, 64, dtype=f32), z(50, 64, dtype=f32), None, 2, 1, SCALE)
    with pytest.raises(RuntimeError, match="cos / sin must be 16-byte aligned"):
        H.rope_gqa_attention256(z(1, 50, 4 * D), z(50 * 128 + 4, dtype=f32)[2:-2].view(50, 128), tab, None, 2, 1, SCALE)
    g = torch.ones(D, dtype=f32, device="cuda")
    with pytest.raises(RuntimeError, match="q_norm and k_norm go together"):
        H.rope_gqa_attention256(z(1, 50, 4 * D), tab, tab, None, 2, 1, SCALE, -1, None, g, None, EPS)
    with pytest.raises(RuntimeError, match="norm_eps must be > 0"):
        H.rope_gqa_attention256(z(1, 50, 4 * D), tab, tab, None, 2, 1, SCALE, -1, None, g, g, 0.0)
    with pytest.raises(RuntimeError, match=r"q_norm / k_norm must be \[256\]"):
        H.rope_gqa_attention256(z(1, 50, 4 * D), tab, tab, None, 2, 1, SCALE, -1, None, g[:128], g[:128], EPS)
    with pytest.raises(RuntimeError, match="q_norm / k_norm must be 16-byte aligned"):
        H.rope_gqa_attention256(z(1, 50, 4 * D), tab, tab, None, 2, 1, SCALE, -1, None,
                                torch.ones(D + 4, dtype=f32, device="cuda")[2:-2], g, EPS)


@pytest.mark.parametrize("window,normed", [(-1, False), (40, True)])
def test_op_reaches_the_kernel(window, normed):
    """RopeGQAttentionOp on the device is the kernel's launch bit for bit; its torch path lies within the bound too."""
    from rust_tensorflow_serving2_amd.graph.patterns import RopeGQAttentionOp
    b, s, h, k = 2, 129, 4, 2
    qkv, tab, adder = inputs(b, s, h, k), tables(s), one_image_padded(b, s)
    norm = gammas() if normed else None
    ref, bound = gb.rope_gqa256_ref(qkv, tab[0], tab[1], h, k, SCALE, window, norm, adder)
    direct = run(qkv, tab, adder, h, k, window, norm)
    for use_hip in (True, False):
        op = RopeGQAttentionOp(h, k, D, s, SCALE, -10000.0, tab[0], tab[1], torch.device("cuda"), use_hip, norm, window)
        (y,) = op(None, None, [qkv.cuda().reshape(b * s, -1), adder.cuda().reshape(b, 1, 1, s)])
        assert y.dtype == BF and y.shape == (b * s, h * D)
        if use_hip:
            assert torch.equal(y.reshape(b, s, -1), direct)
        what = f"RopeGQAttentionOp D=256 window={window} norm={normed} use_hip={use_hip}"
        print(f"{what}: worst err/bound {kb.assert_within(y.reshape(b, s, -1), ref, bound, what):.3f}")
