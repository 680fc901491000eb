"""rope_gqa_attention with a QK-norm (kernels/gqattn128.hip, NORM builds) against
qknorm_bounds.qknorm_rope_gqa_ref: test_gqattn128_gpu's lengths and head groupings
(both sides of the 64-key block and of every query-block height; G = 1, 2, 4 at 256
threads and 8 at 512).  In every input one token is all zeros (0 * rsqrt(eps): an
exact-zero q and k, no NaN) and another is multiplied by 64, which the norm removes."""
import pytest
import torch

import kernel_bounds as kb
import qknorm_bounds as qb

from test_gqattn128_gpu import BF, D, HEADS, NAN, SCALE, hip, inputs, padding_adder, tables

pytestmark = pytest.mark.gpu
EPS = 1e-6
_REF = {}


def normed_inputs(b, s, h, k):
    qkv = inputs(b, s, h, k)
    qkv[0, s // 2] = 0
    qkv[b - 1, s // 3] *= 64
    return qkv


def gammas(seed=11):
    """Distinct q_norm / k_norm, f32 [128]: 1 + 0.25 N(0, 1)."""
    return 1 + kb.rnd(D, scale=0.25, seed=seed), 1 + kb.rnd(D, scale=0.25, seed=seed + 1)


def run(qkv, tab, adder, h, k, gam, out=None, eps=EPS):
    return hip().rope_gqa_attention(qkv.cuda(), tab[0].cuda(), tab[1].cuda(), None if adder is None else adder.cuda(),
                                    h, k, SCALE, out, gam[0].cuda(), gam[1].cuda(), eps)


def reference(qkv, tab, h, k, gam, adder, tag):
    if tag not in _REF:
        _REF[tag] = qb.qknorm_rope_gqa_ref(qkv, tab[0], tab[1], h, k, SCALE, gam[0], gam[1], EPS, adder)
    return _REF[tag]


@pytest.mark.parametrize("padded", [False, True], ids=["no-adder", "right-padded"])
@pytest.mark.parametrize("h,k", HEADS)
@pytest.mark.parametrize("s", [1, 17, 64, 65, 129, 200])
def test_within_bound_inside_guard_bands(s, h, k, padded):
    """out is a view into a NaN-filled buffer."""
    b = 2
    qkv, tab, gam = normed_inputs(b, s, h, k), tables(s), gammas()
    adder = padding_adder(b, s) if padded else None
    n_out, guard = b * s * h * D, 4096
    big_out = torch.full((guard + n_out + guard,), NAN, dtype=BF, device="cuda")
    out = big_out[guard:guard + n_out].view(b, s, h * D)
    y = run(qkv, tab, adder, h, k, gam, out)
    assert y.data_ptr() == out.data_ptr()
    ref, bound = reference(qkv, tab, h, k, gam, adder, (s, h, k, padded))
    worst = kb.assert_within(y, ref, bound, f"qk-norm rope gqa attention S={s} H={h}/{k} padded={padded}")
    print(f"qk-norm rope gqa attention S={s} H={h}/{k} padded={padded}: worst err/bound {worst:.3f}")
    assert torch.isnan(big_out[:guard]).all() and torch.isnan(big_out[guard + n_out:]).all(), "a guard element was written"


@pytest.mark.parametrize("cut", [63, 64])
def test_rows_do_not_see_later_tokens(cut):
    """Tokens > cut overwritten with +-3e4 (finite): rows <= cut are bit-equal."""
    b, s, h, k = 2, 200, 4, 2
    qkv, tab, gam = normed_inputs(b, s, h, k), tables(s), gammas()
    first = run(qkv, tab, None, h, k, gam)
    later = qkv.clone()
    later[:, cut + 1:] = torch.where(kb.rnd(b, s - cut - 1, qkv.shape[2], seed=5) > 0, 3e4, -3e4).to(BF)
    second = run(later, tab, None, h, k, gam)
    assert torch.isfinite(second).all()
    assert torch.equal(first[:, :cut + 1], second[:, :cut + 1])


def test_rerun_is_bit_equal():
    b, s, h, k = 2, 200, 4, 2
    x, tab, a, gam = normed_inputs(b, s, h, k), tables(s), padding_adder(b, s), gammas()
    first = run(x, tab, a, h, k, gam).clone()
    run(inputs(b, 320, 8, 1), tables(320), None, 8, 1, gammas(3))         # leaves other values in LDS
    assert torch.equal(run(x, tab, a, h, k, gam), first)


def test_swapped_gammas_show():
    """q_norm and k_norm crossed: outside the bound."""
    b, s, h, k = 2, 65, 4, 2
    qkv, tab, gam = normed_inputs(b, s, h, k), tables(s), gammas()
    ref, bound = reference(qkv, tab, h, k, gam, None, (s, h, k, False))
    crossed = run(qkv, tab, None, h, k, gam[::-1])
    assert ((kb.d(crossed) - ref).abs() > bound).any()


def test_interface():
    H = hip()

    def z(*shape, dtype=BF):
        return torch.zeros(*shape, dtype=dtype, device="cuda")

    def call(width=D, q=None, k=None, eps=EPS):
        t = z(50, width // 2, dtype=torch.float32)
        return H.rope_gqa_attention(z(1, 50, 4 * width), t, t, None, 2, 1, width ** -0.5, None, q, k, eps)
    g = torch.ones(D, device="cuda")
    assert H.rope_gqa_attention_supported(50, 128, 4, 2, qk_norm=True) and H.rope_gqa_attention_supported(50, 64, 4, 2)
    assert not H.rope_gqa_attention_supported(50, 64, 4, 2, qk_norm=True)
    assert call(q=g, k=g).shape == (1, 50, 2 * D)
    for kw, message in [(dict(q=g), "q_norm and k_norm go together"), (dict(k=g), "q_norm and k_norm go together"),
                        (dict(width=64, q=g[:64].clone(), k=g[:64].clone()), "qk norm needs head_dim 128"),
                        (dict(q=g.double(), k=g), "q_norm has dtype"), (dict(q=g, k=g.cpu()), "k_norm must be a GPU tensor"),
                        (dict(q=g, k=torch.ones(64, device="cuda")), r"q_norm / k_norm must be \[128\]"),
                        (dict(q=torch.ones(D + 8, device="cuda")[2:-6], k=g), "q_norm / k_norm must be 16-byte aligned"),
                        (dict(q=g, k=g, eps=0.0), "norm_eps must be > 0")]:
        with pytest.raises(RuntimeError, match=message):
            call(**kw)


def test_op_reaches_the_kernel():
    """RopeGQAttentionOp(qk_norm=...) on the device is the kernel's launch bit for bit; its torch path lies within the
    bound too."""
    from rust_tensorflow_serving2_amd.graph.patterns import RopeGQAttentionOp
    b, s, h, k = 2, 129, 4, 2
    qkv, tab, adder, gam = normed_inputs(b, s, h, k), tables(s), padding_adder(b, s), gammas()
    ref, bound = reference(qkv, tab, h, k, gam, adder, (s, h, k, True))
    direct = run(qkv, tab, adder, h, k, gam)
    for use_hip in (True, False):
        op = RopeGQAttentionOp(h, k, D, s, SCALE, -10000.0, tab[0], tab[1], torch.device("cuda"), use_hip,
                               qk_norm=(gam[0], gam[1], EPS))
        (y,) = op(None, None, [qkv.cuda().reshape(b * s, -1), adder.cuda().reshape(b, 1, 1, s)])
        assert y.dtype == BF and y.shape == (b * s, h * D)
        if use_hip:
            assert torch.equal(y.reshape(b, s, -1), direct)
        worst = kb.assert_within(y.reshape(b, s, -1), ref, bound, f"RopeGQAttentionOp qk_norm use_hip={use_hip}")
        print(f"RopeGQAttentionOp qk_norm use_hip={use_hip}: worst err/bound {worst:.3f}")
