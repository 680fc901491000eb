"""patch_tokens (kernels/misc.hip): class token + patches + position embedding.

    y[b, 0, :]     = bf16(T[0, :])
    y[b, 1 + p, :] = bf16(float(x[b, p, :]) + T[1 + p, :])

against an fp64 reference.  x is already bf16 and T fp32, so the reference sum
is exact in fp64 and the kernel adds two roundings: the fp32 add (E |ref|,
kernel_bounds' per-operation figure) and ONE round-to-nearest store to bf16,
half an ulp of bf16 at the result:

    bound = E |ref| + ulp_bf16(|ref| (1 + E)) / 2,   ulp_bf16(v) = 2^(floor(log2 v) - 7)

Half an ulp lies between 2^-9 |ref| (top of a binade) and 2^-8 |ref| (bottom:
1 + 2^-8 stored as 1 or 1 + 2^-7 is off by 2^-8), so this is the exact form of
"one output rounding"; a flat 2^-9 |ref| would reject a correctly rounded
result in the lower half of every binade, a flat 2^-8 |ref| (kb.U_BF16) is up
to twice as wide.  A truncating store, or a second rounding, fails it.
"""
import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")


def hip():
    from rust_tensorflow_serving2_amd.ops import hip as _hip
    return _hip()


def operands(b, p, c, seed=0):
    x = kb.rnd(b, p, c, seed=seed + 1).to(BF)
    table = kb.rnd(p + 1, c, scale=0.5, seed=seed + 2)
    return x, table


def reference(x, table):
    """(ref, bound) [B, P + 1, C] in fp64."""
    b, p, c = x.shape
    t = kb.d(table)
    ref = torch.cat([t[0].expand(b, 1, c), kb.d(x) + t[1:]], dim=1)
    mag = ref.abs() * (1 + kb.E)
    half_ulp = torch.where(mag > 0, torch.exp2(torch.floor(torch.log2(mag.clamp_min(1e-300))) - 8),
                           torch.zeros_like(mag))
    # the class row is one rounding of T[0] itself (no add)
    bound = half_ulp + kb.E * ref.abs()
    return ref, bound


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("p", [1, 4, 196])
@pytest.mark.parametrize("c", [8, 192, 384, 768, 1000])
def test_patch_tokens_within_bound(c, p, b):
    x, table = operands(b, p, c, seed=c + p)
    assert hip().patch_tokens_supported(b, p, c)
    y = hip().patch_tokens(x.cuda(), table.cuda())
    assert y.shape == (b, p + 1, c) and y.dtype == BF
    ref, bound = reference(x, table)
    worst = kb.assert_within(y, ref, bound, f"patch_tokens B={b} P={p} C={c}")
    flat = int(((kb.d(y) - ref).abs() > 2.0 ** -9 * ref.abs() + kb.E * ref.abs()).sum())
    print(f"patch_tokens B={b} P={p} C={c}: worst err/bound {worst:.3f}; {flat} of {ref.numel()} correctly "
          f"rounded elements lie above a flat 2^-9 |ref|")


@pytest.mark.parametrize("b,p,c", [(3, 4, 8), (2, 196, 384), (1, 1, 1000)])
def test_patch_tokens_guard_bands(b, p, c):
    """x, table and out are views into larger NaN-filled buffers: the result is
    finite and within bound, every guard element is still NaN."""
    x, table = operands(b, p, c, seed=7)
    guard = 1024                                                    # elements: a 16-B multiple for bf16 and fp32
    n_x, n_t, n_y = x.numel(), table.numel(), b * (p + 1) * c
    big_x = torch.full((guard + n_x + guard,), NAN, dtype=BF, device="cuda")
    big_t = torch.full((guard + n_t + guard,), NAN, dtype=torch.float32, device="cuda")
    big_y = torch.full((guard + n_y + guard,), NAN, dtype=BF, device="cuda")
    big_x[guard:guard + n_x] = x.cuda().reshape(-1)
    big_t[guard:guard + n_t] = table.cuda().reshape(-1)
    out = big_y[guard:guard + n_y].view(b, p + 1, c)
    y = hip().patch_tokens(big_x[guard:guard + n_x].view(b, p, c), big_t[guard:guard + n_t].view(p + 1, c), out)
    assert y.data_ptr() == out.data_ptr()
    assert torch.isfinite(y).all()
    ref, bound = reference(x, table)
    kb.assert_within(y, ref, bound, f"guarded patch_tokens {(b, p, c)}")
    assert torch.isnan(big_y[:guard]).all() and torch.isnan(big_y[guard + n_y:]).all(), "a guard element was written"


@pytest.mark.parametrize("poison", [float("inf"), NAN])
def test_class_row_is_independent_of_x(poison):
    """The class row reads a clamped x chunk and drops it by a select: +Inf
    (or NaN) in x[b, 0, :] reaches patch row 1 only."""
    b, p, c = 2, 4, 64
    x, table = operands(b, p, c, seed=11)
    clean = hip().patch_tokens(x.cuda(), table.cuda())
    bad = x.clone()
    bad[:, 0, :] = poison
    y = hip().patch_tokens(bad.cuda(), table.cuda())
    assert torch.equal(y[:, 0], clean[:, 0]) and torch.isfinite(y[:, 0]).all()
    assert torch.equal(y[:, 2:], clean[:, 2:])
    assert not torch.isfinite(y[:, 1]).any()


def test_patch_tokens_rejections():
    H = hip()
    x, table = operands(2, 4, 16)
    with pytest.raises(RuntimeError, match="C % 8"):
        H.patch_tokens(torch.zeros(2, 4, 12, dtype=BF, device="cuda"), torch.zeros(5, 12, device="cuda"))
    assert not H.patch_tokens_supported(2, 4, 12)
    with pytest.raises(RuntimeError, match=r"table must be \[P \+ 1, C\]"):
        H.patch_tokens(x.cuda(), torch.zeros(4, 16, device="cuda"))
    with pytest.raises(RuntimeError, match="x must be 16-byte aligned"):
        big = torch.zeros(x.numel() + 8, dtype=BF, device="cuda")
        H.patch_tokens(big[1:1 + x.numel()].view(2, 4, 16), table.cuda())
    with pytest.raises(RuntimeError, match="table must be 16-byte aligned"):
        big = torch.zeros(table.numel() + 4, device="cuda")
        H.patch_tokens(x.cuda(), big[1:1 + table.numel()].view(5, 16))
    with pytest.raises(RuntimeError, match="out must be 16-byte aligned"):
        big = torch.zeros(2 * 5 * 16 + 8, dtype=BF, device="cuda")
        H.patch_tokens(x.cuda(), table.cuda(), big[1:1 + 2 * 5 * 16].view(2, 5, 16))
    with pytest.raises(RuntimeError, match="expected"):
        H.patch_tokens(x.cuda().float(), table.cuda())
