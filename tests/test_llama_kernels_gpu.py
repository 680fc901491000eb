"""rmsnorm and swiglu (kernels/llama.hip) against gqattn_bounds' fp64 references.

rmsnorm: one row length per lane layout (16 / 32 / 64 lanes per row, 4 and 8
chunks per lane) and 37 rows, no multiple of any rows-per-workgroup (16, 8, 4),
with and without the residual and its second output, all inside NaN guard bands.
swiglu: the shortest row and one of 64 chunks, gates out to +-30."""
import pytest
import torch

import gqattn_bounds as gb
import kernel_bounds as kb

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")
GUARD = 4096


def hip():
    from rust_tensorflow_serving2_amd.ops import hip as _hip
    return _hip()


def banded(n):
    """(buffer, view): n bf16 elements between two NaN guard bands."""
    big = torch.full((GUARD + n + GUARD,), NAN, dtype=BF, device="cuda")
    return big, big[GUARD:GUARD + n]


def guards_intact(big):
    return bool(torch.isnan(big[:GUARD]).all() and torch.isnan(big[-GUARD:]).all())


@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("cols", [8, 256, 2048, 4096])
def test_rmsnorm_within_bound(cols, residual):
    rows, eps = 37, 1e-5
    x = kb.rnd(rows, cols, scale=1.5, seed=cols).to(BF)
    r = kb.rnd(rows, cols, seed=cols + 1).to(BF) if residual else None
    gamma = 1.0 + 0.2 * kb.rnd(cols, seed=cols + 2)
    big_x, xv = banded(rows * cols)
    xv.copy_(x.reshape(-1))
    big_y, yv = banded(rows * cols)
    big_z, zv = banded(rows * cols)
    y = hip().rmsnorm(xv.view(rows, cols), gamma.cuda(), eps, None if r is None else r.cuda(), yv.view(rows, cols),
                      zv.view(rows, cols) if residual else None)
    ref, bound, zref, zbound = gb.rmsnorm_ref(x, gamma, eps, r)
    worst = kb.assert_within(y, ref, bound, f"rmsnorm C={cols} residual={residual}")
    print(f"rmsnorm C={cols} residual={residual}: worst err/bound {worst:.3f}")
    if residual:
        kb.assert_within(zv.view(rows, cols), zref, zbound, f"rmsnorm sum C={cols}")
    else:
        assert torch.isnan(zv).all(), "sum_out was not given"
    assert guards_intact(big_x) and guards_intact(big_y) and guards_intact(big_z)


@pytest.mark.parametrize("f", [8, 512])
def test_swiglu_within_bound(f):
    m = 37
    gu = kb.rnd(m, 2 * f, scale=3.0, seed=f)
    gu[::5, :f] = torch.where(gu[::5, :f] > 0, 30.0, -30.0)         # both saturated ends of the sigmoid
    gu = gu.to(BF)
    big_in, iv = banded(m * 2 * f)
    iv.copy_(gu.reshape(-1))
    big_out, ov = banded(m * f)
    y = hip().swiglu(iv.view(m, 2 * f), ov.view(m, f))
    ref, bound = gb.swiglu_ref(gu)
    worst = kb.assert_within(y, ref, bound, f"swiglu F={f}")
    print(f"swiglu F={f}: worst err/bound {worst:.3f}")
    assert guards_intact(big_in) and guards_intact(big_out)


def test_rejections():
    H = hip()
    x = torch.zeros(4, 64, dtype=BF, device="cuda")
    g = torch.ones(64, device="cuda")
    with pytest.raises(RuntimeError, match="C % 8 == 0"):
        H.rmsnorm(torch.zeros(4, 12, dtype=BF, device="cuda"), torch.ones(12, device="cuda"), 1e-5)
    with pytest.raises(RuntimeError, match="C % 8 == 0"):
        H.rmsnorm(x, torch.ones(32, device="cuda"), 1e-5)
    with pytest.raises(RuntimeError, match="residual shape"):
        H.rmsnorm(x, g, 1e-5, x[:2].contiguous())
    with pytest.raises(RuntimeError, match="dtype"):
        H.rmsnorm(x.float(), g, 1e-5)
    with pytest.raises(RuntimeError, match="F % 8 == 0"):
        H.swiglu(torch.zeros(4, 24, dtype=BF, device="cuda"))
    with pytest.raises(RuntimeError, match="wrong size"):
        H.swiglu(x, x)
