"""geglu (kernels/llama.hip) against rattn_bounds.geglu_ref: the shortest row, a
row length that is no multiple of the 256-thread launch's chunks, and
ModernBERT's F = 1152; gates at +-0, out to +-30, and an Inf row beside clean ones."""
import pytest
import torch

import kernel_bounds as kb
import rattn_bounds as rb

from test_llama_kernels_gpu import BF, banded, guards_intact, hip

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("f", [8, 72, 1152])
def test_geglu_within_bound(f):
    m = 37
    gu = kb.rnd(m, 2 * f, scale=3.0, seed=f)
    gu[::5, :f] = torch.where(gu[::5, :f] > 0, 30.0, -30.0)         # erf saturated at both ends
    gu[1, :f:2], gu[1, 1:f:2] = 0.0, -0.0
    gu = gu.to(BF)
    big_in, iv = banded(m * 2 * f)
    iv.copy_(gu.reshape(-1))
    big_out, ov = banded(m * f)
    y = hip().geglu(iv.view(m, 2 * f), ov.view(m, f))
    ref, bound = rb.geglu_ref(gu)
    worst = kb.assert_within(y, ref, bound, f"geglu F={f}")
    print(f"geglu F={f}: worst err/bound {worst:.3f}")
    assert guards_intact(big_in) and guards_intact(big_out)
    # an Inf row leaves its neighbours bit-equal
    bad = gu.clone()
    bad[2] = float("inf")
    z = hip().geglu(bad.cuda())
    keep = [i for i in range(m) if i != 2]
    assert torch.equal(z[keep], y[keep]) and not torch.isfinite(z[2]).any()


def test_rejections():
    H = hip()
    x = torch.zeros(4, 64, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError, match="F % 8 == 0"):
        H.geglu(torch.zeros(4, 24, dtype=BF, device="cuda"))
    with pytest.raises(RuntimeError, match="wrong size"):
        H.geglu(x, x)
