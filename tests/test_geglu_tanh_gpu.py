"""geglu(approximate=True) (kernels/llama.hip, the tanh-approximate gate) against an fp64
reference.  The bound is rattn_bounds.geglu_ref's with the activation swapped: the fp32
gelu_tanh's own error (kernel_bounds.act_abs; the gate is an exact bf16 value, so no
Lipschitz term) times |up|, one more product and the bf16 store.  Widths on both sides of
one 16-B vector (8, 16) and of the 256-thread launch's row tile (2040, 2048, 2056), and
Gemma-3-1B's F = 6912."""
import pytest
import torch

import kernel_bounds as kb
from kernel_bounds import out_bound

from test_llama_kernels_gpu import BF, banded, guards_intact, hip

pytestmark = pytest.mark.gpu


def geglu_tanh_ref(gu):
    f = gu.shape[-1] // 2
    gate, up = kb.d(gu)[..., :f], kb.d(gu)[..., f:]
    ref = kb.act64("gelu_tanh", gate) * up
    return ref, out_bound(ref, kb.act_abs("gelu_tanh", gate) * up.abs() + kb.E * ref.abs(), False)


@pytest.mark.parametrize("f", [8, 16, 2040, 2048, 2056, 6912])
def test_geglu_tanh_within_bound(f):
    m = 5
    gu = kb.rnd(m, 2 * f, scale=3.0, seed=f)
    gu[::3, :f] = torch.where(gu[::3, :f] > 0, 30.0, -30.0)         # tanh saturated at both ends
    gu[1, :f:2], gu[1, 1:f:2] = 0.0, -0.0
    gu = gu.to(BF)
    big_in, iv = banded(m * 2 * f)
    iv.copy_(gu.reshape(-1))
    big_out, ov = banded(m * f)
    y = hip().geglu(iv.view(m, 2 * f), ov.view(m, f), True)
    ref, bound = geglu_tanh_ref(gu)
    worst = kb.assert_within(y, ref, bound, f"geglu tanh F={f}")
    print(f"geglu tanh F={f}: worst err/bound {worst:.3f}")
    assert guards_intact(big_in) and guards_intact(big_out)
    assert torch.equal(hip().geglu(gu.cuda(), None, False), hip().geglu(gu.cuda()))    # the default is the erf form
