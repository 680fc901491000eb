"""fp64 reference and elementwise bound for patch_tokens (kernels/misc.hip); a plain helper module like
interact_bounds and wattn_bounds.  test_patch_tokens_gpu.py derives the bound in its docstring:

    bound = E |ref| + ulp_bf16(|ref| (1 + E)) / 2,   ulp_bf16(v) = 2^(floor(log2 v) - 7)
"""
import torch

import kernel_bounds as kb


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
