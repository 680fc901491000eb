"""fp64 reference and elementwise bound for kernels/battn.hip (attention with a
relative-position bias).  A plain helper module.

The kernel's arithmetic is attention.hip's with two adders, as in wattn.hip:
s = ((q . k) scale + T[h][j - i + S - 1]) + key_adder[j] in fp32, the table read as
it is (no pre-multiplied copy: no further rounding).  kernel_bounds.attention_ref
takes the dense bias plus the key adder as one 4-D adder and models one fp32 add;
with a key adder the second add rounds once more, by at most E |t|, t = (q . k)
scale + bias: wattn_bounds' term (docs/numerics.md, "Relative-bias attention").
No new constant.
"""
import torch

import kernel_bounds as KB


def dense_bias(table, s):
    """table [H, 2 S - 1] -> [1, H, S, S] fp64: entry (i, j) = table[h, j - i + S - 1]."""
    pos = torch.arange(s)
    return KB.d(table)[:, pos[None, :] - pos[:, None] + (s - 1)][None]


def bias_attention_ref(qkv, table, heads, scale, adder=None):
    """qkv [B, S, 3 H 64] bf16-valued, table [H, 2 S - 1], adder None / [B | 1, S] -> (ref, bound) [B, S, H 64]."""
    b, s, w3 = qkv.shape
    dh = w3 // (3 * heads)
    bias = dense_bias(table, s)
    if adder is None:
        return KB.attention_ref(qkv, heads, scale, bias.expand(b, -1, -1, -1))
    ka = KB.d(adder)[:, None, None, :]
    ref, bound = KB.attention_ref(qkv, heads, scale, (bias + ka).expand(b, -1, -1, -1))
    q, k, v = KB.d(qkv).reshape(b, s, 3, heads, dh).permute(2, 0, 3, 1, 4)
    t = q @ k.transpose(-1, -2) * scale + bias
    p = torch.softmax(t + ka, -1)
    ds2 = torch.where(p > 0, KB.E * t.abs(), torch.zeros_like(t))
    extra = ((p * ds2) @ v.abs() + (p @ v.abs()) * (p * ds2).sum(-1, keepdim=True)) * (1 + KB.U_BF16)
    return ref, bound + extra.permute(0, 2, 1, 3).reshape(b, s, heads * dh)


def table_for(heads, s, seed=0):
    """A unit-scale random table: asymmetric in j - i and different per head."""
    return KB.rnd(heads, 2 * s - 1, seed=9000 + 13 * s + heads + seed)
