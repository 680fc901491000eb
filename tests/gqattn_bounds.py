"""fp64 references and elementwise bounds for the Llama kernels (a helper module
like kernel_bounds, which it builds on; docs/numerics.md, "RoPE + GQA attention",
"RMSNorm" and "SwiGLU", has the derivations in prose).

rope_gqa_attention (kernels/gqattn.hip): kernel_bounds.attention_ref's model with
one more term in the score error ds_j.  The kernel hands the MFMA
q^ = bf16(fp32(q~)), k^ = bf16(fp32(k~)) instead of the exact rotations.  With
qm = |x1| |cos| + |x2| |sin| >= |q~| (the magnitude the fp32 rotation works at:
two products and one subtraction, <= 2 E qm, carried through the bf16 rounding
<= 3 E qm) and km likewise:

    |q^ . k^ - q~ . k~| <= (2 U + U^2) |q~| . |k~_j| + 8 E qm . km_j

(U = U_BF16: one rounding per operand and their product; 6 E for the two
rotations, 2 E spare for the cross terms and for the accumulation running over
the rounded operands).
"""
import torch

import swish_bounds as swb
from kernel_bounds import E, U_BF16, d, out_bound

D = 64


def rope_gqa_ref(qkv, cos, sin, heads, kv_heads, scale, adder=None):
    """qkv [B, S, (H + 2 Hkv) 64] bf16-valued, cos / sin [S, 32], adder None / [B | 1, S] -> (ref, bound) [B, S, H 64]."""
    b, s, _ = qkv.shape
    h, k, g = heads, kv_heads, heads // kv_heads
    x, c, sn = d(qkv), d(cos)[None, :, None, :], d(sin)[None, :, None, :]

    def rot(t):                      # -> (rotated, magnitude)
        t1, t2 = t[..., :D // 2], t[..., D // 2:]
        mag = t1.abs() * c.abs() + t2.abs() * sn.abs()
        return torch.cat([t1 * c - t2 * sn, t2 * c + t1 * sn], -1), torch.cat([mag, mag], -1)

    def heads_first(t):              # [B, S, n, 64] -> [B, H, S, 64], each head repeated for its group
        return t.repeat_interleave(h // t.shape[2], 2).permute(0, 2, 1, 3)
    (q, qm), (kk, km) = rot(x[..., :h * D].reshape(b, s, h, D)), rot(x[..., h * D:(h + k) * D].reshape(b, s, k, D))
    v = heads_first(x[..., (h + k) * D:].reshape(b, s, k, D))
    q, qm, kk, km = heads_first(q), heads_first(qm), heads_first(kk), heads_first(km)
    sc = q @ kk.transpose(-1, -2) * scale
    asc = q.abs() @ kk.abs().transpose(-1, -2) * scale
    rot_err = (2 * U_BF16 + U_BF16 ** 2) * asc + 8 * E * (qm @ km.transpose(-1, -2)) * scale
    sc = sc + torch.triu(torch.full((s, s), float("-inf"), dtype=torch.float64), 1)
    if adder is not None:
        sc = sc + d(adder)[:, None, None, :]
    p = torch.softmax(sc, -1)
    assert torch.isfinite(p).all(), "a query row with no open key has no defined result"
    ds = (D + 4) * E * asc + E * torch.where(p > 0, sc.abs(), torch.zeros_like(sc)) + rot_err
    ds = torch.where(p > 0, ds, torch.zeros_like(ds))
    pav, ref = p @ v.abs(), p @ v
    num = (p * (U_BF16 + ds)) @ v.abs()
    den = (p * ds).sum(-1, keepdim=True) + (s + 16) * E
    bound = (num + pav * den) * (1 + U_BF16) + U_BF16 * ref.abs()
    assert g * k == h
    return [t.permute(0, 2, 1, 3).reshape(b, s, h * D) for t in (ref, bound)]


def rmsnorm_ref(x, gamma, eps, residual=None):
    """(ref, bound, sum ref, sum bound) of kernels/llama.hip rmsnorm: kernel_bounds.layernorm_ref's derivation
    without the mean, so every term is relative to |ref|.  z = x + r is one fp32 addition (E); mean(z^2) is a
    cols-deep fp32 dot product (cols E), divided by cols (E) and carrying z's error twice (2 E); + eps (E); rsqrt
    halves that and adds its own ulp (E); two products (2 E):  (cols / 2 + 6) E, two spare -> (cols / 2 + 8) E."""
    z = d(x) if residual is None else d(x) + d(residual)
    cols = z.shape[-1]
    ref = z * torch.rsqrt((z * z).mean(-1, keepdim=True) + eps) * d(gamma)
    return ref, out_bound(ref, (cols / 2 + 8) * E * ref.abs(), False), z, out_bound(z, E * z.abs(), False)


def swiglu_ref(gu):
    """(ref, bound) of swiglu: swish_bounds.swish_own for the fp32 swish, times |up|, and one more product."""
    f = gu.shape[-1] // 2
    gate, up = d(gu)[..., :f], d(gu)[..., f:]
    ref = swb.swish64(gate) * up
    return ref, out_bound(ref, swb.swish_own(gate) * up.abs() + E * ref.abs(), False)
