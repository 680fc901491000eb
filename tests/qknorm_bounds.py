"""fp64 reference and elementwise bound for rope_gqa_attention with a QK-norm
(kernels/gqattn128.hip, NORM builds; docs/numerics.md, "QK-norm"): a helper like
rattn_bounds.  gqattn_bounds.rope_gqa_ref's model at D = 128 with q and k
normalised per head in fp64 first, x^ = x rsqrt(mean(x^2) + eps) gamma, and one
more term in the score error ds_j.

The kernel rotates x^' = fp32(x^) where the reference rotates x^.  Each operand
carries the relative error gqattn_bounds.rmsnorm_ref derives for a 128-deep row,
dn = (D / 2 + 8) E, so

    |q^' . k^' - q^ . k^| <= (2 dn + dn^2) |q^| . |k^|  ->  (D + 16 + 2) E asc

(D + 16) E for 2 dn; 2 E spare for dn^2 = 72^2 E^2 < 0.001 E and for the cross
terms of dn with the operands' bf16 roundings, 2 dn (2 U + U^2) < 1.2 E).  The
rotation's magnitudes qm / km are taken of the normalised values.  The kernel
rounds x^ nowhere, so no U term is added: the unfused graph's rounding of the
norm's output is what the fusion removes.
"""
import torch

from kernel_bounds import E, U_BF16, d

D = 128


def qknorm_rope_gqa_ref(qkv, cos, sin, heads, kv_heads, scale, q_gamma, k_gamma, eps, adder=None):
    """qkv [B, S, (H + 2 Hkv) 128] bf16-valued, cos / sin [S, 64], gammas [128] -> (ref, bound) [B, S, H 128]."""
    b, s, _ = qkv.shape
    h, k = heads, kv_heads
    x, c, sn = d(qkv), d(cos)[None, :, None, :], d(sin)[None, :, None, :]

    def norm(t, gamma):
        return t * torch.rsqrt((t * t).mean(-1, keepdim=True) + eps) * d(gamma)

    def rot(t):                      # -> (rotated, magnitude)
        t1, t2 = t[..., :D // 2], t[..., D // 2:]
        mag = t1.abs() * c.abs() + t2.abs() * sn.abs()
        return torch.cat([t1 * c - t2 * sn, t2 * c + t1 * sn], -1), torch.cat([mag, mag], -1)

    def heads_first(t):              # [B, S, n, 128] -> [B, H, S, 128], each head repeated for its group
        return t.repeat_interleave(h // t.shape[2], 2).permute(0, 2, 1, 3)
    q, qm = rot(norm(x[..., :h * D].reshape(b, s, h, D), q_gamma))
    kk, km = rot(norm(x[..., h * D:(h + k) * D].reshape(b, s, k, D), k_gamma))
    v = heads_first(x[..., (h + k) * D:].reshape(b, s, k, D))
    q, qm, kk, km = heads_first(q), heads_first(qm), heads_first(kk), heads_first(km)
    sc = q @ kk.transpose(-1, -2) * scale
    asc = q.abs() @ kk.abs().transpose(-1, -2) * scale
    rot_err = (2 * U_BF16 + U_BF16 ** 2) * asc + 8 * E * (qm @ km.transpose(-1, -2)) * scale
    norm_err = (D + 16 + 2) * E * asc
    sc = sc + torch.triu(torch.full((s, s), float("-inf"), dtype=torch.float64), 1)
    if adder is not None:
        sc = sc + d(adder)[:, None, None, :]
    p = torch.softmax(sc, -1)
    assert torch.isfinite(p).all(), "a query row with no open key has no defined result"
    ds = (D + 4) * E * asc + E * torch.where(p > 0, sc.abs(), torch.zeros_like(sc)) + rot_err + norm_err
    ds = torch.where(p > 0, ds, torch.zeros_like(ds))
    pav, ref = p @ v.abs(), p @ v
    num = (p * (U_BF16 + ds)) @ v.abs()
    den = (p * ds).sum(-1, keepdim=True) + (s + 16) * E
    bound = (num + pav * den) * (1 + U_BF16) + U_BF16 * ref.abs()
    return [t.permute(0, 2, 1, 3).reshape(b, s, h * D) for t in (ref, bound)]
