"""fp64 references and elementwise bounds for the ModernBERT kernels (docs/numerics.md,
"RoPE encoder attention" and "GeGLU").  rope_attention: gqattn_bounds.rope_gqa_ref's
error model with H = Hkv and the -inf triangle replaced by the window |i - j| <= w
(w < 0: every key open).  No new constant: the rotation term, the (D + 4) E
dot-product term and the (s + 16) E denominator term stay as derived there.
"""
import torch

from kernel_bounds import E, U_BF16, act64, act_abs, d, out_bound

D = 64


def rope_attention_ref(qkv, cos, sin, heads, scale, window=-1, adder=None):
    """qkv [B, S, 3 H 64] bf16-valued, cos / sin [S, 32], adder None / [B | 1, S] -> (ref, bound) [B, S, H 64]."""
    b, s, _ = qkv.shape
    h = heads
    x, c, sn = d(qkv).reshape(b, s, 3, h, D).permute(2, 0, 3, 1, 4), d(cos), d(sin)

    def rot(t):                      # [B, H, S, 64] -> (rotated, magnitude)
        t1, t2 = t[..., :D // 2], t[..., D // 2:]
        mag = t1.abs() * c.abs() + t2.abs() * sn.abs()
        return torch.cat([t1 * c - t2 * sn, t2 * c + t1 * sn], -1), torch.cat([mag, mag], -1)
    (q, qm), (kk, km), v = rot(x[0]), rot(x[1]), x[2]
    sc = q @ kk.transpose(-1, -2) * scale
    asc = q.abs() @ kk.abs().transpose(-1, -2) * scale
    rot_err = (2 * U_BF16 + U_BF16 ** 2) * asc + 8 * E * (qm @ km.transpose(-1, -2)) * scale
    if window >= 0:
        pos = torch.arange(s)
        sc = sc.masked_fill((pos[:, None] - pos[None, :]).abs() > window, float("-inf"))
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
    return [t.permute(0, 2, 1, 3).reshape(b, s, h * D) for t in (ref, bound)]


def geglu_ref(gu):
    """(ref, bound) of geglu: the fp32 erf GELU's own error (kernel_bounds.act_abs; the gate is an exact bf16
    value, so the L_ACT term of an epilogue, Lipschitz constant times the pre-activation's error, is zero) times
    |up|, and one more product."""
    f = gu.shape[-1] // 2
    gate, up = d(gu)[..., :f], d(gu)[..., f:]
    ref = act64("gelu_erf", gate) * up
    return ref, out_bound(ref, act_abs("gelu_erf", gate) * up.abs() + E * ref.abs(), False)
