"""fp64 reference and elementwise bound for rope_gqa_attention256 (kernels/gqattn256.hip;
docs/numerics.md, "RoPE + GQA attention, D = 256"): a helper like rattn_bounds.

It is qknorm_bounds.qknorm_rope_gqa_ref's model at D = 256 with a sliding window.  The
D-dependent terms follow the depth of the dot products: the score is a 256-deep fp32
accumulation, (D + 4) E asc; with a QK-norm each operand carries the relative error of a
256-deep RMSNorm, dn = (D / 2 + 8) E, so the normalised score moves by (2 dn + dn^2) asc ->
(D + 16 + 2) E asc = (D + 18) E asc (dn^2 = 136^2 E^2 < 0.002 E and the cross terms with the
bf16 roundings stay inside the 2 E spare).  Without a norm that term is absent, which is
gqattn_bounds.rope_gqa_ref's model.  Key j is open for query i iff 0 <= i - j <= window
(window < 0: j <= i); a closed key weighs exactly 0 and adds no error.
"""
import torch

from kernel_bounds import E, U_BF16, d

D = 256


def rope_gqa256_ref(qkv, cos, sin, heads, kv_heads, scale, window=-1, qk_norm=None, adder=None):
    """qkv [B, S, (H + 2 Hkv) 256] bf16-valued, cos / sin [S, 128], qk_norm None | (q_gamma [256], k_gamma [256],
    eps), adder None | [B | 1, S] -> (ref, bound) [B, S, H 256]."""
    b, s, _ = qkv.shape
    h, k = heads, kv_heads
    x, c, sn = d(qkv), d(cos)[None, :, None, :], d(sin)[None, :, None, :]

    def norm(t, gamma):
        if qk_norm is None:
            return t
        return t * torch.rsqrt((t * t).mean(-1, keepdim=True) + qk_norm[2]) * d(gamma)

    def rot(t):                      # -> (rotated, magnitude)
        t1, t2 = t[..., :D // 2], t[..., D // 2:]
        mag = t1.abs() * c.abs() + t2.abs() * sn.abs()
        return torch.cat([t1 * c - t2 * sn, t2 * c + t1 * sn], -1), torch.cat([mag, mag], -1)

    def heads_first(t):              # [B, S, n, 256] -> [B, H, S, 256], each head repeated for its group
        return t.repeat_interleave(h // t.shape[2], 2).permute(0, 2, 1, 3)
    qg, kg = qk_norm[:2] if qk_norm is not None else (None, None)
    q, qm = rot(norm(x[..., :h * D].reshape(b, s, h, D), qg))
    kk, km = rot(norm(x[..., h * D:(h + k) * D].reshape(b, s, k, D), kg))
    v = heads_first(x[..., (h + k) * D:].reshape(b, s, k, D))
    q, qm, kk, km = heads_first(q), heads_first(qm), heads_first(kk), heads_first(km)
    sc = q @ kk.transpose(-1, -2) * scale
    asc = q.abs() @ kk.abs().transpose(-1, -2) * scale
    rot_err = (2 * U_BF16 + U_BF16 ** 2) * asc + 8 * E * (qm @ km.transpose(-1, -2)) * scale
    norm_err = (D + 18) * E * asc if qk_norm is not None else 0.0
    diff = torch.arange(s)[:, None] - torch.arange(s)[None, :]
    open_ = (diff >= 0) & ((diff <= window) if window >= 0 else (diff >= 0))
    sc = sc + torch.where(open_, 0.0, float("-inf")).to(torch.float64)
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
