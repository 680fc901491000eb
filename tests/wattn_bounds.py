"""fp64 reference and elementwise bound for kernels/wattn.hip (windowed
attention), plus pure-torch window layouts.  A plain helper module.

The kernel's arithmetic is attention.hip's register kernel with two adders:
s = ((q . k) scale + bias[h]) + mask[w] in fp32.  kernel_bounds.attention_ref
takes the sum bias + mask as one broadcast 4-D adder and models one fp32 add;
the second add rounds once more, by at most E |t| with t = (q . k) scale +
bias the first sum (docs/numerics.md, "Windowed attention").  That term joins
ds_j wherever a mask is added (without one the kernel adds an exact 0.0):

    extra = ( sum_j p_j E |t_j| |v_j| + (P |V|) sum_j p_j E |t_j| ) (1 + 2^-8)
"""
import torch

import kernel_bounds as KB


def window_adder(bias, mask, windows):
    """bias [H, S, S], mask [nW, S, S] | None -> the fp64 adder [windows, H, S, S]; window bw takes mask bw % nW."""
    add = KB.d(bias)[None].expand(windows, -1, -1, -1)
    if mask is not None:
        idx = torch.arange(windows) % mask.shape[0]
        add = add + KB.d(mask)[idx][:, None]
    return add


def window_attention_ref(qkv, bias, mask, heads, scale):
    """qkv [Bw * S, 3 H D] bf16-valued in window order -> (ref, bound) [Bw * S, H D]."""
    S = bias.shape[1]
    R, w3 = qkv.shape
    bw, dh = R // S, w3 // (3 * heads)
    q3 = qkv.reshape(bw, S, w3)
    ref, bound = KB.attention_ref(q3, heads, scale, window_adder(bias, mask, bw))
    if mask is not None:
        q, k, v = KB.d(q3).reshape(bw, S, 3, heads, dh).permute(2, 0, 3, 1, 4)
        t = q @ k.transpose(-1, -2) * scale + KB.d(bias)[None]
        p = torch.softmax(t + window_adder(torch.zeros_like(bias), mask, bw), -1)
        ds2 = torch.where(p > 0, KB.E * t.abs(), torch.zeros_like(t))
        extra = ((p * ds2) @ v.abs() + (p @ v.abs()) * (p * ds2).sum(-1, keepdim=True)) * (1 + KB.U_BF16)
        bound = bound + extra.permute(0, 2, 1, 3).reshape(bw, S, heads * dh)
    return ref.reshape(R, heads * dh), bound.reshape(R, heads * dh)


# ---------------------------------------------------------------- layouts
def to_windows(x, B, Hf, Wf, ws, shift):
    """[B * Hf * Wf, C] in image order -> [Bw * ws * ws, C] in window order: Roll(-shift) then partition."""
    C = x.shape[-1]
    x = x.reshape(B, Hf, Wf, C)
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    x = x.reshape(B, Hf // ws, ws, Wf // ws, ws, C).permute(0, 1, 3, 2, 4, 5)
    return x.reshape(-1, C)


def from_windows(y, B, Hf, Wf, ws, shift):
    """The inverse: reverse the partition, then Roll(+shift)."""
    C = y.shape[-1]
    y = y.reshape(B, Hf // ws, Wf // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hf, Wf, C)
    if shift:
        y = torch.roll(y, (shift, shift), (1, 2))
    return y.reshape(-1, C)


def grid_rows(B, Hf, Wf, ws, shift):
    """The kernel's row formula: [Bw, ws * ws] int64, row of token (i, j) of window (b, wy, wx)."""
    rows = []
    for b in range(B):
        for wy in range(Hf // ws):
            for wx in range(Wf // ws):
                rows.append([b * Hf * Wf + ((wy * ws + i + shift) % Hf) * Wf + ((wx * ws + j + shift) % Wf)
                             for i in range(ws) for j in range(ws)])
    return torch.tensor(rows, dtype=torch.int64)


def window_attention_grid_ref(qkv, bias, mask, heads, scale, grid):
    """qkv [B * Hf * Wf, 3 H D] in image order -> (ref, bound) in image order, by explicit roll / partition / reverse."""
    Hf, Wf, ws, shift = grid
    B = qkv.shape[0] // (Hf * Wf)
    ref, bound = window_attention_ref(to_windows(qkv, B, Hf, Wf, ws, shift), bias, mask, heads, scale)
    return from_windows(ref, B, Hf, Wf, ws, shift), from_windows(bound, B, Hf, Wf, ws, shift)


# ---------------------------------------------------------------- inputs
def inputs(rows, heads, S, nW=None, seed=0, dh=32, qk_scale=1.0):
    """(qkv bf16 [rows, 3 H D], bias [H, S, S], mask [nW, S, S] | None): unit-scale q / k / v, a unit-scale
    bias, and a 0 / -100 mask that differs from window to window."""
    qkv = KB.rnd(rows, 3 * heads * dh, scale=qk_scale, seed=seed).to(KB.BF)
    bias = KB.rnd(heads, S, S, seed=seed + 1)
    mask = None
    if nW is not None:
        g = torch.Generator(device="cpu").manual_seed(seed + 2)
        region = torch.randint(0, 3, (nW, S), generator=g)
        mask = torch.where(region[:, :, None] != region[:, None, :], -100.0, 0.0).float().contiguous()
    return qkv, bias, mask
