"""The error model of kernels/wattn.hip on the CPU: the kernel's scheme,
emulated in fp32 torch with P rounded to bf16, meets wattn_bounds' bound; three
wrong schemes do not; the kernel's row formula is Roll / partition."""
import pytest
import torch

import kernel_bounds as KB
import wattn_bounds as WB

H, SCALE = 3, 32 ** -0.5


def emulate(qkv, bias, mask, heads, scale, head_shift=0, clamp_mask=False):
    """The kernel's arithmetic on rows in window order: fp32 scores, two fp32 adds, keys summed unrounded,
    P rounded to bf16 for P V, one division, one rounding.  ``head_shift`` reads the bias of head h +
    head_shift; ``clamp_mask`` indexes the mask by min(bw, nW - 1) instead of bw % nW (both wrong)."""
    S = bias.shape[1]
    R, w3 = qkv.shape
    bw, dh = R // S, w3 // (3 * heads)
    q, k, v = qkv.float().reshape(bw, S, 3, heads, dh).permute(2, 0, 3, 1, 4)
    sc = (q @ k.transpose(-1, -2)) * scale + torch.roll(bias, -head_shift, 0)[None]
    if mask is not None:
        idx = torch.arange(bw).clamp(max=mask.shape[0] - 1) if clamp_mask else torch.arange(bw) % mask.shape[0]
        sc = sc + mask[idx][:, None]
    p = torch.exp(sc - sc.max(-1, keepdim=True).values)
    o = (p.to(KB.BF).float() @ v) / p.sum(-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(R, heads * dh).to(KB.BF)


@pytest.mark.parametrize("S", [16, 25, 49, 64])
@pytest.mark.parametrize("nW", [None, 4])
def test_kernel_scheme_meets_the_bound(S, nW):
    qkv, bias, mask = WB.inputs(8 * S, H, S, nW, seed=S)
    ref, bound = WB.window_attention_ref(qkv, bias, mask, H, SCALE)
    worst = KB.assert_within(emulate(qkv, bias, mask, H, SCALE), ref, bound, f"S={S} nW={nW}")
    assert worst > 0.0


def test_bias_of_the_next_head_violates_the_bound():
    qkv, bias, mask = WB.inputs(8 * 49, H, 49, None, seed=1)
    ref, bound = WB.window_attention_ref(qkv, bias, mask, H, SCALE)
    with pytest.raises(AssertionError, match="outside the bound"):
        KB.assert_within(emulate(qkv, bias, mask, H, SCALE, head_shift=1), ref, bound)


def test_clamped_mask_index_violates_the_bound():
    qkv, bias, mask = WB.inputs(8 * 16, H, 16, 4, seed=2)           # windows 4 .. 7 take masks 0 .. 3
    ref, bound = WB.window_attention_ref(qkv, bias, mask, H, SCALE)
    y = emulate(qkv, bias, mask, H, SCALE, clamp_mask=True)
    with pytest.raises(AssertionError, match="outside the bound"):
        KB.assert_within(y, ref, bound)
    KB.assert_within(y[:4 * 16], ref[:4 * 16], bound[:4 * 16])      # (the first image is right either way)


def test_roll_in_the_opposite_direction_violates_the_bound():
    grid = (8, 8, 4, 2)
    qkv, bias, mask = WB.inputs(2 * 64, H, 16, 4, seed=3)
    ref, bound = WB.window_attention_grid_ref(qkv, bias, mask, H, SCALE, grid)
    right = WB.from_windows(emulate(WB.to_windows(qkv, 2, *grid), bias, mask, H, SCALE).float(), 2, *grid)
    KB.assert_within(right, ref, bound)
    wrong_grid = (8, 8, 4, -2)
    wrong = WB.from_windows(emulate(WB.to_windows(qkv, 2, *wrong_grid), bias, mask, H, SCALE).float(), 2, *wrong_grid)
    with pytest.raises(AssertionError, match="outside the bound"):
        KB.assert_within(wrong, ref, bound)


@pytest.mark.parametrize("grid", [(8, 8, 4, 0), (8, 8, 4, 2), (14, 14, 7, 3), (8, 12, 4, 1), (7, 7, 7, 0)])
def test_row_formula_is_roll_and_partition(grid):
    Hf, Wf, ws, shift = grid
    B = 2
    rows = torch.arange(B * Hf * Wf, dtype=torch.float32)[:, None]
    explicit = WB.to_windows(rows, B, Hf, Wf, ws, shift).reshape(-1, ws * ws).long()
    assert torch.equal(WB.grid_rows(B, Hf, Wf, ws, shift), explicit)
    # and the way back: scattering window order through the formula is reverse + Roll(+shift)
    back = torch.empty(B * Hf * Wf, 1)
    back[explicit.reshape(-1)] = torch.arange(B * Hf * Wf, dtype=torch.float32)[:, None]
    assert torch.equal(WB.from_windows(torch.arange(B * Hf * Wf, dtype=torch.float32)[:, None], B, Hf, Wf, ws, shift),
                       back)
