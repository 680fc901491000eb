"""The checker of the grouped-conv bound (gconv_bounds.py) tested on the CPU, as
test_se_bounds_cpu.py tests se_bounds: an fp32 emulation of the kernel -- the K
slots of a group summed in a shuffled order, one round-to-nearest-even store --
passes, and each plausible mistake fails: a truncating store, a dropped tap, a
top / left pad that is off by one, the neighbouring group's filter.  The host
packing of the filter into MFMA fragments is checked here too."""
import pytest
import torch
import torch.nn.functional as F

import gconv_bounds as gb
import kernel_bounds as kb
from kernel_bounds import BF, rnd
from rust_tensorflow_serving2_amd.graph.fused import gconv_ksteps, pack_grouped_filter

N, H, W = 2, 9, 7
CASES = [(4, 24, 1), (8, 24, 2), (16, 32, 1), (32, 64, 2)]        # Cg, C, stride


def inputs(cg, c, seed=0):
    x = rnd(N, H, W, c, seed=seed + 1).to(BF)
    w = rnd(3, 3, cg, c, scale=(9 * cg) ** -0.5, seed=seed + 2).to(BF)
    b = 0.5 + rnd(c, scale=0.3, seed=seed + 3)
    return x, w, b


def emulate(x, w, b, stride, pads, act, seed=0, drop_tap=None, roll_groups=0, truncate=False):
    """gconv2d in fp32 torch: per group, the 9 Cg products of an output summed
    one by one in a shuffled order (an MFMA's order is not specified), then
    bias, activation, one store to bf16.  The mistakes are switches."""
    pt, pb, pl, pr = pads
    cg, c = w.shape[2], w.shape[3]
    g = c // cg
    xp = F.pad(x.float().permute(0, 3, 1, 2), [pl, pr, pt, pb])
    cols = F.unfold(xp, 3, stride=stride)                                   # [N][C * 9][L], (channel, tap) order
    n, _, L = cols.shape
    cols = cols.reshape(n, g, cg, 9, L).permute(0, 1, 3, 2, 4).reshape(n, g, 9 * cg, L)     # K = (tap, channel)
    wf = w.float().reshape(9, cg, g, cg).permute(2, 0, 1, 3).reshape(g, 9 * cg, cg)        # [g][K][out]
    wf = wf.roll(roll_groups, 0)
    if drop_tap is not None:
        wf = wf.clone()
        wf[:, drop_tap * cg:(drop_tap + 1) * cg] = 0
    order = torch.randperm(9 * cg, generator=torch.Generator().manual_seed(seed))
    acc = torch.zeros(n, g, cg, L)
    for k in order.tolist():
        acc = acc + cols[:, :, k, None, :] * wf[None, :, k, :, None]       # one fp32 rounding per K slot
    ho = (H + pt + pb - 3) // stride + 1
    y = acc.reshape(n, c, ho, -1).permute(0, 2, 3, 1) + b
    y = torch.relu(y) if act == "relu" else y
    if truncate:
        return (y.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return y.to(BF)


@pytest.mark.parametrize("cg,c,stride", CASES)
@pytest.mark.parametrize("act", ["none", "relu"])
def test_emulation_within_bound(cg, c, stride, act):
    x, w, b = inputs(cg, c)
    pads = (1, 1, 1, 1)
    ref, bound = gb.gconv_ref(x, w, b, stride, pads, act)
    worst = kb.assert_within(emulate(x, w, b, stride, pads, act), ref, bound, f"gconv emulation {cg} {c} {act}")
    assert worst <= 1.0
    if act == "relu":
        assert 0.05 < (ref == 0).double().mean() < 0.6         # the ReLU really clamps


@pytest.mark.parametrize("cg,c,stride", CASES)
@pytest.mark.parametrize("mistake", [dict(truncate=True), dict(drop_tap=0), dict(drop_tap=8), dict(roll_groups=1)])
def test_mistakes_fail(cg, c, stride, mistake):
    x, w, b = inputs(cg, c)
    pads = (1, 1, 1, 1)
    ref, bound = gb.gconv_ref(x, w, b, stride, pads, "none")
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within(emulate(x, w, b, stride, pads, "none", **mistake), ref, bound, str(mistake))


@pytest.mark.parametrize("wrong", [(0, 2, 1, 1), (1, 1, 0, 2), (2, 0, 1, 1), (1, 1, 2, 0)])
def test_pad_off_by_one_fails(wrong):
    """The same output size, the window shifted by one row or column."""
    x, w, b = inputs(8, 24)
    ref, bound = gb.gconv_ref(x, w, b, 1, (1, 1, 1, 1), "none")
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within(emulate(x, w, b, 1, wrong, "none"), ref, bound, str(wrong))


def test_k_slots_follow_the_kernel():
    assert [gb.k_slots(cg) for cg in (4, 8, 16, 32)] == [64, 96, 160, 288]
    assert [32 * gconv_ksteps(cg) for cg in (4, 8, 16, 32)] == [64, 96, 160, 288]


@pytest.mark.parametrize("cg,c", [(4, 24), (8, 16), (16, 48), (32, 64)])
def test_packed_filter_is_the_mfma_b_operand(cg, c):
    """Element j of lane l of fragment (g, ks, nt) is B[k = 32 ks + 8 (l >> 4) +
    j][col = 16 nt + (l & 15)] of group g, K in (tap, channel) order; the K
    padding and the columns past Cg are zero, and nothing of another group is
    in a group's fragments."""
    w = rnd(3, 3, cg, c, seed=cg).to(BF)
    g, ks, nt = c // cg, gconv_ksteps(cg), 2 if cg == 32 else 1
    p = pack_grouped_filter(w.float(), cg)
    assert p.dtype == BF and p.numel() == g * ks * nt * 64 * 8
    p = p.float().reshape(g, ks, nt, 64, 8)
    wk = w.float().reshape(9 * cg, c)
    for gi in range(g):
        for s in range(ks):
            for t in range(nt):
                for lane in (0, 5, 17, 31, 47, 63):
                    for j in (0, 3, 7):
                        k, col = 32 * s + 8 * (lane >> 4) + j, 16 * t + (lane & 15)
                        want = wk[k, gi * cg + col].item() if k < 9 * cg and col < cg else 0.0
                        assert p[gi, s, t, lane, j].item() == want, (gi, s, t, lane, j)
    assert p.abs().sum().item() == pytest.approx(wk.abs().sum().item(), rel=1e-6)
