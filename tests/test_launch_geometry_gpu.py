"""The HIP kernels under the elementwise bounds at many-tile launch geometries (MI355X).

test_kernel_bounds_gpu.py checks that one tile computes the right value: its
convs have 2 to 5 M-tiles, its GEMMs one.  This module runs the code that only
a launch of many tiles reaches -- the persistent halo kernel's walk over
several tiles per workgroup, the XCD-aware tile remap at tile counts that are
no multiple of 8, interior halo tiles with no masked tap, more than two
N-tiles, K loops much longer than the LDS ring, the in-kernel split-K fixup
over hundreds of tiles, attention with more workgroups than CUs -- against the
same fp64 references and bounds (kernel_bounds.py, unchanged; no tolerance of
its own).  Worst err / bound per family goes to KERNEL_BOUNDS_REPORT with the
other module's families.

Shapes
------
* conv: 3x3 on (11, 24, 24, 64), M = 6336 rows = 99 tiles of 64 rows
  (8*12 + 3), 49.5 -> 50 of 128 (8*6 + 2), 24.75 -> 25 of 256 (8*3 + 1); no BM
  makes all three a multiple of 8, so no further image count is needed
  (test_tile_counts_are_no_multiple_of_8 asserts it per config).  Cout = 72
  (an N tail on the second tile) and 200 (four N-tiles of 64 with a tail).
  Stride 2 on (11, 47, 47, 64) gives the same M; pads (0, 2, 1, 0) give
  M = 6072 (95 / 48 / 24 tiles).  The halo family splits 64-channel chunks, so
  its split-K case has 128 input channels.
* linear: M = 6341 (a 5-row tail), N = 200, K = 2880.  The deepest LDS ring of
  any GEMM config is 5 slots (kernels/tile_configs.h: cgemm config id 75,
  launch_cfg<128, 96, 4, 2, 5>; the igemm stages peak at 4, bgemm.hip
  ping-pongs two), and the deepest k-tile is 256 (igemm config 13).
  2880 = 45 k-tiles of 64 = 22.5 of 128 = 11.25 of 256: more than 2 * 5
  k-tiles for every config, with a partial k-tile for the deep ones.
* conv2d_dual / conv_chain: M = 13 * 22 * 22 = 6292 (98.3 tiles of 64) and
  M = 6341.
* persistent halo (config 146): image counts found with the launcher's own
  tile rule (hip().halo_persist_tiles) so that tiles == CUs, CUs + 1 and a
  count in (2 CUs, 3 CUs) that is no multiple of 8.

Unwritten output cannot look right: every output the test can hand to a
binding is prefilled with NaN, and every output a binding allocates itself
comes from a block this module has just filled with NaN and freed (the call
fails if the output's address is not one of those blocks)."""
import functools
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import kernel_bounds as kb  # noqa: E402
import test_kernel_bounds_gpu as base  # noqa: E402  (config lists, pack_w and the report's WORST table)
from kernel_bounds import BF, rnd  # noqa: E402
from rust_tensorflow_serving2_amd.ops import ACT, hip  # noqa: E402

DEV = base.DEV
dev, within, family_of, pack_w = base.dev, base.within, base.family_of, base.pack_w
IGEMM_CFGS, CGEMM_CFGS, BGEMM_CFGS, HALO_CFGS = base.IGEMM_CFGS, base.CGEMM_CFGS, base.BGEMM_CFGS, base.HALO_CFGS
CUS = torch.cuda.get_device_properties(0).multi_processor_count
NAN = float("nan")
POISONED_SIZES = set()          # (numel, dtype) of every block poisoned for a binding's own allocation


# ------------------------------------------------------------------ unwritten output must fail
def nan_out(shape, dtype=BF):
    """A caller-provided output, NaN everywhere."""
    return torch.full(tuple(shape), NAN, device=DEV, dtype=dtype)


def poison(*specs):
    """Allocate one block per (numel, dtype), in the order the binding will
    allocate, fill them with NaN and free them: the caching allocator is back
    in the state it was in, so the binding's own requests replay these and get
    the same blocks.  Returns their addresses (assert_poisoned checks them)."""
    held = [torch.full((numel,), NAN, device=DEV, dtype=dtype) for numel, dtype in specs]
    ptrs = {t.data_ptr() for t in held}
    POISONED_SIZES.update(specs)
    del held
    return ptrs


def assert_poisoned(ptrs, *outs):
    for o in outs:
        assert o.data_ptr() in ptrs, (f"the output of {tuple(o.shape)} {o.dtype} did not come from a poisoned block: "
                                      "an unwritten element could hold a stale, correct value")


def poison_workspace(m, n, splits):
    """The split-K slabs run_igemm allocates (fp32 [splits][M][N])."""
    if splits > 1:
        poison((splits * m * n, torch.float32))


def test_assert_within_counts_nan_as_violation():
    ref = torch.ones(4, 8, dtype=torch.float64)
    y = ref.clone()
    y[2, 5] = NAN
    with pytest.raises(AssertionError, match=r"1 of 32 elements outside the bound.*\(2, 5\)"):
        kb.assert_within(y, ref, 1.0, "nan")
    with pytest.raises(AssertionError, match="32 of 32"):
        kb.assert_within(nan_out((4, 8)), ref, 1e30, "unwritten")


# ------------------------------------------------------------------ a. the persistent halo walk
# output sizes tried in order; the first image count whose tile count fits is taken
PERSIST_TARGETS = {
    # 16 x 16: two tiles per image
    "tiles == CUs": ([(16, 16), (11, 11)], lambda t: t == CUS),
    # 7 x 7: two images per tile (TI = 2), so the first fitting count is odd and the last tile holds one image;
    # exactly one workgroup walks two tiles
    "tiles == CUs + 1": ([(7, 7), (11, 11)], lambda t: t == CUS + 1),
    # 24 x 24: five blocks of 5 rows per image, the last one partial; some workgroups walk three tiles (the halo
    # buffer index returns to 0), the others two
    "2 CUs < tiles < 3 CUs": ([(24, 24), (11, 11)], lambda t: 2 * CUS < t < 3 * CUS and t % 8 != 0),
}
PERSIST_PADS = [(1, 1, 1, 1), (0, 2, 1, 0)]


@functools.lru_cache(maxsize=None)
def persist_shape(target):
    sizes, want = PERSIST_TARGETS[target]
    for ho, wo in sizes:
        for n in range(1, 3 * CUS + 2):
            tiles, th, tw, ti = hip().halo_persist_tiles(n, ho, wo)
            if want(tiles):
                return n, ho, wo, tiles, th, tw, ti
            if tiles >= 3 * CUS:
                break
    pytest.fail(f"no image count gives {target} on a device of {CUS} CUs")


def check_walk(target, tiles, n, ho, wo, th, tw, ti):
    """The case covers the walk it is named for, on this device."""
    assert PERSIST_TARGETS[target][1](tiles), (target, tiles, CUS)
    assert tiles == -(-n // ti) * -(-ho // th) * -(-wo // tw)
    walked = [len(range(wg, tiles, min(tiles, CUS))) for wg in range(min(tiles, CUS))]
    if target == "tiles == CUs":
        assert set(walked) == {1}
    elif target == "tiles == CUs + 1":
        assert sorted(walked)[-2:] == [1, 2]
        assert n % ti != 0 or ti * th * tw < 128                       # a partial last tile, or tiles of < 128 pixels
    else:
        assert set(walked) == {2, 3} and (ho % th != 0 or wo % tw != 0)   # partial last blocks


@functools.lru_cache(maxsize=None)
def persist_case(target, pads):
    n, ho, wo, *_ = persist_shape(target)
    h, w = ho + 2 - pads[0] - pads[1], wo + 2 - pads[2] - pads[3]
    x, wt, b, _r = kb.conv_inputs(n, h, w, 64, 64, 3, 1, pads, seed=len(target))
    pre, mag = kb.conv_parts(x, wt, b, 1, pads)
    assert pre.shape == (n, ho, wo, 64)
    return (dev(x), pack_w(wt), dev(b)), (pre, mag)


@pytest.mark.parametrize("pads", PERSIST_PADS)
@pytest.mark.parametrize("target", list(PERSIST_TARGETS))
def test_halo_persist_walk_within_bound(target, pads):
    n, ho, wo, tiles, th, tw, ti = persist_shape(target)
    check_walk(target, tiles, n, ho, wo, th, tw, ti)
    (x, wp, b), (pre, mag) = persist_case(target, pads)
    for act in ("relu", "none"):
        y = hip().conv2d(x, wp, b, None, 3, 3, 1, 1, *pads, act=ACT[act], cfg=146, out=nan_out(pre.shape))
        ref, bound = kb.epilogue(pre, mag, 576, 1, act, False)
        within("halo_persist walk", y, ref, bound,
               f"{target}: {tiles} tiles of {ti} x {th} x {tw} on {CUS} CUs, {n} x {ho} x {wo}, pads {pads}, {act}")


@pytest.mark.parametrize("pads", PERSIST_PADS)
def test_halo_persist_walk_exact_integers(pads):
    """The three-tile walk with integer operands: every sum is an integer of
    magnitude <= 256, exact in fp32 and in bf16, so a halo row shifted by one
    pixel, a tile computed from the other halo buffer or a staging row stored
    too late is a wrong integer, not a small error."""
    target = "2 CUs < tiles < 3 CUs"
    n, ho, wo, tiles, th, tw, ti = persist_shape(target)
    check_walk(target, tiles, n, ho, wo, th, tw, ti)
    h, w = ho + 2 - pads[0] - pads[1], wo + 2 - pads[2] - pads[3]
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-1, 2, (n, h, w, 64), generator=g).float()
    wt = torch.randint(-1, 2, (3, 3, 64, 64), generator=g).float()
    b = torch.randint(-2, 3, (64,), generator=g).float()
    xp = torch.nn.functional.pad(x.permute(0, 3, 1, 2), [pads[2], pads[3], pads[0], pads[1]])
    ref = torch.nn.functional.conv2d(xp, wt.permute(3, 2, 0, 1)).permute(0, 2, 3, 1) + b
    assert ref.abs().max() <= 256 and ref.shape == (n, ho, wo, 64)
    for act in ("none", "relu"):
        want = (torch.relu(ref) if act == "relu" else ref).contiguous()
        y = hip().conv2d(dev(x.to(BF)), pack_w(wt), dev(b), None, 3, 3, 1, 1, *pads, act=ACT[act], cfg=146,
                         out=nan_out(ref.shape))
        got = y.float().cpu()
        wrong = (got != want) | torch.isnan(got)
        assert not wrong.any(), (f"{act} pads {pads}: {int(wrong.sum())} wrong elements, the first at "
                                 f"{tuple(int(v) for v in wrong.nonzero()[0])} (n, h, w, c)")
        assert torch.equal(base.bits(y), base.bits(want.to(BF)))


# ------------------------------------------------------------------ b. tile remap and interior tiles
MAIN = (11, 24, 24, 64)
CONV_MAIN = [MAIN + (cout, 3, 1, (1, 1, 1, 1)) for cout in (72, 200)]
CONV_S2 = (11, 47, 47, 64, 72, 3, 2, (1, 1, 1, 1))
CONV_ASYM = (11, 24, 24, 64, 200, 3, 1, (0, 2, 1, 0))
CONV_C128 = (11, 24, 24, 128, 72, 3, 1, (1, 1, 1, 1))         # two 64-channel chunks: the halo family's split-K


def out_rows(case):
    n, h, w, _cin, _cout, k, s, pads = case
    return n * ((h + pads[0] + pads[1] - k) // s + 1) * ((w + pads[2] + pads[3] - k) // s + 1)


def run_conv(cfg, case, variants):
    """variants: (residual, act, splits, fixup); fixup None leaves the default rule."""
    n, h, w, cin, cout, k, s, pads = case
    (x, wp, b, r), parts = base.conv_case(case)
    fam = family_of(cfg) + " conv many tiles"
    prev = hip().get_splitk_fixup()
    try:
        for hr, act, splits, fixup in variants:
            pre, mag = parts[hr]
            hip().set_splitk_fixup(prev if fixup is None else fixup)
            out = nan_out(pre.shape)
            poison_workspace(pre.numel() // cout, cout, splits)          # (after `out`: the slabs are the next request)
            y = hip().conv2d(x, wp, b, r if hr else None, k, k, s, s, *pads, act=ACT[act], cfg=cfg, splits=splits,
                             out=out)
            ref, bound = kb.epilogue(pre, mag, k * k * cin, splits, act, False)
            within(fam, y, ref, bound, f"cfg {cfg} {case} res={hr} {act} splits={splits} fixup={fixup}")
    finally:
        hip().set_splitk_fixup(prev)


SPLIT_VARIANTS = [(True, "relu", 1, None), (False, "none", 1, None), (True, "none", 3, 1), (False, "relu", 3, 1),
                  (True, "relu", 3, 0), (False, "none", 3, 0)]


def test_conv_shapes_have_many_tiles_with_a_tail():
    assert [out_rows(c) for c in CONV_MAIN + [CONV_S2, CONV_ASYM, CONV_C128]] == [6336, 6336, 6336, 6072, 6336]
    assert [-(-6336 // bm) % 8 for bm in (64, 128, 256)] == [3, 2, 1]
    assert [-(-6072 // bm) % 8 for bm in (64, 128, 256)] == [7, 0, 0]


@pytest.mark.parametrize("cfg", IGEMM_CFGS + CGEMM_CFGS)
def test_tile_counts_are_no_multiple_of_8(cfg):
    """The remap's remainder path: every config sees a launch whose tile count
    is no multiple of 8 (the XCD count), and one with more than two N-tiles."""
    bm, bn = hip().config_tile(cfg)
    assert bm in (64, 128, 256)
    counts = [-(-out_rows(c) // bm) * -(-c[4] // bn) for c in CONV_MAIN + [CONV_S2, CONV_ASYM]]
    assert any(t % 8 for t in counts) and min(counts) > 8, counts
    assert 72 % bn and 200 % bn                                # an N tail on the last N-tile
    assert -(-200 // bn) > 2 or bn > 96                        # three or four N-tiles for the narrow tiles


@pytest.mark.parametrize("cfg", IGEMM_CFGS)
def test_conv_igemm_many_tiles_within_bound(cfg):
    plain = [v for v in SPLIT_VARIANTS if v[3] != 0]           # (igemm has no in-kernel fixup: one reduce path)
    for case in CONV_MAIN:
        run_conv(cfg, case, plain)
    for case in (CONV_S2, CONV_ASYM):
        run_conv(cfg, case, [(True, "relu", 1, None), (False, "none", 3, None)])


@pytest.mark.parametrize("cfg", CGEMM_CFGS)
def test_conv_cgemm_many_tiles_within_bound(cfg):
    for case in CONV_MAIN:
        run_conv(cfg, case, SPLIT_VARIANTS)
    for case in (CONV_S2, CONV_ASYM):
        run_conv(cfg, case, [(True, "relu", 1, None), (False, "none", 3, 1), (True, "none", 3, 0)])


@pytest.mark.parametrize("cfg", HALO_CFGS)
def test_conv_halo_many_tiles_within_bound(cfg):
    """Stride 1 only (the family's reach); 64 input channels are one chunk, so
    a split request runs unsplit there and the 128-channel case splits."""
    for case in CONV_MAIN + [CONV_ASYM]:
        run_conv(cfg, case, [(True, "relu", 1, None), (False, "none", 1, None)])
    run_conv(cfg, CONV_C128, [(True, "relu", 1, None), (False, "none", 2, 1), (True, "none", 2, 0)])


# ------------------------------------------------------------------ c. linear
LIN_M, LIN_N, LIN_K = 6336 + 5, 200, 2880


def test_linear_k_outruns_every_ring():
    deepest_ring, deepest_ktile = 5, 256          # cgemm.hip launch_mode case 27; igemm.hip kCfgBK (module docstring)
    assert LIN_K % 64 == 0 and LIN_K > 2 * deepest_ring * deepest_ktile and LIN_K % deepest_ktile and LIN_M % 16


@functools.lru_cache(maxsize=None)
def linear_case():
    x, w, b, r = kb.gemm_inputs(LIN_M, LIN_N, LIN_K)
    return (dev(x), dev(w), dev(b), dev(r)), kb.gemm_parts(x, w, b, r)


@pytest.mark.parametrize("cfg", IGEMM_CFGS + CGEMM_CFGS + BGEMM_CFGS)
def test_linear_many_tiles_deep_k_within_bound(cfg):
    (x, w, b, r), (pre, mag) = linear_case()
    fam = family_of(cfg) + " linear many tiles"
    for act, out_f32, splits in (("relu", False, 1), ("gelu_tanh", False, 3), ("none", True, 1), ("tanh", True, 3)):
        out = nan_out(pre.shape, torch.float32 if out_f32 else BF)
        poison_workspace(LIN_M, LIN_N, splits)
        y = hip().linear(x, w, b, r, ACT[act], cfg, out_f32, splits=splits, out=out)
        ref, bound = kb.epilogue(pre, mag, LIN_K, splits, act, out_f32)
        within(fam + (" f32" if out_f32 else ""), y, ref, bound, f"cfg {cfg} {act} splits={splits}")


# ------------------------------------------------------------------ d. conv2d_dual, conv_chain, the dual-source chain
DUAL_N, DUAL_HO, DUAL_C1, DUAL_C2, DUAL_COUT = 13, 22, 64, 128, 72     # M = 6292 = 98 tiles of 64 + 20 rows


@functools.lru_cache(maxsize=None)
def dual_case(s):
    h = (DUAL_HO - 1) * s + 1
    hh = rnd(DUAL_N, DUAL_HO, DUAL_HO, DUAL_C1, seed=21).to(BF)
    x = rnd(DUAL_N, h, h, DUAL_C2, seed=22).to(BF)
    w1 = rnd(DUAL_COUT, DUAL_C1, scale=1 / math.sqrt(DUAL_C1), seed=23).to(BF)
    w2 = rnd(DUAL_COUT, DUAL_C2, scale=1 / math.sqrt(DUAL_C2), seed=24).to(BF)
    b = rnd(DUAL_COUT, scale=0.3, seed=25)
    a = torch.cat([hh, x[:, ::s, ::s, :]], -1).reshape(-1, DUAL_C1 + DUAL_C2)
    w = torch.cat([w1, w2], 1).contiguous()
    return (dev(hh), dev(x), dev(w), dev(b)), kb.gemm_parts(a, w, b)


@pytest.mark.parametrize("cfg", CGEMM_CFGS)
@pytest.mark.parametrize("s", [1, 2])
def test_conv2d_dual_many_tiles_within_bound(s, cfg):
    (hh, x, w, b), (pre, mag) = dual_case(s)
    m = DUAL_N * DUAL_HO * DUAL_HO
    assert pre.shape == (m, DUAL_COUT) and m % 64
    for act, splits in (("relu", 1), ("none", 2)):
        out = nan_out((DUAL_N, DUAL_HO, DUAL_HO, DUAL_COUT))
        poison_workspace(m, DUAL_COUT, splits)
        y = hip().conv2d_dual(hh, x, w, b, s, s, ACT[act], cfg, out, splits)
        ref, bound = kb.epilogue(pre, mag, DUAL_C1 + DUAL_C2, splits, act, False)
        within("conv2d_dual many tiles", y.reshape(m, DUAL_COUT), ref, bound, f"cfg {cfg} s={s} {act} splits={splits}")


CHAIN_M = LIN_M
CHAIN_SHAPES = [(64, 256, 64, False), (64, 256, 128, False), (128, 512, 128, False), (128, 512, 256, False),
                (128, 256, 64, True)]


@functools.lru_cache(maxsize=None)
def chain_case(k1, n1, n2):
    m = CHAIN_M
    x = rnd(m, k1, seed=61).to(BF)
    w1 = rnd(n1, k1, scale=1 / math.sqrt(k1), seed=62).to(BF)
    b1 = rnd(n1, scale=0.3, seed=63)
    res = rnd(m, n1, seed=64).to(BF)
    w2 = rnd(n2, n1, scale=1 / math.sqrt(n1), seed=65).to(BF)
    b2 = rnd(n2, scale=0.3, seed=66)
    parts = {hr: kb.gemm_parts(x, w1, b1, res if hr else None) for hr in (True, False)}
    return (x, w1, b1, res, w2, b2), parts


@pytest.mark.parametrize("k1,n1,n2,dual", CHAIN_SHAPES)
def test_conv_chain_many_tiles_within_bound(k1, n1, n2, dual):
    """Every built instance (the dual-source one reads its rows from two
    tensors of k1 / 2 channels); y2 is referenced from the kernel's own y1."""
    assert hip().conv_chain_supported(k1, n1, n2, dual)
    m = CHAIN_M
    (x, w1, b1, res, w2, b2), parts = chain_case(k1, n1, n2)
    if dual:
        xa, xb = (dev(t.contiguous().reshape(1, 1, m, k1 // 2)) for t in (x[:, :k1 // 2], x[:, k1 // 2:]))
    else:
        xa, xb = dev(x.reshape(1, 1, m, k1)), None
    w1d, b1d, w2d, b2d, resd = dev(w1), dev(b1), dev(w2), dev(b2), dev(res.reshape(1, 1, m, n1))
    name = "conv_chain dual" if dual else "conv_chain"
    # (the dual-source form is the projecting block, whose shortcut is its second source: no residual)
    for hr, act1, act2 in ((not dual, "relu", "relu"), (False, "none", "relu")):
        ptrs = poison((m * n1, BF), (m * n2, BF))
        y1, y2 = hip().conv_chain(xa, w1d, b1d, resd if hr else None, ACT[act1], w2d, b2d, ACT[act2], x2=xb)
        assert_poisoned(ptrs, y1, y2)
        ref1, bound1 = kb.epilogue(*parts[hr], k1, 1, act1)
        within(name + " y1 many tiles", y1.reshape(m, n1), ref1, bound1, f"{(k1, n1, n2)} {act1} res={hr}")
        ref2, bound2 = kb.epilogue(*kb.gemm_parts(y1.reshape(m, n1).cpu(), w2, b2), n1, 1, act2)
        within(name + " y2 many tiles", y2.reshape(m, n2), ref2, bound2, f"{(k1, n1, n2)} {act2} res={hr}")


# ------------------------------------------------------------------ e. attention
@pytest.mark.parametrize("s", [64, 128])
def test_attention_more_workgroups_than_cus_within_bound(s):
    """batch x heads > 2 CUs, and an adder that closes a different key range in
    every batch row: a workgroup that reads another row's mask, or another
    (batch, head)'s keys, fails."""
    h = 12
    b = (2 * CUS) // h + 1
    assert b * h > 2 * CUS
    scale = 1 / 8
    qkv = rnd(b, s, 3 * h * 64, seed=21 + s).to(BF)
    key = torch.zeros(b, s)
    for i in range(b):
        lo = (5 * i) % (s // 2)
        key[i, lo:lo + s // 4 + i % 3] = -10000.0
    assert len({tuple(row.tolist()) for row in key}) == b       # no two batch rows share a mask
    for name, mask, bstride in (("none", None, 0), ("per-row key ranges", key, s)):
        y = hip().attention(dev(qkv), dev(mask), h, scale, nan_out((b, s, h * 64)), bstride, 0)
        ref, bound = kb.attention_ref(qkv, h, scale, mask)
        within("attention many workgroups", y, ref, bound, f"S={s} b={b} h={h} mask {name}")


# ------------------------------------------------------------------ f. the poisoning mechanism itself
def test_zy_poisoned_blocks_are_handed_back():
    """For every size this module poisoned for a binding's own allocation: the
    next torch.empty of that size gets a poisoned block, NaN throughout."""
    sizes = sorted(POISONED_SIZES | {(CHAIN_M * 256, BF), (CHAIN_M * 64, BF), (3 * LIN_M * LIN_N, torch.float32)},
                   key=str)
    for numel, dtype in sizes:
        ptrs = poison((numel, dtype))
        t = torch.empty((numel,), device=DEV, dtype=dtype)
        assert t.data_ptr() in ptrs, f"{numel} x {dtype}: the allocator did not reuse the poisoned block"
        assert torch.isnan(t).all(), f"{numel} x {dtype}: the reused block is not NaN throughout"
        del t


def test_zz_report_worst_ratios():
    """Not a check: writes the worst err / bound per family when asked to (the
    other module's families included when it ran in the same session)."""
    path = os.environ.get("KERNEL_BOUNDS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(sorted(base.WORST.items())), f, indent=1)
    assert all(v <= 1.0 for v in base.WORST.values())
