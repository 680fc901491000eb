"""Every HIP kernel family under an elementwise error bound (MI355X).

The references are fp64 on the CPU, the bounds come from kernel_bounds.py (each
derived from what the kernel computes; docs/numerics.md) and EVERY output
element is checked -- against |y - ref| <= bound, not a max-norm tolerance
taken from the largest output.  Shapes come from the tile (one full tile plus
a partial one in M, an N tail), not from the workload, so each case is small.

Set KERNEL_BOUNDS_REPORT=<path> to get the worst err / bound per kernel family
as JSON (the table in docs/numerics.md)."""
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
from kernel_bounds import BF, rnd  # noqa: E402
from rust_tensorflow_serving2_amd.ops import ACT, BGEMM, HALO_PERSIST, hip  # noqa: E402

DEV = torch.device("cuda:0")
ACTS = ["none", "relu", "gelu_tanh", "gelu_erf", "tanh"]
WORST = {}


def within(family, y, ref, bound, what):
    r = kb.assert_within(y, ref, bound, f"{family}: {what}")
    WORST[family] = max(WORST.get(family, 0.0), r)
    return r


def dev(t):
    return None if t is None else t.to(DEV)


IGEMM_CFGS = list(range(hip().num_configs()))
BGEMM_CFGS = list(BGEMM)
CGEMM_CFGS = [c for c in hip().cgemm_configs() if c not in BGEMM_CFGS]
HALO_CFGS = [c for c in hip().halo_configs() if c != HALO_PERSIST]


def family_of(cfg):
    if cfg in BGEMM_CFGS:
        return "bgemm"
    if cfg == HALO_PERSIST:
        return "halo_persist"
    if cfg in HALO_CFGS:
        return "halo"
    return "cgemm" if cfg in CGEMM_CFGS else "igemm"


# ------------------------------------------------------------------ linear
@functools.lru_cache(maxsize=None)
def gemm_case(m, n, k):
    x, w, b, r = kb.gemm_inputs(m, n, k)
    parts = {(hb, hr): kb.gemm_parts(x, w, b if hb else None, r if hr else None)
             for hb in (True, False) for hr in (True, False)}
    return (dev(x), dev(w), dev(b), dev(r)), parts


@pytest.mark.parametrize("cfg", IGEMM_CFGS + CGEMM_CFGS + BGEMM_CFGS)
def test_linear_within_bound(cfg):
    """Every tile config: K of one and three k-tiles, bias / residual on and
    off, both output types, all five activations (pre-activations of standard
    deviation ~2), split-K 1 and 3."""
    m, n = kb.tile_shape(*hip().config_tile(cfg))
    fam = family_of(cfg) + " linear"
    for k in (64, 192):
        (x, w, b, r), parts = gemm_case(m, n, k)
        for (hb, hr), (pre, mag) in parts.items():
            for act in ACTS:
                for out_f32 in (False, True):
                    for splits in (1, 3):
                        y = hip().linear(x, w, b if hb else None, r if hr else None, ACT[act], cfg, out_f32,
                                         splits=splits)
                        ref, bound = kb.epilogue(pre, mag, k, splits, act, out_f32)
                        within(fam + (" f32" if out_f32 else ""), y, ref, bound,
                               f"cfg {cfg} k={k} bias={hb} res={hr} {act} splits={splits}")


@pytest.mark.parametrize("cfg", [3, 12, 36, 72, 100, 112, 140])
def test_linear_deep_k_within_bound(cfg):
    m, n = kb.tile_shape(*hip().config_tile(cfg))
    k = 2048
    (x, w, b, r), parts = gemm_case(m, n, k)
    pre, mag = parts[(True, True)]
    for act, out_f32, splits in (("none", False, 1), ("gelu_tanh", False, 3), ("tanh", True, 1), ("relu", True, 3)):
        y = hip().linear(x, w, b, r, ACT[act], cfg, out_f32, splits=splits)
        ref, bound = kb.epilogue(pre, mag, k, splits, act, out_f32)
        within(family_of(cfg) + " linear" + (" f32" if out_f32 else ""), y, ref, bound, f"cfg {cfg} k=2048 {act}")


# ------------------------------------------------------------------ conv2d
def pack_w(w_hwio):
    kh, kw, cin, cout = w_hwio.shape
    k = kh * kw * cin
    kp = -(-k // 64) * 64
    w = w_hwio.permute(3, 0, 1, 2).reshape(cout, k)
    return torch.cat([w, torch.zeros(cout, kp - k)], 1).to(BF).contiguous().to(DEV)


@functools.lru_cache(maxsize=None)
def conv_case(case):
    n, h, w, cin, cout, k, s, pads = case
    x, wt, b, r = kb.conv_inputs(*case)
    parts = {hr: kb.conv_parts(x, wt, b, s, pads, r if hr else None) for hr in (True, False)}
    return (dev(x), pack_w(wt), dev(b), dev(r)), parts


# 3x3 on a 7 x 9 image (five images: more than one 256-row tile), N tail (Cout = 72)
CONV3 = [(5, 7, 9, c, 72, 3, s, p) for c in (64, 128) for s in (1, 2) for p in ((1, 1, 1, 1), (0, 2, 1, 0))]
CONV1 = [(5, 7, 9, 64, 72, 1, 2, (0, 0, 0, 0))]
CONV_C24 = [(1, 9, 9, 24, 40, 3, 2, (0, 1, 0, 1))]


def run_conv_cases(cfg, cases, splits_list=(1, 2, 3), residual=(True, False)):
    fam = family_of(cfg) + " conv"
    for case in cases:
        n, h, w, cin, cout, k, s, pads = case
        (x, wp, b, r), parts = conv_case(case)
        for hr in residual:
            pre, mag = parts[hr]
            for act in ("relu", "none"):
                for splits in splits_list:
                    y = hip().conv2d(x, wp, b, r if hr else None, k, k, s, s, *pads, act=ACT[act], cfg=cfg,
                                     splits=splits)
                    ref, bound = kb.epilogue(pre, mag, k * k * cin, splits, act, False)
                    within(fam, y, ref, bound, f"cfg {cfg} {case} res={hr} {act} splits={splits}")


@pytest.mark.parametrize("cfg", IGEMM_CFGS)
def test_conv_igemm_within_bound(cfg):
    run_conv_cases(cfg, CONV3 + CONV1 + CONV_C24)


@pytest.mark.parametrize("cfg", CGEMM_CFGS)
def test_conv_cgemm_within_bound(cfg):
    run_conv_cases(cfg, CONV3 + CONV1)


@pytest.mark.parametrize("cfg", HALO_CFGS)
def test_conv_halo_within_bound(cfg):
    run_conv_cases(cfg, [c for c in CONV3 if c[6] == 1])


def test_conv_halo_persist_within_bound():
    """Config 146: 64 -> 64 channels, no residual, no split-K."""
    cases = [(5, 7, 9, 64, 64, 3, 1, p) for p in ((1, 1, 1, 1), (0, 2, 1, 0))]
    run_conv_cases(HALO_PERSIST, cases, splits_list=(1,), residual=(False,))


@pytest.mark.parametrize("cfg", CGEMM_CFGS + HALO_CFGS)
def test_conv_post_outputs_within_bound(cfg):
    """out2 = relu(v * scale + shift) beside the block sum, and post_only."""
    for case in (CONV3[0], CONV3[5] if cfg in CGEMM_CFGS else CONV3[1]):
        n, h, w, cin, cout, k, s, pads = case
        (x, wp, b, r), parts = conv_case(case)
        pre, mag = parts[True]
        sc, sh = rnd(cout, seed=35) * 0.5 + 1.0, rnd(cout, seed=36) * 0.2
        for splits in (1, 2):
            ref, bound = kb.epilogue(pre, mag, k * k * cin, splits, "none", False)
            ref2, bound2 = kb.post_output(pre, mag, k * k * cin, splits, sc, sh, "relu")
            out2 = torch.empty(ref.shape, device=DEV, dtype=BF)
            kw = dict(act=0, cfg=cfg, splits=splits, post_scale=dev(sc), post_shift=dev(sh), post_act=ACT["relu"])
            y = hip().conv2d(x, wp, b, r, k, k, s, s, *pads, out2=out2, **kw)
            within("conv post output", y, ref, bound, f"cfg {cfg} {case} splits={splits} (first output)")
            within("conv post output", out2, ref2, bound2, f"cfg {cfg} {case} splits={splits} out2")
            only = hip().conv2d(x, wp, b, r, k, k, s, s, *pads, post_only=True, **kw)
            within("conv post output", only, ref2, bound2, f"cfg {cfg} {case} splits={splits} post_only")


@pytest.mark.parametrize("cfg", CGEMM_CFGS)
@pytest.mark.parametrize("n,ho,c1,h,c2,s,cout", [(1, 5, 64, 9, 128, 2, 72), (2, 7, 128, 7, 64, 1, 136)])
def test_conv2d_dual_within_bound(n, ho, c1, h, c2, s, cout, cfg):
    hh = rnd(n, ho, ho, c1, seed=21).to(BF)
    x = rnd(n, h, h, c2, seed=22).to(BF)
    w1 = rnd(cout, c1, scale=1 / math.sqrt(c1), seed=23).to(BF)
    w2 = rnd(cout, c2, scale=1 / math.sqrt(c2), seed=24).to(BF)
    b = rnd(cout, scale=0.3, seed=25)
    a = torch.cat([hh, x[:, ::s, ::s, :]], -1).reshape(-1, c1 + c2)
    w = torch.cat([w1, w2], 1).contiguous()
    pre, mag = kb.gemm_parts(a, w, b)
    for act in ("relu", "none"):
        for splits in (1, 2):
            y = hip().conv2d_dual(dev(hh), dev(x), dev(w), dev(b), s, s, ACT[act], cfg, None, splits)
            ref, bound = kb.epilogue(pre, mag, c1 + c2, splits, act, False)
            within("conv2d_dual", y.reshape(-1, cout), ref, bound, f"cfg {cfg} {act} splits={splits}")
    # the post-activation output beside the sum
    sc, sh = rnd(cout, seed=46) * 0.5 + 1.0, rnd(cout, seed=47) * 0.2
    out2 = torch.empty(n, ho, ho, cout, device=DEV, dtype=BF)
    y = hip().conv2d_dual(dev(hh), dev(x), dev(w), dev(b), s, s, 0, cfg, None, 1, post_scale=dev(sc),
                          post_shift=dev(sh), post_act=ACT["relu"], out2=out2)
    ref, bound = kb.epilogue(pre, mag, c1 + c2, 1, "none", False)
    ref2, bound2 = kb.post_output(pre, mag, c1 + c2, 1, sc, sh, "relu")
    within("conv2d_dual", y.reshape(-1, cout), ref, bound, f"cfg {cfg} with out2")
    within("conv post output", out2.reshape(-1, cout), ref2, bound2, f"dual cfg {cfg} out2")


# ------------------------------------------------------------------ conv_chain, stem_pool
@pytest.mark.parametrize("k1,n1,n2", [(64, 256, 64), (64, 256, 128), (128, 512, 128), (128, 512, 256)])
@pytest.mark.parametrize("m", [77, 200])
def test_conv_chain_two_step_within_bound(k1, n1, n2, m):
    """y1 under the single-GEMM bound; y2 against the reference computed from
    the kernel's own bf16 y1, so stage 2 is checked as tightly as one GEMM."""
    assert hip().conv_chain_supported(k1, n1, n2)
    x = rnd(m, k1, seed=61).to(BF)
    w1 = rnd(n1, k1, scale=1 / math.sqrt(k1), seed=62).to(BF)
    b1 = rnd(n1, scale=0.3, seed=63)
    res = rnd(m, n1, seed=64).to(BF)
    w2 = rnd(n2, n1, scale=1 / math.sqrt(n1), seed=65).to(BF)
    b2 = rnd(n2, scale=0.3, seed=66)
    for with_res, act1, act2 in ((True, "relu", "relu"), (False, "none", "relu"), (True, "relu", "none")):
        r = res if with_res else None
        y1, y2 = hip().conv_chain(dev(x.reshape(1, 1, m, k1)), dev(w1), dev(b1),
                                  None if r is None else dev(r.reshape(1, 1, m, n1)), ACT[act1], dev(w2), dev(b2),
                                  ACT[act2])
        ref1, bound1 = kb.epilogue(*kb.gemm_parts(x, w1, b1, r), k1, 1, act1)
        within("conv_chain y1", y1.reshape(m, n1), ref1, bound1, f"{act1} res={with_res}")
        ref2, bound2 = kb.epilogue(*kb.gemm_parts(y1.reshape(m, n1).cpu(), w2, b2), n1, 1, act2)
        within("conv_chain y2", y2.reshape(m, n2), ref2, bound2, f"{act2} res={with_res}")


@pytest.mark.parametrize("n,h,w,c", [(1, 33, 35, 3), (1, 17, 19, 1)])
@pytest.mark.parametrize("post", [False, True])
def test_stem_pool_within_bound(n, h, w, c, post):
    """conv 7x7/2 (+bias, ReLU) -> max pool 3x3/2 (-> affine + ReLU).  The
    conv value is rounded to bf16 before the pool; rounding is monotone, so the
    pooled value is the rounded maximum: its error is the largest accumulation
    error in the window, then one rounding.  The affine reads that rounded
    value, whose error it scales by |scale|."""
    cout = 64
    x = torch.rand(n, h, w, c, generator=torch.Generator().manual_seed(h * w)) * 2 - 0.5
    wt = rnd(cout, 7, 7, c, scale=0.05, seed=cout + c)
    w4 = torch.zeros(cout, 8, 8, 4)
    w4[:, :7, :7, :c] = wt
    wk = w4.reshape(cout, 256).to(BF)
    b = rnd(cout, scale=0.1, seed=7)
    sc, sh = rnd(cout, seed=8) * 0.5, rnd(cout, seed=9) * 0.2
    kw = dict(post_scale=dev(sc), post_shift=dev(sh), post_act=ACT["relu"]) if post else {}
    whwio = wk.float().reshape(cout, 8, 8, 4)[:, :7, :7, :c].permute(1, 2, 3, 0)
    pre, mag = kb.conv_parts(x.to(BF), whwio, b, 2, (3, 3, 3, 3))
    conv = torch.relu(pre)
    acc = kb.acc_bound(pre, mag, 256, 1, "relu")

    def pool(t):
        return kb.maxpool_ref(t, 3, 3, 2, 2, 1, 1, 1, 1)
    refp, accp = pool(conv), pool(acc)
    if post:
        dp = kb.out_bound(refp, accp, False)
        pre2 = refp * sc.double() + sh.double()
        ref = torch.relu(pre2)
        bound = kb.out_bound(ref, dp * sc.double().abs() + 2 * kb.E * ((refp * sc.double()).abs() + sh.double().abs()),
                             False)
    else:
        ref, bound = refp, kb.out_bound(refp, accp, False)
    ys = []
    for xin in (x, x.to(BF)):
        y = hip().stem_pool(dev(xin), dev(wk), dev(b), 3, 3, 3, 3, ACT["relu"], 1, 1, 1, 1, **kw)
        within("stem_pool", y, ref, bound, f"{(n, h, w, c)} post={post} input {xin.dtype}")
        ys.append(y)
    assert torch.equal(ys[0], ys[1])


# ------------------------------------------------------------------ LayerNorm family
@pytest.mark.parametrize("cols", [64, 128, 520, 768, 2048, 4104])
def test_layernorm_within_bound(cols):
    x = (rnd(37, cols, seed=41) * 3 + 5).to(BF)          # offset mean: the two-pass variance matters
    r = rnd(37, cols, seed=42).to(BF)
    gm, bt = rnd(cols, seed=43), rnd(cols, seed=44)
    for res in (r, None):
        y = hip().layernorm(dev(x), dev(res), dev(gm), dev(bt), 1e-5)
        z = x.double() + (res.double() if res is not None else 0)
        ref, bound = kb.layernorm_ref(z, gm, bt, 1e-5)
        within("layernorm", y, ref, bound, f"cols={cols} res={res is not None}")


@pytest.mark.parametrize("hd", [64, 520, 768])
def test_embed_ln_within_bound(hd):
    S = 16
    ids = torch.randint(0, 50, (2 * S,), dtype=torch.int32, generator=torch.Generator().manual_seed(hd))
    ids[3], ids[7] = -1, 50
    tt = torch.randint(0, 3, (2 * S,), dtype=torch.int32, generator=torch.Generator().manual_seed(hd + 1))
    tt[5] = 9
    word, typ, pos = rnd(50, hd, seed=31).to(BF), rnd(3, hd, seed=32).to(BF), rnd(S, hd, seed=33).to(BF)
    gm, bt = rnd(hd, seed=34), rnd(hd, seed=35)
    e = hip().embed_ln(dev(ids), dev(tt), dev(word), dev(pos), dev(typ), dev(gm), dev(bt), 1e-6, S)
    ref, bound = kb.layernorm_ref(kb.embed_sum(ids, tt, word, pos, typ, S), gm, bt, 1e-6)
    within("embed_ln", e, ref, bound, f"hd={hd}")
    e2 = hip().embed_ln(dev(ids), None, dev(word), None, None, dev(gm), dev(bt), 1e-6, S)
    z2 = kb.embed_sum(ids, None, word, None, None, S)
    keep = z2.abs().sum(-1) > 0                      # (an all-zero row has zero variance: eps decides, not checked here)
    ref2, bound2 = kb.layernorm_ref(z2[keep], gm, bt, 1e-6)
    within("embed_ln", e2[keep.to(DEV)], ref2, bound2, f"hd={hd} word only")


@pytest.mark.parametrize("m,n,k", [(33, 512, 1024), (100, 768, 768)])
@pytest.mark.parametrize("bm", [16, 32])
def test_linear_ln_within_bound(m, n, k, bm):
    """GEMM + bias + residual + LayerNorm in one launch: the GEMM's fp32
    accumulation error enters the LayerNorm as dz."""
    from rust_tensorflow_serving2_amd.graph.fused import ln_weight_frags
    assert hip().linear_ln_supported(m, n, k, bm)
    x = rnd(m, k, seed=61).to(BF)
    w = (rnd(n, k, seed=62) / math.sqrt(k)).to(BF)
    b = rnd(n, seed=63)
    r = (rnd(m, n, seed=64) * 2 + 3).to(BF)
    gm, bt = rnd(n, seed=65), rnd(n, seed=66)
    for bias, res in ((b, r), (None, None)):
        y = hip().linear_ln(dev(x), dev(ln_weight_frags(w)), dev(bias), dev(res), dev(gm), dev(bt), 1e-12, bm)
        pre, mag = kb.gemm_parts(x, w, bias, res)
        ref, bound = kb.layernorm_ref(pre, gm, bt, 1e-12, dz=(k + 5) * kb.E * mag)
        within("linear_ln", y, ref, bound, f"{(m, n, k)} bm={bm} bias/res={bias is not None}")


# Deferred LayerNorm (hip().linear_lnx): GEMMs whose A rows / residual rows are
# pre-LayerNorm sums that arrive with (sum, sum sq) partials.
LNX_CFGS = [36, 47, 100, 72, 123, 38, 114, 37, 44, 45]


@pytest.mark.parametrize("cfg", LNX_CFGS)
@pytest.mark.parametrize("m,n,k", [(77, 256, 128), (130, 512, 64)])
def test_linear_lnx_residual_side_within_bound(m, n, k, cfg):
    x = rnd(m, k, seed=61).to(BF)
    w = rnd(n, k, scale=1 / math.sqrt(k), seed=62).to(BF)
    b = rnd(n, scale=0.1, seed=63)
    zr = (rnd(m, n, seed=64) * 2 + 0.5).to(BF)               # the residual before its LayerNorm
    g, bt = 1 + rnd(n, scale=0.1, seed=65), rnd(n, scale=0.1, seed=66)
    for parts in (1, 3):
        y, st = hip().linear_lnx(dev(x), dev(w), dev(b), dev(zr), 0, cfg, r_st=dev(kb.row_partials(zr, parts)),
                                 r_gamma=dev(g), r_beta=dev(bt), r_eps=1e-12, stats=True)
        ref, bound = kb.lnx_ref(x, w, b, "none", zr=zr, r_parts=parts, r_gamma=g, r_beta=bt, r_eps=1e-12)
        within("linear_lnx residual side", y, ref, bound, f"cfg {cfg} {(m, n, k)} parts={parts}")
        # the emitted partials are the stored rows' sums
        assert st.shape[0] == m and st.shape[2] == 2
        sums, sbound = kb.stats_bound(y, st.shape[1])
        within("linear_lnx row statistics", st.double().sum(1), sums, sbound, f"cfg {cfg} {(m, n, k)}")


@pytest.mark.parametrize("cfg", LNX_CFGS)
@pytest.mark.parametrize("m,n,k", [(77, 256, 128), (130, 512, 64)])
def test_linear_lnx_input_side_within_bound(m, n, k, cfg):
    z = (rnd(m, k, seed=71) * 1.5 + 0.3).to(BF)                # A before its LayerNorm
    W = rnd(k, n, scale=1 / math.sqrt(k), seed=72)
    b = rnd(n, scale=0.1, seed=73)
    g, bt = 1 + rnd(k, scale=0.1, seed=74), rnd(k, scale=0.1, seed=75)
    wf = (W * g[:, None]).t().contiguous().to(BF)              # gamma folded into the weights,
    bf = b + bt @ W                                            # beta into the bias
    colsum = wf.double().sum(1).float()
    for act in ("gelu_tanh", "none"):
        y, st = hip().linear_lnx(dev(z), dev(wf), dev(bf), None, ACT[act], cfg, a_st=dev(kb.row_partials(z, 2)),
                                 a_colsum=dev(colsum), a_eps=1e-12)
        assert st.numel() == 0
        ref, bound = kb.lnx_ref(z, wf, bf, act, a_parts=2, a_eps=1e-12, colsum=colsum)
        within("linear_lnx input side", y, ref, bound, f"cfg {cfg} {(m, n, k)} {act}")


# ------------------------------------------------------------------ attention
def closed_first_block(b, s, fill):
    mask = torch.zeros(b, s)
    mask[:, :64] = fill
    return mask


def check_attention(s, b, h, plds):
    scale = 1 / 8
    qkv = rnd(b, s, 3 * h * 64, seed=21 + s).to(BF)
    key = torch.zeros(b, s)
    key[b - 1, s // 2:] = -10000.0
    full = torch.triu(torch.full((s, s), -10000.0), 1).expand(b, 1, s, s).contiguous()
    masks = [("none", None, 0, 0), ("key", key, s, 0), ("full", full, s * s, s)]
    if s > 64:
        for name, fill in (("-10000", -10000.0), ("-inf", float("-inf")), ("f32 min", torch.finfo(torch.float32).min)):
            masks.append((f"first 64 keys {name}", closed_first_block(b, s, fill), s, 0))
    prev = hip().set_attention_plds(plds)
    try:
        for name, mask, bstride, qstride in masks:
            y = hip().attention(dev(qkv), dev(mask), h, scale, None, bstride, qstride)
            ref, bound = kb.attention_ref(qkv, h, scale, mask)
            assert torch.isfinite(y).all(), f"S={s} {name}: non-finite output"
            within("attention", y, ref, bound, f"S={s} b={b} h={h} plds={plds} mask {name}")
    finally:
        hip().set_attention_plds(prev)


# P in registers (0) at every S; P through LDS (1) is a layout of the fixed-S kernels only
ATTN_CASES = [(s, plds) for s in (1, 16, 33, 64, 100, 128, 192, 256, 320) for plds in (0, 1)
              if not plds or s in (64, 128, 192, 256)]


@pytest.mark.parametrize("s,plds", ATTN_CASES)
@pytest.mark.parametrize("b,h", [(1, 1), (2, 3)])
def test_attention_within_bound(s, plds, b, h):
    check_attention(s, b, h, plds)


def test_attention_one_workgroup_per_head_within_bound():
    check_attention(128, 22, 12, 0)


# ------------------------------------------------------------------ pools, heads, softmax
@pytest.mark.parametrize("n,hw,c", [(3, 1, 72), (2, 9, 520), (1, 49, 4096)])
def test_global_avgpool_within_bound(n, hw, c):
    g = rnd(n, hw, 1, c, seed=hw + c).to(BF)
    ref, bound, _ = kb.gap_ref(g)
    within("global_avgpool", hip().global_avgpool(dev(g)), ref, bound, f"{(n, hw, c)}")


@pytest.mark.parametrize("m,hw,k,np_,n,seed", kb.HEAD_CASES)
@pytest.mark.parametrize("fused", ["0", "16"])
def test_classifier_head_within_bound(monkeypatch, fused, m, hw, k, np_, n, seed):
    """Three launches (TFSERVE_HEAD_FUSED=0) and the one-launch small-batch head."""
    monkeypatch.setenv("TFSERVE_HEAD_FUSED", fused)
    x, w, b = kb.head_inputs(m, hw, k, np_, seed)
    probs, cls = hip().classifier_head(dev(x), dev(w), dev(b), n)
    p, bound, logits, dlogit = kb.head_ref(x, w, b, n)
    within("classifier_head", probs, p, bound, f"{(m, hw, k, np_, n)} fused={fused}")
    assert kb.argmax_checked(cls, logits, dlogit) == 1.0


@pytest.mark.parametrize("fused", ["0", "16"])
def test_classifier_head_nan_row_class_in_range(monkeypatch, fused):
    """A NaN activation makes its row's logits NaN: the class must still lie
    in [0, n), and the other rows are untouched."""
    monkeypatch.setenv("TFSERVE_HEAD_FUSED", fused)
    m, hw, k, np_, n, seed = kb.HEAD_CASES[0]
    x, w, b = kb.head_inputs(m, hw, k, np_, seed)
    want_p, want_c = hip().classifier_head(dev(x), dev(w), dev(b), n)
    x[1, 0, 0, 5] = float("nan")
    probs, cls = hip().classifier_head(dev(x), dev(w), dev(b), n)
    assert cls[1].item() == 0 and torch.isnan(probs[1]).all()
    keep = [0, 2]
    assert torch.equal(probs[keep], want_p[keep]) and torch.equal(cls[keep], want_c[keep])


@pytest.mark.parametrize("b,n,k", [(32, 2, 768), (5, 3, 1024), (1, 16, 64)])
def test_dense_softmax_within_bound(b, n, k):
    x = rnd(b, k, seed=31)
    w = rnd(n + 3, k, scale=1 / math.sqrt(k), seed=32).to(BF)
    bias = rnd(n + 3, scale=0.5, seed=33)
    p, bound = kb.dense_softmax_ref(x, w, bias, n)
    within("dense_softmax", hip().dense_softmax(dev(x), dev(w), dev(bias), n), p, bound, f"{(b, n, k)}")


# seeds at which no row's top two logits tie after bf16 rounding (argmax_checked compares every row)
SOFTMAX_CASES = [(2, 10, 1), (3, 1001, 1), (1, 4096, 1), (2, 5000, 1)]


def softmax_logits(rows, cols, seed, bf16):
    lg = rnd(rows, cols, scale=4, seed=seed * 1000 + rows + cols)
    return lg.to(BF) if bf16 else lg


@pytest.mark.parametrize("rows,cols,seed", SOFTMAX_CASES)
@pytest.mark.parametrize("bf16", [False, True])
def test_softmax_argmax_within_bound(rows, cols, seed, bf16):
    lg = softmax_logits(rows, cols, seed, bf16)
    ref, bound = kb.softmax_ref(lg)
    p, c = hip().softmax_argmax(dev(lg))
    within("softmax_argmax", p, ref, bound, f"{(rows, cols)} bf16={bf16}")
    assert kb.argmax_checked(c, lg, 0.0) == 1.0
    # one output only, and caller-provided outputs
    p1, c1 = hip().softmax_argmax(dev(lg), want_classes=False)
    assert c1 is None and torch.equal(p1, p)
    p2, c2 = hip().softmax_argmax(dev(lg), want_probs=False)
    assert p2 is None and torch.equal(c2, c)
    po = torch.full((rows, cols), -1.0, device=DEV)
    co = torch.full((rows,), -1, device=DEV, dtype=torch.long)
    p3, c3 = hip().softmax_argmax(dev(lg), True, True, po, co)
    assert p3.data_ptr() == po.data_ptr() and c3.data_ptr() == co.data_ptr()
    assert torch.equal(po, p) and torch.equal(co, c)
    # a row-strided view whose padding columns must never be read
    ld = -(-cols // 8) * 8 + 8
    full = torch.full((rows, ld), 1e4, dtype=lg.dtype)
    full[:, :cols] = lg
    p4, c4 = hip().softmax_argmax(dev(full)[:, :cols])
    assert torch.equal(p4, p) and torch.equal(c4, c)


@pytest.mark.parametrize("cols", [10, 1001, 5000])
@pytest.mark.parametrize("bf16", [False, True])
def test_softmax_argmax_non_finite_rows(cols, bf16):
    lg = rnd(4, cols, scale=4, seed=cols)
    lg[1, cols // 3] = float("inf")
    big = 3e38
    lg[2] = torch.where(rnd(cols, seed=cols + 1) > 0, big, -big)
    lg[2, 0] = -big
    lg[3] = float("nan")
    if bf16:
        lg = lg.to(BF)
    p, c = hip().softmax_argmax(dev(lg))
    c = c.cpu()
    ref, bound = kb.softmax_ref(lg[[0, 2]])
    within("softmax_argmax", p[[0, 2]], ref, bound, f"cols={cols} finite rows")
    assert c[0] == lg[0].double().argmax() and c[2] == int((lg[2].double() > 0).nonzero()[0])
    assert c[1] == cols // 3                               # the +inf logit wins
    assert torch.isnan(p[1]).all()                         # exp(inf - inf): NaN, as torch.softmax gives
    assert 0 <= c[3] < cols and c[3] == 0                  # an all-NaN row: class 0, never out of range
    only_c = hip().softmax_argmax(dev(lg), want_probs=False)[1].cpu()
    assert torch.equal(only_c, c)


# ------------------------------------------------------------------ exact (bitwise) cases
def cast_values(numel, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(numel, generator=g) * torch.exp(torch.randn(numel, generator=g) * 8)
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), 1e-40, -1e-40, 2 ** -133.0, 1.17549435e-38,
                            3.3895314e38, -3.3895314e38, 1.00390625, 1.01171875, 1.0 + 2 ** -8, 65504.0])
    x[:min(numel, special.numel())] = special[:numel]
    return x


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


@pytest.mark.parametrize("shape", [(1,), (7,), (8,), (9,), (3, 37), (1031,), (2, 3, 5, 7), (70001,)])
def test_cast_bf16_bit_exact(shape):
    numel = math.prod(shape)
    x = cast_values(numel, numel).reshape(shape)
    want = bits(x.to(BF))
    assert torch.equal(bits(hip().cast_bf16(dev(x))), want)
    out = torch.zeros(shape, device=DEV, dtype=BF)
    assert hip().cast_bf16(dev(x), out).data_ptr() == out.data_ptr() and torch.equal(bits(out), want)
    host = x.clone().pin_memory()
    out2 = torch.zeros(shape, device=DEV, dtype=BF)
    hip().cast_bf16_from_host(host, out2)
    torch.cuda.synchronize()
    assert torch.equal(bits(out2), want)


@pytest.mark.parametrize("n,h,w,c", [(1, 1, 1, 1), (1, 3, 3, 3), (2, 5, 7, 4), (3, 37, 29, 3), (1, 33, 31, 2)])
def test_ingest_c4_from_host_bit_exact(n, h, w, c):
    x = cast_values(n * h * w * c, h * w + c).reshape(n, h, w, c)
    want = torch.zeros(n, h, w, 4, dtype=BF)
    want[..., :c] = x.to(BF)
    y = hip().ingest_c4(dev(x))
    assert torch.equal(bits(y), bits(want))
    out = torch.full((n, h, w, 4), 7.0, device=DEV, dtype=BF)
    hip().ingest_c4_from_host(x.clone().pin_memory(), out)
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(want))


@pytest.mark.parametrize("c", [8, 520])
def test_maxpool_asymmetric_window_bit_exact(c):
    """kh != kw, sh != sw, all four pads different (a window of padding only
    included: its maximum is -inf)."""
    x = rnd(2, 9, 13, c, seed=c).to(BF)
    y = hip().maxpool(dev(x), 3, 2, 2, 1, 0, 1, 2, 0)
    ref = kb.maxpool_ref(x, 3, 2, 2, 1, 0, 1, 2, 0)
    assert y.shape == ref.shape and torch.equal(y.double().cpu(), ref)
    x2 = rnd(3, 10, 6, c, seed=c + 1).to(BF)
    y2 = hip().maxpool(dev(x2), 2, 3, 1, 2, 1, 0, 0, 2)
    assert torch.equal(y2.double().cpu(), kb.maxpool_ref(x2, 2, 3, 1, 2, 1, 0, 0, 2))


def test_zz_report_worst_ratios():
    """Not a check: writes the worst err / bound per family when asked to."""
    path = os.environ.get("KERNEL_BOUNDS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(dict(sorted(WORST.items())), f, indent=1)
    assert all(v <= 1.0 for v in WORST.values())
