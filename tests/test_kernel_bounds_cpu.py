"""The bound checker (tests/kernel_bounds.py) tested on the CPU.

For every kernel family an *ideal* kernel is emulated in torch -- fp32 math,
the same bf16 roundings the HIP kernel makes -- and two things are asserted:

 (a) the ideal kernel is within the bound at every element, at the shapes the
     GPU module (test_kernel_bounds_gpu.py) uses;
 (b) each mutant (a subtly wrong kernel) is rejected.

So the bounds are neither so tight that a correct kernel fails nor so loose
that a wrong activation, a dropped bias / K tail, a shifted padding mask, a
truncating store, a 1 % softmax scale error or an unbiased variance passes."""
import math

import pytest
import torch
import torch.nn.functional as F

import kernel_bounds as kb
from kernel_bounds import BF, rnd


def bf_round(t):
    return t.to(BF).float()


def bf_trunc(t):
    """fp32 -> bf16 by dropping the low 16 bits (the wrong store)."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def rejected(y, ref, bound, what="mutant"):
    try:
        kb.assert_within(y, ref, bound, what)
    except AssertionError as e:
        assert "outside the bound" in str(e)
        return
    pytest.fail(f"the bound did not reject: {what}")


def act32(act, x):
    return kb.act64(act, x.float())


# ------------------------------------------------------------------ the checker itself
def test_assert_within_reports_and_returns_worst_ratio():
    ref = torch.tensor([[1.0, 2.0], [3.0, 4.0]], dtype=torch.float64)
    bound = torch.full((2, 2), 0.1, dtype=torch.float64)
    assert kb.assert_within(ref + 0.05, ref, bound, "ok") == pytest.approx(0.5)
    assert kb.assert_within(ref, ref, torch.zeros(2, 2), "exact") == 0.0
    y = ref.clone()
    y[1, 0] += 0.25
    with pytest.raises(AssertionError) as e:
        kb.assert_within(y, ref, bound, "probe")
    msg = str(e.value)
    assert "probe" in msg and "1 of 4" in msg and "2.500" in msg and "(1, 0)" in msg and "ref = 3" in msg
    y[0, 1] = float("nan")
    with pytest.raises(AssertionError, match="2 of 4"):
        kb.assert_within(y, ref, bound, "nan")
    with pytest.raises(AssertionError, match="shape"):
        kb.assert_within(ref[0], ref, bound, "shape")


# ------------------------------------------------------------------ GEMM epilogue
def ideal_gemm(x, w, b, r, act, out_f32, drop_k=0, drop_k_last_row=0, bias_cols=None, trunc=False):
    xf, wf = x.float().clone(), w.float()
    k = xf.shape[1]
    if drop_k:
        xf[:, k - drop_k:] = 0
    if drop_k_last_row:
        xf[-1, k - drop_k_last_row:] = 0
    pre = xf @ wf.t()
    if b is not None:
        bb = b.clone()
        if bias_cols is not None:
            bb[bias_cols:] = 0
        pre = pre + bb
    if r is not None:
        pre = pre + r.float()
    y = act32(act, pre)
    if out_f32:
        return y
    return bf_trunc(y) if trunc else bf_round(y)


# the issue's four shapes, then what tile_shape() gives the GPU module: tiles of 64 / 128 / 256 rows by
# 64 .. 256 columns, K in {64, 192, 2048}
GEMM_SHAPES = [(8, 72, 64), (33, 136, 576), (32, 1000, 2048), (40, 72, 3072),
               (88, 72, 64), (88, 72, 192), (88, 104, 192), (152, 136, 64), (152, 264, 192), (280, 152, 64),
               (280, 200, 192), (280, 264, 192), (152, 264, 2048), (280, 264, 2048)]
ACTS = ["none", "relu", "gelu_tanh", "gelu_erf", "tanh"]


@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_gemm_ideal_within_bound(m, n, k):
    x, w, b, r = kb.gemm_inputs(m, n, k)
    for bias, res in ((b, r), (b, None), (None, r), (None, None)):
        pre, mag = kb.gemm_parts(x, w, bias, res)
        for act in ACTS:
            for out_f32 in (False, True):
                for splits in (1, 3):
                    ref, bound = kb.epilogue(pre, mag, k, splits, act, out_f32)
                    ratio = kb.assert_within(ideal_gemm(x, w, bias, res, act, out_f32), ref, bound,
                                             f"{act} f32={out_f32}")
                    assert ratio <= 1.0


@pytest.mark.parametrize("m,n,k", GEMM_SHAPES[:4] + [(88, 72, 192), (152, 264, 2048)])
@pytest.mark.parametrize("act", ACTS)
def test_gemm_tail_and_store_mutants_rejected(m, n, k, act):
    x, w, b, r = kb.gemm_inputs(m, n, k)
    pre, mag = kb.gemm_parts(x, w, b, r)
    for out_f32 in (False, True):
        ref, bound = kb.epilogue(pre, mag, k, 3, act, out_f32)
        rejected(ideal_gemm(x, w, b, r, act, out_f32, bias_cols=n - 8), ref, bound, f"bias tail f32={out_f32}")
        rejected(ideal_gemm(x, w, b, r, act, out_f32, drop_k=32), ref, bound, f"K - 32 f32={out_f32}")
        rejected(ideal_gemm(x, w, b, r, act, out_f32, drop_k_last_row=8), ref, bound, f"last row K - 8 f32={out_f32}")
    if k <= 576:
        # a truncating store is off by up to 2^-7 |ref|: it shows where 2^-8 |ref|
        # exceeds the accumulation term, i.e. at shallow K
        ref, bound = kb.epilogue(pre, mag, k, 3, act, False)
        rejected(ideal_gemm(x, w, b, r, act, False, trunc=True), ref, bound, "truncating store")


@pytest.mark.parametrize("m,n,k", GEMM_SHAPES)
def test_relu_gelu_swap_rejected(m, n, k):
    x, w, b, r = kb.gemm_inputs(m, n, k)
    pre, mag = kb.gemm_parts(x, w, b, r)
    for out_f32 in (False, True):
        for want, got in (("relu", "gelu_tanh"), ("gelu_tanh", "relu"), ("relu", "gelu_erf"), ("gelu_erf", "relu"),
                          ("tanh", "none"), ("none", "relu")):
            ref, bound = kb.epilogue(pre, mag, k, 1, want, out_f32)
            rejected(ideal_gemm(x, w, b, r, got, out_f32), ref, bound)


@pytest.mark.parametrize("m,n", [(8, 72), (88, 72), (152, 136), (280, 264)])
def test_gelu_flavour_swap_rejected_at_k64(m, n):
    """tanh-GELU and erf-GELU differ by at most ~5e-4: only a shallow K keeps
    the worst-case accumulation term below that (the issue's K = 64)."""
    k = 64
    x, w, b, r = kb.gemm_inputs(m, n, k)
    pre, mag = kb.gemm_parts(x, w, b, r)
    for want, got in (("gelu_tanh", "gelu_erf"), ("gelu_erf", "gelu_tanh")):
        ref, bound = kb.epilogue(pre, mag, k, 1, want, True)
        rejected(ideal_gemm(x, w, b, r, got, True), ref, bound)
        kb.assert_within(ideal_gemm(x, w, b, r, want, True), ref, bound, want)


def test_activation_error_constants_cover_the_folded_forms():
    """common.h's sigm2 / folded gelu_tanh evaluated in fp32 with exact-ish
    exp / reciprocal stay inside act_abs (the constants are right, and the
    bound is not vacuous: a 1e-4 relative error in a folded constant fails)."""
    x = torch.linspace(-12, 12, 20001, dtype=torch.float32)
    xd = x.double()

    def gelu_folded(k0, k1):
        t = torch.addcmul(torch.tensor(k0, dtype=torch.float32), x * x, torch.tensor(k1, dtype=torch.float32))
        return x * (1.0 / (1.0 + torch.exp2(x * t)))
    tanh_folded = 2.0 * (1.0 / (1.0 + torch.exp(-2.0 * x))) - 1.0
    kb.assert_within(gelu_folded(-2.302208198144325, -0.1029432395800235), kb.act64("gelu_tanh", xd),
                     kb.act_abs("gelu_tanh", xd), "gelu_tanh folded")
    kb.assert_within(tanh_folded, torch.tanh(xd), kb.act_abs("tanh", xd), "tanh folded")
    kb.assert_within(F.gelu(x), kb.act64("gelu_erf", xd), kb.act_abs("gelu_erf", xd), "gelu_erf")
    rejected(gelu_folded(-2.302208198144325 * (1 + 1e-4), -0.1029432395800235), kb.act64("gelu_tanh", xd),
             kb.act_abs("gelu_tanh", xd))
    rejected(gelu_folded(-2.302208198144325, -0.1029432395800235 * (1 + 1e-3)), kb.act64("gelu_tanh", xd),
             kb.act_abs("gelu_tanh", xd))


# ------------------------------------------------------------------ conv
# the GPU module's cases: 3x3 on five 7 x 9 images, 64 / 128 channels, two pad sets, stride 1 / 2, an N tail;
# 1x1 stride 2; the 24-channel igemm case
CONV_CASES = ([(5, 7, 9, c, 72, 3, st, p) for c in (64, 128) for st in (1, 2) for p in ((1, 1, 1, 1), (0, 2, 1, 0))]
              + [(5, 7, 9, 64, 72, 1, 2, (0, 0, 0, 0)), (1, 9, 9, 24, 40, 3, 2, (0, 1, 0, 1))])


def ideal_conv(x, wt, b, r, s, pads, act, masked_tap_col=None):
    pt, pb, pl, pr = pads
    xp = F.pad(x.float().permute(0, 3, 1, 2), [pl, pr, pt, pb])
    y = F.conv2d(xp, wt.permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1)
    if masked_tap_col is not None:
        # tap (0, 0)'s padding mask one pixel off: it also masks an in-bounds output column
        tap = F.conv2d(xp[:, :, :xp.shape[2] - (wt.shape[0] - 1), :xp.shape[3] - (wt.shape[1] - 1)],
                       wt[:1, :1].permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1)
        y[:, :, masked_tap_col] -= tap[:, :, masked_tap_col]
    y = y + b
    if r is not None:
        y = y + r.float()
    return bf_round(act32(act, y))


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_ideal_within_bound_and_mutants_rejected(case):
    n, h, w, cin, cout, k, s, pads = case
    x, wt, b, r = kb.conv_inputs(*case)
    for res in (r, None):
        pre, mag = kb.conv_parts(x, wt, b, s, pads, res)
        for act in ("none", "relu"):
            for splits in (1, 2, 3):
                ref, bound = kb.epilogue(pre, mag, k * k * cin, splits, act, False)
                kb.assert_within(ideal_conv(x, wt, b, res, s, pads, act), ref, bound, f"conv {act}")
            if k == 3:
                rejected(ideal_conv(x, wt, b, res, s, pads, act, masked_tap_col=1), ref, bound)
    # the post-activation output, computed from the fp32 epilogue value
    sc, sh = rnd(cout, seed=35) * 0.5 + 1.0, rnd(cout, seed=36) * 0.2
    pre, mag = kb.conv_parts(x, wt, b, s, pads, r)
    ref2, bound2 = kb.post_output(pre, mag, k * k * cin, 1, sc, sh, "relu")
    pt, pb, pl, pr = pads
    v = F.conv2d(F.pad(x.float().permute(0, 3, 1, 2), [pl, pr, pt, pb]), wt.permute(3, 2, 0, 1),
                 stride=s).permute(0, 2, 3, 1) + b + r.float()
    kb.assert_within(bf_round(torch.relu(v * sc + sh)), ref2, bound2, "post")
    rejected(bf_round(torch.relu(v * sc)), ref2, bound2)


# ------------------------------------------------------------------ many-tile launch geometries
# The shapes of test_launch_geometry_gpu.py.  A wrong tile walk or a tile remap
# that is no bijection leaves whole tiles unwritten, stale or exchanged; the
# mutants below are those, on 128-row tiles of the flattened [M, N] output.
def test_nan_against_finite_reference_is_a_violation_with_its_index():
    ref = rnd(6, 9, seed=1).double()
    y = ref.clone()
    y[4, 7] = float("nan")
    with pytest.raises(AssertionError) as e:
        kb.assert_within(y, ref, 1e30, "unwritten")
    assert "1 of 54" in str(e.value) and "(4, 7)" in str(e.value) and "inf" in str(e.value)
    rejected(torch.full((6, 9), float("nan"), dtype=BF), ref, 1e30)
    rejected(torch.full((6, 9), float("inf")), ref, 1e30)


def tile_mutants(y, bm=128, grid=8):
    """(name, mutated copy) of a [M, N] output computed in bm-row tiles by a
    grid of `grid` persistent workgroups."""
    m = y.shape[0]
    tiles = -(-m // bm)
    assert tiles > grid + 2
    t = tiles // 2 + grid                      # an interior tile with a predecessor `grid` positions earlier

    def rows(i):
        return slice(i * bm, min((i + 1) * bm, m))
    nan, zero, stale, swapped = y.clone(), y.clone(), y.clone(), y.clone()
    nan[rows(t)] = float("nan")
    zero[rows(t)] = 0
    stale[rows(t)] = y[rows(t - grid)]
    swapped[rows(t)], swapped[rows(t - 1)] = y[rows(t - 1)], y[rows(t)]
    return [("a tile left as NaN", nan), ("a tile left as zeros", zero),
            ("a tile holding the tile gridDim positions earlier", stale), ("two tiles swapped", swapped)]


# 1a at the 256 CUs of an MI355X (tiles == CUs, CUs + 1, 2 CUs + 3), both pad sets; 1b: the 11-image conv with
# Cout 72 / 200, stride 2 and the asymmetric pads, and the halo family's 128-channel split case
GEOMETRY_CONVS = ([(n, ho + 2 - p[0] - p[1], wo + 2 - p[2] - p[3], 64, 64, 3, 1, p)
                   for n, ho, wo in ((128, 16, 16), (513, 7, 7), (103, 24, 24)) for p in ((1, 1, 1, 1), (0, 2, 1, 0))]
                  + [(11, 24, 24, 64, 72, 3, 1, (1, 1, 1, 1)), (11, 24, 24, 64, 200, 3, 1, (1, 1, 1, 1)),
                     (11, 47, 47, 64, 72, 3, 2, (1, 1, 1, 1)), (11, 24, 24, 64, 200, 3, 1, (0, 2, 1, 0)),
                     (11, 24, 24, 128, 72, 3, 1, (1, 1, 1, 1))])


@pytest.mark.parametrize("case", GEOMETRY_CONVS)
def test_geometry_conv_ideal_within_bound_and_tile_mutants_rejected(case):
    n, h, w, cin, cout, k, s, pads = case
    x, wt, b, r = kb.conv_inputs(*case)
    res = None if cout == 64 else r                            # (the persistent kernel takes no residual)
    pre, mag = kb.conv_parts(x, wt, b, s, pads, res)
    for act in ("none", "relu"):
        y = ideal_conv(x, wt, b, res, s, pads, act)
        for splits in (1, 3):
            ref, bound = kb.epilogue(pre, mag, k * k * cin, splits, act, False)
            assert kb.assert_within(y, ref, bound, f"conv {act}") <= 1.0
        for name, bad in tile_mutants(y.reshape(-1, cout)):
            rejected(bad.reshape(y.shape), ref, bound, f"{case} {act}: {name}")


def test_geometry_linear_ideal_within_bound_and_tile_mutants_rejected():
    m, n, k = 6336 + 5, 200, 2880
    x, w, b, r = kb.gemm_inputs(m, n, k)
    pre, mag = kb.gemm_parts(x, w, b, r)
    for act, out_f32, splits in (("relu", False, 1), ("gelu_tanh", False, 3), ("none", True, 1), ("tanh", True, 3)):
        ref, bound = kb.epilogue(pre, mag, k, splits, act, out_f32)
        y = ideal_gemm(x, w, b, r, act, out_f32)
        assert kb.assert_within(y, ref, bound, f"{act} f32={out_f32}") <= 1.0
        for name, bad in tile_mutants(y):
            rejected(bad, ref, bound, f"linear {act} f32={out_f32}: {name}")
        short = y.clone()                                      # the 5-row M tail never written
        short[m - 5:] = float("nan")
        rejected(short, ref, bound, "M tail unwritten")


# ------------------------------------------------------------------ chain / head (bf16 intermediates)
@pytest.mark.parametrize("k1,n1,n2,m", [(64, 256, 64, 77), (128, 512, 256, 200)])
def test_chain_two_step_check(k1, n1, n2, m):
    x = rnd(m, k1, seed=61).to(BF)
    w1 = rnd(n1, k1, scale=1 / math.sqrt(k1), seed=62).to(BF)
    b1 = rnd(n1, scale=0.1, seed=63)
    res = rnd(m, n1, seed=64).to(BF)
    w2 = rnd(n2, n1, scale=1 / math.sqrt(n1), seed=65).to(BF)
    b2 = rnd(n2, scale=0.1, seed=66)
    y1 = ideal_gemm(x, w1, b1, res, "relu", False)
    y2 = ideal_gemm(y1.to(BF), w2, b2, None, "relu", False)
    ref1, bound1 = kb.epilogue(*kb.gemm_parts(x, w1, b1, res), k1, 1, "relu")
    kb.assert_within(y1, ref1, bound1, "y1")
    ref2, bound2 = kb.epilogue(*kb.gemm_parts(y1, w2, b2), n1, 1, "relu")     # from the kernel's own y1
    kb.assert_within(y2, ref2, bound2, "y2")
    rejected(ideal_gemm(y1.to(BF), w2, b2, None, "relu", False, drop_k_last_row=8), ref2, bound2)


@pytest.mark.parametrize("m,hw,k,np_,n,seed", kb.HEAD_CASES)
def test_head_ideal_within_bound(m, hw, k, np_, n, seed):
    x, w, b = kb.head_inputs(m, hw, k, np_, seed)
    p, bound, logits, dlogit = kb.head_ref(x, w, b, n)
    pooled = bf_round(x.float().mean((1, 2)))
    lg = (pooled @ w.float().t() + b)[:, :n]
    kb.assert_within(torch.softmax(lg, -1), p, bound, "head")
    assert kb.argmax_checked(lg.argmax(-1), logits, dlogit) == 1.0
    lg2 = (pooled @ w.float().t())[:, :n]                      # bias dropped
    rejected(torch.softmax(lg2, -1), p, bound, "bias")


# ------------------------------------------------------------------ attention
def attn_inputs(b, s, h, seed=21):
    return rnd(b, s, 3 * h * 64, seed=seed).to(BF)


def ideal_attention(qkv, h, scale, mask, drop_last_key=False, roll_mask=False):
    b, s, _ = qkv.shape
    q, k, v = qkv.float().reshape(b, s, 3, h, 64).permute(2, 0, 3, 1, 4)
    sc = q @ k.transpose(-1, -2) * torch.tensor(scale, dtype=torch.float32)
    if mask is not None:
        m = mask.float()
        if roll_mask:
            m = torch.roll(m, 1, -1)
        sc = sc + (m[:, None, None, :] if m.dim() == 2 else m)
    if drop_last_key:
        sc[..., -1] = float("-inf")
    p = torch.exp(sc - sc.amax(-1, keepdim=True))
    o = (bf_round(p) @ v) / p.sum(-1, keepdim=True)
    return bf_round(o.permute(0, 2, 1, 3).reshape(b, s, h * 64))


@pytest.mark.parametrize("s", [1, 16, 33, 64, 100, 128, 192, 256, 320])
def test_attention_ideal_within_bound_and_mutants_rejected(s):
    b, h, scale = 2, 3, 1 / 8
    qkv = attn_inputs(b, s, h)
    key = torch.zeros(b, s)
    key[1, s // 2:] = -10000.0
    causal = torch.triu(torch.full((s, s), -10000.0), 1).expand(b, 1, s, s).contiguous()
    for mask in (None, key, causal):
        ref, bound = kb.attention_ref(qkv, h, scale, mask)
        kb.assert_within(ideal_attention(qkv, h, scale, mask), ref, bound, f"attention S={s}")
    if s >= 33:
        ref, bound = kb.attention_ref(qkv, h, scale, key)
        rejected(ideal_attention(qkv, h, scale * 1.01, key), ref, bound)
        rejected(ideal_attention(qkv, h, scale, key, roll_mask=True), ref, bound)
        ref, bound = kb.attention_ref(qkv, h, scale, None)
        rejected(ideal_attention(qkv, h, scale, None, drop_last_key=True), ref, bound)


@pytest.mark.parametrize("s", [100, 128, 320])
@pytest.mark.parametrize("fill", [-10000.0, float("-inf"), torch.finfo(torch.float32).min])
def test_attention_reference_with_a_closed_first_block(s, fill):
    """First 64 keys closed, later keys open: the reference is the softmax over
    the open keys (finite), whatever the fill value."""
    b, h, scale = 1, 2, 1 / 8
    qkv = attn_inputs(b, s, h)
    mask = torch.zeros(b, s)
    mask[:, :64] = fill
    ref, bound = kb.attention_ref(qkv, h, scale, mask)
    open_only = kb.attention_ref(qkv[:, 64:].contiguous(), h, scale, None)[0]
    q_rows = kb.attention_ref(torch.cat([qkv[:, :64], qkv[:, 64:]], 1), h, scale, mask)[0]
    assert torch.isfinite(ref).all() and torch.equal(ref, q_rows)
    assert (ref[:, 64:] - open_only).abs().max() < 1e-12
    kb.assert_within(ideal_attention(qkv, h, scale, mask), ref, bound, "closed first block")


# ------------------------------------------------------------------ LayerNorm
def ideal_layernorm(z32, gamma, beta, eps, unbiased=False):
    mu = z32.mean(-1, keepdim=True)
    c = z32 - mu
    var = (c * c).sum(-1, keepdim=True) / (z32.shape[-1] - (1 if unbiased else 0))
    return bf_round(c * torch.rsqrt(var + eps) * gamma + beta)


@pytest.mark.parametrize("cols", [64, 128, 520, 768, 2048, 4104])
def test_layernorm_ideal_within_bound_and_unbiased_variance_rejected(cols):
    x = (rnd(37, cols, seed=41) * 3 + 5).to(BF)
    r = rnd(37, cols, seed=42).to(BF)
    gm, bt = rnd(cols, seed=43), rnd(cols, seed=44)
    for res in (r, None):
        z32 = x.float() + (res.float() if res is not None else 0)
        z64 = x.double() + (res.double() if res is not None else 0)
        ref, bound = kb.layernorm_ref(z64, gm, bt, 1e-5)
        kb.assert_within(ideal_layernorm(z32, gm, bt, 1e-5), ref, bound, f"LN {cols}")
        if cols <= 768:
            rejected(ideal_layernorm(z32, gm, bt, 1e-5, unbiased=True), ref, bound)


@pytest.mark.parametrize("m,n,k", [(33, 512, 1024), (100, 768, 768)])
def test_linear_ln_ideal_within_bound(m, n, k):
    x = rnd(m, k, seed=61).to(BF)
    w = (rnd(n, k, seed=62) / math.sqrt(k)).to(BF)
    b = rnd(n, seed=63)
    r = (rnd(m, n, seed=64) * 2 + 3).to(BF)
    gm, bt = rnd(n, seed=65), rnd(n, seed=66)
    pre, mag = kb.gemm_parts(x, w, b, r)
    ref, bound = kb.layernorm_ref(pre, gm, bt, 1e-12, dz=(k + 5) * kb.E * mag)
    z32 = x.float() @ w.float().t() + b + r.float()
    kb.assert_within(ideal_layernorm(z32, gm, bt, 1e-12), ref, bound, "linear_ln")
    # (the GEMM's worst-case accumulation term hides an unbiased variance here:
    # that mutant is rejected on the plain LayerNorm, widths <= 768)
    z32[-1] -= x.float()[-1, -8:] @ w.float()[:, -8:].t()
    rejected(ideal_layernorm(z32, gm, bt, 1e-12), ref, bound, "K tail")


def ideal_lnx_stats(st, length, eps):
    a, b = st[:, :, 0].sum(1), st[:, :, 1].sum(1)
    mean = a * (1.0 / length)
    return mean[:, None], torch.rsqrt(torch.clamp(b * (1.0 / length) - mean * mean, min=0) + eps)[:, None]


@pytest.mark.parametrize("m,n,k", [(77, 256, 128), (130, 512, 64)])
def test_linear_lnx_ideal_within_bound_and_mutants_rejected(m, n, k):
    """The deferred-LayerNorm GEMM as the kernel computes it (one-pass
    statistics from fp32 partials, x w^T - mean colsum): both sides."""
    z = (rnd(m, k, seed=71) * 1.5 + 0.3).to(BF)
    W = rnd(k, n, scale=1 / math.sqrt(k), seed=72)
    b = rnd(n, scale=0.1, seed=73)
    g, bt = 1 + rnd(k, scale=0.1, seed=74), rnd(k, scale=0.1, seed=75)
    wf = (W * g[:, None]).t().contiguous().to(BF)
    bf = b + bt @ W
    colsum = wf.double().sum(1).float()
    ref, bound = kb.lnx_ref(z, wf, bf, "gelu_tanh", a_parts=2, a_eps=1e-12, colsum=colsum)
    mean, rstd = ideal_lnx_stats(kb.row_partials(z, 2), k, 1e-12)
    acc = z.float() @ wf.float().t()
    kb.assert_within(bf_round(act32("gelu_tanh", rstd * (acc - mean * colsum) + bf)), ref, bound, "lnx input side")
    rejected(bf_round(act32("gelu_tanh", rstd * (acc - mean * colsum) + b)), ref, bound, "beta not folded")
    rejected(bf_round(act32("gelu_tanh", rstd * acc + bf)), ref, bound, "mean colsum dropped")
    mean_u, rstd_u = mean, rstd * math.sqrt((k - 1) / k)
    rejected(bf_round(act32("gelu_tanh", rstd_u * (acc - mean_u * colsum) + bf)), ref, bound, "unbiased variance")
    # residual side
    x = rnd(m, k, seed=61).to(BF)
    w = rnd(n, k, scale=1 / math.sqrt(k), seed=62).to(BF)
    zr = (rnd(m, n, seed=64) * 2 + 0.5).to(BF)
    g2, b2 = 1 + rnd(n, scale=0.1, seed=65), rnd(n, scale=0.1, seed=66)
    for parts in (1, 3):
        ref, bound = kb.lnx_ref(x, w, b, "none", zr=zr, r_parts=parts, r_gamma=g2, r_beta=b2, r_eps=1e-12)
        mean, rstd = ideal_lnx_stats(kb.row_partials(zr, parts), n, 1e-12)
        t = x.float() @ w.float().t() + b
        y = bf_round(t + ((zr.float() - mean) * rstd * g2 + b2))
        kb.assert_within(y, ref, bound, "lnx residual side")
        rejected(bf_round(t + ((zr.float() - mean) * rstd + b2)), ref, bound, "gamma dropped")
        rejected(bf_round(t + ((zr.float() - mean) * rstd * math.sqrt((n - 1) / n) * g2 + b2)), ref, bound,
                 "unbiased variance")
        sums, sbound = kb.stats_bound(y, 4)
        st = torch.stack([y.sum(1), (y * y).sum(1)], 1)
        kb.assert_within(st, sums, sbound, "row statistics")
        rejected(torch.stack([y[:, :-1].sum(1), (y * y).sum(1)], 1), sums, sbound, "last column missing")


# ------------------------------------------------------------------ pools, softmax
@pytest.mark.parametrize("n,hw,c", [(3, 1, 72), (2, 9, 520), (1, 49, 4096)])
def test_gap_ideal_within_bound_and_wrong_divisor_rejected(n, hw, c):
    g = rnd(n, hw, 1, c, seed=hw + c).to(BF)
    ref, bound, _ = kb.gap_ref(g)
    kb.assert_within(bf_round(g.float().sum((1, 2)) * (1.0 / hw)), ref, bound, "gap")
    rejected(bf_round(g.float().sum((1, 2)) / (hw + 1)), ref, bound)
    if hw > 1:       # (the mean of one bf16 value is exact: nothing to truncate)
        rejected(bf_trunc(g.float().sum((1, 2)) * (1.0 / hw)), ref, bound)


@pytest.mark.parametrize("rows,cols", [(2, 10), (3, 1001), (1, 4096), (2, 5000)])
def test_softmax_ideal_within_bound(rows, cols):
    lg = rnd(rows, cols, scale=4, seed=rows + cols)
    p, bound = kb.softmax_ref(lg)
    kb.assert_within(torch.softmax(lg, -1), p, bound, "softmax")
    rejected(torch.softmax(lg * (1 + 1e-4), -1), p, bound)
    lb = lg.to(BF)
    p, bound = kb.softmax_ref(lb)
    kb.assert_within(torch.softmax(lb.float(), -1), p, bound, "softmax bf16 logits")
    assert kb.argmax_checked(lg.argmax(-1), lg, 0.0) == 1.0


@pytest.mark.parametrize("b,n,k", [(32, 2, 768), (5, 3, 1024), (1, 16, 64)])
def test_dense_softmax_ideal_within_bound(b, n, k):
    x = rnd(b, k, seed=31)
    w = rnd(n + 3, k, scale=1 / math.sqrt(k), seed=32).to(BF)
    bias = rnd(n + 3, scale=0.5, seed=33)
    p, bound = kb.dense_softmax_ref(x, w, bias, n)
    kb.assert_within(torch.softmax(x @ w[:n].float().t() + bias[:n], -1), p, bound, "dense_softmax")
    rejected(torch.softmax(x @ w[:n].float().t(), -1), p, bound)


def test_maxpool_reference_asymmetric_window():
    x = rnd(2, 9, 13, 8, seed=3).to(BF)
    ref = kb.maxpool_ref(x, 3, 2, 2, 1, 0, 1, 2, 0)
    assert ref.shape == (2, (9 + 1 - 3) // 2 + 1, (13 + 2 - 2) // 1 + 1, 8)
    assert ref[0, 0, 0, 0] == float("-inf")                          # two left pad columns: a window of padding only
    assert ref[0, 0, 1, 0] == x[0, 0:3, 0:1, 0].double().max()
    assert ref[0, -1, -1, 0] == x[0, 6:9, 11:13, 0].double().max()
