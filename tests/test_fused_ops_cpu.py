"""The fused graph ops' weight packing, and the op-level cases of
test_fused_ops_gpu.py tested on the CPU.

 (a) Packing is bit-exact: each op class is constructed with use_hip=True on
     the CPU device, its packed weights are unpacked through the documented
     layouts (fused_op_refs.unpack_*) and compared bit for bit with the bf16
     weights the test started from; every padding element is exactly zero.
 (b) The cases can see the bugs they exist for: at the shapes the GPU module
     runs, an ideal fp32 emulation stays inside the bound at every element and
     each mutant (a subtly wrong op) is rejected."""
import pytest
import torch
import torch.nn.functional as F

import fused_op_refs as fr
import kernel_bounds as kb
from kernel_bounds import BF, rnd
from rust_tensorflow_serving2_amd.graph import fused as FU

CPU = torch.device("cpu")


def bf_round(t):
    return t.to(BF).float()


def rejected(y, ref, bound, what="mutant"):
    try:
        kb.assert_within(y, ref, bound, what)
    except AssertionError as e:
        assert "outside the bound" in str(e), str(e)
        return
    pytest.fail(f"the bound did not reject: {what}")


def all_zero_bits(t):
    return t.numel() == 0 or not t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32).any()


# ================================================================== (a) packing
@pytest.mark.parametrize("kh,kw,cin,cout", fr.CONV_SHAPES)
def test_conv_packing_bit_exact(kh, kw, cin, cout):
    wt = rnd(kh, kw, cin, cout, seed=kh * kw + cin).to(BF)
    b = rnd(cout, seed=3)
    op = FU.FusedConv(wt.float(), b, (1, 1), "SAME", (0, 0, 0, 0), "relu", CPU, True, "c")
    assert op.w.dtype == BF and op.w.shape[0] == cout and op.w.shape[1] % 64 == 0 and op.w.is_contiguous()
    assert op.c4 == (fr.conv_branch(kh, kw, cin, cout) == "c4")
    if op.c4:
        assert op.khp % 2 == 0 and op.khp in (kh, kh + 1) and op.w.shape[1] >= op.khp * 32
        got, rest = fr.unpack_c4(op.w, kh, kw, cin)
    else:
        assert op.khp == kh
        got, rest = fr.unpack_dense(op.w, kh, kw, cin)
    assert fr.same_bits(got.contiguous(), wt), "packed weights differ from the HWIO weights"
    assert all_zero_bits(rest), "padding taps / rows / channels / K tail must be exactly zero"
    assert fr.same_bits(op.b, b)
    assert op.post_ok() == (cin % 64 == 0 and cout % 8 == 0)


def test_dual_conv_packing_bit_exact():
    c1, c2, cout = 64, 128, 72
    w1, w2 = rnd(1, 1, c1, cout, seed=1).to(BF), rnd(1, 1, c2, cout, seed=2).to(BF)
    b1, b2 = rnd(cout, seed=3), rnd(cout, seed=4)
    ch = FU.FusedConv(w1.float(), b1, (1, 1), "SAME", (0, 0, 0, 0), "none", CPU, True, "h")
    cx = FU.FusedConv(w2.float(), b2, (2, 2), "SAME", (0, 0, 0, 0), "none", CPU, True, "x")
    op = FU.FusedDualConv(ch, cx, "relu", CPU, True, "d")
    assert (op.c1, op.c2, op.cout, op.sh, op.sw, op.act) == (c1, c2, cout, 2, 2, "relu")
    assert op.w.dtype == BF and op.w.shape == (cout, c1 + c2) and op.w.is_contiguous()
    g1, g2, rest = fr.unpack_dual(op.w, c1, c2)
    assert fr.same_bits(g1.contiguous(), w1.reshape(c1, cout)) and fr.same_bits(g2.contiguous(), w2.reshape(c2, cout))
    assert all_zero_bits(rest)
    assert fr.same_bits(op.b, b1 + b2) and op.b.is_contiguous()
    # the conv whose stride the dual conv takes is x's, whichever order the pass found them in
    assert (FU.FusedDualConv(cx, ch, "none", CPU, True, "d2").sh, ch.sh) == (1, 1)


@pytest.mark.parametrize("k,n,pad_n", [(64, 13, False), (64, 13, True), (72, 13, True), (20, 13, True)])
def test_matmul_packing_bit_exact(k, n, pad_n):
    w = rnd(k, n, seed=k + n).to(BF)
    b = rnd(n, seed=5)
    op = FU.FusedMatMul(w.float(), b, "none", True, CPU, True, "m", pad_n=pad_n)
    if k % 8:
        # the torch fallback: no packed weights, the fp32 ones as given
        assert op.use_hip is False and not hasattr(op, "w")
        assert fr.same_bits(op.w_ref, w.float()) and fr.same_bits(op.b_ref, b) and op.np == n
        return
    assert op.use_hip is True
    np_ = 16 if (pad_n and k % 64 == 0) else n        # pad_n only where the pipelined kernel applies (K % 64 == 0)
    assert op.np == np_ and op.w.shape == (np_, k) and op.b.shape == (np_,) and op.w.dtype == BF
    gw, gb, pad, tail_b = fr.unpack_matmul(op.w, op.b, k, n)
    assert fr.same_bits(gw.contiguous(), w) and fr.same_bits(gb.contiguous(), b)
    assert all_zero_bits(pad), "pad_n weight rows / the K padding must be exactly zero"
    assert all_zero_bits(tail_b), "pad_n tail bias must be exactly zero"
    # the slice a padded matmul launches with when it gets a residual
    assert fr.same_bits(op.w[:op.n].t().contiguous(), w) and op.w[:op.n].is_contiguous()


def test_matmul_without_bias_gets_a_zero_bias():
    op = FU.FusedMatMul(rnd(64, 13, seed=1), None, "none", False, CPU, True, "m", pad_n=True)
    assert op.b.shape == (16,) and all_zero_bits(op.b)


def test_classifier_head_shares_the_padded_matmul_weights():
    mm = FU.FusedMatMul(rnd(512, 13, seed=1), rnd(13, seed=2), "none", True, CPU, True, "m", pad_n=True)
    head = FU.ClassifierHead(mm, torch.int32, True)
    assert head.use_hip and head.n == 13 and head.w is mm.w and head.b is mm.b and head.w.shape == (16, 512)
    mm2 = FU.FusedMatMul(rnd(576, 13, seed=1), rnd(13, seed=2), "none", True, CPU, True, "m", pad_n=True)
    assert not FU.ClassifierHead(mm2, torch.int64, True).use_hip          # k outside the kernel's set


# ================================================================== (b) ideal emulations and mutants
def ideal_conv(x, wt, b, r, strides, p, act, post=None, res_after_act=False, post_from_rounded=False):
    """The op done right in fp32: pad, conv, + bias, + residual, act, one bf16
    store; the post output from the fp32 epilogue value."""
    pt, pb, pl, pr = p
    v = F.conv2d(F.pad(x.float().permute(0, 3, 1, 2), [pl, pr, pt, pb]), wt.permute(3, 2, 0, 1),
                 stride=tuple(strides)).permute(0, 2, 3, 1) + b
    if r is not None and not res_after_act:
        v = v + r.float()
    y = kb.act64(act, v)
    if r is not None and res_after_act:
        y = y + r.float()
    outs = [bf_round(y)]
    if post is not None:
        sc, sf, act2, mode = post
        src = outs[0] if post_from_rounded else v
        z = bf_round(kb.act64(act2, src * sc + sf))
        outs = [outs[0], z] if mode == "dual" else [z]
    return outs


def swap_hw(wt):
    """kh / kw swapped in the packing: the [kw][kh] order read as [kh][kw]."""
    kh, kw, cin, cout = wt.shape
    return wt.permute(1, 0, 2, 3).reshape(kh, kw, cin, cout)


@pytest.mark.parametrize("case", fr.CONV_CASES, ids=fr.conv_case_id)
def test_conv_cases_ideal_within_bound_and_mutants_rejected(case):
    (kh, kw, cin, cout), (tag, even, strides, padding, pads) = case
    x, wt, b, r, sc, sf = fr.conv_case_inputs(case)
    p = fr.tf_pads(x.shape[1], x.shape[2], kh, kw, strides[0], strides[1], padding, pads)
    op = FU.FusedConv(wt, b, strides, padding, pads, "none", CPU, False, "c")
    assert op.pads_for(x.shape[1], x.shape[2]) == p
    for res in (r, None):
        pre, mag, k = fr.conv_parts_tf(x, wt, b, strides, padding, pads, res)
        for act in ("relu", "none"):
            ideal = ideal_conv(x, wt, b, res, strides, p, act)[0]
            for splits in (16, 1):
                ref, bound = kb.epilogue(pre, mag, k, splits, act, False)
                kb.assert_within(ideal, ref, bound, f"ideal {act}")
            # the op's own CPU path (fp32 torch on the folded parameters) is such an ideal op too
            op.act = act
            y = op(None, None, [x] + ([res] if res is not None else []))[0]
            kb.assert_within(bf_round(y), ref, bound, f"CPU op {act}")
            if p[0] != p[1] or p[2] != p[3]:
                rejected(ideal_conv(x, wt, b, res, strides, (p[1], p[0], p[3], p[2]), act)[0], ref, bound,
                         "pads on the other side")
            if kh != kw:
                rejected(ideal_conv(x, swap_hw(wt), b, res, strides, p, act)[0], ref, bound, "kh / kw swapped")
            if fr.conv_branch(kh, kw, cin, cout) == "c4" and kh % 2:
                # the image buffer sized for kh rows instead of kh + 1: the kernel's own output
                # height (from the padded filter) loses the last row, which stays unwritten
                y = ideal_conv(x, wt, b, res, strides, p, act)[0].clone()
                y[:, -1] = 0
                rejected(y, ref, bound, "filter rows not padded to even")
            if res is not None and act == "relu":
                rejected(ideal_conv(x, wt, b, res, strides, p, act, res_after_act=True)[0], ref, bound,
                         "residual added after the activation")
    if cin % 64 == 0:
        pre, mag, k = fr.conv_parts_tf(x, wt, b, strides, padding, pads, r)
        for mode in ("dual", "only"):
            post = (sc, sf, "relu", mode)
            want = fr.with_post(pre, mag, k, 1, "none", post)
            got = ideal_conv(x, wt, b, r, strides, p, "none", post)
            assert len(got) == len(want) == (2 if mode == "dual" else 1)
            for y, (ref, bound) in zip(got, want):
                kb.assert_within(y, ref, bound, f"ideal post {mode}")
            bad = ideal_conv(x, wt, b, r, strides, p, "none", post, post_from_rounded=True)
            rejected(bad[-1], *want[-1], "post affine read from the rounded first output")
            # a wrong post_mode: the first output of one mode where the other's is expected
            other = ideal_conv(x, wt, b, r, strides, p, "none", (sc, sf, "relu", "only" if mode == "dual" else "dual"))
            rejected(other[0], *want[0], "wrong post_mode")


def test_same_padding_mutant_is_seen_where_it_matters():
    """The cases include SAME at an even size with stride 2 and an odd filter
    (TF pads less on top / left there) for every filter shape but 1x1."""
    seen = set()
    for (kh, kw, cin, cout), (tag, even, (sh, sw), padding, pads) in fr.CONV_CASES:
        if padding == "SAME" and even and (sh, sw) == (2, 2):
            n, h, w = fr.conv_images((kh, kw, cin, cout), even)
            pt, pb = fr.same_pads(h, kh, sh)
            pl, pr = fr.same_pads(w, kw, sw)
            if pt != pb or pl != pr:
                seen.add((kh, kw, cin, cout))
    assert seen == {s for s in fr.CONV_SHAPES if s[:2] != (1, 1)}
    assert fr.same_pads(8, 3, 2) == (0, 1) and fr.same_pads(7, 3, 2) == (1, 1) and fr.same_pads(16, 7, 2) == (2, 3)
    assert fr.same_pads(18, 8, 1) == (3, 4) and fr.same_pads(9, 1, 2) == (0, 0)


@pytest.mark.parametrize("case", fr.DUAL_CASES)
def test_dual_cases_ideal_within_bound_and_mutants_rejected(case):
    n, ho, wo, c1, c2, cout, s = case
    h, x, w1, w2, b1, b2, sc, sf = fr.dual_case_inputs(case)

    def ideal(bias, xs, act, post=None):
        v = h.float() @ w1.reshape(c1, cout) + xs.float() @ w2.reshape(c2, cout) + bias
        outs = [bf_round(kb.act64(act, v))]
        if post is not None:
            outs.append(bf_round(torch.relu(v * post[0] + post[1])))
        return outs
    xs = x[:, ::s, ::s, :]
    for act in ("relu", "none"):
        (ref, bound), = fr.dual_ref(h, x, w1, w2, b1, b2, (s, s), act, 1)
        kb.assert_within(ideal(b1 + b2, xs, act)[0], ref, bound, f"ideal dual {act}")
        rejected(ideal(b1, xs, act)[0], ref, bound, "biases not summed")
        if s > 1:
            rejected(ideal(b1 + b2, x[:, :ho, :wo, :], act)[0], ref, bound, "stride dropped on x")
    want = fr.dual_ref(h, x, w1, w2, b1, b2, (s, s), "none", 1, (sc, sf, "relu", "dual"))
    for y, (ref, bound) in zip(ideal(b1 + b2, xs, "none", (sc, sf)), want):
        kb.assert_within(y, ref, bound, "ideal dual post")
    # the CPU op computes the same thing
    ch = FU.FusedConv(w1, b1, (1, 1), "SAME", (0, 0, 0, 0), "none", CPU, False, "h")
    cx = FU.FusedConv(w2, b2, (s, s), "SAME", (0, 0, 0, 0), "none", CPU, False, "x")
    op = FU.FusedDualConv(ch, cx, "none", CPU, False, "d")
    op.set_post(sc, sf, "relu", "dual")
    for y, (ref, bound) in zip(op(None, None, [h, x]), want):
        kb.assert_within(bf_round(y), ref, bound, "CPU dual op")


@pytest.mark.parametrize("k,n", fr.MATMUL_KN)
def test_matmul_cases_ideal_within_bound_and_mutants_rejected(k, n):
    m = fr.MATMUL_M
    x, w, b, r = fr.matmul_inputs(m, k, n)
    for res in (r, None):
        for out_f32 in (False, True):
            ref, bound = fr.matmul_ref(x, w, b, res, "none", out_f32)
            v = x.float() @ w + b + (res.float() if res is not None else 0)
            kb.assert_within(v if out_f32 else bf_round(v), ref, bound, "ideal matmul")
    # pad_n: the whole [M, ceil8(N)] buffer is checked, its tail columns are exactly zero
    np_ = -(-n // 8) * 8
    wp = torch.cat([w, torch.zeros(k, np_ - n)], 1)
    bp = torch.cat([b, torch.zeros(np_ - n)])
    ref, bound = fr.matmul_ref(x, wp, bp, None, "none", True)
    assert not ref[:, n:].any() and not bound[:, n:].any()
    kb.assert_within(x.float() @ wp + bp, ref, bound, "ideal padded matmul")
    bad = bp.clone()
    bad[n:] = 2.0 ** -20
    rejected(x.float() @ wp + bad, ref, bound, "pad_n tail bias not zero")


def test_deep_matmul_ideal_within_bound_at_every_split():
    x, w, b, r = fr.matmul_inputs(40, 2048, 72)
    for splits in (1, 2, 4, 8, 16):
        ref, bound = fr.matmul_ref(x, w, b, r, "relu", False, splits)
        # K split into slabs summed in fp32, as split-K does
        v = sum(x.float()[:, c] @ w[c] for c in torch.tensor_split(torch.arange(2048), splits))
        kb.assert_within(bf_round(torch.relu(v + b + r.float())), ref, bound, f"splits {splits}")
    rejected(bf_round(torch.relu(x.float()[:, :-8] @ w[:-8] + b + r.float())), ref, bound, "K tail dropped")


@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("pool_padding", ["SAME", "VALID"])
@pytest.mark.parametrize("even", [True, False])
def test_stem_pool_ideal_within_bound_and_mutants_rejected(even, pool_padding, post):
    case = ((7, 7, 3, 16), ("same-s2", even, (2, 2), "SAME", (0, 0, 0, 0)))
    x, wt, b, _r, sc, sf = fr.conv_case_inputs(case)
    pargs = (sc, sf, "relu") if post else None
    ref, bound = fr.stem_pool_ref(x, wt, b, "SAME", "relu", pool_padding, pargs)

    def ideal(p, pp):
        conv = ideal_conv(x, wt, b, None, (2, 2), p, "relu")[0]
        y = F.max_pool2d(F.pad(conv.permute(0, 3, 1, 2), [pp[2], pp[3], pp[0], pp[1]], value=float("-inf")),
                         (3, 3), (2, 2)).permute(0, 2, 3, 1)
        return bf_round(torch.relu(y * sc + sf)) if post else y
    p = fr.tf_pads(x.shape[1], x.shape[2], 7, 7, 2, 2, "SAME")
    hc, wc = fr.out_hw(x.shape[1], x.shape[2], 7, 7, 2, 2, p)
    pp = fr.tf_pads(hc, wc, 3, 3, 2, 2, pool_padding)
    kb.assert_within(ideal(p, pp), ref, bound, "ideal stem + pool")
    if p[0] != p[1]:
        rejected(ideal((p[1], p[0], p[3], p[2]), pp), ref, bound, "conv pads on the other side")
    if pp[0] != pp[1] or pp[2] != pp[3]:
        rejected(ideal(p, (pp[1], pp[0], pp[3], pp[2])), ref, bound, "pool pads on the other side")


# ================================================================== (c) the window geometry the conv and pool ops share
def windows(k, s, padding, pads):
    """One op of every class that is a window, k x k at stride s (C = 8, the grouped conv in two groups)."""
    conv = (rnd(8, seed=1), (s, s), padding, pads, "none", CPU, False)
    return [FU.FusedConv(rnd(k, k, 8, 8, seed=2), *conv, "dense"),
            FU.FusedDepthwiseConv(rnd(k, k, 8, seed=3), *conv, "depthwise"),
            FU.FusedGroupedConv(rnd(k, k, 4, 8, seed=4), *conv, "grouped", 8),
            FU.MaxPool((k, k), (s, s), padding, False, pads)]


@pytest.mark.parametrize("padding", ["SAME", "VALID", "EXPLICIT"])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("k", [1, 3, 5, 7])
def test_window_geometry_is_tensorflows(k, s, padding):
    """pads_for and out_hw of every window class against fused_op_refs, for odd
    and even sizes 1..9 (h and w differ, w = 10 - h), and against the shape of
    what the ops compute wherever the padded input holds a window."""
    pads = (1, 2, 0, 1)                 # EXPLICIT: uneven on both axes
    x9 = rnd(1, 9, 9, 8, seed=5)
    for op in windows(k, s, padding, pads):
        for h in range(1, 10):
            w = 10 - h
            p = fr.tf_pads(h, w, k, k, s, s, padding, pads)
            assert op.pads_for(h, w) == p
            want = fr.out_hw(h, w, k, k, s, s, p)
            assert op.out_hw(h, w, p) == want, (type(op).__name__, h, w)
            if min(want) >= 1:
                y = op(None, None, [x9[:, :h, :w]])[0]
                assert tuple(y.shape) == (1,) + want + (8,), (type(op).__name__, h, w, tuple(y.shape))


def test_window_same_split_is_uneven_at_stride_2():
    """An even size under an odd filter at stride 2: one row / column of padding, behind."""
    for op in windows(3, 2, "SAME", (0, 0, 0, 0)):
        assert op.pads_for(8, 6) == (0, 1, 0, 1) and op.out_hw(8, 6, (0, 1, 0, 1)) == (4, 3)
        assert op.pads_for(9, 7) == (1, 1, 1, 1) and op.out_hw(9, 7, (1, 1, 1, 1)) == (5, 4)


@pytest.mark.parametrize("k,s", [(7, 2), (3, 1), (5, 2)])
def test_window_override_is_the_padded_rgba_filter(k, s):
    """FusedConv's RGB(A) path computes with a khp x 8 filter over an image it
    sizes itself: out_hw with that extent gives the plain conv's output size back."""
    op = FU.FusedConv(rnd(k, k, 3, 16, seed=6), rnd(16, seed=7), (s, s), "SAME", (0, 0, 0, 0), "none", CPU, True, "c")
    assert op.c4 and op.khp == k + 1
    for h, w in ((9, 6), (8, 7), (4, 5)):
        p = op.pads_for(h, w)
        ho, wo = op.out_hw(h, w, p)
        assert (ho, wo) == fr.out_hw(h, w, k, k, s, s, p)
        hp, wp = (ho - 1) * s + op.khp, (wo - 1) * s + 8
        assert op.out_hw(hp, wp, (0, 0, 0, 0), op.khp, 8) == (ho, wo) == fr.out_hw(hp, wp, op.khp, 8, s, s, (0,) * 4)
