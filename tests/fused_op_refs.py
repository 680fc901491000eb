"""fp64 references for the fused graph ops, in TensorFlow's terms.

A plain helper module like kernel_bounds.py (no fixtures, nothing at collection
time).  The op classes of graph/fused.py take HWIO weights, (sh, sw) strides,
"SAME" | "VALID" | "EXPLICIT" padding, a residual, an activation and a post
scale / shift / activation with its mode; so do the references here, and they
hand the work to kernel_bounds: every (ref, bound) pair is what kernel_bounds
gives for the kernel the op launches, with no constant of its own.

Every operand is bf16-valued (weights, inputs, residuals) and every bias and
post parameter a multiple of 2^-6, so the packing the ops do is exact, the sum
of two biases is exact in fp32 and the kernel bounds apply unchanged.

The unpackers invert the documented weight layouts: they return the logical
weights and, separately, everything else the packed tensor holds (the padding),
which must be exactly zero.

The case lists are shared by test_fused_ops_cpu.py (an ideal fp32 emulation
stays inside the bound, each mutant is rejected) and test_fused_ops_gpu.py (the
op classes on the kernels).  The second half does the same for the op classes
of the later model families, with the bounds of their own kernel modules."""
import math

import torch
import torch.nn.functional as F

import dwconv_bounds as db
import dwln_bounds as lb
import interact_bounds as ib
import kernel_bounds as kb
import se_bounds as sb
import swish_bounds as wb
import wattn_bounds as ab
from kernel_bounds import BF, rnd
from patch_tokens_bounds import reference as pt_reference


# ---------------------------------------------------------------- TF padding
def same_pads(size, k, s):
    """TensorFlow's SAME padding of one axis: out = ceil(size / s), the total
    max((out - 1) s + k - size, 0) is split with the SMALLER half in front
    (top / left) -- on an even size at stride 2 with an odd filter the two
    sides differ."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return total // 2, total - total // 2


def tf_pads(h, w, kh, kw, sh, sw, padding, pads=(0, 0, 0, 0)):
    """(top, bottom, left, right)."""
    if padding == "SAME":
        return same_pads(h, kh, sh) + same_pads(w, kw, sw)
    if padding == "EXPLICIT":
        return tuple(pads)
    assert padding == "VALID", padding
    return (0, 0, 0, 0)


def out_hw(h, w, kh, kw, sh, sw, p):
    return (h + p[0] + p[1] - kh) // sh + 1, (w + p[2] + p[3] - kw) // sw + 1


# ---------------------------------------------------------------- references
def with_post(pre, mag, k, splits, act, post, out_f32=False):
    """The op's outputs as [(ref, bound), ...]: [y] / [y, post] / [post]."""
    first = kb.epilogue(pre, mag, k, splits, act, out_f32)
    if post is None:
        return [first]
    scale, shift, act2, mode = post
    assert act == "none", "the kernels apply the post affine to the pre-activation sum"
    second = kb.post_output(pre, mag, k, splits, scale, shift, act2, out_f32)
    return [first, second] if mode == "dual" else [second]


def conv_parts_tf(x, w_hwio, bias, strides, padding, pads=(0, 0, 0, 0), res=None):
    """(pre, mag, K) of Conv2D + bias (+ residual) in TF terms; K = the number
    of products per output (zero padding taps the kernels add are exact)."""
    kh, kw, cin, _ = w_hwio.shape
    p = tf_pads(x.shape[1], x.shape[2], kh, kw, strides[0], strides[1], padding, pads)
    pre, mag = kb.conv_parts(x, w_hwio, bias, tuple(strides), p, res)
    return pre, mag, kh * kw * cin


def conv_ref(x, w_hwio, bias, strides, padding, pads=(0, 0, 0, 0), res=None, act="none", splits=1, post=None):
    pre, mag, k = conv_parts_tf(x, w_hwio, bias, strides, padding, pads, res)
    return with_post(pre, mag, k, splits, act, post)


def dual_parts(h, x, w1_hwio, w2_hwio, b1, b2, strides):
    """conv1x1(h) + conv1x1(x, strides) + b1 + b2 as one K-concatenated GEMM."""
    sh, sw = strides
    c1, c2, cout = w1_hwio.shape[2], w2_hwio.shape[2], w1_hwio.shape[3]
    a = torch.cat([kb.d(h), kb.d(x)[:, ::sh, ::sw, :]], -1)
    w = torch.cat([kb.d(w1_hwio).reshape(c1, cout), kb.d(w2_hwio).reshape(c2, cout)], 0).t()
    pre, mag = kb.gemm_parts(a.reshape(-1, c1 + c2), w, kb.d(b1) + kb.d(b2))
    return pre.reshape(*h.shape[:3], cout), mag.reshape(*h.shape[:3], cout), c1 + c2


def dual_ref(h, x, w1_hwio, w2_hwio, b1, b2, strides, act="none", splits=1, post=None):
    pre, mag, k = dual_parts(h, x, w1_hwio, w2_hwio, b1, b2, strides)
    return with_post(pre, mag, k, splits, act, post)


def matmul_parts(x, w_kn, bias=None, res=None):
    """x [..., K] @ w [K, N] (+ bias, + residual) -> (pre, mag, K), shaped like the output."""
    k, n = w_kn.shape
    pre, mag = kb.gemm_parts(kb.d(x).reshape(-1, k), kb.d(w_kn).t(), bias, None if res is None else kb.d(res).reshape(-1, n))
    shape = list(x.shape[:-1]) + [n]
    return pre.reshape(shape), mag.reshape(shape), k


def matmul_ref(x, w_kn, bias=None, res=None, act="none", out_f32=False, splits=1):
    pre, mag, k = matmul_parts(x, w_kn, bias, res)
    return kb.epilogue(pre, mag, k, splits, act, out_f32)


def affine_after(ref, dref, scale, shift, act2="relu"):
    """(ref2, bound2) of act2(y * scale + shift) read from a STORED bf16 y with
    elementwise error bound dref (the max-pool and stem-pool post outputs):
    y's error scaled by |scale|, two fp32 roundings, the activation, one store."""
    scale, shift = kb.d(scale), kb.d(shift)
    pre2 = ref * scale + shift
    acc = dref * scale.abs() + 2 * kb.E * ((ref * scale).abs() + shift.abs())
    ref2 = kb.act64(act2, pre2)
    return ref2, kb.out_bound(ref2, kb.L_ACT[act2] * acc + kb.act_abs(act2, pre2), False)


def stem_pool_ref(x, w_hwio, bias, conv_padding, act, pool_padding, post=None):
    """conv 7x7 / 2 (+ bias, act) -> max pool 3x3 / 2 (-> affine + act2).
    The conv value is rounded to bf16 before the pool; rounding is monotone,
    so the pooled value is the rounded maximum: its error is the largest
    accumulation error in the window, then one rounding."""
    pre, mag, k = conv_parts_tf(x, w_hwio, bias, (2, 2), conv_padding)
    conv = kb.act64(act, pre)
    acc = kb.acc_bound(pre, mag, k, 1, act)
    hc, wc = conv.shape[1], conv.shape[2]
    pp = tf_pads(hc, wc, 3, 3, 2, 2, pool_padding)
    refp = kb.maxpool_ref(conv, 3, 3, 2, 2, *pp)
    # (the error bound is pooled with zero padding: -inf would poison a maximum of bounds)
    accp = _pool_zero_pad(acc, pp)
    bound = kb.out_bound(refp, accp, False)
    if post is None:
        return refp, bound
    return affine_after(refp, bound, post[0], post[1], post[2])


def _pool_zero_pad(t, pp):
    pt, pb, pl, pr = pp
    xp = F.pad(t.permute(0, 3, 1, 2), [pl, pr, pt, pb], value=0.0)
    return F.max_pool2d(xp, (3, 3), (2, 2)).permute(0, 2, 3, 1)


# ---------------------------------------------------------------- unpackers
def unpack_dense(w, kh, kw, cin):
    """[Cout][Kpad] (K = kh kw cin, tap-major, channel-minor) -> (HWIO, K padding)."""
    cout = w.shape[0]
    k = kh * kw * cin
    return w[:, :k].reshape(cout, kh, kw, cin).permute(1, 2, 3, 0), w[:, k:]


def unpack_c4(w, kh, kw, cin):
    """The RGBA stem layout [Cout][khp][8 taps][4 channels] with kh padded to
    even -> (HWIO, everything outside the kh x kw x cin block as one vector)."""
    cout = w.shape[0]
    khp = kh + kh % 2
    assert w.shape[1] >= khp * 32 and w.shape[1] % 64 == 0, tuple(w.shape)
    w4 = w[:, :khp * 32].reshape(cout, khp, 8, 4)
    rest = w4.clone()
    rest[:, :kh, :kw, :cin] = 0
    return w4[:, :kh, :kw, :cin].permute(1, 2, 3, 0), torch.cat([rest.reshape(cout, -1), w[:, khp * 32:]], 1)


def unpack_dual(w, c1, c2):
    """[Cout][C1 + C2 (+ pad)] -> (w_h [C1, Cout], w_x [C2, Cout], padding)."""
    return w[:, :c1].t(), w[:, c1:c1 + c2].t(), w[:, c1 + c2:]


def unpack_matmul(w, b, k, n):
    """[Np][Kpad], [Np] -> (w [K, N], b [N], padding weights as one vector, tail bias)."""
    pad = torch.cat([w[:n, k:].reshape(-1), w[n:].reshape(-1)])
    return w[:n, :k].t(), b[:n], pad, b[n:]


def same_bits(a, b):
    """Bit-for-bit equality of two tensors of one dtype (NaN- and -0-safe)."""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
    it = torch.int16 if a.dtype == BF else torch.int32
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ---------------------------------------------------------------- shared inputs
def q6(t):
    """Multiples of 2^-6: sums and differences of a few are exact in fp32."""
    return torch.round(t * 64) / 64


# kh, kw, cin, cout.  5x8x1x8 is the kw == 8 edge of the RGBA layout, 3x9x3x8 has kw > 8 (not RGBA).
CONV_SHAPES = [(7, 7, 3, 16), (3, 3, 4, 8), (5, 8, 1, 8), (3, 9, 3, 8), (3, 3, 12, 8), (3, 3, 24, 40),
               (1, 1, 64, 72), (3, 3, 64, 72)]


def conv_branch(kh, kw, cin, cout):
    """The dispatch branch FusedConv takes on the GPU."""
    if cin <= 4 and kw <= 8:
        return "c4"
    if cin % 8:
        return "f32"
    return "aligned" if cin % 64 == 0 else "bf16"


def conv_images(shape, even):
    """(n, h, w): one full 256-row tile plus a partial one at stride 1.  The
    thin-channel (request-reading) branches get two stem-like images, the others five small ones."""
    if conv_branch(*shape) in ("c4", "f32"):
        return (2, 16, 18) if even else (2, 17, 19)
    return (5, 8, 10) if even else (5, 7, 9)


EXPLICIT_PADS = (2, 0, 1, 3)       # four different pads (top and left within the halo kernel's limit of 2)


def conv_geometries():
    """(tag, even image, (sh, sw), padding, pads)."""
    out = [(f"same-{'even' if even else 'odd'}-s{s}", even, (s, s), "SAME", (0, 0, 0, 0))
           for even in (True, False) for s in (1, 2)]
    out += [("valid", False, (1, 1), "VALID", (0, 0, 0, 0)), ("explicit", True, (2, 2), "EXPLICIT", EXPLICIT_PADS),
            ("explicit-s1", False, (1, 1), "EXPLICIT", EXPLICIT_PADS), ("same-s12", True, (1, 2), "SAME", (0, 0, 0, 0))]
    return out


CONV_CASES = [(shape, geo) for shape in CONV_SHAPES for geo in conv_geometries()]


def conv_case_id(case):
    (kh, kw, cin, cout), geo = case
    return f"{kh}x{kw}x{cin}x{cout}-{geo[0]}"


def conv_case_inputs(case):
    """x (bf16-valued fp32 NHWC), HWIO weights (bf16-valued fp32), bias, residual (bf16), post scale / shift."""
    (kh, kw, cin, cout), (_tag, even, strides, padding, pads) = case
    n, h, w = conv_images((kh, kw, cin, cout), even)
    seed = 1000 * kh + 100 * kw + cin + cout + h
    x = rnd(n, h, w, cin, seed=seed + 1).to(BF).float()
    wt = rnd(kh, kw, cin, cout, scale=1.0 / math.sqrt(kh * kw * cin), seed=seed + 2).to(BF).float()
    b = q6(rnd(cout, scale=0.3, seed=seed + 3))
    p = tf_pads(h, w, kh, kw, strides[0], strides[1], padding, pads)
    ho, wo = out_hw(h, w, kh, kw, strides[0], strides[1], p)
    r = rnd(n, ho, wo, cout, seed=seed + 4).to(BF)
    sc, sf = q6(rnd(cout, seed=seed + 5) * 0.5 + 1.0), q6(rnd(cout, seed=seed + 6) * 0.2)
    return x, wt, b, r, sc, sf


# (n, ho, wo, c1, c2, cout, stride)
DUAL_CASES = [(5, 7, 9, 64, 128, 72, 1), (5, 4, 5, 64, 128, 72, 2)]


def dual_case_inputs(case):
    n, ho, wo, c1, c2, cout, s = case
    hx, wx = (ho - 1) * s + 1 + (s - 1), (wo - 1) * s + 1      # (an even height at stride 2: the last row is unread)
    h = rnd(n, ho, wo, c1, seed=21 + s).to(BF)
    x = rnd(n, hx, wx, c2, seed=22 + s).to(BF)
    w1 = rnd(1, 1, c1, cout, scale=1 / math.sqrt(c1), seed=23).to(BF).float()
    w2 = rnd(1, 1, c2, cout, scale=1 / math.sqrt(c2), seed=24).to(BF).float()
    b1, b2 = q6(rnd(cout, scale=0.3, seed=25)), q6(rnd(cout, scale=0.3, seed=26))
    sc, sf = q6(rnd(cout, seed=27) * 0.5 + 1.0), q6(rnd(cout, seed=28) * 0.2)
    return h, x, w1, w2, b1, b2, sc, sf


# (m, k, n): one 64-row tile plus a partial one, 13 = an N tail that is no multiple of 8
MATMUL_M = 88
MATMUL_KN = [(64, 13), (72, 13), (20, 13)]


def matmul_inputs(m, k, n, seed=0):
    x, w_nk, b, r = kb.gemm_inputs(m, n, k, seed=seed + k + n)
    return x, w_nk.float().t().contiguous(), q6(b), r


# ================================================================ the ops added since MobileNet
# Depthwise conv, depthwise 7x7 + LayerNorm, patch tokens, windowed attention,
# embedding bag and dot interaction: (ref, bound) for what the op classes take,
# each bound from the module that holds the kernel's (dwconv_bounds, se_bounds,
# swish_bounds, dwln_bounds, wattn_bounds, interact_bounds, and the patch-token
# bound of patch_tokens_bounds).
DW_ACTS = ("none", "relu", "relu6", "hard_swish", "swish")


def dw_parts_tf(x, w_hwc, bias, strides, padding, pads=(0, 0, 0, 0)):
    """(pre, mag, taps) of a depthwise conv + bias in TF terms (dwconv_bounds.dw_parts under tf_pads)."""
    kh, kw, _c = w_hwc.shape
    p = tf_pads(x.shape[1], x.shape[2], kh, kw, strides[0], strides[1], padding, pads)
    pre, mag = db.dw_parts(x, w_hwc, bias, tuple(strides), p)
    return pre, mag, kh * kw


def dw_epilogue(pre, mag, taps, act):
    """(ref, bound) of one of DW_ACTS on the parts: se_bounds for hard-swish, swish_bounds for swish, and
    dwconv_bounds.dw_ref's own line for none / relu / relu6 (test_fused_ops_cpu.py holds the two equal)."""
    if act in ("hard_swish", "swish"):
        return (sb.hard_swish_dw if act == "hard_swish" else wb.swish_dw)(pre, mag, taps)
    ref = db.act64x(act, pre)
    return ref, kb.out_bound(ref, (taps + 2) * kb.E * mag, out_f32=False)


def dw_ref(x, w_hwc, bias, strides, padding, pads=(0, 0, 0, 0), act="none"):
    """FusedDepthwiseConv: an HWC fp32 filter, (sh, sw), TF padding, one of DW_ACTS."""
    return dw_epilogue(*dw_parts_tf(x, w_hwc, bias, strides, padding, pads), act)


def dwln_ref(x, w_hwc, bias, gamma, beta, eps, padding, pads=(0, 0, 0, 0), fused=True):
    """FusedDepthwiseLN.  gamma / beta: [C] or one element each.

    fused: the kernel keeps the conv value in fp32, dwln_bounds.dwln_ref.
    Not fused (FusedDepthwiseLN._pair): dwconv2d stores bf16(v) first, with v the
    fp32 conv value of dwconv_bounds, |v - pre| <= acc = (49 + 2) E mag.  The
    LayerNorm therefore reads z with |z - pre| <= 2^-8 (|pre| + acc) + acc, which
    is dwconv_bounds' own out_bound(pre, acc); that is the `dz` handed to
    kernel_bounds.layernorm_ref, whose bound then covers the LayerNorm kernel's
    statistics, affine and store as it does for linear_ln's accumulation error."""
    c = w_hwc.shape[2]
    p = tf_pads(x.shape[1], x.shape[2], 7, 7, 1, 1, padding, pads)
    gamma, beta = gamma.reshape(-1).expand(c), beta.reshape(-1).expand(c)
    if fused:
        return lb.dwln_ref(x, w_hwc, bias, gamma, beta, eps, p)
    pre, mag = db.dw_parts(x, w_hwc, bias, 1, p)
    return kb.layernorm_ref(pre, gamma, beta, eps, dz=kb.out_bound(pre, (lb.TAPS + 2) * kb.E * mag, False))


def patch_tokens_ref(x, cls, pos, batch):
    """PatchTokens: concat([cls repeated batch times, reshape(x, [-1, P, C])], 1) + pos, pos [P + 1, C] or
    [1, P + 1, C].  The bound is patch_tokens_bounds.reference's, E |ref| + ulp_bf16(|ref| (1 + E)) / 2, on
    the exact fp64 table.  Row 0 gets one more term: PatchTokens.__init__ forms cls + pos[0] with ONE fp32
    addition before the kernel sees it, so the table row the kernel rounds is off by at most half an ulp of
    fp32, 2^-24 |cls + pos[0]|."""
    c = cls.numel()
    pos64 = kb.d(pos).reshape(-1, c)
    table = pos64.clone()
    table[0] += kb.d(cls).reshape(c)
    xr = x.reshape(-1, pos64.shape[0] - 1, c)
    assert xr.shape[0] == batch, (tuple(x.shape), batch)
    ref, bound = pt_reference(xr, table)
    bound[:, 0] += kb.U_F32 * ref[:, 0].abs()
    return ref, bound


def wattn_ref(qkv, bias, mask, heads, scale, grid=None):
    """WindowAttentionOp.  qkv [R, 3 H D]; grid None: rows in window order, mask window bw % nW;
    grid (Hf, Wf, ws, shift): rows in image order.  Partition, cyclic shift and reverse are written
    out here (TF's Roll(-shift) -> window partition ... window reverse -> Roll(+shift))."""
    if grid is None:
        return ab.window_attention_ref(qkv, bias, mask, heads, scale)
    hf, wf, ws, shift = grid
    b = qkv.shape[0] // (hf * wf)

    def part(t):
        t = torch.roll(t.reshape(b, hf, wf, -1), (-shift, -shift), (1, 2))
        return t.reshape(b, hf // ws, ws, wf // ws, ws, -1).transpose(2, 3).reshape(b * hf * wf, -1)

    def back(t):
        t = t.reshape(b, hf // ws, wf // ws, ws, ws, -1).transpose(2, 3).reshape(b, hf, wf, -1)
        return torch.roll(t, (shift, shift), (1, 2)).reshape(b * hf * wf, -1)
    ref, bound = ab.window_attention_ref(part(qkv), bias, mask, heads, scale)
    return back(ref), back(bound)


def bag_ref(ids, tables, hot, dense=None):
    """EmbeddingBagOp: ids [B, T] or a list of [B, L_f]; tables fp32 [V_f, D] holding bf16 values (so the
    op's one rounding of the blob is exact); -> (ref, bound) [B, F0 + F, D]."""
    if isinstance(ids, (list, tuple)):
        ids = torch.cat([i.long() for i in ids], 1)
    for t in tables:
        assert torch.equal(t.to(BF).float(), t.float())
    return ib.embag_ref(ids, [t.to(BF) for t in tables], hot, None if dense is None else dense.to(BF))


def tril_order(f, self_interaction):
    """np.tril_indices(f, 0 | -1) spelled out: i ascending, then j ascending, j <= i (j < i)."""
    return [(i, j) for i in range(f) for j in range(f) if (j <= i if self_interaction else j < i)]


def interact_ref(z, dense, self_interaction, pad):
    """DotInteractionOp: [dense | z_i . z_j over tril_order | pad zeros], width Dd + P + pad exactly."""
    k = 0 if self_interaction else -1
    assert ib.tril_pairs(z.shape[1], k) == tril_order(z.shape[1], self_interaction)
    ref, bound = ib.interact_ref(z, dense, k, pad)
    w = dense.shape[1] + len(tril_order(z.shape[1], self_interaction)) + pad
    assert not ref[:, w:].any() and not bound[:, w:].any()
    return ref[:, :w], bound[:, :w]


# ---------------------------------------------------------------- shared cases
# (kh, kw), (n, h, w, c), (sh, sw), padding, pads: a few images of at most 20 x 23, more than one
# strip / block row, odd sizes, C = 8 .. 96 (the 5x5 strip kernel handles 4 channels a thread, the others 8).
def _dw(k, img, s, padding="SAME", pads=(0, 0, 0, 0)):
    return (k, img, s, padding, pads)


DW_EVEN, DW_ODD = (2, 20, 22, 24), (2, 19, 23, 24)
DW_CASES = [_dw(k, img, (s, s)) for k in ((3, 3), (5, 5), (7, 7), (3, 5)) for img in (DW_EVEN, DW_ODD) for s in (1, 2)]
DW_CASES += [_dw(k, DW_ODD, (1, 1), "VALID") for k in ((3, 3), (5, 5), (7, 7), (3, 5))]
DW_CASES += [_dw(k, (3, 9, 11, 96), (s, s), "EXPLICIT", (2, 0, 1, 3)) for k in ((3, 3), (5, 5), (3, 5)) for s in (1, 2)]
DW_CASES += [_dw((3, 3), (3, 9, 11, 96), (s, s), "EXPLICIT", (2, 0, 1, 2)) for s in (1, 2)]      # the strip kernel
DW_CASES += [_dw(k, DW_EVEN, (1, 2)) for k in ((3, 3), (5, 5), (3, 5))]
DW_CASES += [_dw((7, 7), (3, 4, 5, 8), (1, 1)), _dw((5, 5), (3, 2, 3, 8), (2, 2)), _dw((3, 3), (3, 2, 2, 40), (1, 1))]


def dw_case_id(case):
    (kh, kw), (n, h, w, c), (sh, sw), padding, pads = case
    return f"{kh}x{kw}-{n}x{h}x{w}x{c}-s{sh}{sw}-{padding.lower()}" + ("".join(map(str, pads)) if any(pads) else "")


def dw_kernel(case):
    """Which kernel FusedDepthwiseConv launches: the tuned_choice key's first element, None = the generic one."""
    (kh, kw), _img, (sh, sw), _p, _pads = case
    if sh == sw and sh in (1, 2) and (kh, kw) in ((3, 3), (5, 5)):
        return "dwconv" if kh == 3 else "dwconv5x5"
    return None


def dw_padding_only_tail(case):
    """The last window starts beyond the image (a bottom / right pad as large as the filter): TF computes
    act(bias) there; kernels/dwconv.hip's binding refuses the launch."""
    (kh, kw), (_n, h, w, _c), (sh, sw), padding, pads = case
    p = tf_pads(h, w, kh, kw, sh, sw, padding, pads)
    ho, wo = out_hw(h, w, kh, kw, sh, sw, p)
    return (ho - 1) * sh - p[0] >= h or (wo - 1) * sw - p[2] >= w


def dw_case_inputs(case):
    """x bf16-valued fp32 NHWC, an fp32 HWC filter (NOT bf16-valued: the op keeps it fp32), an fp32 bias.
    The pre-activations spread over about +-5: both clamps of relu6 / hard-swish and swish's tail."""
    (kh, kw), (n, h, w, c), _s, _p, _pads = case
    seed = 100 * kh + 10 * kw + h + c
    x = rnd(n, h, w, c, scale=2.0, seed=seed).to(BF).float()
    wt = rnd(kh, kw, c, scale=2.0 / math.sqrt(kh * kw), seed=seed + 1)
    return x, wt, rnd(c, scale=1.5, seed=seed + 2)


# (n, h, w, c), padding, pads
DWLN_CASES = [((2, 9, 11, 96), "SAME", (0, 0, 0, 0)), ((3, 4, 4, 40), "SAME", (0, 0, 0, 0)),
              ((3, 2, 2, 8), "SAME", (0, 0, 0, 0)), ((2, 9, 8, 24), "VALID", (0, 0, 0, 0)),
              ((2, 5, 6, 16), "EXPLICIT", (2, 4, 5, 0)), ((2, 5, 6, 16), "EXPLICIT", (0, 7, 2, 1))]


def dwln_case_id(case):
    return "x".join(map(str, case[0])) + "-" + case[1].lower() + ("".join(map(str, case[2])) if any(case[2]) else "")


def dwln_padding_only_tail(case):
    (n, h, w, c), padding, pads = case
    return dw_padding_only_tail(((7, 7), (n, h, w, c), (1, 1), padding, pads))


def dwln_case_inputs(case, scalar=False):
    (n, h, w, c), _p, _pads = case
    x = rnd(n, h, w, c, seed=h + c).to(BF).float()
    wt = rnd(7, 7, c, scale=1 / 7, seed=h + c + 1)
    b = rnd(c, scale=0.5, seed=h + c + 2)
    if scalar:
        return x, wt, b, torch.tensor([1.25]), torch.tensor([-0.375])
    return x, wt, b, 1 + rnd(c, scale=0.3, seed=h + c + 3), rnd(c, scale=0.3, seed=h + c + 4)


# (batch, (h, w), c)
PATCH_CASES = [(3, (2, 3), 8), (2, (3, 5), 40), (1, (1, 1), 96)]


def patch_case_inputs(case, pos_rank):
    b, (h, w), c = case
    x = rnd(b, h, w, c, seed=c).to(BF).float()
    cls = rnd(1, 1, c, seed=c + 1)
    pos = rnd(h * w + 1, c, scale=0.5, seed=c + 2)
    return x, cls, pos if pos_rank == 2 else pos[None]


# (windows or images, heads, S, nW, grid): S = 49 and 36 (no multiple of 16), H = 3, one and several images
WATTN_CASES = [(4, 3, 49, None, None), (6, 3, 49, 3, None), (6, 2, 36, 2, None),
               (2, 3, 49, None, (14, 21, 7, 0)), (2, 3, 49, 6, (14, 21, 7, 3)), (1, 2, 36, 6, (12, 18, 6, 2)),
               (3, 2, 16, 4, (8, 8, 4, 1))]


def wattn_case_inputs(case, dh=32):
    n, heads, s, nw, grid = case
    rows = n * s if grid is None else n * grid[0] * grid[1]
    return ab.inputs(rows, heads, s, nw, seed=s + heads, dh=dh)


# (vocab, hot, d): tables of different V, hotness mixes with 1
BAG_TABLES = [((5, 9, 3), (2, 1, 3), 16), ((4, 7), (1, 1), 8), ((6, 11, 2, 8), (4, 1, 1, 2), 40)]
BAG_BATCHES = (1, 3, 65)


def bag_case_inputs(vocab, hot, d, b, dtype=torch.int64, lead=False):
    ids, tables = ib.embag_inputs(b, vocab, hot, d, seed=b + d)
    dense = rnd(b, d, seed=b + d + 1).to(BF).float() if lead else None
    return ids.to(dtype), [t.float() for t in tables], dense


INTERACT_F, INTERACT_D, INTERACT_DD = (2, 17, 27), (32, 128), 16


def interact_pads(f, self_interaction):
    """0 and the smallest pad > 0 that leaves Dd + P + pad short of the kernel's ceil8 width."""
    w = INTERACT_DD + len(tril_order(f, self_interaction))
    return (0, next(p for p in range(1, 9) if (w + p) % 8))


def interact_case_inputs(b, f, d, dd=INTERACT_DD):
    z = rnd(b, f, d, seed=f + d).to(BF)
    return z, rnd(b, dd, seed=f + d + 1).to(BF)
