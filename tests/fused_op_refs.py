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

The case lists at the bottom are shared by test_fused_ops_cpu.py (an ideal fp32
emulation stays inside the bound, each mutant is rejected) and
test_fused_ops_gpu.py (the op classes on the kernels)."""
import math

import torch
import torch.nn.functional as F

import kernel_bounds as kb
from kernel_bounds import BF, rnd


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
