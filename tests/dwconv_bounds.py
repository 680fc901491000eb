"""fp64 references and elementwise bounds for the depthwise conv kernel and the
ReLU6 epilogues (a helper module like kernel_bounds, which it builds on;
docs/numerics.md has the derivations in prose).

Depthwise (kernels/dwconv.hip): the accumulator starts at the fp32 bias and
takes one fp32 FMA per tap, KH KW of them, each rounded once; then the
activation and one round-to-nearest-even store to bf16.  With
mag = sum |x| |w| + |bias| the fp32 value is off by at most

    (KH KW + 2) E mag        (one rounding per FMA, the bias, one spare)

and the store adds 2^-8 of the result: out_bound(ref, (KH KW + 2) E mag).
ReLU and ReLU6 are exact and 1-Lipschitz, and 0 and 6 are bf16 numbers, so the
clamp commutes with the output rounding and adds nothing.

GEMM / conv ReLU6: the same argument on top of acc_bound(..., act="relu").
"""
import torch
import torch.nn.functional as F

from kernel_bounds import E, acc_bound, act64, d, out_bound


def act64x(act, x):
    if act == "relu6":
        return torch.clamp(x, 0.0, 6.0)
    return act64(act, x)


def dw_parts(x, w, bias, stride, pads):
    """NHWC x, w [KH][KW][C], bias [C], stride int or (sh, sw), pads (top,
    bottom, left, right) -> (pre, mag), NHWC fp64, on the exactly upcast
    operands (mag: the same conv on |x|, |w|, plus |bias|)."""
    pt, pb, pl, pr = pads
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    x, w, bias = d(x), d(w), d(bias)
    kh, kw, c = w.shape

    def conv(xx, ww):
        wt = ww.permute(2, 0, 1).reshape(c, 1, kh, kw)
        return F.conv2d(F.pad(xx.permute(0, 3, 1, 2), [pl, pr, pt, pb]), wt, stride=(sh, sw),
                        groups=c).permute(0, 2, 3, 1)
    return conv(x, w) + bias, conv(x.abs(), w.abs()) + bias.abs()


def dw_ref(x, w, bias, stride, pads, act):
    """(ref, bound) of dwconv2d."""
    pre, mag = dw_parts(x, w, bias, stride, pads)
    taps = w.shape[0] * w.shape[1]
    ref = act64x(act, pre)
    return ref, out_bound(ref, (taps + 2) * E * mag, out_f32=False)


def relu6_epilogue(pre, mag, k, splits=1, out_f32=False):
    """(ref, bound) of a GEMM / conv epilogue with act = relu6."""
    ref = torch.clamp(pre, 0.0, 6.0)
    return ref, out_bound(ref, acc_bound(pre, mag, k, splits, "relu"), out_f32)
