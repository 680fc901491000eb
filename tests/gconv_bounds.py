"""fp64 reference and elementwise bound for the grouped conv kernel (a helper
module like dwconv_bounds, built on kernel_bounds; docs/numerics.md, "Grouped
conv", has the derivation in prose).

kernels/gconv.hip computes every output as ONE chain of
v_mfma_f32_16x16x32_bf16 into one fp32 accumulator that starts at zero: bf16 x
bf16 products are exact in fp32, so the only roundings are the accumulator's,
one per K slot in whatever order the matrix core adds them.  The kernel's K
runs over (tap, channel) and is rounded up to whole 32-deep MFMA steps,

    k_slots(Cg) = 32 * ceil(9 Cg / 32)       (gconv.hip KS = gconv_ksteps(CG):
                                              64, 96, 160, 288 for Cg = 4, 8, 16, 32)

with the slots past 9 Cg zero in both operands: they add nothing to
mag = sum |x| |w| + |bias| but they are additions the hardware performs, so
they count.  Then the bias is added (one fp32 addition), the activation (none
or ReLU: exact) applied, and the value stored with one round-to-nearest-even
to bf16: kernel_bounds.epilogue(pre, mag, k_slots, splits=1, act), whose
(K + splits + 4) E mag already has the room for the bias addition.
"""
import torch.nn.functional as F

from kernel_bounds import d, epilogue


def k_slots(cg):
    return 32 * ((9 * cg + 31) // 32)


def gconv_parts(x, w_hwio, bias, stride, pads):
    """NHWC x, w [3][3][Cg][C] (HWIO with in-depth C / groups), bias [C], pads
    (top, bottom, left, right) -> (pre, mag), NHWC fp64, on the exactly upcast
    operands (mag: the same conv on |x|, |w|, plus |bias|)."""
    pt, pb, pl, pr = pads
    x, w, bias = d(x), d(w_hwio), d(bias)
    groups = x.shape[3] // w.shape[2]

    def conv(xx, ww):
        return F.conv2d(F.pad(xx.permute(0, 3, 1, 2), [pl, pr, pt, pb]), ww.permute(3, 2, 0, 1), stride=stride,
                        groups=groups).permute(0, 2, 3, 1)
    return conv(x, w) + bias, conv(x.abs(), w.abs()) + bias.abs()


def gconv_ref(x, w_hwio, bias, stride, pads, act):
    """(ref, bound) of gconv2d."""
    pre, mag = gconv_parts(x, w_hwio, bias, stride, pads)
    return epilogue(pre, mag, k_slots(w_hwio.shape[2]), splits=1, act=act)
