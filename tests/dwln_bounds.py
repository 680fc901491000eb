"""fp64 reference and elementwise bound for the fused depthwise 7x7 + bias +
LayerNorm kernel (kernels/dwln.hip), from the two existing pieces (a helper
module like dwconv_bounds and kernel_bounds; docs/numerics.md has the
derivation in prose).

The kernel's conv result v stays in fp32: the accumulator starts at the fp32
bias and takes one fp32 FMA per tap, 49 of them, so with mag = sum |x| |w| +
|bias| (dwconv_bounds.dw_parts)

    |v - pre| <= (49 + 2) E mag        (one rounding per FMA, the bias, one spare)

and that is the `dz` of kernel_bounds.layernorm_ref, whose bound covers the
fp32 two-pass statistics, xhat * gamma + beta and the one bf16 store.  There is
NO bf16 rounding of v in it: the unfused pair (dwconv2d's bf16 output, then
layernorm) is off by 2^-9 |v| rstd |gamma| and violates it, which
test_dwln_bounds_cpu.py checks, so that the GPU test cannot pass on a kernel
that rounds in between.
"""
import dwconv_bounds as db
import kernel_bounds as kb

TAPS = 49


def dwln_ref(x, w, bias, gamma, beta, eps, pads):
    """NHWC x (bf16 values), w [7][7][C], bias / gamma / beta [C], pads (top,
    bottom, left, right) -> (ref, bound), NHWC fp64."""
    pre, mag = db.dw_parts(x, w, bias, 1, pads)
    return kb.layernorm_ref(pre, gamma, beta, eps, dz=(TAPS + 2) * kb.E * mag)


SAME = (3, 3, 3, 3)        # TF SAME padding of a 7x7 / stride-1 filter
VALID = (0, 0, 0, 0)


def out_hw(h, w, pads):
    return h + pads[0] + pads[1] - 6, w + pads[2] + pads[3] - 6
