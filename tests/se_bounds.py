"""fp64 references and elementwise bounds for the hard-swish epilogues and the
squeeze-excite kernels (a helper module like kernel_bounds and dwconv_bounds,
which it builds on; docs/numerics.md, "Hard-swish and squeeze-excite", has the
derivations in prose).  E = 2^-23 per fp32 operation, with the house "one
spare".

Hard-swish h(x) = x clamp(x + 3, 0, 6) / 6.  h' = (2x + 3) / 6 on [-3, 3], 0
below and 1 above: Lipschitz 1.5.  The kernels compute it as one add, two
clamps (exact) and two products with the constant 1/6 rounded to fp32: four
roundings of values no larger than 1 + |x| (where the clamp is not reached
|x| |x + 3| / 6 <= 3; elsewhere the result is 0 or x), so its own error is
<= 4 E (1 + |pre|).  Pushed through an accumulation error
`acc` of the pre-activation: 1.5 acc + 4 E (1 + |pre|).

Hard-sigmoid s(x) = clamp(x + 3, 0, 6) / 6: Lipschitz 1/6, values in [0, 1],
three roundings (the add, the product, the constant): <= 3 E absolute.

se_gate (kernels/se.hip), everything fp32, sums in any order:
    p    = (1 / HW) sum x          |dp|    <= (HW + 1) E mean|x|
    pre1 = p w1 + b1               |dpre1| <= |dp| |w1| + (C + 2) E (|p| |w1| + |b1|)
    h    = act1(pre1)              |dh|    <= |dpre1|          (none / relu: exact, 1-Lipschitz)
    pre2 = h w2 + b2               |dpre2| <= |dh| |w2| + (Cr + 2) E (|h| |w2| + |b2|)
    gate = s(pre2)                 |dgate| <= |dpre2| / 6 + 3 E
The gate is stored as fp32: no output rounding.

se_scale: one fp32 product and one round-to-nearest-even store:
out_bound(ref, E |ref|) for the gate it was given; for the op (gate, then
scale) the gate's error comes on top: out_bound(ref, |x| dgate + E |ref|).
"""
import torch

from kernel_bounds import E, d, out_bound

L_HARD_SWISH = 1.5


def hard_sigmoid64(x):
    return torch.clamp(x + 3.0, 0.0, 6.0) / 6.0


def hard_swish64(x):
    return x * hard_sigmoid64(x)


def hard_swish_own(pre):
    return 4 * E * (1.0 + pre.abs())


def hard_swish_dw(pre, mag, taps):
    """(ref, bound) of dwconv2d with act = hard_swish; pre, mag from dwconv_bounds.dw_parts."""
    ref = hard_swish64(pre)
    return ref, out_bound(ref, L_HARD_SWISH * (taps + 2) * E * mag + hard_swish_own(pre), out_f32=False)


def hard_swish_epilogue(pre, mag, k, splits=1, out_f32=False):
    """(ref, bound) of a GEMM / conv epilogue with act = hard_swish."""
    ref = hard_swish64(pre)
    return ref, out_bound(ref, L_HARD_SWISH * (k + splits + 4) * E * mag + hard_swish_own(pre), out_f32)


def act1_64(act1, x):
    assert act1 in ("none", "relu"), act1
    return torch.relu(x) if act1 == "relu" else x


def se_gate_parts(x, w1, b1, w2, b2, act1):
    """x [B,H,W,C] (bf16-valued), w1 [C,Cr], b1 [Cr], w2 [Cr,C], b2 [C] ->
    (gate, dgate, pre2), fp64 [B,C]."""
    x, w1, b1, w2, b2 = d(x), d(w1), d(b1), d(w2), d(b2)
    b, h, w, c = x.shape
    hw, cr = h * w, w1.shape[1]
    p = x.mean(dim=(1, 2))
    dp = (hw + 1) * E * x.abs().mean(dim=(1, 2))
    pre1 = p @ w1 + b1
    dpre1 = dp @ w1.abs() + (c + 2) * E * (p.abs() @ w1.abs() + b1.abs())
    hid = act1_64(act1, pre1)
    pre2 = hid @ w2 + b2
    dpre2 = dpre1 @ w2.abs() + (cr + 2) * E * (hid.abs() @ w2.abs() + b2.abs())
    return hard_sigmoid64(pre2), dpre2 / 6.0 + 3 * E, pre2


def se_gate_ref(x, w1, b1, w2, b2, act1):
    """(ref, bound) of se_gate."""
    gate, dgate, _pre2 = se_gate_parts(x, w1, b1, w2, b2, act1)
    return gate, dgate


def se_scale_ref(x, gate, dgate=None):
    """(ref, bound) of se_scale for the fp32 gate it is given (dgate: the
    gate's own error, for the op)."""
    x, gate = d(x), d(gate)
    ref = x * gate[:, None, None, :]
    acc = E * ref.abs()
    if dgate is not None:
        acc = acc + x.abs() * d(dgate)[:, None, None, :]
    return ref, out_bound(ref, acc, out_f32=False)


def se_op_ref(x, w1, b1, w2, b2, act1):
    """(ref, bound) of the op: se_gate, then se_scale."""
    gate, dgate = se_gate_ref(x, w1, b1, w2, b2, act1)
    return se_scale_ref(x, gate, dgate)


def se_inputs(b, h, w, c, cr, act1="relu", seed=0):
    """x (bf16), w1, b1, w2, b2 (fp32) with pooled values ~ N(0, 1), FC1
    pre-activations ~ N(0, 4^2) (so a ReLU6 in place of the ReLU shows) and
    gate pre-activations ~ N(0, 3^2): about 16 % of the gates clamp on each side."""
    from kernel_bounds import BF, rnd
    x = (rnd(b, h, w, c, seed=seed + 1) + rnd(b, 1, 1, c, seed=seed + 2)).to(BF)
    w1 = rnd(c, cr, scale=4.0 / c ** 0.5, seed=seed + 3)
    b1 = rnd(cr, scale=0.3, seed=seed + 4)
    second = 16.0 * (0.5 if act1 == "relu" else 1.0)           # E[h^2]
    w2 = rnd(cr, c, scale=3.0 / (second * cr) ** 0.5, seed=seed + 5)
    b2 = rnd(c, scale=0.3, seed=seed + 6)
    return x, w1, b1, w2, b2
