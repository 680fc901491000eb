"""fp64 references and elementwise bounds for the swish epilogues and the
sigmoid-gated squeeze-excite kernel (a helper module like se_bounds, which it
builds on; docs/numerics.md, "Swish and sigmoid", has the derivations in prose).
E = 2^-23 per fp32 operation, with the house "one spare".

What the kernels emit (kernels/common.h):

    sigmoid(x) = rcp(1 + exp2(x * c)),   c = fp32(-log2 e)
    swish(x)   = x * sigmoid(x)

* the argument t = x c: the rounded constant and the product's rounding are
  1.5 E relative to t, i.e. 1.5 E |t| ln 2 = 1.5 E |x| relative to e = exp2(t);
  v_exp_f32 adds 1 ulp (= E):                      de / e <= (1 + 1.5 |x|) E;
* s = 1 + e, one rounding, and sigma = rcp(s), 1 ulp.  d sigma / d e = -sigma^2,
  so an error of e reaches sigma damped by e sigma = 1 - sigma:
      d sigma <= sigma ((1 - sigma) (1 + 1.5 |x|) + 2) E;
* swish's final product is one more rounding; with one spare
      d sigmoid <= sigma ((1 - sigma) (1 + 1.5 |x|) + 3) E          (sigmoid_own)
      d swish   <= |x| sigma ((1 - sigma) (1 + 1.5 |x|) + 4) E      (swish_own)
  (|x| sigma (1 - sigma) |x| <= 0.9: no term grows with |x| beyond |x| itself);
* the flushed tail: v_rcp_f32 returns 0 where 1 + e >= 2^126 (its result would
  be a denormal), so for x <~ -87.3 sigmoid gives 0 and swish -0 where the true
  values are at most e^-87 = 1.6e-38 and 87 e^-87 = 1.5e-36 < 2^-119.  Both
  bounds carry that absolute floor, FLOOR = 2^-119, everywhere.

Swish is 1.1-Lipschitz (sup |d/dx x sigma(x)| = 1.09984 at x = 2.3994) and the
sigmoid 1/4-Lipschitz, so an error `acc` of the pre-activation gives
1.1 acc + swish_own, and dpre2 / 4 + sigmoid_own for the gate.

se_gate with act1 = swish and a sigmoid gate: se_bounds.se_gate_parts' chain
with  |dh| <= 1.1 |dpre1| + swish_own(pre1)  and
      |dgate| <= |dpre2| / 4 + sigmoid_own(pre2).
"""
import torch

import se_bounds as sb
from kernel_bounds import E, d, out_bound

L_SWISH = 1.1
L_SIGMOID = 0.25
FLOOR = 2.0 ** -119


def sigmoid64(x):
    return torch.sigmoid(x)


def swish64(x):
    return x * torch.sigmoid(x)


def _arg_term(pre):
    s = torch.sigmoid(pre)
    return s, (1.0 - s) * (1.0 + 1.5 * pre.abs())


def sigmoid_own(pre):
    s, arg = _arg_term(pre)
    return s * (arg + 3.0) * E + FLOOR


def swish_own(pre):
    s, arg = _arg_term(pre)
    return pre.abs() * s * (arg + 4.0) * E + FLOOR


def swish_dw(pre, mag, taps):
    """(ref, bound) of dwconv2d with act = swish; pre, mag from dwconv_bounds.dw_parts."""
    ref = swish64(pre)
    return ref, out_bound(ref, L_SWISH * (taps + 2) * E * mag + swish_own(pre), out_f32=False)


def swish_epilogue(pre, mag, k, splits=1, out_f32=False):
    """(ref, bound) of a GEMM / conv epilogue with act = swish."""
    ref = swish64(pre)
    return ref, out_bound(ref, L_SWISH * (k + splits + 4) * E * mag + swish_own(pre), out_f32)


def se_gate_parts(x, w1, b1, w2, b2, act1, gate):
    """se_bounds.se_gate_parts for act1 in none / relu / swish and gate in
    hard_sigmoid / sigmoid -> (gate, dgate, pre2), fp64 [B,C]."""
    assert act1 in ("none", "relu", "swish") and gate in ("hard_sigmoid", "sigmoid"), (act1, gate)
    x, w1, b1, w2, b2 = d(x), d(w1), d(b1), d(w2), d(b2)
    _b, h, w, c = x.shape
    hw, cr = h * w, w1.shape[1]
    p = x.mean(dim=(1, 2))
    dp = (hw + 1) * E * x.abs().mean(dim=(1, 2))
    pre1 = p @ w1 + b1
    dpre1 = dp @ w1.abs() + (c + 2) * E * (p.abs() @ w1.abs() + b1.abs())
    if act1 == "swish":
        hid, dh = swish64(pre1), L_SWISH * dpre1 + swish_own(pre1)
    else:
        hid, dh = sb.act1_64(act1, pre1), dpre1
    pre2 = hid @ w2 + b2
    dpre2 = dh @ w2.abs() + (cr + 2) * E * (hid.abs() @ w2.abs() + b2.abs())
    if gate == "sigmoid":
        return sigmoid64(pre2), L_SIGMOID * dpre2 + sigmoid_own(pre2), pre2
    return sb.hard_sigmoid64(pre2), dpre2 / 6.0 + 3 * E, pre2


def se_op_ref(x, w1, b1, w2, b2, act1, gate):
    """(ref, bound) of the op: se_gate, then se_scale."""
    g, dgate, _pre2 = se_gate_parts(x, w1, b1, w2, b2, act1, gate)
    return sb.se_scale_ref(x, g, dgate)


def se_inputs(b, h, w, c, cr, act1="swish", seed=0):
    """se_bounds.se_inputs; a swish hidden layer has nearly the ReLU's second
    moment at this spread (FC1 pre-activations ~ N(0, 4^2)), so it takes the
    ReLU's scaling: gate pre-activations ~ N(0, 3^2), both sigmoid tails."""
    return sb.se_inputs(b, h, w, c, cr, act1="relu" if act1 == "swish" else act1, seed=seed)


# ---------------------------------------------------------------- fp32 emulations (CPU)
LOG2E_F32 = torch.tensor(-1.4426950408889634, dtype=torch.float32)


def sigmoid_f32(x):
    """common.h sigmoid() step by step in fp32 torch."""
    x = x.float()
    return 1.0 / (1.0 + torch.exp2(x * LOG2E_F32))


def swish_f32(x):
    x = x.float()
    return x * sigmoid_f32(x)
