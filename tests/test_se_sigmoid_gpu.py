"""se_gate (kernels/se.hip) with a sigmoid gate and a swish inner activation
under its elementwise bound (swish_bounds.py; docs/numerics.md, "Swish and
sigmoid"): test_se_gpu.py's shapes plus EfficientNet-B0's own (C, Cr) pairs whose
Cr is no multiple of 8.  EVERY gate is checked, every output buffer is
pre-filled with NaN; the gate pre-activations are ~ N(0, 3^2) and reach both
sigmoid tails, asserted on the reference.  Each test prints its worst
error / bound."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import kernel_bounds as kb  # noqa: E402
import swish_bounds as wb  # noqa: E402
from kernel_bounds import BF  # noqa: E402
from rust_tensorflow_serving2_amd.ops import ACT, hip  # noqa: E402

DEV = torch.device("cuda:0")

# (B, H, W, C, Cr): test_se_gpu.GATE_SHAPES, then B0's blocks 2, 3 / 4, 5 and 16
GATE_SHAPES = [(1, 1, 1, 8, 8), (3, 7, 5, 24, 8), (2, 14, 14, 72, 24), (1, 28, 28, 120, 32), (2, 7, 7, 960, 240),
               (33, 4, 4, 16, 8), (2, 3, 3, 2048, 512),
               (2, 4, 4, 96, 4), (2, 4, 4, 144, 6), (2, 2, 2, 240, 10), (2, 1, 1, 1152, 48)]
COMBOS = [("swish", "sigmoid"), ("relu", "sigmoid"), ("none", "sigmoid"), ("swish", "hard_sigmoid")]


@functools.lru_cache(maxsize=None)
def gate_case(shape, act1, gate):
    ins = wb.se_inputs(*shape, act1=act1, seed=GATE_SHAPES.index(shape) * 10 + 2000)
    ref, bound, pre2 = wb.se_gate_parts(*ins, act1, gate)
    return tuple(t.to(DEV) for t in ins), ref, bound, pre2


def run_gate(ins, act1, gate, x=None):
    b, c = ins[0].shape[0], ins[0].shape[3]
    out = torch.full((b, c), float("nan"), device=DEV)
    g = hip().se_gate(ins[0] if x is None else x, *ins[1:], ACT[act1], ACT[gate], out)
    assert g.data_ptr() == out.data_ptr()
    return g


@pytest.mark.parametrize("act1,gate", COMBOS)
@pytest.mark.parametrize("shape", GATE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_se_gate_within_bound(shape, act1, gate):
    ins, ref, bound, pre2 = gate_case(shape, act1, gate)
    if pre2.numel() >= 64:
        # both tails and the middle (the 8 gates of the smallest shape cannot promise it)
        assert (pre2 < -3).any() and (pre2 > 3).any() and ((pre2 > -3) & (pre2 < 3)).any()
    worst = kb.assert_within(run_gate(ins, act1, gate), ref, bound, f"se_gate {shape} {act1} {gate}")
    print(f"se_gate {shape} {act1} {gate}: worst err / bound = {worst:.3f}")


@pytest.mark.parametrize("shape", [(3, 7, 5, 24, 8), (2, 7, 7, 960, 240), (2, 4, 4, 144, 6)],
                         ids=lambda s: "x".join(map(str, s)))
def test_se_gate_inf_pixel_stays_in_its_image(shape):
    ins, ref, bound, _pre2 = gate_case(shape, "swish", "sigmoid")
    xi = ins[0].clone()
    xi[0, 0, 0, :] = float("inf")
    g = run_gate(ins, "swish", "sigmoid", x=xi)
    assert torch.isfinite(g[1:]).all()
    kb.assert_within(g[1:], ref[1:], bound[1:], f"se_gate inf {shape}")
    # the last pixel of the last image too: the clamped reads of dead lanes land on it
    xl = ins[0].clone()
    xl[-1, -1, -1, :] = float("inf")
    g = run_gate(ins, "swish", "sigmoid", x=xl)
    assert torch.isfinite(g[:-1]).all()
    kb.assert_within(g[:-1], ref[:-1], bound[:-1], f"se_gate inf in the last pixel {shape}")


@pytest.mark.parametrize("shape", [(3, 7, 5, 24, 8), (2, 7, 7, 960, 240), (2, 1, 1, 1152, 48)],
                         ids=lambda s: "x".join(map(str, s)))
def test_se_gate_is_deterministic(shape):
    ins, _ref, _bound, _pre2 = gate_case(shape, "swish", "sigmoid")
    a, b = run_gate(ins, "swish", "sigmoid"), run_gate(ins, "swish", "sigmoid")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_se_gate_binding_takes_the_new_codes_and_no_others():
    def call(act1=ACT["swish"], gate_act=ACT["sigmoid"]):
        c, cr = 16, 8
        return hip().se_gate(torch.zeros(2, 3, 3, c, dtype=BF, device=DEV), torch.zeros(c, cr, device=DEV),
                             torch.zeros(cr, device=DEV), torch.zeros(cr, c, device=DEV), torch.zeros(c, device=DEV),
                             act1, gate_act)
    assert torch.equal(call().cpu(), torch.full((2, 16), 0.5))
    assert torch.equal(call(act1=0).cpu(), torch.full((2, 16), 0.5))
    assert torch.equal(call(gate_act=ACT["hard_sigmoid"]).cpu(), torch.full((2, 16), 0.5))
    for gate_act in (9, 0, 1, 5, 7, -1, 10):
        with pytest.raises(RuntimeError, match="gate_act"):
            call(gate_act=gate_act)
    for act1 in (8, 5, 2, 6, 7, 10):
        with pytest.raises(RuntimeError, match="act1"):
            call(act1=act1)


@pytest.mark.parametrize("shape", [(3, 7, 5, 24, 8), (2, 4, 4, 144, 6)], ids=lambda s: "x".join(map(str, s)))
def test_sigmoid_squeeze_excite_op_within_bound(shape):
    """graph/fused.py SqueezeExcite(gate="sigmoid") from fp32 parameters, HIP
    path (se_gate then se_scale) against the op bound."""
    from rust_tensorflow_serving2_amd.graph.fused import SqueezeExcite
    ins, _ref, _bound, _pre2 = gate_case(shape, "swish", "sigmoid")
    x, w1, b1, w2, b2 = ins
    op = SqueezeExcite(w1.cpu(), b1.cpu(), w2.cpu(), b2.cpu(), "swish", 1.0 / 6.0, False, (1, 2), [-1, 1, 1, shape[3]], DEV,
                       True, "se", gate="sigmoid")
    (y,) = op(None, None, [x])
    assert y.dtype == BF and y.is_cuda
    ref, bound = wb.se_op_ref(*ins, "swish", "sigmoid")
    worst = kb.assert_within(y, ref, bound, f"SqueezeExcite sigmoid {shape}")
    print(f"SqueezeExcite sigmoid {shape}: worst err / bound = {worst:.3f}")
