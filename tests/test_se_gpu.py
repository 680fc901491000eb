"""The squeeze-excite kernels (kernels/se.hip) under their elementwise bounds.

fp64 references and bounds from se_bounds.py (docs/numerics.md, "Hard-swish and
squeeze-excite"); EVERY output element is checked and every output buffer is
pre-filled with NaN.  The shapes are the smallest at which the kernels can go
wrong: one chunk, odd H W with a batch stride, lane groups that do not divide
256, the long pooling loop, V3's widest block (the pooled vector spans all
waves, FC2 has more outputs than threads), more images than one XCD round, and
the limits C = 2048, Cr = 512.  Inputs are scaled so that the gate
pre-activations are ~ N(0, 3^2): both clamps of the hard-sigmoid are occupied,
asserted on the reference."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import kernel_bounds as kb  # noqa: E402
import se_bounds as sb  # noqa: E402
from kernel_bounds import BF, rnd  # noqa: E402
from rust_tensorflow_serving2_amd.ops import ACT, hip  # noqa: E402

DEV = torch.device("cuda:0")
HSIG = ACT["hard_sigmoid"]

# (B, H, W, C, Cr)
GATE_SHAPES = [(1, 1, 1, 8, 8), (3, 7, 5, 24, 8), (2, 14, 14, 72, 24), (1, 28, 28, 120, 32), (2, 7, 7, 960, 240),
               (33, 4, 4, 16, 8), (2, 3, 3, 2048, 512)]
SCALE_SHAPES = [(1, 1, 1, 8), (2, 7, 5, 24), (3, 14, 14, 72), (2, 33, 33, 136)]


@functools.lru_cache(maxsize=None)
def gate_case(shape, act1):
    ins = sb.se_inputs(*shape, act1=act1, seed=GATE_SHAPES.index(shape) * 10)
    ref, bound, pre2 = sb.se_gate_parts(*ins, act1)
    return tuple(t.to(DEV) for t in ins), ref, bound, pre2


def run_gate(ins, act1, x=None):
    b, c = ins[0].shape[0], ins[0].shape[3]
    out = torch.full((b, c), float("nan"), device=DEV)
    g = hip().se_gate(ins[0] if x is None else x, *ins[1:], ACT[act1], HSIG, out)
    assert g.data_ptr() == out.data_ptr()
    return g


@pytest.mark.parametrize("act1", ["relu", "none"])
@pytest.mark.parametrize("shape", GATE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_se_gate_within_bound(shape, act1):
    ins, ref, bound, pre2 = gate_case(shape, act1)
    if pre2.numel() >= 64:
        # both clamps occupied (the 8 gates of the smallest shape cannot promise it)
        assert (pre2 < -3).any() and (pre2 > 3).any() and ((pre2 > -3) & (pre2 < 3)).any()
    worst = kb.assert_within(run_gate(ins, act1), ref, bound, f"se_gate {shape} {act1}")
    print(f"se_gate {shape} {act1}: worst err / bound = {worst:.3f}")


@pytest.mark.parametrize("shape", [(3, 7, 5, 24, 8), (2, 7, 7, 960, 240), (33, 4, 4, 16, 8)],
                         ids=lambda s: "x".join(map(str, s)))
def test_se_gate_inf_pixel_stays_in_its_image(shape):
    """+Inf in one pixel of image 0: the gates of the other images are finite
    and within the bound (a workgroup reads its own image only, and a lane
    past the last pixel is masked by a select, not by a product with 0)."""
    ins, ref, bound, _pre2 = gate_case(shape, "relu")
    xi = ins[0].clone()
    xi[0, 0, 0, :] = float("inf")
    g = run_gate(ins, "relu", x=xi)
    assert torch.isfinite(g[1:]).all()
    kb.assert_within(g[1:], ref[1:], bound[1:], f"se_gate inf {shape}")
    # the last pixel of the last image too: the clamped reads of dead lanes land on it
    xl = ins[0].clone()
    xl[-1, -1, -1, :] = float("inf")
    g = run_gate(ins, "relu", x=xl)
    assert torch.isfinite(g[:-1]).all()
    kb.assert_within(g[:-1], ref[:-1], bound[:-1], f"se_gate inf in the last pixel {shape}")


@pytest.mark.parametrize("shape", [(3, 7, 5, 24, 8), (2, 7, 7, 960, 240)], ids=lambda s: "x".join(map(str, s)))
def test_se_gate_is_deterministic(shape):
    ins, _ref, _bound, _pre2 = gate_case(shape, "relu")
    a, b = run_gate(ins, "relu"), run_gate(ins, "relu")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_se_gate_binding_rejects_what_the_kernel_does_not_take():
    def call(c=16, cr=8, act1=1, gate_act=HSIG, **over):
        t = dict(x=torch.zeros(2, 3, 3, c, dtype=BF, device=DEV), w1=torch.zeros(c, cr, device=DEV),
                 b1=torch.zeros(cr, device=DEV), w2=torch.zeros(cr, c, device=DEV), b2=torch.zeros(c, device=DEV))
        t.update(over)
        return hip().se_gate(t["x"], t["w1"], t["b1"], t["w2"], t["b2"], act1, gate_act)
    g = call()
    assert g.shape == (2, 16) and g.dtype == torch.float32 and torch.equal(g.cpu(), torch.full((2, 16), 0.5))
    assert hip().se_gate_supported(2, 9, 16, 8) and hip().se_gate_supported(1, 1, 2048, 512)
    assert not hip().se_gate_supported(2, 9, 12, 8) and not hip().se_gate_supported(2, 9, 2056, 8)
    assert not hip().se_gate_supported(2, 9, 16, 520) and not hip().se_gate_supported(2, 0, 16, 8)
    with pytest.raises(RuntimeError, match="C % 8"):
        call(c=12)
    with pytest.raises(RuntimeError, match="2048"):
        call(c=2056)
    with pytest.raises(RuntimeError, match="512"):
        call(cr=520)
    for gate_act in (0, 1, 5, 7, -1):
        with pytest.raises(RuntimeError, match="gate_act"):
            call(gate_act=gate_act)
    for act1 in (5, 2, 6, 7):
        with pytest.raises(RuntimeError, match="act1"):
            call(act1=act1)
    with pytest.raises(RuntimeError, match="w1"):
        call(w1=torch.zeros(8, 16, device=DEV))
    with pytest.raises(RuntimeError, match="w2"):
        call(w2=torch.zeros(16, 8, device=DEV))
    with pytest.raises(RuntimeError, match="b1"):
        call(b1=torch.zeros(16, device=DEV))
    with pytest.raises(RuntimeError, match="b2"):
        call(b2=torch.zeros(8, device=DEV))
    with pytest.raises(RuntimeError, match="dtype"):
        call(w1=torch.zeros(16, 8, device=DEV, dtype=BF))
    with pytest.raises(RuntimeError, match="dtype"):
        call(x=torch.zeros(2, 3, 3, 16, device=DEV))
    with pytest.raises(RuntimeError, match="empty image"):
        call(x=torch.zeros(2, 0, 3, 16, dtype=BF, device=DEV))


# ---------------------------------------------------------------- se_scale
@pytest.mark.parametrize("shape", SCALE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_se_scale_within_bound(shape):
    b, h, w, c = shape
    seed = 300 + SCALE_SHAPES.index(shape) * 10
    x = rnd(*shape, scale=3.0, seed=seed).to(BF)
    gate = torch.rand(b, c, generator=torch.Generator().manual_seed(seed + 1))
    gate[:, 0], gate[:, -1] = 0.0, 1.0                 # exact 0 and exact 1
    ref, bound = sb.se_scale_ref(x, gate)
    out = torch.full(shape, float("nan"), dtype=BF, device=DEV)
    y = hip().se_scale(x.to(DEV), gate.to(DEV), out)
    assert y.data_ptr() == out.data_ptr()
    worst = kb.assert_within(y, ref, bound, f"se_scale {shape}")
    print(f"se_scale {shape}: worst err / bound = {worst:.3f}")
    yc = y.float().cpu()
    assert torch.equal(yc[..., -1], x.float()[..., -1]) and (yc[..., 0] == 0).all()
    a2 = hip().se_scale(x.to(DEV), gate.to(DEV))
    assert torch.equal(a2.view(torch.int16), y.view(torch.int16))


def test_se_scale_inf_pixel():
    """An Inf pixel stays in its own elements: Inf times a gate in (0, 1] is Inf,
    and Inf times the gate 0 is NaN by IEEE 754 -- which is the reference's
    value too (torch's fp64 product gives the same NaN), so it is asserted as
    such; every other element is finite and within the bound."""
    shape = (2, 7, 5, 24)
    x = rnd(*shape, scale=3.0, seed=401).to(BF)
    gate = torch.rand(2, 24, generator=torch.Generator().manual_seed(402))
    gate[:, 0] = 0.0
    x[0, 3, 2, :] = float("inf")
    y = hip().se_scale(x.to(DEV), gate.to(DEV)).float().cpu()
    ref64 = kb.d(x) * kb.d(gate)[:, None, None, :]
    assert torch.isnan(ref64[0, 3, 2, 0]) and torch.isnan(y[0, 3, 2, 0])
    assert torch.isinf(y[0, 3, 2, 1:]).all()
    clean = torch.ones(shape, dtype=torch.bool)
    clean[0, 3, 2, :] = False
    x0 = x.clone()
    x0[0, 3, 2, :] = 0.0
    ref, bound = sb.se_scale_ref(x0, gate)
    assert torch.isfinite(y[clean]).all()
    kb.assert_within(y[clean], ref[clean], bound[clean], "se_scale around an Inf pixel")


def test_se_scale_binding_rejects_what_the_kernel_does_not_take():
    x = torch.zeros(2, 3, 3, 16, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="C % 8"):
        hip().se_scale(torch.zeros(2, 3, 3, 12, dtype=BF, device=DEV), torch.zeros(2, 12, device=DEV))
    with pytest.raises(RuntimeError, match="gate"):
        hip().se_scale(x, torch.zeros(2, 8, device=DEV))
    with pytest.raises(RuntimeError, match="dtype"):
        hip().se_scale(x, torch.zeros(2, 16, device=DEV, dtype=BF))


# ---------------------------------------------------------------- the op
@pytest.mark.parametrize("shape", [(3, 7, 5, 24, 8), (2, 7, 7, 960, 240)], ids=lambda s: "x".join(map(str, s)))
def test_squeeze_excite_op_within_bound(shape):
    """graph/fused.py SqueezeExcite from fp32 parameters, HIP path (se_gate then
    se_scale) against the op bound; and an x the kernels do not take (C % 8
    != 0) goes down the torch path instead of raising."""
    from rust_tensorflow_serving2_amd.graph.fused import SqueezeExcite
    ins, _ref, _bound, _pre2 = gate_case(shape, "relu")
    x, w1, b1, w2, b2 = ins
    op = SqueezeExcite(w1.cpu(), b1.cpu(), w2.cpu(), b2.cpu(), "relu", 1.0 / 6.0, True, (1, 2), None, DEV, True, "se")
    assert op.w1.dtype == torch.float32 and op.w2.dtype == torch.float32
    (y,) = op(None, None, [x])
    assert y.dtype == BF and y.is_cuda
    ref, bound = sb.se_op_ref(*ins, "relu")
    worst = kb.assert_within(y, ref, bound, f"SqueezeExcite {shape}")
    print(f"SqueezeExcite {shape}: worst err / bound = {worst:.3f}")


def test_squeeze_excite_op_torch_path_outside_the_limits():
    from rust_tensorflow_serving2_amd.graph.fused import SqueezeExcite
    x, w1, b1, w2, b2 = sb.se_inputs(2, 3, 3, 12, 4, seed=77)
    op = SqueezeExcite(w1, b1, w2, b2, "relu", 1.0 / 6.0, True, (1, 2), None, DEV, True, "se")
    (y,) = op(None, None, [x.to(DEV)])
    ref, _ = sb.se_op_ref(x, w1, b1, w2, b2, "relu")
    assert y.shape == x.shape
    torch.testing.assert_close(y.float().cpu().double(), ref, atol=2e-2, rtol=2e-2)
