"""``_FusedGroupedConv2D`` on the device, reached through the passes.

Graphs of ``[Pad ->] Conv2D (grouped) -> FusedBatchNormV3 -> Relu`` are
compiled with default_passes() on the GPU and run once.  A kernel shape is
compared, element by element, with the fp64 value of the operands the kernel is
given -- the BatchNorm folded in fp32 as the pass folds it, the filter then
rounded to bf16, the request rounded to bf16 -- under gconv_bounds' bound.  A
shape the kernel does not take, and any shape under TFSERVE_GCONV=0, runs
torch's grouped conv on the device in fp32 and stores bf16: the library's
algorithm is opaque (direct, Winograd or a GEMM), so its fp32 error gets
2^-16 of mag -- 512 fp32 roundings, 1/256 of a bf16 ulp of mag -- in place of
the kernel's K-slot count, and the one bf16 store its usual 2^-8."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import gconv_bounds as gb  # noqa: E402
import kernel_bounds as kb  # noqa: E402
from kernel_bounds import BF  # noqa: E402
from rust_tensorflow_serving2_amd.graph.builder import DType, GraphBuilder  # noqa: E402
from rust_tensorflow_serving2_amd.ops import hip  # noqa: E402
from rust_tensorflow_serving2_amd.utils import tensors as T  # noqa: E402

DEV = torch.device("cuda:0")
F32 = DType(T.DT_FLOAT)
EPS = 1e-3
HW = (13, 18)


def build(c, cg, cout, stride, pad_node, k=3, seed=0):
    """(graph, x, folded fp32 filter, folded bias, pads)."""
    rng = np.random.default_rng(seed)
    g = GraphBuilder()
    x = g.placeholder("x", T.DT_FLOAT, [-1, HW[0], HW[1], c])
    y = x
    p = k // 2
    if pad_node:
        pv = g.const("paddings", np.array([[0, 0], [p, p], [p, p], [0, 0]], np.int32))
        y = g.node("Pad", "pad", [y, pv], T=F32, Tpaddings=DType(T.DT_INT32))
    wv = (rng.standard_normal((k, k, cg, cout)) * (k * k * cg) ** -0.5).astype(np.float32)
    w = g.const("w", wv)
    y = g.node("Conv2D", "conv", [y, w], T=F32, strides=[1, stride, stride, 1], padding="VALID" if pad_node else "SAME",
               data_format="NHWC", dilations=[1, 1, 1, 1], use_cudnn_on_gpu=True, explicit_paddings=[])
    bn = {name: v.astype(np.float32) for name, v in (
        ("gamma", 1 + 0.1 * rng.standard_normal(cout)), ("beta", 0.3 + 0.1 * rng.standard_normal(cout)),
        ("mean", 0.1 * rng.standard_normal(cout)), ("var", 1 + 0.1 * np.abs(rng.standard_normal(cout))))}
    y = g.node("FusedBatchNormV3", "bn", [y] + [g.const(name, v) for name, v in bn.items()], T=F32, U=F32,
               epsilon=EPS, data_format="NHWC", is_training=False, exponential_avg_factor=1.0)
    g.node("Relu", "out", [y], T=F32)
    # the fold of fuse_grouped_conv / _bn_affine, in fp32
    t = {name: torch.from_numpy(v) for name, v in bn.items()}
    scale = t["gamma"] * torch.rsqrt(t["var"] + EPS)
    shift = t["beta"] - t["mean"] * scale
    xin = torch.from_numpy(rng.standard_normal((3, HW[0], HW[1], c)).astype(np.float32))
    if pad_node:
        pads = (p, p, p, p)
    else:
        from rust_tensorflow_serving2_amd.graph.ops import tf_same_pads
        pads = tf_same_pads(HW[0], k, stride) + tf_same_pads(HW[1], k, stride)
    return g, xin, torch.from_numpy(wv) * scale, torch.zeros(cout) * scale + shift, pads


def compiled(g, passes=True):
    from rust_tensorflow_serving2_amd.graph.compiler import compile_program
    from rust_tensorflow_serving2_amd.graph.fused import default_passes
    from rust_tensorflow_serving2_amd.graph.ir import from_graph_def
    if not passes:
        return compile_program(from_graph_def(g.graph), ["x:0"], ["out:0"])
    return compile_program(from_graph_def(g.graph), ["x:0"], ["out:0"], device=DEV, passes=default_passes())


class Spy:
    def __init__(self, monkeypatch):
        self.calls = 0
        self.real = hip().gconv2d
        monkeypatch.setattr(hip(), "gconv2d", self)

    def __call__(self, *a, **k):
        self.calls += 1
        return self.real(*a, **k)


@pytest.mark.parametrize("cg,c", [(4, 32), (8, 96), (16, 48), (32, 64)])
@pytest.mark.parametrize("stride,pad_node", [(1, False), (2, False), (2, True)])
def test_fused_grouped_conv_within_bound(monkeypatch, cg, c, stride, pad_node):
    g, x, wf, bf, pads = build(c, cg, c, stride, pad_node, seed=cg + stride)
    prog = compiled(g)
    hist = prog.op_histogram()
    assert hist.get("_FusedGroupedConv2D") == 1, hist
    for op in ("Conv2D", "FusedBatchNormV3", "Relu", "Pad", "_FusedConv2D"):
        assert op not in hist, hist
    spy = Spy(monkeypatch)
    y = prog.run([x.to(DEV)])[0]
    torch.cuda.synchronize()
    assert spy.calls == 1 and y.is_cuda and y.dtype == BF
    ref, bound = gb.gconv_ref(x.to(BF), wf.to(BF), bf, stride, pads, "relu")
    kb.assert_within(y, ref, bound, f"_FusedGroupedConv2D Cg {cg} C {c} s{stride} pad node {pad_node}")


def torch_path_bound(x, wf, bf, stride, pads):
    pre, mag = gb.gconv_parts(x, wf, bf, stride, pads)
    ref = torch.relu(pre)
    return ref, kb.out_bound(ref, 2.0 ** -16 * mag, out_f32=False)


@pytest.mark.parametrize("c,cg,cout,k", [(128, 64, 128, 3), (32, 4, 16, 3), (32, 4, 32, 5)],
                         ids=["cg64", "unequal_widths", "5x5"])
def test_unsupported_shapes_take_the_torch_path(monkeypatch, c, cg, cout, k):
    g, x, wf, bf, pads = build(c, cg, cout, 1, False, k=k, seed=9)
    prog = compiled(g)
    assert prog.op_histogram().get("_FusedGroupedConv2D") == 1
    spy = Spy(monkeypatch)
    y = prog.run([x.to(DEV)])[0]
    torch.cuda.synchronize()
    assert spy.calls == 0 and y.is_cuda and y.dtype == BF
    ref, bound = torch_path_bound(x, wf, bf, 1, pads)
    kb.assert_within(y, ref, bound, f"torch path C {c} Cg {cg} Cout {cout} {k}x{k}")
    # and the fp32 interpreter of the original graph, to bf16 accuracy
    interp = torch.as_tensor(compiled(g, passes=False).run([x])[0])
    kb.assert_within(interp, ref, 2.0 ** -16 * gb.gconv_parts(x, wf, bf, 1, pads)[1], "interpreter")


def test_tfserve_gconv_0_gives_the_torch_path(monkeypatch):
    g, x, wf, bf, pads = build(32, 4, 32, 1, False, seed=11)
    prog = compiled(g)
    spy = Spy(monkeypatch)
    monkeypatch.setenv("TFSERVE_GCONV", "0")
    y = prog.run([x.to(DEV)])[0]
    torch.cuda.synchronize()
    assert spy.calls == 0 and y.is_cuda and y.dtype == BF
    # (this op was built for the kernel: its filter is the bf16 one the kernel reads; the request stays fp32)
    ref, bound = torch_path_bound(x, wf.to(BF), bf, 1, pads)
    kb.assert_within(y, ref, bound, "TFSERVE_GCONV=0")
    monkeypatch.delenv("TFSERVE_GCONV")
    prog.run([x.to(DEV)])
    assert spy.calls == 1
