"""MobileNet V1 / V2 through the fusion passes on the CPU: the fused graph (fp32
reference of the fused ops, same folded parameters the HIP kernels use) ==
the unfused reference interpreter, every depthwise conv, BatchNorm and ReLU6 is
absorbed, and the depthwise convs the pass must leave alone are left alone."""
import os

import numpy as np
import pytest
import torch

from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions

OUTS = ["classes", "probabilities"]
GONE = ("DepthwiseConv2dNative", "Relu6", "FusedBatchNorm", "FusedBatchNormV2", "FusedBatchNormV3", "Conv2D", "Pad",
        "AddV2")


def _pair(path):
    return (Servable("m", 1, path, ServableOptions(device="cpu")),
            Servable("m", 1, path, ServableOptions(device="cpu", fuse=True)))


@pytest.fixture(scope="module", params=["v1", "v2"])
def tiny_mobilenet(request, models_dir):
    from rust_tensorflow_serving2_amd.models import mobilenet
    path = os.path.join(str(models_dir), f"tiny_mobilenet_{request.param}", "1")
    mobilenet.export(path, version=request.param, alpha=0.25, image_size=32, num_classes=11, seed=5)
    ref, fused = _pair(path)
    hist = fused.runner("serving_default", ["input"], OUTS).program.op_histogram()
    return request.param, ref, fused, hist


def test_mobilenet_fused_matches_interpreter(tiny_mobilenet):
    _version, ref, fused, _hist = tiny_mobilenet
    x = np.random.default_rng(0).random((3, 32, 32, 3), dtype=np.float32)
    a = ref.run("serving_default", {"input": x}, OUTS)
    b = fused.run("serving_default", {"input": x}, OUTS)
    assert a["probabilities"].shape == (3, 11)
    np.testing.assert_allclose(a["probabilities"], b["probabilities"], atol=1e-5)
    np.testing.assert_array_equal(a["classes"], b["classes"])


def test_mobilenet_fully_fused(tiny_mobilenet):
    """V1: 13 depthwise + 14 dense convs and the classifier head; V2: 17
    depthwise + 35 dense convs (the projections take the AddV2 shortcuts);
    nothing of the original conv / BN / ReLU6 / Pad vocabulary is left."""
    version, _ref, _fused, hist = tiny_mobilenet
    if version == "v1":
        assert hist.get("_FusedDepthwiseConv2D") == 13 and hist.get("_FusedConv2D") == 14, hist
        assert hist.get("_ClassifierHead") == 1, hist
    else:
        assert hist.get("_FusedDepthwiseConv2D") == 17 and hist.get("_FusedConv2D") == 35, hist
    for op in GONE:
        assert op not in hist, hist


def test_mobilenet_full_size_layer_counts():
    """The exporter at full width: V1 has 13 depthwise layers and 27 ReLU6s, V2
    17 and 35, channels are multiples of 8, and V2 pads its stride-2 convs
    explicitly (Pad + VALID) while V1 uses SAME."""
    from rust_tensorflow_serving2_amd.models import mobilenet
    for version, n_dw, n_relu6, n_pad in (("v1", 13, 27, 0), ("v2", 17, 35, 5)):
        g, sigs, _saver = mobilenet.build_graph(version)
        ops = [n.op for n in g.graph.node]
        assert ops.count("DepthwiseConv2dNative") == n_dw and ops.count("Relu6") == n_relu6, version
        assert ops.count("Pad") == n_pad, version
        assert set(sigs) == {"serving_default", "predict"}
        for name, arr in g.variables.items():
            if name.endswith("kernel") and arr.ndim == 4 and arr.shape[2] != 3:
                assert arr.shape[2] % 8 == 0 and (arr.shape[3] % 8 == 0 or arr.shape[3] == 1), (name, arr.shape)


# ------------------------------------------------------------------ leave-alone cases
def _dw_graph(mult=1, dilation=1, fetch_bn_stat=False, c=8):
    """x -> DepthwiseConv2dNative 3x3 SAME -> FusedBatchNormV3 -> Relu6."""
    from rust_tensorflow_serving2_amd.graph.builder import DType, GraphBuilder
    from rust_tensorflow_serving2_amd.utils import tensors as T
    f32 = DType(T.DT_FLOAT)
    rng = np.random.default_rng(7)
    g = GraphBuilder()
    x = g.placeholder("x", T.DT_FLOAT, [-1, 9, 9, c])
    w = g.const("w", rng.standard_normal((3, 3, c, mult)).astype(np.float32))
    y = g.node("DepthwiseConv2dNative", "dw", [x, w], T=f32, strides=[1, 1, 1, 1], padding="SAME",
               data_format="NHWC", dilations=[1, dilation, dilation, 1], explicit_paddings=[])
    co = c * mult
    params = [g.const(k, v.astype(np.float32)) for k, v in (
        ("gamma", 1 + 0.1 * rng.standard_normal(co)), ("beta", 0.1 * rng.standard_normal(co)),
        ("mean", 0.1 * rng.standard_normal(co)), ("var", 1 + 0.1 * np.abs(rng.standard_normal(co))))]
    bn = g.node("FusedBatchNormV3", "bn", [y] + params, T=f32, U=f32, epsilon=1e-3, data_format="NHWC",
                is_training=False, exponential_avg_factor=1.0)
    out = g.node("Relu6", "out", [bn], T=f32)
    return g, ["out:0"] + (["bn:1"] if fetch_bn_stat else [])


def _run_both(g, fetches, x):
    from rust_tensorflow_serving2_amd.graph.compiler import compile_program
    from rust_tensorflow_serving2_amd.graph.fused import default_passes
    from rust_tensorflow_serving2_amd.graph.ir import from_graph_def
    ref = compile_program(from_graph_def(g.graph), ["x:0"], fetches)
    fused = compile_program(from_graph_def(g.graph), ["x:0"], fetches, passes=default_passes())
    a = ref.run([torch.from_numpy(x)])
    b = fused.run([torch.from_numpy(x)])
    for u, v in zip(a, b):
        np.testing.assert_allclose(np.asarray(u), np.asarray(v), atol=1e-5)
    return fused.op_histogram()


def test_plain_depthwise_chain_fuses():
    g, fetches = _dw_graph()
    hist = _run_both(g, fetches, np.random.default_rng(1).standard_normal((2, 9, 9, 8)).astype(np.float32) * 3)
    assert hist.get("_FusedDepthwiseConv2D") == 1, hist
    for op in ("DepthwiseConv2dNative", "FusedBatchNormV3", "Relu6"):
        assert op not in hist, hist


@pytest.mark.parametrize("kw", [dict(mult=2), dict(dilation=2)])
def test_depthwise_left_alone(kw):
    """Channel multiplier 2 and dilation 2 stay on the reference op."""
    g, fetches = _dw_graph(**kw)
    hist = _run_both(g, fetches, np.random.default_rng(2).standard_normal((2, 9, 9, 8)).astype(np.float32) * 3)
    assert hist.get("DepthwiseConv2dNative") == 1 and "_FusedDepthwiseConv2D" not in hist, hist
    assert hist.get("FusedBatchNormV3") == 1 and hist.get("Relu6") == 1, hist


def test_depthwise_batchnorm_with_a_fetched_output_is_not_folded():
    """A BatchNorm one of whose other outputs is fetched keeps running as
    itself (its statistics outputs must exist), and so does the ReLU6 behind it."""
    g, fetches = _dw_graph(fetch_bn_stat=True)
    hist = _run_both(g, fetches, np.random.default_rng(3).standard_normal((2, 9, 9, 8)).astype(np.float32) * 3)
    assert hist.get("FusedBatchNormV3") == 1 and hist.get("Relu6") == 1, hist


def test_candidates_offer_relu6_launches_igemm_configs_only():
    """ReLU6 is an igemm epilogue: ops.candidates(relu6=True) offers none of
    the cgemm / bgemm / halo configs, and the keyword defaults to today's list."""
    from rust_tensorflow_serving2_amd import ops
    assert ops.ACT["relu6"] == 5
    others = set(ops.CGEMM) | set(ops.HALO)
    for m, n, k, flags in ((2048, 256, 256, dict(aligned64=True)), (1024, 64, 576, dict(aligned64=True, halo=True)),
                           (4096, 32, 128, dict(aligned64=True, stem=True)), (100, 1008, 1024, dict(aligned64=True))):
        default = ops.candidates(m, n, k, **flags)
        assert default == ops.candidates(m, n, k, relu6=False, **flags)
        with6 = ops.candidates(m, n, k, relu6=True, **flags)
        assert with6 == [cs for cs in default if cs[0] not in others]
        assert with6 and {c for c, _s in default} & others


def test_unfused_depthwise_takes_a_bf16_activation():
    """A depthwise conv the pass leaves alone (multiplier 2) may follow a fused
    op, whose GPU output is bf16, while its filter constant is fp32: the
    reference op converts the filter instead of raising on the mixed types."""
    from rust_tensorflow_serving2_amd.graph import ops as O
    from rust_tensorflow_serving2_amd.graph.ir import Node
    node = Node(name="dw", op="DepthwiseConv2dNative", inputs=[],
                attrs={"strides": [1, 1, 1, 1], "padding": b"SAME", "data_format": b"NHWC"})
    g = torch.Generator().manual_seed(0)
    x, w = torch.randn(1, 5, 5, 8, generator=g), torch.randn(3, 3, 8, 2, generator=g)
    y32 = O.OPS["DepthwiseConv2dNative"](None, node, [x, w])[0]
    y16 = O.OPS["DepthwiseConv2dNative"](None, node, [x.to(torch.bfloat16), w])[0]
    assert y16.dtype == torch.bfloat16 and y16.shape == (1, 5, 5, 16)
    torch.testing.assert_close(y16.float(), y32, atol=0.15, rtol=0.05)
