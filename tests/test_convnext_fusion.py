"""ConvNeXt through the fusion passes on the CPU: the fused graph (fp32
reference of the fused ops, same folded parameters the HIP kernels use) == the
unfused reference interpreter; every block becomes one _FusedDepthwiseLN and
two _FusedConv2D (the first closed by the erf GELU, the second with the layer
scale folded in and the shortcut as its residual); the near misses of
fuse_depthwise_layernorm and of the GELU closing activation are left alone (and
still compute what the interpreter computes); the exporter's default graph is
pinned."""
import hashlib
import os

import numpy as np
import pytest

import test_mobilenet_v3_fusion as v3f
from rust_tensorflow_serving2_amd.graph.builder import DType, GraphBuilder
from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
from rust_tensorflow_serving2_amd.utils import tensors as T

OUTS = ["classes", "probabilities"]
DEPTHS, DIMS = (1, 1, 2, 1), (16, 24, 32, 40)
GONE = ("DepthwiseConv2dNative", "Conv2D", "Erf", "Mul", "AddV2", "Add", "RealDiv", "BiasAdd", "_FusedDepthwiseConv2D",
        "SquaredDifference", "Rsqrt")
F32 = DType(T.DT_FLOAT)


@pytest.fixture(scope="module")
def tiny_convnext(models_dir):
    from rust_tensorflow_serving2_amd.models import convnext
    path = os.path.join(str(models_dir), "tiny_convnext", "1")
    convnext.export(path, depths=DEPTHS, dims=DIMS, image_size=32, num_classes=11, seed=5)
    ref = Servable("m", 1, path, ServableOptions(device="cpu"))
    fused = Servable("m", 1, path, ServableOptions(device="cpu", fuse=True))
    hist = fused.runner("serving_default", ["input"], OUTS).program.op_histogram()
    return ref, fused, hist


def test_convnext_fused_matches_interpreter(tiny_convnext):
    ref, fused, _hist = tiny_convnext
    x = np.random.default_rng(0).standard_normal((3, 32, 32, 3)).astype(np.float32)
    a = ref.run("serving_default", {"input": x}, OUTS)
    b = fused.run("serving_default", {"input": x}, OUTS)
    assert a["probabilities"].shape == (3, 11)
    assert np.ptp(a["probabilities"], axis=0).max() > 1e-3          # (the image reaches the output)
    np.testing.assert_allclose(a["probabilities"], b["probabilities"], atol=1e-5)
    np.testing.assert_array_equal(a["classes"], b["classes"])


def test_convnext_fully_fused(tiny_convnext):
    """5 blocks: one _FusedDepthwiseLN and two pointwise convs each; 14 convs
    = the stem, 3 downsampling convs and the 10 pointwise ones (the layer scale
    and the shortcut are inside the second).  The LayerNorms of the stem, the 3
    downsampling blocks and the head stay _LayerNorm."""
    _ref, _fused, hist = tiny_convnext
    assert hist.get("_FusedDepthwiseLN") == sum(DEPTHS), hist
    assert hist.get("_FusedConv2D") == 4 + 2 * sum(DEPTHS), hist
    assert hist.get("_LayerNorm") == 5, hist
    for op in GONE:
        assert op not in hist, hist


def test_convnext_tiny_layer_table():
    from rust_tensorflow_serving2_amd.models import convnext
    g, sigs, _saver = convnext.build_graph()
    ops = [n.op for n in g.graph.node]
    assert ops.count("DepthwiseConv2dNative") == 18 and ops.count("Conv2D") == 4 + 36 and ops.count("Erf") == 18
    assert ops.count("SquaredDifference") == 18 + 1 + 3 + 1 and ops.count("MatMul") == 1
    assert set(sigs) == {"serving_default", "predict"}
    dw = sorted(a.shape[2] for n, a in g.variables.items() if n.endswith("depthwise_kernel"))
    assert dw == [96] * 3 + [192] * 3 + [384] * 9 + [768] * 3
    assert all(a.shape[:2] == (7, 7) for n, a in g.variables.items() if n.endswith("depthwise_kernel"))
    assert g.variables["convnext/stem/conv/kernel"].shape == (4, 4, 3, 96)
    assert g.variables["head_layer/predictions/kernel"].shape == (768, 1000)
    scales = [a for n, a in g.variables.items() if n.endswith("layer_scale/gamma")]
    assert len(scales) == 18 and all(abs(float(a.mean()) - convnext.LAYER_SCALE_INIT) < 0.1 for a in scales)
    with pytest.raises(ValueError, match="multiple of 32"):
        convnext.build_graph(image_size=100)
    with pytest.raises(ValueError, match="four stages"):
        convnext.build_graph(depths=(1, 1, 1))


# ------------------------------------------------------------------ fuse_depthwise_layernorm on small graphs
def _ln(g, x, c, rng, name, eps=1e-6):
    """models/bert.py layer_norm (the tf.nn.moments + batch_normalization
    spelling) with constants for gamma and beta."""
    I32 = DType(T.DT_INT32)
    with g.scope(name):
        gamma = g.const("gamma", (1.0 + 0.2 * rng.standard_normal(c)).astype(np.float32))
        beta = g.const("beta", (0.2 * rng.standard_normal(c)).astype(np.float32))
        mean = g.node("Mean", "mean", [x, g.const("mean/axes", np.array([-1], np.int32))], T=F32, Tidx=I32,
                      keep_dims=True)
        sqd = g.node("SquaredDifference", "sqd", [x, g.node("StopGradient", "sg", [mean], T=F32)], T=F32)
        var = g.node("Mean", "variance", [sqd, g.const("variance/axes", np.array([-1], np.int32))], T=F32, Tidx=I32,
                     keep_dims=True)
        rs = g.node("Rsqrt", "Rsqrt", [g.node("AddV2", "add", [var, g.const("eps", np.array(eps, np.float32))], T=F32)],
                    T=F32)
        mul = g.node("Mul", "mul", [rs, gamma], T=F32)
        sub = g.node("Sub", "sub", [beta, g.node("Mul", "mul_2", [mean, mul], T=F32)], T=F32)
        return g.node("AddV2", "add_1", [g.node("Mul", "mul_1", [x, mul], T=F32), sub], T=F32)


def _dwln_graph(k=7, stride=1, relu=False, second_reader=False, fetch_dw=False, mult=1, c=8, bias=True):
    rng = np.random.default_rng(7)
    g = GraphBuilder()
    x = g.placeholder("x", T.DT_FLOAT, [-1, 9, 10, c])
    w = g.const("dw", (rng.standard_normal((k, k, c, mult)) / k).astype(np.float32))
    y = g.node("DepthwiseConv2dNative", "depthwise", [x, w], T=F32, strides=[1, stride, stride, 1], padding="SAME",
               data_format="NHWC", dilations=[1, 1, 1, 1], explicit_paddings=[])
    if bias:
        y = g.node("BiasAdd", "bias", [y, g.const("b", rng.standard_normal(c * mult).astype(np.float32))], T=F32)
    if relu:
        y = g.node("Relu", "relu", [y], T=F32)
    dw_out = y
    y = _ln(g, y, c * mult, rng, "ln")
    g.node("Identity", "out", [y], T=F32)
    fetches = ["out:0"]
    if second_reader:
        g.node("Neg", "reader", [dw_out], T=F32)
        fetches.append("reader:0")
    if fetch_dw:
        fetches.append(dw_out + ":0")
    return g, fetches


@pytest.mark.parametrize("kw", [dict(), dict(bias=False), dict(c=40)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()) or "plain")
def test_depthwise_layernorm_is_matched(kw):
    g, fetches = _dwln_graph(**kw)
    hist = v3f._run_both(g, fetches, {"x": v3f._x((2, 9, 10, kw.get("c", 8)), seed=4)})
    assert hist.get("_FusedDepthwiseLN") == 1, hist
    for gone in ("_FusedDepthwiseConv2D", "_LayerNorm", "DepthwiseConv2dNative", "BiasAdd"):
        assert gone not in hist, hist


@pytest.mark.parametrize("kw", [dict(relu=True), dict(second_reader=True), dict(fetch_dw=True), dict(stride=2),
                                dict(k=5), dict(mult=2)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_depthwise_layernorm_near_misses_are_left_as_the_pair(kw):
    g, fetches = _dwln_graph(**kw)
    hist = v3f._run_both(g, fetches, {"x": v3f._x((2, 9, 10, 8), seed=4)})
    assert "_FusedDepthwiseLN" not in hist and hist.get("_LayerNorm") == 1, hist
    # (channel multiplier 2 is not fuse_depthwise's either: the reference op stays)
    assert hist.get("DepthwiseConv2dNative" if kw.get("mult") else "_FusedDepthwiseConv2D") == 1, hist


def test_dwln_env_switch_keeps_the_pair(monkeypatch):
    monkeypatch.setenv("TFSERVE_DWLN", "0")
    g, fetches = _dwln_graph()
    hist = v3f._run_both(g, fetches, {"x": v3f._x((2, 9, 10, 8), seed=4)})
    assert "_FusedDepthwiseLN" not in hist and hist.get("_LayerNorm") == 1 and hist.get("_FusedDepthwiseConv2D") == 1


def test_an_input_of_another_rank_or_depth_runs_the_two_ops():
    """The op's run-time guard: it was built for C = 8; 16 channels fail as the
    depthwise op itself fails on them (one error, not a wrong answer)."""
    import torch
    from rust_tensorflow_serving2_amd.graph.fused import FusedDepthwiseConv, FusedDepthwiseLN
    from rust_tensorflow_serving2_amd.graph.patterns import LayerNormOp
    dev = torch.device("cpu")
    dw = FusedDepthwiseConv(torch.randn(7, 7, 8), torch.randn(8), (1, 1), "SAME", (0, 0, 0, 0), "none", dev, False, "dw")
    ln = LayerNormOp(torch.randn(8), torch.randn(8), 1e-6, dev, False)
    op = FusedDepthwiseLN(dw, ln, False, "dwln")
    x = torch.randn(2, 5, 6, 8)
    torch.testing.assert_close(op(None, None, [x])[0], ln(None, None, dw(None, None, [x]))[0], atol=1e-5, rtol=0)
    with pytest.raises(RuntimeError):
        op(None, None, [torch.randn(2, 5, 6, 16)])


# ------------------------------------------------------------------ GELU as fuse_conv's closing activation
def _conv_gelu_graph(form="erf", half=0.5, outside_reader=False, residual=False, layer_scale=False):
    from rust_tensorflow_serving2_amd.models.bert import gelu
    from rust_tensorflow_serving2_amd.models.convnext import _gelu_erf
    rng = np.random.default_rng(3)
    g = GraphBuilder()
    x = g.placeholder("x", T.DT_FLOAT, [-1, 6, 6, 8])
    w = g.const("w", (rng.standard_normal((1, 1, 8, 8)) * 0.5).astype(np.float32))
    y = g.node("Conv2D", "conv", [x, w], T=F32, strides=[1, 1, 1, 1], padding="SAME", data_format="NHWC",
               dilations=[1, 1, 1, 1], explicit_paddings=[])
    y = g.node("BiasAdd", "bias", [y, g.const("b", rng.standard_normal(8).astype(np.float32))], T=F32)
    if layer_scale:
        y = g.node("Mul", "scale", [y, g.const("ls", (0.5 + rng.random(8)).astype(np.float32))], T=F32)
    if residual:
        y = g.node("AddV2", "shortcut", [x, y], T=F32)
    pre = y
    if form == "tanh":
        y = gelu(g, y)
    else:
        if half == 0.5:
            y = _gelu_erf(g, y, "gelu")
        else:                                  # models/convnext.py _gelu_erf with another constant
            h = g.node("Mul", "gelu/mul", [g.const("gelu/mul/x", np.array(half, np.float32)), y], T=F32)
            q = g.node("RealDiv", "gelu/truediv", [y, g.const("gelu/Cast/x", np.array(np.sqrt(2.0), np.float32))], T=F32)
            a = g.node("AddV2", "gelu/add", [g.const("gelu/add/x", np.array(1.0, np.float32)),
                                             g.node("Erf", "gelu/Erf", [q], T=F32)], T=F32)
            y = g.node("Mul", "gelu/mul_1", [h, a], T=F32)
    g.node("Identity", "out", [y], T=F32)
    fetches = ["out:0"]
    if outside_reader:
        g.node("Neg", "reader", [pre], T=F32)
        fetches.append("reader:0")
    return g, fetches


@pytest.mark.parametrize("kw", [dict(), dict(form="tanh"), dict(residual=True), dict(layer_scale=True, residual=True),
                                dict(form="tanh", residual=True)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()) or "erf")
def test_gelu_closes_a_conv_chain(kw):
    """Also after a folded residual: add first, then the activation (the
    interpreter's order, which _run_both compares against)."""
    g, fetches = _conv_gelu_graph(**kw)
    hist = v3f._run_both(g, fetches, {"x": v3f._x((2, 6, 6, 8), seed=4, scale=2.0)})
    assert hist.get("_FusedConv2D") == 1, hist
    for gone in ("Erf", "Tanh", "Pow", "Mul", "AddV2", "RealDiv", "BiasAdd"):
        assert gone not in hist, hist
    from rust_tensorflow_serving2_amd.graph.compiler import compile_program
    from rust_tensorflow_serving2_amd.graph.fused import default_passes
    from rust_tensorflow_serving2_amd.graph.ir import from_graph_def
    prog = compile_program(from_graph_def(g.graph), ["x:0"], fetches, passes=default_passes())
    impl = next(n.attrs["_impl"] for _f, n, _i, _o in prog.steps if n.op == "_FusedConv2D")
    assert impl.act == ("gelu_tanh" if kw.get("form") == "tanh" else "gelu_erf")


@pytest.mark.parametrize("kw", [dict(outside_reader=True), dict(half=0.4)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_gelu_near_misses_are_left_alone(kw):
    g, fetches = _conv_gelu_graph(**kw)
    hist = v3f._run_both(g, fetches, {"x": v3f._x((2, 6, 6, 8), seed=4, scale=2.0)})
    assert hist.get("_FusedConv2D") == 1 and hist.get("Erf") == 1 and hist.get("Mul", 0) >= 2, hist


def test_layer_scale_and_shortcut_are_fuse_convs_chain():
    """Conv2D -> BiasAdd -> Mul(gamma[C]) -> AddV2(shortcut) needs no pass of its own."""
    rng = np.random.default_rng(3)
    g = GraphBuilder()
    x = g.placeholder("x", T.DT_FLOAT, [-1, 6, 6, 8])
    w = g.const("w", (rng.standard_normal((1, 1, 8, 8)) * 0.5).astype(np.float32))
    y = g.node("Conv2D", "conv", [x, w], T=F32, strides=[1, 1, 1, 1], padding="SAME", data_format="NHWC",
               dilations=[1, 1, 1, 1], explicit_paddings=[])
    y = g.node("BiasAdd", "bias", [y, g.const("b", rng.standard_normal(8).astype(np.float32))], T=F32)
    y = g.node("Mul", "scale", [y, g.const("ls", (0.5 + rng.random(8)).astype(np.float32))], T=F32)
    g.node("AddV2", "out", [x, y], T=F32)
    hist = v3f._run_both(g, ["out:0"], {"x": v3f._x((2, 6, 6, 8), seed=4)})
    assert dict(hist).get("_FusedConv2D") == 1 and "Mul" not in hist and "AddV2" not in hist, hist


# ------------------------------------------------------------------ the exporter
# sha256 of the GraphDef (deterministic serialization) and of the variables (sorted by name: name bytes, then
# the array's bytes) of build_graph()'s defaults, and the number of variables
PINNED = ("64a3f884a9f1e01d521c5cfce3f8b9cde8237fd3da9a587bdf427fe56675a18b",
          "321807425533b1aebdcce506591b64dac084b1828a94ea44166bf685512e1b9a", 182)


def test_default_export_is_pinned():
    from rust_tensorflow_serving2_amd.models import convnext
    g, _sigs, _saver = convnext.build_graph()
    h = hashlib.sha256()
    for name in sorted(g.variables):
        h.update(name.encode())
        h.update(np.ascontiguousarray(g.variables[name]).tobytes())
    got = (hashlib.sha256(g.graph.SerializeToString(deterministic=True)).hexdigest(), h.hexdigest(), len(g.variables))
    assert got == PINNED, got
