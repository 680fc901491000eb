"""MobileNetV3 Large / Small through the fusion passes on the CPU: the fused
graph (fp32 reference of the fused ops, same folded parameters the HIP kernels
use) == the unfused reference interpreter; every hard activation, squeeze-excite
block, depthwise conv and BatchNorm is absorbed; the near misses of
fuse_hard_activations and fuse_squeeze_excite are left alone (and still compute
what the interpreter computes)."""
import os

import numpy as np
import pytest
import torch

from rust_tensorflow_serving2_amd.graph.builder import DType, GraphBuilder
from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
from rust_tensorflow_serving2_amd.utils import tensors as T

OUTS = ["classes", "probabilities"]
GONE = ("Relu6", "Mul", "Mean", "AddV2", "Add", "Conv2D", "DepthwiseConv2dNative", "FusedBatchNormV3", "Pad",
        "_HardSwish", "_HardSigmoid")
F32 = DType(T.DT_FLOAT)
N_SE = {"v3_large": 8, "v3_small": 9}
N_DW = {"v3_large": 15, "v3_small": 11}


def n_fused_convs(version):
    """From the table: the stem, an expand conv in every block but the first, a
    projection in every block, the last 1x1 conv and the head's two."""
    from rust_tensorflow_serving2_amd.models import mobilenet
    blocks = len(mobilenet.V3_LARGE if version == "v3_large" else mobilenet.V3_SMALL)
    return 1 + (blocks - 1) + blocks + 1 + 2


@pytest.fixture(scope="module", params=["v3_large", "v3_small"])
def tiny_v3(request, models_dir):
    from rust_tensorflow_serving2_amd.models import mobilenet
    path = os.path.join(str(models_dir), f"tiny_mobilenet_{request.param}", "1")
    mobilenet.export(path, version=request.param, alpha=0.25, image_size=32, num_classes=11, seed=5)
    ref = Servable("m", 1, path, ServableOptions(device="cpu"))
    fused = Servable("m", 1, path, ServableOptions(device="cpu", fuse=True))
    hist = fused.runner("serving_default", ["input"], OUTS).program.op_histogram()
    return request.param, ref, fused, hist


def test_v3_fused_matches_interpreter(tiny_v3):
    _version, ref, fused, _hist = tiny_v3
    x = np.random.default_rng(0).random((3, 32, 32, 3), dtype=np.float32)
    a = ref.run("serving_default", {"input": x}, OUTS)
    b = fused.run("serving_default", {"input": x}, OUTS)
    assert a["probabilities"].shape == (3, 11)
    np.testing.assert_allclose(a["probabilities"], b["probabilities"], atol=1e-5)
    np.testing.assert_array_equal(a["classes"], b["classes"])


def test_v3_fully_fused(tiny_v3):
    version, _ref, _fused, hist = tiny_v3
    assert hist.get("_SqueezeExcite") == N_SE[version], hist
    assert hist.get("_FusedDepthwiseConv2D") == N_DW[version], hist
    assert n_fused_convs("v3_large") == 33 and n_fused_convs("v3_small") == 25
    assert hist.get("_FusedConv2D") == n_fused_convs(version), hist
    for op in GONE:
        assert op not in hist, hist
    assert hist.get("_GlobalAvgPool") == 1, hist           # the head's; the blocks' pools are inside _SqueezeExcite


def _gates(servable, x):
    """The squeeze-excite gates of the fp32 interpreter, one [B,1,1,C] tensor per block."""
    from rust_tensorflow_serving2_amd.graph.compiler import compile_program
    g = servable.fresh_graph()
    names = sorted(n for n, nd in g.nodes.items() if nd.op == "Mul" and n.endswith("squeeze_excite/hard_sigmoid/mul"))
    return [torch.as_tensor(t) for t in compile_program(g, ["input_tensor:0"], names).run([torch.from_numpy(x)])]


def test_v3_gates_do_not_saturate(tiny_v3):
    """The SE tests would test a constant otherwise: on the fp32 interpreter at
    this file's inputs at least a quarter of all gate values lie strictly inside
    (0, 1), and within one block the gates are not all equal."""
    version, ref, _fused, _hist = tiny_v3
    gates = _gates(ref, np.random.default_rng(0).random((3, 32, 32, 3), dtype=np.float32))
    assert len(gates) == N_SE[version]
    allg = torch.cat([g.reshape(-1) for g in gates])
    inside = ((allg > 0) & (allg < 1)).float().mean().item()
    assert inside >= 0.25, inside
    for g in gates:
        assert g.min() < g.max()


def test_v3_full_size_layer_counts():
    from rust_tensorflow_serving2_amd.models import mobilenet
    for version, n_pad, n_k5 in (("v3_large", 4, 6), ("v3_small", 4, 8)):
        g, sigs, _saver = mobilenet.build_graph(version)
        ops = [n.op for n in g.graph.node]
        assert ops.count("DepthwiseConv2dNative") == N_DW[version] and ops.count("Mean") == N_SE[version] + 1
        assert ops.count("Pad") == n_pad, (version, ops.count("Pad"))
        assert set(sigs) == {"serving_default", "predict"}
        k5 = [a.shape for n, a in g.variables.items() if n.endswith("depthwise_kernel") and a.shape[0] == 5]
        assert len(k5) == n_k5, (version, len(k5))
        for name, arr in g.variables.items():
            if name.endswith("kernel") and arr.ndim == 4 and arr.shape[2] != 3:
                assert arr.shape[2] % 8 == 0 and (arr.shape[3] % 8 == 0 or arr.shape[3] in (1, 1001)), (name, arr.shape)
    with pytest.raises(ValueError, match="'v1', 'v2', 'v3_large' or 'v3_small'"):
        mobilenet.build_graph("v4")


# ------------------------------------------------------------------ small graphs
def _run_both(g, fetches, feeds, atol=1e-5):
    """{feed name: array} -> the fused program's histogram, after comparing
    every fetch of the fused program against the interpreter."""
    from rust_tensorflow_serving2_amd.graph.compiler import compile_program
    from rust_tensorflow_serving2_amd.graph.fused import default_passes
    from rust_tensorflow_serving2_amd.graph.ir import from_graph_def
    names = [f"{k}:0" for k in feeds]
    vals = [torch.from_numpy(v) for v in feeds.values()]
    ref = compile_program(from_graph_def(g.graph), names, fetches)
    fused = compile_program(from_graph_def(g.graph), names, fetches, passes=default_passes())
    a, b = ref.run(vals), fused.run(vals)
    for u, v in zip(a, b):
        np.testing.assert_allclose(np.asarray(u), np.asarray(v), atol=atol)
    return fused.op_histogram()


def _x(shape=(2, 5, 5, 8), seed=1, scale=3.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def _hard_graph(offset=3.0, inner="Relu6", scale=1.0 / 6.0, vector_three=False, swish=True, slim=False, swap=False,
                other_y=False, second_reader=False, fetch_inner=False):
    g = GraphBuilder()
    x = g.placeholder("x", T.DT_FLOAT, [-1, 5, 5, 8])
    three = g.const("three", np.full(8 if vector_three else (), offset, np.float32))
    c = g.const("sixth", np.array(scale, np.float32))
    add = g.node("AddV2", "add", [three, x] if swap else [x, three], T=F32)
    r = g.node(inner, "inner", [add], T=F32)
    fetches = ["out:0"]
    if slim:
        m = g.node("Mul", "xr", [r, x] if swap else [x, r], T=F32)
        g.node("Mul", "out", [c, m] if swap else [m, c], T=F32)
    else:
        hs = g.node("Mul", "hs" if swish else "out", [c, r] if swap else [r, c], T=F32)
        if swish:
            y = g.node("Neg", "y", [x], T=F32) if other_y else x
            g.node("Mul", "out", [hs, y] if swap else [y, hs], T=F32)
    if second_reader:
        g.node("Neg", "reader", [r], T=F32)
        fetches.append("reader:0")
    if fetch_inner:
        fetches.append("inner:0")
    return g, fetches


@pytest.mark.parametrize("kw,op", [(dict(), "_HardSwish"), (dict(swap=True), "_HardSwish"),
                                   (dict(slim=True, scale=0.16667), "_HardSwish"),
                                   (dict(slim=True, swap=True), "_HardSwish"), (dict(swish=False), "_HardSigmoid"),
                                   (dict(swish=False, swap=True, scale=0.16667), "_HardSigmoid")])
def test_hard_activations_are_matched(kw, op):
    g, fetches = _hard_graph(**kw)
    hist = _run_both(g, fetches, {"x": _x()})
    assert hist.get(op) == 1, hist
    for gone in ("Mul", "Relu6", "AddV2"):
        assert gone not in hist, hist


@pytest.mark.parametrize("kw", [dict(offset=2.5), dict(inner="Relu"), dict(scale=1.0 / 3.0), dict(vector_three=True),
                                dict(fetch_inner=True), dict(second_reader=True)])
def test_hard_activation_near_misses_are_left_alone(kw):
    g, fetches = _hard_graph(**kw)
    hist = _run_both(g, fetches, {"x": _x()})
    assert "_HardSwish" not in hist and "_HardSigmoid" not in hist, hist
    assert hist.get("Mul") == 2, hist


def test_hard_sigmoid_of_x_times_another_tensor_is_no_hard_swish():
    g, fetches = _hard_graph(other_y=True)
    hist = _run_both(g, fetches, {"x": _x()})
    assert hist.get("_HardSigmoid") == 1 and hist.get("Mul") == 1 and "_HardSwish" not in hist, hist


def test_hard_swish_closes_conv_and_depthwise_chains():
    rng = np.random.default_rng(3)
    g = GraphBuilder()
    x = g.placeholder("x", T.DT_FLOAT, [-1, 6, 6, 8])
    w = g.const("w", (rng.standard_normal((1, 1, 8, 16)) * 0.8).astype(np.float32))
    y = g.node("Conv2D", "conv", [x, w], T=F32, strides=[1, 1, 1, 1], padding="SAME", data_format="NHWC",
               dilations=[1, 1, 1, 1], explicit_paddings=[])
    y = g.node("BiasAdd", "bias", [y, g.const("b", rng.standard_normal(16).astype(np.float32))], T=F32)

    def hswish(t, name):
        a = g.node("AddV2", name + "/add", [t, g.const(name + "/three", np.array(3.0, np.float32))], T=F32)
        a = g.node("Relu6", name + "/relu6", [a], T=F32)
        a = g.node("Mul", name + "/mul", [a, g.const(name + "/sixth", np.array(1.0 / 6.0, np.float32))], T=F32)
        return g.node("Mul", name + "/out", [t, a], T=F32)
    y = hswish(y, "h1")
    dw = g.const("dw", (rng.standard_normal((5, 5, 16, 1)) * 0.4).astype(np.float32))
    y = g.node("DepthwiseConv2dNative", "depthwise", [y, dw], T=F32, strides=[1, 2, 2, 1], padding="SAME",
               data_format="NHWC", dilations=[1, 1, 1, 1], explicit_paddings=[])
    y = hswish(y, "h2")
    g.node("Identity", "out", [y], T=F32)
    hist = _run_both(g, ["out:0"], {"x": _x((2, 6, 6, 8), seed=4, scale=2.0)})
    assert hist.get("_FusedConv2D") == 1 and hist.get("_FusedDepthwiseConv2D") == 1, hist
    for gone in ("_HardSwish", "Mul", "Relu6", "AddV2"):
        assert gone not in hist, hist


def _se_graph(c=8, cr=4, rank3=False, other_z=False, axes=(1, 2), keep=True, reshape=False, k=1, stride=1,
              fed_filter=False, act1="Relu", gate="hard_sigmoid", second_reader=False, fetch_gate=False, bias=True,
              swap=False):
    rng = np.random.default_rng(11)
    g = GraphBuilder()
    x = g.placeholder("x", T.DT_FLOAT, [-1, 5, 8] if rank3 else [-1, 5, 5, c])
    z = g.placeholder("z", T.DT_FLOAT, [-1, 5, 5, c]) if other_z else x
    ax = g.const("axes", np.array(axes, np.int32))
    p = g.node("Mean", "pool", [z, ax], T=F32, Tidx=DType(T.DT_INT32), keep_dims=keep)
    if reshape:
        p = g.node("Reshape", "reshape", [p, g.const("shape", np.array([-1, 1, 1, c], np.int32))], T=F32,
                   Tshape=DType(T.DT_INT32))
    w1v = (rng.standard_normal((k, k, c, cr)) * 1.5).astype(np.float32)
    w1 = g.placeholder("w1", T.DT_FLOAT, [k, k, c, cr]) if fed_filter else g.const("w1", w1v)

    def conv(t, w, name, s=1):
        return g.node("Conv2D", name, [t, w], T=F32, strides=[1, s, s, 1], padding="SAME", data_format="NHWC",
                      dilations=[1, 1, 1, 1], explicit_paddings=[])
    h = conv(p, w1, "fc1", stride)
    if bias:
        h = g.node("BiasAdd", "fc1/bias", [h, g.const("b1", rng.standard_normal(cr).astype(np.float32))], T=F32)
    if act1:
        h = g.node(act1, "act1", [h], T=F32)
    h = conv(h, g.const("w2", (rng.standard_normal((1, 1, cr, c)) * 1.5).astype(np.float32)), "fc2")
    if bias:
        h = g.node("BiasAdd", "fc2/bias", [h, g.const("b2", rng.standard_normal(c).astype(np.float32))], T=F32)
    if gate == "hard_sigmoid":
        h = g.node("AddV2", "gate/add", [h, g.const("three", np.array(3.0, np.float32))], T=F32)
        h = g.node("Relu6", "gate/relu6", [h], T=F32)
        h = g.node("Mul", "gate", [h, g.const("sixth", np.array(1.0 / 6.0, np.float32))], T=F32)
    else:
        h = g.node(gate, "gate", [h], T=F32)
    g.node("Mul", "out", [h, x] if swap else [x, h], T=F32)
    fetches = ["out:0"]
    if second_reader:
        g.node("Neg", "reader", [h], T=F32)
        fetches.append("reader:0")
    if fetch_gate:
        fetches.append("gate:0")
    feeds = {"x": _x((2, 5, 8) if rank3 else (2, 5, 5, c), seed=12, scale=2.0)}
    if other_z:
        feeds["z"] = _x((2, 5, 5, c), seed=13, scale=2.0)
    if fed_filter:
        feeds["w1"] = w1v
    return g, fetches, feeds


@pytest.mark.parametrize("kw", [dict(), dict(swap=True), dict(keep=False, reshape=True), dict(bias=False),
                                dict(act1=None), dict(axes=(-3, -2))])
def test_squeeze_excite_is_matched(kw):
    g, fetches, feeds = _se_graph(**kw)
    hist = _run_both(g, fetches, feeds)
    assert hist.get("_SqueezeExcite") == 1, hist
    for gone in ("Mul", "Conv2D", "_GlobalAvgPool", "Mean", "_HardSigmoid", "BiasAdd", "Relu", "Reshape"):
        assert gone not in hist, hist


@pytest.mark.parametrize("kw", [dict(other_z=True), dict(axes=(1,)), dict(keep=False), dict(k=3), dict(stride=2),
                                dict(fed_filter=True), dict(act1="Relu6"), dict(gate="Sigmoid"),
                                dict(second_reader=True), dict(fetch_gate=True)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_squeeze_excite_near_misses_are_left_alone(kw):
    g, fetches, feeds = _se_graph(**kw)
    if kw == dict(keep=False):
        # Mean without keep_dims hands the 1x1 conv a rank-2 tensor: the graph itself is ill-formed, and
        # the interpreter and the fused program must both say so
        from rust_tensorflow_serving2_amd.graph import ops as O
        from rust_tensorflow_serving2_amd.graph.compiler import compile_program
        from rust_tensorflow_serving2_amd.graph.fused import default_passes
        from rust_tensorflow_serving2_amd.graph.ir import from_graph_def
        vals = [torch.from_numpy(v) for v in feeds.values()]
        ref = compile_program(from_graph_def(g.graph), ["x:0"], fetches)
        fused = compile_program(from_graph_def(g.graph), ["x:0"], fetches, passes=default_passes())
        assert "_SqueezeExcite" not in fused.op_histogram()
        for program in (ref, fused):
            with pytest.raises(O.OpError, match="Conv2D"):
                program.run(vals)
        return
    hist = _run_both(g, fetches, feeds)
    assert "_SqueezeExcite" not in hist, hist


def test_squeeze_excite_on_a_rank_3_tensor_keeps_the_original_semantics():
    """The pass cannot see the rank: it may fire, and the op then does what the
    nodes did -- here the Conv2D of the original graph refuses a rank-3 input,
    and so does the fused program."""
    from rust_tensorflow_serving2_amd.graph.compiler import compile_program
    from rust_tensorflow_serving2_amd.graph.fused import default_passes
    from rust_tensorflow_serving2_amd.graph.ir import from_graph_def
    g, fetches, feeds = _se_graph(rank3=True)
    vals = [torch.from_numpy(v) for v in feeds.values()]
    ref = compile_program(from_graph_def(g.graph), ["x:0"], fetches)
    fused = compile_program(from_graph_def(g.graph), ["x:0"], fetches, passes=default_passes())
    with pytest.raises(Exception):
        ref.run(vals)
    with pytest.raises(Exception):
        fused.run(vals)


def test_squeeze_excite_op_on_rank_3_matches_the_nodes_when_they_run():
    """Called directly on a tensor that is not NHWC, the op computes Mean over
    the axes the pass saw, the reshape and the 1x1 convs one by one."""
    from rust_tensorflow_serving2_amd.graph.fused import SqueezeExcite
    rng = torch.Generator().manual_seed(0)
    w1, b1, w2, b2 = torch.randn(8, 4, generator=rng), torch.randn(4, generator=rng), torch.randn(4, 8, generator=rng), \
        torch.randn(8, generator=rng)
    op = SqueezeExcite(w1, b1, w2, b2, "relu", 1.0 / 6.0, False, (-3, -2), [-1, 1, 1, 8], torch.device("cpu"), False, "se")
    x = torch.randn(6, 5, 8, generator=rng)              # Mean over axes 0, 1 -> [8] -> [1, 1, 1, 8]
    (y,) = op(None, None, [x])
    p = x.mean(dim=(0, 1)).reshape(1, 8)
    gate = torch.clamp(torch.relu(p @ w1 + b1) @ w2 + b2 + 3.0, 0.0, 6.0) / 6.0
    torch.testing.assert_close(y, x * gate.reshape(1, 1, 1, 8), atol=1e-5, rtol=1e-5)


def test_hard_swish_launches_tune_over_the_igemm_configs_only():
    from rust_tensorflow_serving2_amd import ops
    assert ops.ACT["hard_sigmoid"] == 6 and ops.ACT["hard_swish"] == 7 and ops.ACT["relu6"] == 5
    others = set(ops.CGEMM) | set(ops.HALO)
    for m, n, k, flags in ((2048, 256, 256, dict(aligned64=True)), (1024, 64, 576, dict(aligned64=True, halo=True))):
        default = ops.candidates(m, n, k, **flags)
        assert ops.candidates(m, n, k, igemm_act=True, **flags) == ops.candidates(m, n, k, relu6=True, **flags) == \
            [cs for cs in default if cs[0] not in others]


def test_existing_model_histograms_are_unchanged(models_dir, monkeypatch):
    """ResNet-50, BERT and MobileNet V1 / V2 do not contain the new patterns:
    their fused programs have the pinned op counts, and the very histogram that
    the pass list without the two new passes gives."""
    from rust_tensorflow_serving2_amd.graph import fused
    from rust_tensorflow_serving2_amd.models import bert, mobilenet, resnet
    with_new = fused.default_passes
    new = (fused.fuse_hard_activations, fused.fuse_squeeze_excite)
    tiny_bert = bert.BertConfig(vocab_size=100, hidden=64, layers=2, heads=2, intermediate=128, max_position=32,
                                seq_len=16)
    image = (["input"], OUTS)
    for name, export, (ins, outs), want in (
            ("resnet", lambda p: resnet.export(p, image_size=32, num_classes=11, seed=1), image,
             {"_StemPool": 1, "_FusedConv2D": 52, "_ClassifierHead": 1}),
            ("bert", lambda p: bert.export(p, tiny_bert, seed=1),
             (["input_ids", "input_mask", "segment_ids"], ["probabilities", "pooled_output"]),
             {"_EmbeddingLN": 1, "_FusedQKV": 2, "_Attention": 2, "_FusedMatMul": 7, "_LayerNorm": 4, "_DenseSoftmax": 1}),
            ("v1", lambda p: mobilenet.export(p, version="v1", alpha=0.25, image_size=32, num_classes=11, seed=5), image,
             {"_FusedDepthwiseConv2D": 13, "_FusedConv2D": 14, "_ClassifierHead": 1}),
            ("v2", lambda p: mobilenet.export(p, version="v2", alpha=0.25, image_size=32, num_classes=11, seed=5), image,
             {"_FusedDepthwiseConv2D": 17, "_FusedConv2D": 35})):
        path = os.path.join(str(models_dir), f"v3_stability_{name}", "1")
        export(path)

        def histogram():
            return Servable("m", 1, path, ServableOptions(device="cpu", fuse=True)).runner(
                "serving_default", ins, outs).program.op_histogram()
        hist = histogram()
        print(name, dict(hist))
        for op in ("_HardSwish", "_HardSigmoid", "_SqueezeExcite"):
            assert op not in hist, (name, hist)
        for op, n in want.items():
            assert hist.get(op) == n, (name, hist)
        with monkeypatch.context() as m:
            m.setattr(fused, "default_passes", lambda options=None: [p for p in with_new(options) if p not in new])
            assert histogram() == hist, name
