"""ResNeXt through the fusion passes on the CPU: the fused graph (fp32 reference
of the fused ops, the folded parameters the HIP kernel uses) == the unfused
interpreter, every grouped conv becomes a ``_FusedGroupedConv2D``, the near
misses are left to whoever computes them right, and the ResNet exporter's
defaults still write the graphs they wrote before it learned ``groups``."""
import collections
import hashlib
import os

import numpy as np
import pytest
import torch

from rust_tensorflow_serving2_amd.graph.builder import DType, GraphBuilder
from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
from rust_tensorflow_serving2_amd.utils import tensors as T

OUTS = ["classes", "probabilities"]
F32 = DType(T.DT_FLOAT)


# ------------------------------------------------------------------ the tiny model
@pytest.fixture(scope="module")
def tiny_resnext(models_dir):
    from rust_tensorflow_serving2_amd.models import resnet
    path = os.path.join(str(models_dir), "tiny_resnext", "1")
    resnet.export(path, blocks=(1, 1, 1, 1), width=16, groups=4, width_per_group=16, image_size=32, num_classes=11,
                  seed=5)
    ref = Servable("m", 1, path, ServableOptions(device="cpu"))
    fused = Servable("m", 1, path, ServableOptions(device="cpu", fuse=True))
    return ref, fused


def test_resnext_fused_matches_interpreter(tiny_resnext):
    ref, fused = tiny_resnext
    x = np.random.default_rng(0).random((3, 32, 32, 3), dtype=np.float32)
    a = ref.run("serving_default", {"input": x}, OUTS)
    b = fused.run("serving_default", {"input": x}, OUTS)
    assert a["probabilities"].shape == (3, 11)
    np.testing.assert_allclose(a["probabilities"], b["probabilities"], atol=1e-5)
    np.testing.assert_array_equal(a["classes"], b["classes"])


def test_resnext_fully_fused(tiny_resnext):
    _ref, fused = tiny_resnext
    hist = fused.runner("serving_default", ["input"], OUTS).program.op_histogram()
    assert hist.get("_FusedGroupedConv2D") == 4, hist
    for op in ("Conv2D", "FusedBatchNormV3", "Relu", "Pad"):
        assert op not in hist, hist


# ------------------------------------------------------------------ near misses
def _conv_graph(c=32, cg=4, cout=32, known=True, dilation=1, fetch_bn_stat=False, closing="Relu", k=3):
    """x [-1,9,9,c] -> Conv2D(filter [k,k,cg,cout], SAME) -> FusedBatchNormV3 -> closing."""
    rng = np.random.default_rng(7)
    g = GraphBuilder()
    x = g.placeholder("x", T.DT_FLOAT, [-1, 9, 9, c] if known else [-1, -1, -1, -1])
    w = g.const("w", (rng.standard_normal((k, k, cg, cout)) * (k * k * cg) ** -0.5).astype(np.float32))
    y = g.node("Conv2D", "conv", [x, w], T=F32, strides=[1, 1, 1, 1], padding="SAME", data_format="NHWC",
               dilations=[1, dilation, dilation, 1], use_cudnn_on_gpu=True, explicit_paddings=[])
    params = [g.const(name, v.astype(np.float32)) for name, v in (
        ("gamma", 1 + 0.1 * rng.standard_normal(cout)), ("beta", 0.1 * rng.standard_normal(cout)),
        ("mean", 0.1 * rng.standard_normal(cout)), ("var", 1 + 0.1 * np.abs(rng.standard_normal(cout))))]
    bn = g.node("FusedBatchNormV3", "bn", [y] + params, T=F32, U=F32, epsilon=1e-3, data_format="NHWC",
                is_training=False, exponential_avg_factor=1.0)
    g.node(closing, "out", [bn], T=F32)
    return g, ["out:0"] + (["bn:1"] if fetch_bn_stat else [])


def _programs(g, fetches):
    from rust_tensorflow_serving2_amd.graph.compiler import compile_program
    from rust_tensorflow_serving2_amd.graph.fused import default_passes
    from rust_tensorflow_serving2_amd.graph.ir import from_graph_def
    return (compile_program(from_graph_def(g.graph), ["x:0"], fetches),
            compile_program(from_graph_def(g.graph), ["x:0"], fetches, passes=default_passes()))


def _run_both(g, fetches, c=32, seed=1):
    x = torch.from_numpy(np.random.default_rng(seed).standard_normal((2, 9, 9, c)).astype(np.float32))
    ref, fused = _programs(g, fetches)
    a, b = ref.run([x]), fused.run([x])
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert tuple(np.asarray(u).shape) == tuple(np.asarray(v).shape)
        np.testing.assert_allclose(np.asarray(u), np.asarray(v), atol=1e-5)
    return fused.op_histogram()


def test_the_issue_s_example_runs_fused():
    """x [-1,9,9,32] -> Conv2D(filter [3,3,4,32]) -> BN -> Relu: 8 groups of 4."""
    hist = _run_both(*_conv_graph())
    assert hist.get("_FusedGroupedConv2D") == 1, hist
    for op in ("Conv2D", "_FusedConv2D", "FusedBatchNormV3", "Relu"):
        assert op not in hist, hist


def test_groups_1_is_still_a_fused_conv():
    hist = _run_both(*_conv_graph(c=32, cg=32))
    assert hist.get("_FusedConv2D") == 1 and "_FusedGroupedConv2D" not in hist and "Conv2D" not in hist, hist


def test_unknown_channels_fuse_and_the_op_checks_its_input():
    """A placeholder of unknown shape: fuse_conv takes the conv as before, and
    FusedConv, given 32 channels for a filter of in-depth 4, computes the
    grouped conv the original op computes."""
    hist = _run_both(*_conv_graph(known=False))
    assert hist.get("_FusedConv2D") == 1 and "_FusedGroupedConv2D" not in hist and "Conv2D" not in hist, hist


def test_channels_no_multiple_of_the_in_depth_is_left_alone_with_the_interpreter_s_error():
    from rust_tensorflow_serving2_amd.graph import ops as O
    g, fetches = _conv_graph(c=30, cg=4)
    ref, fused = _programs(g, fetches)
    hist = fused.op_histogram()
    assert hist.get("Conv2D") == 1 and "_FusedConv2D" not in hist and "_FusedGroupedConv2D" not in hist, hist
    x = torch.zeros(2, 9, 9, 30)
    errs = []
    for prog in (ref, fused):
        with pytest.raises(O.OpError) as e:
            prog.run([x])
        errs.append(str(e.value))
    assert errs[0] == errs[1] and "Conv2D node 'conv'" in errs[0], errs


def test_unknown_channels_no_multiple_raises_the_interpreter_s_text():
    """The same mismatch behind a placeholder of unknown shape: FusedConv's
    run-time check raises what the interpreter's Conv2D raises (the node's
    name and op aside)."""
    from rust_tensorflow_serving2_amd.graph import ops as O
    g, fetches = _conv_graph(known=False, closing="Identity")
    ref, fused = _programs(g, fetches)
    x = torch.zeros(2, 9, 9, 30)
    errs = []
    for prog in (ref, fused):
        with pytest.raises(O.OpError) as e:
            prog.run([x])
        errs.append(str(e.value).split(": ", 1)[1])
    assert errs[0] == errs[1], errs


def test_dilation_2_is_left_alone():
    hist = _run_both(*_conv_graph(dilation=2))
    assert hist.get("Conv2D") == 1 and "_FusedGroupedConv2D" not in hist and "_FusedConv2D" not in hist, hist
    assert hist.get("FusedBatchNormV3") == 1 and hist.get("Relu") == 1, hist


def test_in_depth_1_is_left_alone():
    """A depthwise conv spelled as Conv2D: neither pass takes it."""
    hist = _run_both(*_conv_graph(c=8, cg=1, cout=8), c=8)
    assert hist.get("Conv2D") == 1 and "_FusedGroupedConv2D" not in hist and "_FusedConv2D" not in hist, hist


def test_batchnorm_with_a_fetched_statistics_output_is_not_folded():
    hist = _run_both(*_conv_graph(fetch_bn_stat=True))
    assert hist.get("_FusedGroupedConv2D") == 1 and hist.get("FusedBatchNormV3") == 1 and hist.get("Relu") == 1, hist


def test_a_closing_relu6_stays_a_node():
    hist = _run_both(*_conv_graph(closing="Relu6"))
    assert hist.get("_FusedGroupedConv2D") == 1 and hist.get("Relu6") == 1, hist
    assert "Conv2D" not in hist and "FusedBatchNormV3" not in hist, hist


def test_unsupported_group_shapes_still_fuse_on_the_cpu():
    """Cg 64, unequal widths per group and a 5x5 filter are no kernel shapes:
    the op is the same, its CPU reference the same torch grouped conv."""
    for kw, c in ((dict(c=128, cg=64, cout=128), 128), (dict(c=32, cg=4, cout=16), 32), (dict(k=5), 32)):
        hist = _run_both(*_conv_graph(**kw), c=c)
        assert hist.get("_FusedGroupedConv2D") == 1 and "Conv2D" not in hist, (kw, hist)


def test_channels_of():
    from rust_tensorflow_serving2_amd.graph.fused import _channels_of
    from rust_tensorflow_serving2_amd.graph.ir import from_graph_def
    from rust_tensorflow_serving2_amd.graph.compiler import _fold

    def folded(g):
        ir = from_graph_def(g.graph)            # (the passes run on the constant-folded IR)
        _fold(ir, list(ir.order), set())
        return ir
    g, _ = _conv_graph(c=32, cg=4, cout=48)
    ir = folded(g)
    assert _channels_of(ir, ("x", 0)) == 32
    assert _channels_of(ir, ("conv", 0)) == 48 and _channels_of(ir, ("bn", 0)) == 48
    assert _channels_of(ir, ("out", 0)) == 48 and _channels_of(ir, ("bn", 1)) is None
    assert _channels_of(ir, ("out", 0), fed={"out"}) is None
    assert _channels_of(ir, ("out", 0), depth=1) is None
    g, _ = _conv_graph(known=False)
    assert _channels_of(folded(g), ("x", 0)) is None and _channels_of(folded(g), ("conv", 0)) == 32


# ------------------------------------------------------------------ the exporter
# sha256 of the GraphDef (deterministic serialization) and of the variables (sorted by name: name bytes, then
# the array's bytes) that build_graph() wrote before it took ``groups`` / ``width_per_group``
PINNED = {
    "v1.5": ("bb1979d7fbb1449bad972c8f9785b9891a2b766b014a13d2d49e137445e011c5",
             "1689b9880878885311a793035362f1631ac5cf93028b2e7b29b53d5291fc9c54", 267),
    "v2": ("3b8de6dbe38be816dc3d88db274bd6049a775fb6588f7bc9dabaad944b625b05",
           "f495017c79a31e136b6e1e1380a70fc8f224380e6474894bc77f4a0680183822", 251),
}


@pytest.mark.parametrize("version", sorted(PINNED))
def test_default_export_is_byte_identical(version):
    from rust_tensorflow_serving2_amd.models import resnet
    g, _sigs, _saver = resnet.build_graph(version)
    h = hashlib.sha256()
    for name in sorted(g.variables):
        h.update(name.encode())
        h.update(np.ascontiguousarray(g.variables[name]).tobytes())
    got = (hashlib.sha256(g.graph.SerializeToString(deterministic=True)).hexdigest(), h.hexdigest(), len(g.variables))
    assert got == PINNED[version]


def test_default_resnet_histogram(models_dir):
    """The op histogram tests/test_fusion.py expects of the tiny v1.5 ResNet."""
    from rust_tensorflow_serving2_amd.models import resnet
    path = os.path.join(str(models_dir), "tiny_resnet_for_resnext", "1")
    resnet.export(path, version="v1.5", blocks=(1, 1, 1, 1), width=16, image_size=32, num_classes=11, seed=5)
    fused = Servable("m", 1, path, ServableOptions(device="cpu", fuse=True))
    hist = fused.runner("serving_default", ["input"], OUTS).program.op_histogram()
    assert "_FusedGroupedConv2D" not in hist, hist
    for op in ("Conv2D", "FusedBatchNormV3", "Relu", "AddV2", "Pad"):
        assert op not in hist, hist


def test_resnext50_full_size_layer_counts():
    """32x4d: 16 grouped 3x3s with 4 / 8 / 16 / 32 channels per group in (3, 4,
    6, 3) proportion and inner widths 128 ... 1024; the three stride-2 ones
    behind a Pad."""
    from rust_tensorflow_serving2_amd.models import resnet
    g, sigs, _saver = resnet.build_graph(groups=32, width_per_group=4)
    assert set(sigs) == {"serving_default", "predict"}
    grouped = collections.Counter()
    for name, arr in g.variables.items():
        if name.endswith("kernel") and arr.ndim == 4 and arr.shape[0] == 3:
            assert arr.shape[3] == 32 * arr.shape[2], (name, arr.shape)
            grouped[arr.shape[2]] += 1
            assert abs(arr.std() - np.sqrt(2.0 / (9 * arr.shape[2]))) < 0.05 * arr.std()      # He-normal, own fan-in
    assert dict(grouped) == {4: 3, 8: 4, 16: 6, 32: 3}
    nodes = {n.name: n for n in g.graph.node}
    pads = [n for n in nodes.values() if n.op == "Pad"]
    before_grouped = [p for p in pads if "/conv2/" in p.name]
    # (the others: the stem's, and the zero-wide ones of the three strided 1x1 shortcuts)
    assert len(pads) == 7 and len(before_grouped) == 3
    for p in before_grouped:
        conv = nodes[p.name.rsplit("/", 1)[0] + "/Conv2D"]
        assert conv.input[0] == p.name and list(conv.attr["strides"].list.i) == [1, 2, 2, 1]
    with pytest.raises(ValueError):
        resnet.build_graph("v2", groups=32, width_per_group=4)
