"""MobileNet V1 and V2 SavedModel exporter with random-init weights.

Two graph layouts, so that both padding forms of a strided depthwise conv are
covered:

* ``v1`` follows the TF-slim export: ``Conv2D`` 3x3/2 SAME, then 13 separable
  blocks ``DepthwiseConv2dNative`` 3x3 (SAME, stride 1 or 2) -> ``FusedBatchNormV3``
  -> ``Relu6`` -> ``Conv2D`` 1x1 -> ``FusedBatchNormV3`` -> ``Relu6``.
* ``v2`` follows the Keras application: strided 3x3 convs are a ``Pad`` (Keras
  ``correct_pad``) + a VALID conv; inverted residual blocks ``Conv2D`` 1x1 expand
  (x6) -> BN -> ``Relu6`` -> depthwise 3x3 -> BN -> ``Relu6`` -> ``Conv2D`` 1x1
  project -> BN (linear bottleneck), ``AddV2`` shortcut where stride is 1 and
  the channel counts agree; a final 1x1 conv to 1280 channels.

Channel counts are rounded to multiples of 8 (``_make_divisible``, as the real
models do).  The head is ``Mean`` over H,W -> ``MatMul`` + ``BiasAdd`` ->
``ArgMax`` (``classes``, int64) and ``Softmax`` (``probabilities``); the
interface is ResNet's (models/resnet.py): alias ``"input"``, signatures
``serving_default`` and ``predict``.  Weights are random (He-normal convs, mild
BN statistics); the exported bytes are a genuine TF1 SavedModel.
"""
from __future__ import annotations

import numpy as np

from ..graph.builder import PREDICT_METHOD, DType, GraphBuilder, signature, tensor_info
from ..savedmodel.saved_model import write_saved_model
from ..utils import tensors as T
from .resnet import _bn, _Init

F32 = DType(T.DT_FLOAT)
NUM_CLASSES = 1001

# V1: (pointwise filters, depthwise stride) of the 13 separable blocks
V1_BLOCKS = ((64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2), (512, 1), (512, 1), (512, 1), (512, 1),
             (512, 1), (1024, 2), (1024, 1))
# V2: (expansion t, channels c, repeats n, first stride s)
V2_BLOCKS = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))


def _make_divisible(v: float, divisor: int = 8) -> int:
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def _relu6(g, x):
    return g.node("Relu6", "Relu6", [x], T=F32)


def _correct_pad(g, x, size: int, k: int = 3):
    """Keras ``correct_pad`` + ``ZeroPadding2D`` in front of a strided VALID conv."""
    adjust = 1 - size % 2
    correct = k // 2
    beg, end = correct - adjust, correct
    pads = g.const("pad/paddings", np.array([[0, 0], [beg, end], [beg, end], [0, 0]], np.int32))
    return g.node("Pad", "pad", [x, pads], T=F32, Tpaddings=DType(T.DT_INT32)), size + beg + end


def _conv(g, init, x, k, cin, cout, stride, padding, name):
    with g.scope(name):
        w = g.variable("kernel", init.conv(k, k, cin, cout))
        return g.node("Conv2D", "Conv2D", [x, w], T=F32, strides=[1, stride, stride, 1], padding=padding,
                      data_format="NHWC", dilations=[1, 1, 1, 1], use_cudnn_on_gpu=True, explicit_paddings=[])


def _depthwise(g, init, x, c, stride, padding, name, k=3):
    with g.scope(name):
        # He-normal over the k x k taps of the one input channel each output reads
        w = g.variable("depthwise_kernel", (init.rng.standard_normal((k, k, c, 1)) *
                                            np.sqrt(2.0 / (k * k))).astype(np.float32))
        return g.node("DepthwiseConv2dNative", "depthwise", [x, w], T=F32, strides=[1, stride, stride, 1],
                      padding=padding, data_format="NHWC", dilations=[1, 1, 1, 1], explicit_paddings=[])


def _out_size(size: int, k: int, stride: int, padding: str) -> int:
    return -(-size // stride) if padding == "SAME" else (size - k) // stride + 1


def _build_v1(g, init, x, alpha, size):
    with g.scope("MobilenetV1"):
        c = _make_divisible(32 * alpha)
        y = _conv(g, init, x, 3, 3, c, 2, "SAME", "Conv2d_0")
        y = _relu6(g, _bn(g, init, y, c, "Conv2d_0/BatchNorm", eps=1e-3))
        size = _out_size(size, 3, 2, "SAME")
        for i, (filters, stride) in enumerate(V1_BLOCKS, 1):
            cout = _make_divisible(filters * alpha)
            y = _depthwise(g, init, y, c, stride, "SAME", f"Conv2d_{i}_depthwise")
            y = _relu6(g, _bn(g, init, y, c, f"Conv2d_{i}_depthwise/BatchNorm", eps=1e-3))
            y = _conv(g, init, y, 1, c, cout, 1, "SAME", f"Conv2d_{i}_pointwise")
            y = _relu6(g, _bn(g, init, y, cout, f"Conv2d_{i}_pointwise/BatchNorm", eps=1e-3))
            size = _out_size(size, 3, stride, "SAME")
            c = cout
    return y, c


def _build_v2(g, init, x, alpha, size):
    with g.scope("mobilenetv2"):
        c = _make_divisible(32 * alpha)
        with g.scope("Conv1"):
            y, padded = _correct_pad(g, x, size)
        y = _conv(g, init, y, 3, 3, c, 2, "VALID", "Conv1")
        y = _relu6(g, _bn(g, init, y, c, "bn_Conv1", eps=1e-3))
        size = _out_size(padded, 3, 2, "VALID")
        block = 0
        for t, ch, reps, first_stride in V2_BLOCKS:
            cout = _make_divisible(ch * alpha)
            for r in range(reps):
                stride = first_stride if r == 0 else 1
                name = "expanded_conv" if block == 0 else f"block_{block}"
                with g.scope(name):
                    inp, h, hidden = y, y, c * t
                    if t != 1:
                        h = _conv(g, init, h, 1, c, hidden, 1, "SAME", "expand")
                        h = _relu6(g, _bn(g, init, h, hidden, "expand_BN", eps=1e-3))
                    if stride == 2:
                        h, padded = _correct_pad(g, h, size)
                        h = _depthwise(g, init, h, hidden, 2, "VALID", "depthwise")
                        size = _out_size(padded, 3, 2, "VALID")
                    else:
                        h = _depthwise(g, init, h, hidden, 1, "SAME", "depthwise")
                    h = _relu6(g, _bn(g, init, h, hidden, "depthwise_BN", eps=1e-3))
                    h = _conv(g, init, h, 1, hidden, cout, 1, "SAME", "project")
                    h = _bn(g, init, h, cout, "project_BN", gamma_scale=0.5 if (stride == 1 and c == cout) else 1.0,
                            eps=1e-3)
                    if stride == 1 and c == cout:
                        h = g.node("AddV2", "add", [inp, h], T=F32)
                    y, c = h, cout
                block += 1
        last = _make_divisible(1280 * alpha) if alpha > 1.0 else 1280
        y = _conv(g, init, y, 1, c, last, 1, "VALID", "Conv_1")
        y = _relu6(g, _bn(g, init, y, last, "Conv_1_bn", eps=1e-3))
    return y, last


def build_graph(version: str = "v1", alpha: float = 1.0, image_size: int = 224, num_classes: int = NUM_CLASSES,
                seed: int = 0):
    if version not in ("v1", "v2"):
        raise ValueError(f"MobileNet version must be 'v1' or 'v2', got {version!r}")
    g = GraphBuilder()
    init = _Init(seed)
    x = g.placeholder("input_tensor", T.DT_FLOAT, [-1, image_size, image_size, 3])
    y, cin = (_build_v1 if version == "v1" else _build_v2)(g, init, x, alpha, image_size)
    axes = g.const("Mean/reduction_indices", np.array([1, 2], np.int32))
    y = g.node("Mean", "Mean", [y, axes], T=F32, Tidx=DType(T.DT_INT32), keep_dims=False)
    with g.scope("Logits"):
        w = g.variable("kernel", (init.rng.standard_normal((cin, num_classes)) * np.sqrt(1.0 / cin)).astype(np.float32))
        b = g.variable("bias", (0.01 * init.rng.standard_normal(num_classes)).astype(np.float32))
        y = g.node("MatMul", "MatMul", [y, w], T=F32, transpose_a=False, transpose_b=False)
        y = g.node("BiasAdd", "BiasAdd", [y, b], T=F32, data_format="NHWC")
    logits = g.node("Identity", "final_dense", [y], T=F32)
    dim = g.const("ArgMax/dimension", np.array(1, np.int32))
    classes = g.node("ArgMax", "ArgMax", [logits, dim], T=F32, Tidx=DType(T.DT_INT32), output_type=DType(T.DT_INT64))
    probs = g.node("Softmax", "softmax_tensor", [logits], T=F32)
    saver = g.add_saver()
    ins = {"input": tensor_info(x, T.DT_FLOAT, [-1, image_size, image_size, 3])}
    outs = {"classes": tensor_info(classes, T.DT_INT64, [-1]),
            "probabilities": tensor_info(probs, T.DT_FLOAT, [-1, num_classes])}
    sig = signature(ins, outs, PREDICT_METHOD)
    return g, {"serving_default": sig, "predict": sig}, saver


def export(export_dir: str, version: str = "v1", alpha: float = 1.0, image_size: int = 224,
           num_classes: int = NUM_CLASSES, seed: int = 0) -> str:
    g, sigs, saver = build_graph(version, alpha, image_size, num_classes, seed)
    return write_saved_model(export_dir, g.graph, sigs, g.variables, g.var_dtypes, saver)
