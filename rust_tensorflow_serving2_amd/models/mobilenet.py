"""MobileNet V1, V2 and V3 (Large / Small) SavedModel exporter with random-init
weights.

The graph layouts cover both padding forms of a strided depthwise conv:

* ``v1`` follows the TF-slim export: ``Conv2D`` 3x3/2 SAME, then 13 separable
  blocks ``DepthwiseConv2dNative`` 3x3 (SAME, stride 1 or 2) -> ``FusedBatchNormV3``
  -> ``Relu6`` -> ``Conv2D`` 1x1 -> ``FusedBatchNormV3`` -> ``Relu6``.
* ``v2`` follows the Keras application: strided 3x3 convs are a ``Pad`` (Keras
  ``correct_pad``) + a VALID conv; inverted residual blocks ``Conv2D`` 1x1 expand
  (x6) -> BN -> ``Relu6`` -> depthwise 3x3 -> BN -> ``Relu6`` -> ``Conv2D`` 1x1
  project -> BN (linear bottleneck), ``AddV2`` shortcut where stride is 1 and
  the channel counts agree; a final 1x1 conv to 1280 channels.
* ``v3_large`` / ``v3_small`` follow the Keras application: stem ``Conv2D``
  3x3/2 (16 channels) -> BN -> hard-swish; the bneck tables of the paper
  (``V3_LARGE`` / ``V3_SMALL``: kernel, expansion, out, SE, activation,
  stride) -- 15 blocks in Large (SE in 4-6 and 11-15, hard-swish from 7 on),
  11 in Small (SE in 1 and 4-11, hard-swish from 4 on).  A block is ``Conv2D``
  1x1 expand -> BN -> act (none in block 1) -> depthwise 3x3 or 5x5 (stride 2:
  ``Pad`` by ``correct_pad`` + VALID) -> BN -> act -> [squeeze-excite] ->
  ``Conv2D`` 1x1 project -> BN, ``AddV2`` shortcut where the shapes agree.
  Squeeze-excite is ``Mean`` (H, W, keep_dims) -> ``Conv2D`` 1x1 + ``BiasAdd``
  (width ``_make_divisible(expansion / 4)``) -> ``Relu`` -> ``Conv2D`` 1x1 +
  ``BiasAdd`` -> hard-sigmoid -> ``Mul(x, gate)``.  The hard activations are
  spelled as Keras exports them: hard-sigmoid ``AddV2(x, 3) -> Relu6 ->
  Mul(., 1/6)``, hard-swish ``Mul(x, hard_sigmoid(x))``.  Then ``Conv2D`` 1x1 to
  960 / 576 -> BN -> hard-swish -> ``Mean`` (keep_dims) -> ``Conv2D`` 1x1 +
  bias to 1280 / 1024 -> hard-swish -> ``Conv2D`` 1x1 + bias to the classes ->
  ``Reshape`` [-1, classes].  The second SE layer's init is scaled so that the
  gates spread over (0, 1) instead of sitting at one value.

Channel counts are rounded to multiples of 8 (``_make_divisible``, as the real
models do).  The head is ``Mean`` over H,W -> ``MatMul`` + ``BiasAdd`` (V1 / V2) ->
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


# V3: (kernel, expansion channels, out channels, squeeze-excite, activation, stride)
V3_LARGE = ((3, 16, 16, False, "relu", 1), (3, 64, 24, False, "relu", 2), (3, 72, 24, False, "relu", 1),
            (5, 72, 40, True, "relu", 2), (5, 120, 40, True, "relu", 1), (5, 120, 40, True, "relu", 1),
            (3, 240, 80, False, "hard_swish", 2), (3, 200, 80, False, "hard_swish", 1),
            (3, 184, 80, False, "hard_swish", 1), (3, 184, 80, False, "hard_swish", 1),
            (3, 480, 112, True, "hard_swish", 1), (3, 672, 112, True, "hard_swish", 1),
            (5, 672, 160, True, "hard_swish", 2), (5, 960, 160, True, "hard_swish", 1),
            (5, 960, 160, True, "hard_swish", 1))
V3_SMALL = ((3, 16, 16, True, "relu", 2), (3, 72, 24, False, "relu", 2), (3, 88, 24, False, "relu", 1),
            (5, 96, 40, True, "hard_swish", 2), (5, 240, 40, True, "hard_swish", 1), (5, 240, 40, True, "hard_swish", 1),
            (5, 120, 48, True, "hard_swish", 1), (5, 144, 48, True, "hard_swish", 1),
            (5, 288, 96, True, "hard_swish", 2), (5, 576, 96, True, "hard_swish", 1),
            (5, 576, 96, True, "hard_swish", 1))
V3_LAST_POINT = {"v3_large": 1280, "v3_small": 1024}
VERSIONS = ("v1", "v2", "v3_large", "v3_small")
# std of the second squeeze-excite FC = sqrt(SE_FC2_GAIN / Cr): gate pre-activations of about
# N(0, 1.5^2), so the gates spread over (0, 1) and a few clamp (a He-normal init leaves them all near 0.5)
SE_FC2_GAIN = 14.0
# init gains, on top of He-normal, of the projection behind a squeeze-excite (the gates average about
# 1/2) and of the expand conv.  They place each random net between two failures (docs/numerics.md,
# "MobileNetV3 end to end"; scripts/bf16_emulation.py prints both figures on the CPU):
#  * too low, and nothing of the image is left in the logits.  Small gates 9 of its 11 blocks: at a
#    gated gain of 1 its logits' spread over a batch is 1 % of their spread over the classes (7 % at
#    1.5); Large at 0.9 / 0.9 has no row whose top-1 is decidable;
#  * too high, and the net is chaotic: a perturbation of an activation grows from block to block, the
#    rounding of every stored bf16 layer included.  Small at a gated gain of 2 is off by up to 12 % of
#    the logit spread in bf16, Large at 1 / 1 by 4-6 %; with the values below 2 % and 2-4 %.
V3_GATED_PROJECT_GAIN = {"v3_large": 0.9, "v3_small": 1.5}
V3_EXPAND_GAIN = {"v3_large": 0.95, "v3_small": 1.0}


def _make_divisible(v: float, divisor: int = 8) -> int:
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new_v < 0.9 * v:
        new_v += divisor
    return new_v


def _relu6(g, x):
    return g.node("Relu6", "Relu6", [x], T=F32)


def _hard_sigmoid(g, x):
    """The Keras node form: AddV2(x, 3) -> Relu6 -> Mul(., 1/6)."""
    y = g.node("AddV2", "add", [x, g.const("add/y", np.array(3.0, np.float32))], T=F32)
    y = g.node("Relu6", "Relu6", [y], T=F32)
    return g.node("Mul", "mul", [y, g.const("mul/y", np.array(1.0 / 6.0, np.float32))], T=F32)


def _hard_swish(g, x, name="hard_swish"):
    with g.scope(name):
        return g.node("Mul", "mul_1", [x, _hard_sigmoid(g, x)], T=F32)


def _act(g, x, act, name):
    if act == "hard_swish":
        return _hard_swish(g, x, name)
    with g.scope(name):
        return g.node("Relu", "Relu", [x], T=F32)


def _bias(g, init, x, c, scale=0.1):
    b = g.variable("bias", (scale * init.rng.standard_normal(c)).astype(np.float32))
    return g.node("BiasAdd", "BiasAdd", [x, b], T=F32, data_format="NHWC")


def _squeeze_excite(g, init, x, c, cr):
    with g.scope("squeeze_excite"):
        axes = g.const("AvgPool/reduction_indices", np.array([1, 2], np.int32))
        p = g.node("Mean", "AvgPool", [x, axes], T=F32, Tidx=DType(T.DT_INT32), keep_dims=True)
        with g.scope("Conv"):
            h = _bias(g, init, _conv(g, init, p, 1, c, cr, 1, "SAME", "conv"), cr)
        h = g.node("Relu", "Relu", [h], T=F32)
        with g.scope("Conv_1"):
            w = g.variable("kernel", (init.rng.standard_normal((1, 1, cr, c)) *
                                      np.sqrt(SE_FC2_GAIN / cr)).astype(np.float32))
            h = g.node("Conv2D", "Conv2D", [h, w], T=F32, strides=[1, 1, 1, 1], padding="SAME", data_format="NHWC",
                       dilations=[1, 1, 1, 1], use_cudnn_on_gpu=True, explicit_paddings=[])
            h = _bias(g, init, h, c, scale=0.5)
        with g.scope("hard_sigmoid"):
            gate = _hard_sigmoid(g, h)
        return g.node("Mul", "Mul", [x, gate], T=F32)


def _correct_pad(g, x, size: int, k: int = 3):
    """Keras ``correct_pad`` + ``ZeroPadding2D`` in front of a strided VALID conv."""
    adjust = 1 - size % 2
    correct = k // 2
    beg, end = correct - adjust, correct
    pads = g.const("pad/paddings", np.array([[0, 0], [beg, end], [beg, end], [0, 0]], np.int32))
    return g.node("Pad", "pad", [x, pads], T=F32, Tpaddings=DType(T.DT_INT32)), size + beg + end


def _conv(g, init, x, k, cin, cout, stride, padding, name, gain=1.0):
    with g.scope(name):
        w = g.variable("kernel", init.conv(k, k, cin, cout) * np.float32(gain))
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


def _build_v3(g, init, x, alpha, size, version):
    """-> (feature map, channels, hidden width of the head's first 1x1 conv)."""
    table = V3_LARGE if version == "v3_large" else V3_SMALL
    with g.scope("MobilenetV3" + ("large" if version == "v3_large" else "small")):
        c = 16
        y = _conv(g, init, x, 3, 3, c, 2, "SAME", "Conv")
        y = _hard_swish(g, _bn(g, init, y, c, "Conv/BatchNorm", eps=1e-3), "Conv/hard_swish")
        size = _out_size(size, 3, 2, "SAME")
        for i, (k, exp, out, se, act, stride) in enumerate(table):
            hidden, cout = _make_divisible(exp * alpha), _make_divisible(out * alpha)
            with g.scope("expanded_conv" if i == 0 else f"expanded_conv_{i}"):
                inp, h = y, y
                if i == 0:
                    hidden = c                 # block 1 has no expand conv
                else:
                    h = _conv(g, init, h, 1, c, hidden, 1, "SAME", "expand", gain=V3_EXPAND_GAIN[version])
                    h = _act(g, _bn(g, init, h, hidden, "expand/BatchNorm", eps=1e-3), act, "expand/act")
                if stride == 2:
                    with g.scope("depthwise"):
                        h, padded = _correct_pad(g, h, size, k)
                    h = _depthwise(g, init, h, hidden, 2, "VALID", "depthwise", k)
                    size = _out_size(padded, k, 2, "VALID")
                else:
                    h = _depthwise(g, init, h, hidden, 1, "SAME", "depthwise", k)
                h = _act(g, _bn(g, init, h, hidden, "depthwise/BatchNorm", eps=1e-3), act, "depthwise/act")
                if se:
                    h = _squeeze_excite(g, init, h, hidden, _make_divisible(hidden / 4))
                h = _conv(g, init, h, 1, hidden, cout, 1, "SAME", "project",
                          gain=V3_GATED_PROJECT_GAIN[version] if se else 1.0)
                h = _bn(g, init, h, cout, "project/BatchNorm", gamma_scale=0.5 if (stride == 1 and c == cout) else 1.0,
                        eps=1e-3)
                if stride == 1 and c == cout:
                    h = g.node("AddV2", "Add", [inp, h], T=F32)
                y, c = h, cout
        last = _make_divisible(c * 6)
        y = _conv(g, init, y, 1, c, last, 1, "SAME", "Conv_1")
        y = _hard_swish(g, _bn(g, init, y, last, "Conv_1/BatchNorm", eps=1e-3), "Conv_1/hard_swish")
    point = V3_LAST_POINT[version]
    return y, last, _make_divisible(point * alpha) if alpha > 1.0 else point


def build_graph(version: str = "v1", alpha: float = 1.0, image_size: int = 224, num_classes: int = NUM_CLASSES,
                seed: int = 0):
    if version not in VERSIONS:
        raise ValueError(f"MobileNet version must be 'v1', 'v2', 'v3_large' or 'v3_small', got {version!r}")
    g = GraphBuilder()
    init = _Init(seed)
    x = g.placeholder("input_tensor", T.DT_FLOAT, [-1, image_size, image_size, 3])
    axes = g.const("Mean/reduction_indices", np.array([1, 2], np.int32))
    if version in ("v3_large", "v3_small"):
        y, cin, point = _build_v3(g, init, x, alpha, image_size, version)
        y = g.node("Mean", "Mean", [y, axes], T=F32, Tidx=DType(T.DT_INT32), keep_dims=True)
        with g.scope("Conv_2"):
            y = _bias(g, init, _conv(g, init, y, 1, cin, point, 1, "SAME", "conv"), point, scale=0.01)
            y = _hard_swish(g, y)
        with g.scope("Logits"):
            w = g.variable("kernel", (init.rng.standard_normal((1, 1, point, num_classes)) *
                                      np.sqrt(1.0 / point)).astype(np.float32))
            y = g.node("Conv2D", "Conv2D", [y, w], T=F32, strides=[1, 1, 1, 1], padding="SAME", data_format="NHWC",
                       dilations=[1, 1, 1, 1], use_cudnn_on_gpu=True, explicit_paddings=[])
            y = _bias(g, init, y, num_classes, scale=0.01)
            shape = g.const("Reshape/shape", np.array([-1, num_classes], np.int32))
            y = g.node("Reshape", "Reshape", [y, shape], T=F32, Tshape=DType(T.DT_INT32))
    else:
        y, cin = (_build_v1 if version == "v1" else _build_v2)(g, init, x, alpha, image_size)
        y = g.node("Mean", "Mean", [y, axes], T=F32, Tidx=DType(T.DT_INT32), keep_dims=False)
        with g.scope("Logits"):
            w = g.variable("kernel", (init.rng.standard_normal((cin, num_classes)) *
                                      np.sqrt(1.0 / cin)).astype(np.float32))
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
