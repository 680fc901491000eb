"""ConvNeXt SavedModel exporter with random-init weights, in the layout of the
Keras application from the stem on (the input is taken as already normalised,
as models/mobilenet.py takes it).  The defaults are ConvNeXt-T.

* Stem: ``Conv2D`` 4x4/4 to ``dims[0]`` + ``BiasAdd`` -> LayerNorm (eps 1e-6).
* Four stages of ``depths[i]`` blocks at ``dims[i]`` channels.  A block is
  ``DepthwiseConv2dNative`` 7x7 SAME + ``BiasAdd`` -> LayerNorm -> ``Conv2D``
  1x1 to 4C + ``BiasAdd`` -> erf GELU (the Keras spelling: ``Mul(0.5, x)``,
  ``RealDiv(x, sqrt 2)`` -> ``Erf`` -> ``AddV2(1, .)`` -> ``Mul``) -> ``Conv2D``
  1x1 to C + ``BiasAdd`` -> ``Mul`` by the ``[C]`` layer scale -> ``AddV2`` with
  the block's input.
* Between stages: LayerNorm -> ``Conv2D`` 2x2/2 + ``BiasAdd``.
* Head: ``Mean`` over H, W -> LayerNorm -> ``MatMul`` + ``BiasAdd`` ->
  ``ArgMax`` (``classes``, int64) and ``Softmax`` (``probabilities``); the
  interface is ResNet's (models/resnet.py).

Every LayerNorm is spelled as ``tf.nn.moments`` + ``tf.nn.batch_normalization``
emit it (``Mean``, ``SquaredDifference`` through ``StopGradient``, ``Rsqrt``,
..., with ``keep_dims``), over the last axis.

The pointwise layers are 1x1 ``Conv2D``s.  Keras spells them as ``Dense`` on a
4-D tensor (Tensordot: ``Reshape -> MatMul -> Reshape``); that spelling stays
correct through the interpreter's ops, but fusing it is out of scope here.

Weights are random (He-normal convs, unit-ish LayerNorm affines); the exported
bytes are a genuine TF1 SavedModel.
"""
from __future__ import annotations

import numpy as np

from ..graph.builder import PREDICT_METHOD, DType, GraphBuilder, signature, tensor_info
from ..savedmodel.saved_model import write_saved_model
from ..utils import tensors as T
from .bert import layer_norm
from .mobilenet import _bias, _conv, _depthwise
from .resnet import _Init

F32 = DType(T.DT_FLOAT)
NUM_CLASSES = 1000
DEPTHS_TINY = (3, 3, 9, 3)
DIMS_TINY = (96, 192, 384, 768)
LN_EPS = 1e-6
# The paper's layer-scale init of 1e-6 makes a random net ignore its blocks (the logits would be the
# stem's and the downsampling convs' alone).  Chosen on the CPU with scripts/bf16_emulation.py --family
# convnext (docs/numerics.md, "ConvNeXt-T end to end"; profiles/convnext/bf16_emulation_layer_scale_cpu.log),
# 64 x 64 images, model seed 3, logit error / logit spread of the bf16 emulation (limit 5 %) and how far
# the logits follow the image (std over the batch / spread over the classes):
#   0.5   2.6-5.0 %   0.24        0.3   2.2-3.7 %   0.22        0.2   2.0-3.3 %   0.21        0.1   1.8-3.2 %   0.20
# The error has a floor of about 2 % that no layer scale removes: the largest of 1000 logits' errors after
# some 25 bf16 roundings of a 768-wide feature vector.  Above 0.3 the 18 blocks add to it visibly; 0.2 sits
# on the floor while the blocks still shape the logits (at 0.1 they start to drop out of them).
LAYER_SCALE_INIT = 0.2


def _gelu_erf(g, x, name):
    """Keras ``gelu(approximate=False)``: 0.5 * x * (1 + erf(x / sqrt(2)))."""
    with g.scope(name):
        half = g.node("Mul", "mul", [g.const("mul/x", np.array(0.5, np.float32)), x], T=F32)
        q = g.node("RealDiv", "truediv", [x, g.const("Cast/x", np.array(np.sqrt(2.0), np.float32))], T=F32)
        e = g.node("Erf", "Erf", [q], T=F32)
        a = g.node("AddV2", "add", [g.const("add/x", np.array(1.0, np.float32)), e], T=F32)
        return g.node("Mul", "mul_1", [half, a], T=F32)


def _conv_bias(g, init, x, k, cin, cout, stride, padding, name):
    y = _conv(g, init, x, k, cin, cout, stride, padding, name)
    with g.scope(name):
        return _bias(g, init, y, cout)


def _block(g, init, x, c, name, layer_scale_init):
    h = _depthwise(g, init, x, c, 1, "SAME", f"{name}_depthwise_conv", 7)
    with g.scope(f"{name}_depthwise_conv"):
        h = _bias(g, init, h, c)
    h = layer_norm(g, h, c, init.rng, LN_EPS, f"{name}_layernorm")
    h = _conv_bias(g, init, h, 1, c, 4 * c, 1, "SAME", f"{name}_pointwise_conv_1")
    h = _gelu_erf(g, h, f"{name}_gelu")
    h = _conv_bias(g, init, h, 1, 4 * c, c, 1, "SAME", f"{name}_pointwise_conv_2")
    with g.scope(f"{name}_layer_scale"):
        gamma = g.variable("gamma", (layer_scale_init * (1.0 + 0.1 * init.rng.standard_normal(c))).astype(np.float32))
        h = g.node("Mul", "mul", [h, gamma], T=F32)
    return g.node("AddV2", f"{name}_add/add", [x, h], T=F32)


def _build(g, init, x, depths, dims, layer_scale_init):
    with g.scope("convnext"):
        y = _conv_bias(g, init, x, 4, 3, dims[0], 4, "VALID", "stem/conv")
        y = layer_norm(g, y, dims[0], init.rng, LN_EPS, "stem/layernorm")
        for stage, (depth, c) in enumerate(zip(depths, dims)):
            if stage > 0:
                y = layer_norm(g, y, dims[stage - 1], init.rng, LN_EPS, f"downsampling_block_{stage - 1}/layernorm")
                y = _conv_bias(g, init, y, 2, dims[stage - 1], c, 2, "VALID", f"downsampling_block_{stage - 1}/conv")
            for b in range(depth):
                y = _block(g, init, y, c, f"stage_{stage}_block_{b}", layer_scale_init)
    return y, dims[-1]


def build_graph(depths=DEPTHS_TINY, dims=DIMS_TINY, image_size: int = 224, num_classes: int = NUM_CLASSES,
                seed: int = 0, layer_scale_init: float = LAYER_SCALE_INIT):
    if len(depths) != 4 or len(dims) != 4:
        raise ValueError(f"depths and dims have four stages each, got {depths!r} and {dims!r}")
    if image_size % 32:
        raise ValueError(f"image_size must be a multiple of 32 (the stem and three 2x2/2 convs), got {image_size}")
    g = GraphBuilder()
    init = _Init(seed)
    x = g.placeholder("input_tensor", T.DT_FLOAT, [-1, image_size, image_size, 3])
    y, cin = _build(g, init, x, tuple(depths), tuple(dims), layer_scale_init)
    axes = g.const("avg_pool/Mean/reduction_indices", np.array([1, 2], np.int32))
    y = g.node("Mean", "avg_pool/Mean", [y, axes], T=F32, Tidx=DType(T.DT_INT32), keep_dims=False)
    y = layer_norm(g, y, cin, init.rng, LN_EPS, "head_layer/layernorm")
    with g.scope("head_layer/predictions"):
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


def export(export_dir: str, depths=DEPTHS_TINY, dims=DIMS_TINY, image_size: int = 224, num_classes: int = NUM_CLASSES,
           seed: int = 0, layer_scale_init: float = LAYER_SCALE_INIT) -> str:
    g, sigs, saver = build_graph(depths, dims, image_size, num_classes, seed, layer_scale_init)
    return write_saved_model(export_dir, g.graph, sigs, g.variables, g.var_dtypes, saver)
