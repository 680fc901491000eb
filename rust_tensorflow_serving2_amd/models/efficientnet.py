"""EfficientNet-B0 SavedModel exporter with random-init weights, in the layout
of the Keras application from the stem's padding on (the input is taken as
already normalised, as models/mobilenet.py takes it).

* Stem: ``Pad`` (Keras ``correct_pad``) + VALID ``Conv2D`` 3x3/2 to 32 ->
  ``FusedBatchNormV3`` (eps 1e-3) -> swish.
* Seven stages of MBConv blocks (``BLOCKS``: kernel, repeats, in, out, expand
  ratio, first stride).  A block is ``Conv2D`` 1x1 expand -> BN -> swish
  (omitted at ratio 1) -> depthwise k x k (stride 2: ``Pad`` + VALID; SAME
  otherwise) -> BN -> swish -> squeeze-excite -> ``Conv2D`` 1x1 project -> BN,
  ``AddV2`` shortcut where the stride is 1 and the channel counts agree.
* Squeeze-excite: ``Mean`` (H, W) -> ``Reshape`` [-1, 1, 1, C] -> ``Conv2D`` 1x1 +
  ``BiasAdd`` -> swish -> ``Conv2D`` 1x1 + ``BiasAdd`` -> ``Sigmoid`` ->
  ``Mul(x, gate)``, of width ``max(1, in / 4)`` of the block's *input* filters
  (B0: 8, 4, 6, 10, 20, 28, 48).
* Tail: ``Conv2D`` 1x1 to 1280 -> BN -> swish -> ``Mean`` over H, W -> ``MatMul``
  + ``BiasAdd`` -> ``ArgMax`` (``classes``, int64) and ``Softmax``
  (``probabilities``); the interface is ResNet's (models/resnet.py).

``swish_form`` picks the spelling of every swish: ``"plain"`` ``Mul(x,
Sigmoid(x))``; ``"beta"`` ``Mul(x, Sigmoid(Mul(x, 1.0)))`` (TF >= 2.4's
``swish_impl``); ``"identity_n"`` the beta form behind output 0 of the
``custom_gradient`` wrapper's ``IdentityN(y, x, beta)``.

``width_coefficient`` / ``depth_coefficient`` scale the filters (to multiples
of 8, ``round_filters``) and the repeats (``ceil``) as the paper's compound
scaling does; (1.0, 1.0) is B0.  Weights are random (He-normal convs with the
gains below, mild BN statistics); the exported bytes are a genuine TF1
SavedModel.
"""
from __future__ import annotations

import math

import numpy as np

from ..graph.builder import PREDICT_METHOD, DType, GraphBuilder, signature, tensor_info
from ..savedmodel.saved_model import write_saved_model
from ..utils import tensors as T
from .mobilenet import _bias, _conv, _correct_pad, _depthwise, _out_size
from .resnet import _bn, _Init

F32 = DType(T.DT_FLOAT)
NUM_CLASSES = 1000

# (kernel, repeats, filters in, filters out, expand ratio, first stride)
BLOCKS = ((3, 1, 32, 16, 1, 1), (3, 2, 16, 24, 6, 2), (5, 2, 24, 40, 6, 2), (3, 3, 40, 80, 6, 2),
          (5, 3, 80, 112, 6, 1), (5, 4, 112, 192, 6, 2), (3, 1, 192, 320, 6, 1))
SWISH_FORMS = ("plain", "beta", "identity_n")
# std of the second squeeze-excite FC = sqrt(SE_FC2_GAIN / Cr), as models/mobilenet.py sets it: gate
# pre-activations of a few units' spread, so the sigmoid gates cover (0, 1) instead of sitting at 1/2
SE_FC2_GAIN = 14.0
# init gains on top of He-normal, chosen on the CPU in scripts/bf16_emulation.py --family efficientnet
# (docs/numerics.md, "EfficientNet-B0 end to end"; profiles/efficientnet/bf16_emulation_gains_cpu.log).
# He-normal assumes a ReLU, which passes half the variance; swish passes less of it at unit scale and the
# sigmoid gates halve the amplitude once more, so the window between the two failures is narrow:
#  * too low, and nothing of the image is left in the logits after 16 blocks: at 1 / 1 their spread over
#    a batch is 0.000 of their spread over the classes, at 1.6 / 1.2 it is 0.03 and no seed of 0..2 has
#    two decidable rows;
#  * too high, and the net is chaotic (every bf16 rounding grows from block to block): 1.8 / 1.2 is off by
#    2.6-4.1 % of the logit spread in the bf16 emulation, limit 5 %, and 2.5 / 1.4 overflows.
# 1.7 / 1.2: image dependence 0.06-0.08, emulated error 1.5-2.2 %.
GATED_PROJECT_GAIN = 1.7
EXPAND_GAIN = 1.2


def round_filters(filters: int, width_coefficient: float, divisor: int = 8) -> int:
    filters *= width_coefficient
    new = max(divisor, int(filters + divisor / 2) // divisor * divisor)
    if new < 0.9 * filters:
        new += divisor
    return int(new)


def round_repeats(repeats: int, depth_coefficient: float) -> int:
    return int(math.ceil(depth_coefficient * repeats))


def _swish(g, x, name, form):
    with g.scope(name):
        if form == "plain":
            return g.node("Mul", "mul", [x, g.node("Sigmoid", "Sigmoid", [x], T=F32)], T=F32)
        beta = g.const("beta", np.array(1.0, np.float32))
        s = g.node("Sigmoid", "Sigmoid", [g.node("Mul", "mul", [x, beta], T=F32)], T=F32)
        y = g.node("Mul", "mul_1", [x, s], T=F32)
        if form == "beta":
            return y
        return g.node("IdentityN", "IdentityN", [y, x, beta], T=[F32, F32, F32])


def _squeeze_excite(g, init, x, c, cr, name, form):
    axes = g.const(f"{name}se_squeeze/Mean/reduction_indices", np.array([1, 2], np.int32))
    p = g.node("Mean", f"{name}se_squeeze/Mean", [x, axes], T=F32, Tidx=DType(T.DT_INT32), keep_dims=False)
    shape = g.const(f"{name}se_reshape/Reshape/shape", np.array([-1, 1, 1, c], np.int32))
    p = g.node("Reshape", f"{name}se_reshape/Reshape", [p, shape], T=F32, Tshape=DType(T.DT_INT32))
    with g.scope(f"{name}se_reduce"):
        h = _bias(g, init, _conv(g, init, p, 1, c, cr, 1, "SAME", "conv"), cr)
    h = _swish(g, h, f"{name}se_reduce/swish", form)
    with g.scope(f"{name}se_expand"):
        w = g.variable("kernel", (init.rng.standard_normal((1, 1, cr, c)) * np.sqrt(SE_FC2_GAIN / cr)).astype(np.float32))
        h = g.node("Conv2D", "Conv2D", [h, w], T=F32, strides=[1, 1, 1, 1], padding="SAME", data_format="NHWC",
                   dilations=[1, 1, 1, 1], use_cudnn_on_gpu=True, explicit_paddings=[])
        h = _bias(g, init, h, c, scale=0.5)
        gate = g.node("Sigmoid", "Sigmoid", [h], T=F32)
    return g.node("Mul", f"{name}se_excite/mul", [x, gate], T=F32)


def _build(g, init, x, width, depth, size, form):
    with g.scope("efficientnet"):
        c = round_filters(32, width)
        with g.scope("stem_conv_pad"):
            y, padded = _correct_pad(g, x, size, 3)
        y = _conv(g, init, y, 3, 3, c, 2, "VALID", "stem_conv")
        y = _swish(g, _bn(g, init, y, c, "stem_bn", eps=1e-3), "stem_activation", form)
        size = _out_size(padded, 3, 2, "VALID")
        for stage, (k, repeats, fin, fout, ratio, first_stride) in enumerate(BLOCKS, 1):
            fin, fout = round_filters(fin, width), round_filters(fout, width)
            for r in range(round_repeats(repeats, depth)):
                stride = first_stride if r == 0 else 1
                cin = fin if r == 0 else fout
                name = f"block{stage}{chr(ord('a') + r)}_"
                inp, h, hidden = y, y, cin * ratio
                if ratio != 1:
                    h = _conv(g, init, h, 1, cin, hidden, 1, "SAME", f"{name}expand_conv", gain=EXPAND_GAIN)
                    h = _swish(g, _bn(g, init, h, hidden, f"{name}expand_bn", eps=1e-3), f"{name}expand_activation", form)
                if stride == 2:
                    with g.scope(f"{name}dwconv_pad"):
                        h, padded = _correct_pad(g, h, size, k)
                    h = _depthwise(g, init, h, hidden, 2, "VALID", f"{name}dwconv", k)
                    size = _out_size(padded, k, 2, "VALID")
                else:
                    h = _depthwise(g, init, h, hidden, 1, "SAME", f"{name}dwconv", k)
                h = _swish(g, _bn(g, init, h, hidden, f"{name}bn", eps=1e-3), f"{name}activation", form)
                h = _squeeze_excite(g, init, h, hidden, max(1, cin // 4), name, form)
                h = _conv(g, init, h, 1, hidden, fout, 1, "SAME", f"{name}project_conv", gain=GATED_PROJECT_GAIN)
                shortcut = stride == 1 and cin == fout
                h = _bn(g, init, h, fout, f"{name}project_bn", gamma_scale=0.5 if shortcut else 1.0, eps=1e-3)
                if shortcut:
                    h = g.node("AddV2", f"{name}add/add", [inp, h], T=F32)
                y = h
            c = fout
        last = round_filters(1280, width)
        y = _conv(g, init, y, 1, c, last, 1, "SAME", "top_conv")
        y = _swish(g, _bn(g, init, y, last, "top_bn", eps=1e-3), "top_activation", form)
    return y, last


def build_graph(width_coefficient: float = 1.0, depth_coefficient: float = 1.0, image_size: int = 224,
                num_classes: int = NUM_CLASSES, seed: int = 0, swish_form: str = "beta"):
    if swish_form not in SWISH_FORMS:
        raise ValueError(f"swish_form must be one of {SWISH_FORMS}, got {swish_form!r}")
    g = GraphBuilder()
    init = _Init(seed)
    x = g.placeholder("input_tensor", T.DT_FLOAT, [-1, image_size, image_size, 3])
    y, cin = _build(g, init, x, width_coefficient, depth_coefficient, image_size, swish_form)
    axes = g.const("avg_pool/Mean/reduction_indices", np.array([1, 2], np.int32))
    y = g.node("Mean", "avg_pool/Mean", [y, axes], T=F32, Tidx=DType(T.DT_INT32), keep_dims=False)
    with g.scope("predictions"):
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


def export(export_dir: str, width_coefficient: float = 1.0, depth_coefficient: float = 1.0, image_size: int = 224,
           num_classes: int = NUM_CLASSES, seed: int = 0, swish_form: str = "beta") -> str:
    g, sigs, saver = build_graph(width_coefficient, depth_coefficient, image_size, num_classes, seed, swish_form)
    return write_saved_model(export_dir, g.graph, sigs, g.variables, g.var_dtypes, saver)
