"""Vision Transformer SavedModel exporter with random-init weights, in the
TF layout with a static sequence length (the input is taken as already
normalised, as models/convnext.py takes it).  The default is ViT-B/16 at 224.

* Front: ``Conv2D`` PxP / P VALID to ``hidden`` + ``BiasAdd`` -> ``Reshape``
  ``[-1, N, C]`` (N = (image / P)^2) -> the ``[1, 1, C]`` class token repeated
  over the batch (``Tile`` by ``Pack([Shape(input)[0], 1, 1])``) ->
  ``ConcatV2`` on axis 1, token first -> ``AddV2`` of the ``[1, N + 1, C]``
  position embedding; flattened once to ``[B * S, C]`` (S = N + 1), as
  models/bert.py does.
* ``layers`` pre-LN blocks.  Attention: LayerNorm (eps 1e-6) -> query / key /
  value dense -> ``Reshape [-1, S, H, 64]`` -> ``Transpose`` ->
  ``BatchMatMulV2(adj_y)`` -> ``RealDiv`` by sqrt(64) -> ``Softmax`` ->
  ``BatchMatMulV2`` -> ``Transpose`` -> ``Reshape`` -> dense -> ``AddV2`` with
  the block's input.  MLP: LayerNorm -> dense to ``mlp`` + erf GELU (the
  Keras spelling, models/convnext.py) -> dense -> ``AddV2``.
* Tail: LayerNorm -> first token (``StridedSlice`` + ``Squeeze``) -> dense
  to ``num_classes`` -> ``ArgMax`` (``classes``, int64) and ``Softmax``
  (``probabilities``): the other image models' interface.

LayerNorms are spelled as models/bert.py spells them.  Heads are 64 wide
(ViT-Ti 192 / 3, ViT-S 384 / 6, ViT-B 768 / 12, DeiT).
"""
from __future__ import annotations

import numpy as np

from ..graph.builder import PREDICT_METHOD, DType, GraphBuilder, signature, tensor_info
from ..savedmodel.saved_model import write_saved_model
from ..utils import tensors as T
from .bert import layer_norm
from .convnext import _conv_bias, _gelu_erf
from .resnet import _Init

F32 = DType(T.DT_FLOAT)
I32 = DType(T.DT_INT32)
NUM_CLASSES = 1000
HEAD_DIM = 64
LN_EPS = 1e-6
# name -> (hidden, layers, heads, mlp)
CONFIGS = {"vit_tiny": (192, 12, 3, 768), "vit_small": (384, 12, 6, 1536), "vit_base": (768, 12, 12, 3072)}
# Init gains, chosen on the CPU with scripts/bf16_emulation.py --family vit (docs/numerics.md, "ViT end
# to end"; profiles/vit/bf16_emulation_gains_cpu.log).  Every dense kernel is N(0, gain / fan-in):
# RESIDUAL_GAIN for the two layers that write into the residual stream (attention output, second MLP
# layer), QK_GAIN for query and key, DENSE_GAIN for the rest.  ViT-S/16 at 224, model seed 3, logit error /
# logit spread of the bf16 emulation over 2 input seeds x 3 trials (limit 5 %) and how far the logits
# follow the image (std over the batch / spread over the classes), as (dense, residual, qk):
#   (1, 0.05, 4)  2.8-4.2 %  0.12      (1, 0.25, 4)  2.7-4.4 %  0.13      (1, 1, 4)  2.3-3.9 %  0.12
#   (1, 2, 4)     2.6-3.4 %  0.12      (1, 4, 4)     2.4-3.3 %  0.12      (1, 0.25, 1)  2.3-3.6 %  0.03
#   (1, 4, 8)     4.6-7.4 %  0.24
# The floor of about 2.5 % is the residual stream held in bf16: 24 roundings of a 384-wide vector, then the
# largest of 1000 logits' errors; no gain removes it.  Small residual branches sit slightly above it (the
# early roundings are never diluted); unit query / key gains give a near-uniform softmax that averages the
# image away; 8 makes the softmax sharp enough that the scores' rounding shows.
DENSE_GAIN = 1.0
RESIDUAL_GAIN = 2.0
QK_GAIN = 4.0
TOKEN_STD = 0.5                  # class token and position embedding


def _dense(g, x, din, dout, rng, name, gain=DENSE_GAIN):
    with g.scope(name):
        w = g.variable("kernel", (rng.standard_normal((din, dout)) * np.sqrt(gain / din)).astype(np.float32))
        b = g.variable("bias", (0.02 * rng.standard_normal(dout)).astype(np.float32))
        y = g.node("MatMul", "MatMul", [x, w], T=F32, transpose_a=False, transpose_b=False)
        return g.node("BiasAdd", "BiasAdd", [y, b], T=F32, data_format="NHWC")


def _heads(g, x, S, nH, name):
    y = g.node("Reshape", f"Reshape_{name}", [x, g.const(f"Reshape_{name}/shape",
                                                        np.array([-1, S, nH, HEAD_DIM], np.int32))], T=F32)
    return g.node("Transpose", f"transpose_{name}", [y, g.const(f"transpose_{name}/perm",
                                                                np.array([0, 2, 1, 3], np.int32))], T=F32, Tperm=I32)


def _attention(g, x, C, S, nH, rng, gains):
    dense_gain, residual_gain, qk_gain = gains
    q = _heads(g, _dense(g, x, C, C, rng, "query", qk_gain), S, nH, "query")
    k = _heads(g, _dense(g, x, C, C, rng, "key", qk_gain), S, nH, "key")
    v = _heads(g, _dense(g, x, C, C, rng, "value", dense_gain), S, nH, "value")
    sc = g.node("BatchMatMulV2", "MatMul", [q, k], T=F32, adj_x=False, adj_y=True)
    sc = g.node("RealDiv", "truediv", [sc, g.const("truediv/y", np.array(np.sqrt(float(HEAD_DIM)), np.float32))], T=F32)
    pr = g.node("Softmax", "Softmax", [sc], T=F32)
    ctx = g.node("BatchMatMulV2", "MatMul_1", [pr, v], T=F32, adj_x=False, adj_y=False)
    ctx = g.node("Transpose", "transpose_out", [ctx, g.const("transpose_out/perm", np.array([0, 2, 1, 3], np.int32))],
                 T=F32, Tperm=I32)
    ctx = g.node("Reshape", "Reshape_out", [ctx, g.const("Reshape_out/shape", np.array([-1, C], np.int32))], T=F32)
    return _dense(g, ctx, C, C, rng, "output", residual_gain)


def _front(g, init, x, image_size, patch, C):
    n = (image_size // patch) ** 2
    rng = init.rng
    y = _conv_bias(g, init, x, patch, 3, C, patch, "VALID", "embedding")
    y = g.node("Reshape", "Reshape", [y, g.const("Reshape/shape", np.array([-1, n, C], np.int32))], T=F32)
    shape = g.node("Shape", "Shape", [x], T=F32, out_type=I32)
    batch = g.node("StridedSlice", "strided_slice",
                   [shape, g.const("strided_slice/stack", np.array([0], np.int32)),
                    g.const("strided_slice/stack_1", np.array([1], np.int32)),
                    g.const("strided_slice/stack_2", np.array([1], np.int32))],
                   T=I32, Index=I32, begin_mask=0, end_mask=0, ellipsis_mask=0, new_axis_mask=0, shrink_axis_mask=1)
    one = g.const("Tile/multiples/1", np.array(1, np.int32))
    mult = g.node("Pack", "Tile/multiples", [batch, one, one], N=3, T=I32, axis=0)
    cls = g.variable("class_token", (TOKEN_STD * rng.standard_normal((1, 1, C))).astype(np.float32))
    cls = g.node("Tile", "Tile", [cls, mult], T=F32, Tmultiples=I32)
    y = g.node("ConcatV2", "concat", [cls, y, g.const("concat/axis", np.array(1, np.int32))], N=2, T=F32, Tidx=I32)
    pos = g.variable("position_embedding", (TOKEN_STD * rng.standard_normal((1, n + 1, C))).astype(np.float32))
    return g.node("AddV2", "add", [y, pos], T=F32), n + 1


def build_graph(config: str = "vit_base", patch: int = 16, image_size: int = 224, num_classes: int = NUM_CLASSES,
                seed: int = 0, layers: int = None, hidden: int = None, heads: int = None, mlp: int = None,
                gains=None):
    if config not in CONFIGS:
        raise ValueError(f"unknown ViT config {config!r}: one of {sorted(CONFIGS)}")
    c_hidden, c_layers, c_heads, c_mlp = CONFIGS[config]
    C, L, nH, M = hidden or c_hidden, c_layers if layers is None else layers, heads or c_heads, mlp or c_mlp
    if C != nH * HEAD_DIM:
        raise ValueError(f"hidden {C} is not heads {nH} x {HEAD_DIM}")
    if patch < 1 or image_size % patch:
        raise ValueError(f"image_size {image_size} is not a multiple of the patch size {patch}")
    gains = tuple(gains) if gains is not None else (DENSE_GAIN, RESIDUAL_GAIN, QK_GAIN)
    g = GraphBuilder()
    init = _Init(seed)
    rng = init.rng
    x = g.placeholder("input_tensor", T.DT_FLOAT, [-1, image_size, image_size, 3])
    with g.scope("vit"):
        y, S = _front(g, init, x, image_size, patch, C)
        y = g.node("Reshape", "Reshape_1", [y, g.const("Reshape_1/shape", np.array([-1, C], np.int32))], T=F32)
        for li in range(L):
            with g.scope(f"encoderblock_{li}"):
                with g.scope("attention"):
                    h = layer_norm(g, y, C, rng, LN_EPS, "LayerNorm")
                    h = _attention(g, h, C, S, nH, rng, gains)
                    y = g.node("AddV2", "add", [h, y], T=F32)
                with g.scope("mlp"):
                    h = layer_norm(g, y, C, rng, LN_EPS, "LayerNorm")
                    h = _gelu_erf(g, _dense(g, h, C, M, rng, "dense_0", gains[0]), "gelu")
                    h = _dense(g, h, M, C, rng, "dense_1", gains[1])
                    y = g.node("AddV2", "add", [h, y], T=F32)
        y = layer_norm(g, y, C, rng, LN_EPS, "encoder_norm")
        seq = g.node("Reshape", "Reshape_2", [y, g.const("Reshape_2/shape", np.array([-1, S, C], np.int32))], T=F32)
        first = g.node("StridedSlice", "strided_slice_1",
                       [seq, g.const("ss/begin", np.array([0, 0, 0], np.int32)),
                        g.const("ss/end", np.array([0, 1, 0], np.int32)),
                        g.const("ss/strides", np.array([1, 1, 1], np.int32))],
                       T=F32, Index=I32, begin_mask=5, end_mask=5, ellipsis_mask=0, new_axis_mask=0,
                       shrink_axis_mask=0)
        first = g.node("Squeeze", "Squeeze", [first], T=F32, squeeze_dims=[1])
    with g.scope("head"):
        w = g.variable("kernel", (rng.standard_normal((C, num_classes)) * np.sqrt(1.0 / C)).astype(np.float32))
        b = g.variable("bias", (0.01 * rng.standard_normal(num_classes)).astype(np.float32))
        y = g.node("MatMul", "MatMul", [first, w], T=F32, transpose_a=False, transpose_b=False)
        y = g.node("BiasAdd", "BiasAdd", [y, b], T=F32, data_format="NHWC")
    logits = g.node("Identity", "final_dense", [y], T=F32)
    dim = g.const("ArgMax/dimension", np.array(1, np.int32))
    classes = g.node("ArgMax", "ArgMax", [logits, dim], T=F32, Tidx=I32, output_type=DType(T.DT_INT64))
    probs = g.node("Softmax", "softmax_tensor", [logits], T=F32)
    saver = g.add_saver()
    ins = {"input": tensor_info(x, T.DT_FLOAT, [-1, image_size, image_size, 3])}
    outs = {"classes": tensor_info(classes, T.DT_INT64, [-1]),
            "probabilities": tensor_info(probs, T.DT_FLOAT, [-1, num_classes])}
    sig = signature(ins, outs, PREDICT_METHOD)
    return g, {"serving_default": sig, "predict": sig}, saver


def export(export_dir: str, config: str = "vit_base", patch: int = 16, image_size: int = 224,
           num_classes: int = NUM_CLASSES, seed: int = 0, **overrides) -> str:
    g, sigs, saver = build_graph(config, patch, image_size, num_classes, seed, **overrides)
    return write_saved_model(export_dir, g.graph, sigs, g.variables, g.var_dtypes, saver)
