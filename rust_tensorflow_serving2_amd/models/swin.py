"""Swin Transformer SavedModel exporter with random-init weights, in the TF
layout with static map sizes (the input is taken as already normalised, as
models/vit.py takes it).  The default is Swin-T at 224 with window 7.

* Front: ``Conv2D`` PxP / P VALID to ``embed`` + ``BiasAdd`` -> ``Reshape``
  ``[-1, C]`` -> LayerNorm.  Between blocks the activations stay flat,
  ``[B * Hf * Wf, C]`` in image row order.
* Stages of ``depths[i]`` blocks with ``heads[i]`` heads of 32, alternating
  shift 0 and ``window // 2``; a stage whose map is one window uses that map as
  its window, shift 0 and no mask.  A block: LayerNorm (eps 1e-5) -> ``Reshape
  [-1, Hf, Wf, C]`` -> [``Roll`` by (-s, -s) on axes (1, 2)] -> partition
  (``Reshape [-1, Hf/ws, ws, Wf/ws, ws, C]`` -> ``Transpose [0, 1, 3, 2, 4, 5]``
  -> ``Reshape [-1, ws * ws, C]``) -> ``Reshape [-1, C]`` -> packed dense to 3C
  -> ``Reshape [-1, S, 3, H, 32]`` -> ``Transpose [2, 0, 3, 1, 4]`` -> ``Unpack``
  -> ``Mul(q, 32 ** -0.5)`` -> ``BatchMatMulV2(adj_y)`` -> ``AddV2`` of the
  relative-position bias (``GatherV2`` of the ``[(2 ws - 1)^2, H]`` table by the
  constant index -> ``Reshape [S, S, H]`` -> ``Transpose [2, 0, 1]`` ->
  ``ExpandDims``) -> on shifted blocks ``Reshape [-1, nW, H, S, S]`` -> ``AddV2``
  of the ``[1, nW, 1, S, S]`` mask (0 / -100) -> ``Reshape [-1, H, S, S]`` ->
  ``Softmax`` -> ``BatchMatMulV2`` -> ``Transpose`` -> ``Reshape [-1, C]`` ->
  dense -> reverse (``Reshape [-1, ws, ws, C]`` -> ``Reshape [-1, Hf/ws, Wf/ws,
  ws, ws, C]`` -> ``Transpose`` -> ``Reshape [-1, Hf, Wf, C]``) -> [``Roll`` by
  (+s, +s)] -> ``Reshape [-1, C]`` -> ``AddV2`` with the block's input.  MLP:
  LayerNorm -> dense to 4C + erf GELU -> dense -> ``AddV2``.
* Patch merging between stages: ``Reshape [-1, Hf, Wf, C]`` -> four strided
  ``StridedSlice``s (rows / columns 0::2 and 1::2) -> ``ConcatV2`` on the
  channels -> ``Reshape [-1, 4C]`` -> LayerNorm -> bias-free dense to 2C.
* Tail: LayerNorm -> ``Reshape [-1, Hf, Wf, C]`` -> ``Mean`` over the tokens (axes 1, 2) -> dense
  to ``num_classes`` -> ``ArgMax`` (``classes``, int64) and ``Softmax``
  (``probabilities``): the other image models' interface.
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
HEAD_DIM = 32
LN_EPS = 1e-5
MASK_VALUE = -100.0
# name -> (embed, depths, heads)
CONFIGS = {"swin_tiny": (96, (2, 2, 6, 2), (3, 6, 12, 24)),
           "swin_small": (96, (2, 2, 18, 2), (3, 6, 12, 24)),
           "swin_base": (128, (2, 2, 18, 2), (4, 8, 16, 32))}
# Init gains, as models/vit.py documents them: every dense kernel is N(0, gain / fan-in), RESIDUAL_GAIN for
# the two layers of a block that write into the residual stream, QK_GAIN for the query and key columns of
# the packed dense, DENSE_GAIN for the rest (scripts/bf16_emulation.py --family swin measures a choice on
# the CPU; docs/numerics.md, "Swin end to end").  The relative-position table is N(0, BIAS_STD): Swin's own
# 0.02 leaves every head position-blind at random init, 0.5 makes the table shape the softmax.
# Swin-T at 224, model seed 3, input seed 0, logit error / logit spread of the bf16 emulation (limit 5 %),
# rows whose fp32 top-1 margin is decidable, and how far the logits follow the image, as (dense, residual, qk):
#   (1, 2, 4)  2.1-2.6 %  3 rows  0.025     (1, 2, 8)  2.8-3.6 %  0 rows  0.056     (1, 4, 4)  2.5-2.7 %  1 row  0.021
#   (2, 2, 4)  3.3-3.5 %  3 rows  0.021     (1, 1, 16)  23-33 %  3 rows  0.16
# The mean over all tokens averages most of the image away whatever the gains (a ViT reads one token);
# sharper softmaxes follow the image more and cost the scores' rounding, as in models/vit.py.
DENSE_GAIN = 1.0
RESIDUAL_GAIN = 2.0
QK_GAIN = 4.0
BIAS_STD = 0.5


def _const_i(g, name, values):
    return g.const(name, np.array(values, np.int32))


def _reshape(g, x, name, shape):
    return g.node("Reshape", name, [x, _const_i(g, f"{name}/shape", shape)], T=F32)


def _transpose(g, x, name, perm):
    return g.node("Transpose", name, [x, _const_i(g, f"{name}/perm", perm)], T=F32, Tperm=I32)


def _roll(g, x, name, s):
    return g.node("Roll", name, [x, _const_i(g, f"{name}/shift", [s, s]), _const_i(g, f"{name}/axis", [1, 2])],
                  T=F32, Tshift=I32, Taxis=I32)


def _dense(g, x, din, dout, rng, name, gain=DENSE_GAIN, bias=True, col_gains=None):
    with g.scope(name):
        w = rng.standard_normal((din, dout)) * np.sqrt(gain / din)
        if col_gains is not None:
            w = w * np.sqrt(np.asarray(col_gains))[None, :]
        w = g.variable("kernel", w.astype(np.float32))
        y = g.node("MatMul", "MatMul", [x, w], T=F32, transpose_a=False, transpose_b=False)
        if not bias:
            return y
        b = g.variable("bias", (0.02 * rng.standard_normal(dout)).astype(np.float32))
        return g.node("BiasAdd", "BiasAdd", [y, b], T=F32, data_format="NHWC")


def relative_position_index(ws: int) -> np.ndarray:
    """[S * S] int32: the row of the [(2 ws - 1)^2, H] table for (query, key), Swin's formula."""
    coords = np.stack(np.meshgrid(np.arange(ws), np.arange(ws), indexing="ij")).reshape(2, -1)
    rel = (coords[:, :, None] - coords[:, None, :]).transpose(1, 2, 0) + (ws - 1)
    return (rel[:, :, 0] * (2 * ws - 1) + rel[:, :, 1]).reshape(-1).astype(np.int32)


def shift_mask(Hf: int, Wf: int, ws: int, shift: int) -> np.ndarray:
    """[nW, S, S] float32: 0 where query and key come from the same region of the
    rolled map, MASK_VALUE where the roll brought them together (Swin's mask)."""
    img = np.zeros((Hf, Wf), np.int32)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[hs, wsl] = cnt
            cnt += 1
    win = img.reshape(Hf // ws, ws, Wf // ws, ws).transpose(0, 2, 1, 3).reshape(-1, ws * ws)
    return np.where(win[:, :, None] != win[:, None, :], MASK_VALUE, 0.0).astype(np.float32)


def _window_attention(g, x, C, nH, Hf, Wf, ws, shift, rng, gains):
    """x: [B * Hf * Wf, C] flat, LayerNormed.  Returns the projected rows, flat, in image order."""
    dense_gain, residual_gain, qk_gain = gains
    S, nW = ws * ws, (Hf // ws) * (Wf // ws)
    h = _reshape(g, x, "Reshape_map", [-1, Hf, Wf, C])
    if shift:
        h = _roll(g, h, "roll", -shift)
    h = _reshape(g, h, "partition/Reshape", [-1, Hf // ws, ws, Wf // ws, ws, C])
    h = _transpose(g, h, "partition/transpose", [0, 1, 3, 2, 4, 5])
    h = _reshape(g, h, "partition/Reshape_1", [-1, S, C])
    h = _reshape(g, h, "Reshape_rows", [-1, C])
    col_gains = np.concatenate([np.full(2 * C, qk_gain / dense_gain), np.ones(C)])
    qkv = _dense(g, h, C, 3 * C, rng, "qkv", dense_gain, col_gains=col_gains)
    qkv = _reshape(g, qkv, "Reshape_qkv", [-1, S, 3, nH, HEAD_DIM])
    qkv = _transpose(g, qkv, "transpose_qkv", [2, 0, 3, 1, 4])
    un = g.node("Unpack", "unstack", [qkv], T=F32, num=3, axis=0)
    q, k, v = un, un + ":1", un + ":2"
    q = g.node("Mul", "mul", [q, g.const("mul/y", np.array(HEAD_DIM ** -0.5, np.float32))], T=F32)
    sc = g.node("BatchMatMulV2", "MatMul", [q, k], T=F32, adj_x=False, adj_y=True)
    table = g.variable("relative_position_bias_table",
                       (BIAS_STD * rng.standard_normal(((2 * ws - 1) ** 2, nH))).astype(np.float32))
    bias = g.node("GatherV2", "GatherV2", [table, g.const("relative_position_index", relative_position_index(ws)),
                                           g.const("GatherV2/axis", np.array(0, np.int32))],
                  Tparams=F32, Tindices=I32, Taxis=I32, batch_dims=0)
    bias = _reshape(g, bias, "Reshape_bias", [S, S, nH])
    bias = _transpose(g, bias, "transpose_bias", [2, 0, 1])
    bias = g.node("ExpandDims", "ExpandDims", [bias, g.const("ExpandDims/dim", np.array(0, np.int32))], T=F32, Tdim=I32)
    sc = g.node("AddV2", "add", [sc, bias], T=F32)
    if shift:
        sc = _reshape(g, sc, "Reshape_mask", [-1, nW, nH, S, S])
        mask = g.const("attn_mask", shift_mask(Hf, Wf, ws, shift)[None, :, None])
        sc = g.node("AddV2", "add_1", [sc, mask], T=F32)
        sc = _reshape(g, sc, "Reshape_scores", [-1, nH, S, S])
    pr = g.node("Softmax", "Softmax", [sc], T=F32)
    ctx = g.node("BatchMatMulV2", "MatMul_1", [pr, v], T=F32, adj_x=False, adj_y=False)
    ctx = _transpose(g, ctx, "transpose_out", [0, 2, 1, 3])
    ctx = _reshape(g, ctx, "Reshape_out", [-1, C])
    h = _dense(g, ctx, C, C, rng, "proj", residual_gain)
    h = _reshape(g, h, "reverse/Reshape", [-1, ws, ws, C])
    h = _reshape(g, h, "reverse/Reshape_1", [-1, Hf // ws, Wf // ws, ws, ws, C])
    h = _transpose(g, h, "reverse/transpose", [0, 1, 3, 2, 4, 5])
    h = _reshape(g, h, "reverse/Reshape_2", [-1, Hf, Wf, C])
    if shift:
        h = _roll(g, h, "roll_1", shift)
    return _reshape(g, h, "Reshape_flat", [-1, C])


def _block(g, y, C, nH, Hf, Wf, ws, shift, rng, gains):
    with g.scope("attention"):
        h = layer_norm(g, y, C, rng, LN_EPS, "LayerNorm")
        h = _window_attention(g, h, C, nH, Hf, Wf, ws, shift, rng, gains)
        y = g.node("AddV2", "add_2", [h, y], T=F32)
    with g.scope("mlp"):
        h = layer_norm(g, y, C, rng, LN_EPS, "LayerNorm")
        h = _gelu_erf(g, _dense(g, h, C, 4 * C, rng, "dense_0", gains[0]), "gelu")
        h = _dense(g, h, 4 * C, C, rng, "dense_1", gains[1])
        return g.node("AddV2", "add", [h, y], T=F32)


def _patch_merging(g, y, C, Hf, Wf, rng, gain):
    x = _reshape(g, y, "Reshape", [-1, Hf, Wf, C])
    parts = []
    for i, (a, b) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        parts.append(g.node("StridedSlice", f"strided_slice_{i}",
                            [x, _const_i(g, f"strided_slice_{i}/stack", [0, a, b, 0]),
                             _const_i(g, f"strided_slice_{i}/stack_1", [0, 0, 0, 0]),
                             _const_i(g, f"strided_slice_{i}/stack_2", [1, 2, 2, 1])],
                            T=F32, Index=I32, begin_mask=9, end_mask=15, ellipsis_mask=0, new_axis_mask=0,
                            shrink_axis_mask=0))
    x = g.node("ConcatV2", "concat", parts + [g.const("concat/axis", np.array(-1, np.int32))], N=4, T=F32, Tidx=I32)
    x = _reshape(g, x, "Reshape_1", [-1, 4 * C])
    x = layer_norm(g, x, 4 * C, rng, LN_EPS, "LayerNorm")
    return _dense(g, x, 4 * C, 2 * C, rng, "reduction", gain, bias=False)


def build_graph(config: str = "swin_tiny", image_size: int = 224, num_classes: int = NUM_CLASSES, seed: int = 0,
                depths=None, embed: int = None, heads=None, window: int = 7, patch: int = 4, gains=None):
    if config not in CONFIGS:
        raise ValueError(f"unknown Swin config {config!r}: one of {sorted(CONFIGS)}")
    c_embed, c_depths, c_heads = CONFIGS[config]
    C = embed or c_embed
    depths = tuple(depths) if depths is not None else c_depths
    heads = tuple(heads) if heads is not None else c_heads
    if len(depths) != len(heads) or not depths:
        raise ValueError(f"depths {depths} and heads {heads} must name the same stages")
    if patch < 1 or image_size % patch:
        raise ValueError(f"image_size {image_size} is not a multiple of the patch size {patch}")
    gains = tuple(gains) if gains is not None else (DENSE_GAIN, RESIDUAL_GAIN, QK_GAIN)
    g = GraphBuilder()
    init = _Init(seed)
    rng = init.rng
    x = g.placeholder("input_tensor", T.DT_FLOAT, [-1, image_size, image_size, 3])
    Hf = Wf = image_size // patch
    with g.scope("swin"):
        with g.scope("patch_embed"):
            y = _conv_bias(g, init, x, patch, 3, C, patch, "VALID", "proj")
            y = _reshape(g, y, "Reshape", [-1, C])
            y = layer_norm(g, y, C, rng, LN_EPS, "LayerNorm")
        for si, (depth, nH) in enumerate(zip(depths, heads)):
            if C != nH * HEAD_DIM:
                raise ValueError(f"stage {si}: width {C} is not heads {nH} x {HEAD_DIM}")
            ws = window
            if min(Hf, Wf) <= window:
                ws = min(Hf, Wf)          # the map is one window: no shift, no mask
            if Hf % ws or Wf % ws:
                raise ValueError(f"stage {si}: the {Hf} x {Wf} map is not a multiple of the window {ws}")
            with g.scope(f"stage_{si}"):
                for bi in range(depth):
                    shift = ws // 2 if bi % 2 and min(Hf, Wf) > window else 0
                    with g.scope(f"block_{bi}"):
                        y = _block(g, y, C, nH, Hf, Wf, ws, shift, rng, gains)
                if si + 1 < len(depths):
                    if Hf % 2 or Wf % 2:
                        raise ValueError(f"stage {si}: the {Hf} x {Wf} map cannot be merged 2 x 2")
                    with g.scope("downsample"):
                        y = _patch_merging(g, y, C, Hf, Wf, rng, gains[0])
                    C, Hf, Wf = 2 * C, Hf // 2, Wf // 2
        y = layer_norm(g, y, C, rng, LN_EPS, "norm")
        y = _reshape(g, y, "Reshape", [-1, Hf, Wf, C])
        y = g.node("Mean", "Mean", [y, g.const("Mean/reduction_indices", np.array([1, 2], np.int32))], T=F32, Tidx=I32,
                   keep_dims=False)
    with g.scope("head"):
        w = g.variable("kernel", (rng.standard_normal((C, num_classes)) * np.sqrt(1.0 / C)).astype(np.float32))
        b = g.variable("bias", (0.01 * rng.standard_normal(num_classes)).astype(np.float32))
        y = g.node("MatMul", "MatMul", [y, w], T=F32, transpose_a=False, transpose_b=False)
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


def export(export_dir: str, config: str = "swin_tiny", image_size: int = 224, num_classes: int = NUM_CLASSES,
           seed: int = 0, **overrides) -> str:
    g, sigs, saver = build_graph(config, image_size, num_classes, seed, **overrides)
    return write_saved_model(export_dir, g.graph, sigs, g.variables, g.var_dtypes, saver)
