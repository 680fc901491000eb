"""ModernBERT-style encoder SavedModel exporter with random-init weights, in the
op vocabulary a TF export of the Hugging Face ModernBERT block produces, at a
static sequence length.

* Front: ``GatherV2`` of the token table, flattened to ``[B * S, C]`` as
  models/llama.py does, then LayerNorm (eps 1e-5) spelled as models/bert.py
  spells it, with a constant zero beta: the model has no biases anywhere.
  There is no position table: positions enter through the rotation of q and k.
* ``layers`` pre-norm blocks; the first has no attention norm (the embedding
  norm stands in).  Attention: one packed bias-free ``Wqkv`` dense ``3 C`` wide
  and ``Split`` three ways (``packed_qkv=False``: three denses), heads 64 wide,
  ``Reshape [-1, S, H, 64]`` -> ``Transpose``; q and k rotated with
  models/llama.py's ``rotate`` (rotate-half, constant tables ``[1, 1, S, 64]``).
  Every third layer, starting with layer 0, is global: theta 160000 and every
  key open.  The others are local: theta 10000 and a constant adder
  ``[1, 1, S, S]``, ``-1e4 * (|i - j| > w)``, added to the scaled scores.  Then
  the padding adder ``(1 - mask) * -1e4`` ``[B, 1, 1, S]``, ``Softmax``, the
  context, a bias-free ``Wo`` and ``AddV2`` with the block's input.
* MLP: LayerNorm -> one bias-free ``Wi`` dense ``2 F`` wide -> ``Split`` in two
  -> ``Mul(gelu_erf(s0), s1)`` (the Keras erf spelling of models/convnext.py)
  -> ``Wo`` -> ``AddV2``.
* Tail: LayerNorm -> ``hidden`` ``[-1, S, C]``; ``cls`` is ``hidden[:, 0]``
  (``StridedSlice`` + ``Squeeze``).

Signature ``serving_default`` (predict): inputs ``input_ids``, ``input_mask``
(int32 [-1, S]); outputs ``hidden`` and ``cls``.
"""
from __future__ import annotations

import math

import numpy as np

from ..graph.builder import PREDICT_METHOD, DType, GraphBuilder, signature, tensor_info
from ..savedmodel.saved_model import write_saved_model
from ..utils import tensors as T
from .bert import _c
from .llama import linear, rope_tables, rotate

F32 = DType(T.DT_FLOAT)
I32 = DType(T.DT_INT32)
HEAD_DIM = 64
LN_EPS = 1e-5
GLOBAL_THETA, LOCAL_THETA = 160000.0, 10000.0
GLOBAL_EVERY = 3
MASK_FILL = 1e4
# The reasoning of models/llama.py's gains, for a stream that a LayerNorm has brought to unit scale.  Every
# dense reads LayerNorm'd (unit) rows and is N(0, gain / fan-in).  QKV_GAIN 2 gives q and k entries of
# variance 2, which the rotation keeps, hence scores of standard deviation 2: a softmax that is neither
# uniform nor one-hot, so closing the keys outside the window moves every row, and so does a one-position
# shift of either table.  The two layers that write into the stream get RESIDUAL_GAIN.  The attention output
# has at most v's variance 2 and the GeGLU product gelu(g) * u of two unit pre-activations a second moment of
# ~0.43, so 0.02 makes branches of standard deviation <= 0.2 and ~0.13 beside the embedding norm's unit
# rows: large enough that an error in either branch shows in ``hidden``, small enough that the stream of
# the 22-layer model stays within a few units.  (The gain does not move the end-to-end figure: the worst
# real hidden row of modernbert_tiny sits at 4.4 % of its spread with 0.02, kernels and torch paths alike,
# and sat at 4.4 % (kernels) / 4.1 % (torch paths) with 0.05.  That is the unit-scale stream stored in bf16
# after every residual add and LayerNorm, not either branch: docs/numerics.md, "ModernBERT end to end",
# which also says what to do if a reseed or another layer takes it past the 5 % limit.)
QKV_GAIN = 2.0
RESIDUAL_GAIN = 0.02
EMBED_STD = 0.1
# name -> (hidden, layers, heads, mlp, seq_len, window, vocab)
CONFIGS = {"modernbert_base": (768, 22, 12, 1152, 1024, 64, 50368), "modernbert_tiny": (128, 3, 2, 192, 200, 24, 503)}


def layer_norm(g, x, dim, rng, eps, name):
    """models/bert.py's layer_norm with the beta a constant of zeros (bias-free)."""
    with g.scope(name):
        gamma = g.variable("gamma", (1.0 + 0.05 * rng.standard_normal(dim)).astype(np.float32))
        beta = g.const("beta", np.zeros(dim, np.float32))
        axes = g.const("moments/mean/reduction_indices", np.array([-1], np.int32))
        mean = g.node("Mean", "moments/mean", [x, axes], T=F32, Tidx=I32, keep_dims=True)
        sg = g.node("StopGradient", "moments/StopGradient", [mean], T=F32)
        sqd = g.node("SquaredDifference", "moments/SquaredDifference", [x, sg], T=F32)
        axes2 = g.const("moments/variance/reduction_indices", np.array([-1], np.int32))
        var = g.node("Mean", "moments/variance", [sqd, axes2], T=F32, Tidx=I32, keep_dims=True)
        rs = g.node("Rsqrt", "batchnorm/Rsqrt", [g.node("AddV2", "batchnorm/add", [var, _c(g, "batchnorm/add/y", eps)],
                                                        T=F32)], T=F32)
        mul = g.node("Mul", "batchnorm/mul", [rs, gamma], T=F32)
        mul1 = g.node("Mul", "batchnorm/mul_1", [x, mul], T=F32)
        sub = g.node("Sub", "batchnorm/sub", [beta, g.node("Mul", "batchnorm/mul_2", [mean, mul], T=F32)], T=F32)
        return g.node("AddV2", "batchnorm/add_1", [mul1, sub], T=F32)


def window_band(S: int, w: int, fill: float = -MASK_FILL) -> np.ndarray:
    """``fill * (|i - j| > w)`` as float32 ``[1, 1, S, S]``."""
    pos = np.arange(S)
    return (fill * (np.abs(pos[:, None] - pos[None, :]) > w)).astype(np.float32)[None, None]


def _heads(g, x, S, nH, name):
    x = g.node("Reshape", f"Reshape_{name}", [x, g.const(f"Reshape_{name}/shape", np.array([-1, S, nH, HEAD_DIM], np.int32))],
               T=F32)
    return g.node("Transpose", f"transpose_{name}", [x, g.const(f"transpose_{name}/perm", np.array([0, 2, 1, 3], np.int32))],
                  T=F32, Tperm=I32)


def attention_core(g, x, C, S, nH, rng, adder, tables, band=None, packed_qkv=True, const_weights=False,
                   key_tables=None, rotate_v=False):
    """Wqkv on x [B * S, C] -> the context [B * S, C] (before Wo).  ``tables`` = (cos, sin) arrays and ``band``
    the constant [1, 1, S, S] adder of a local layer (None: global); ``key_tables`` and ``rotate_v`` spell
    graphs that are NOT ModernBERT's attention; ``const_weights`` writes the kernels as constants."""
    std = math.sqrt(QKV_GAIN / C)
    if packed_qkv:
        qkv = linear(g, x, C, 3 * C, rng, "Wqkv", std, const_weights)
        sp = g.node("Split", "split_qkv", [g.const("split_qkv/split_dim", np.array(-1, np.int32)), qkv], T=F32, num_split=3)
        q, k, v = sp, sp + ":1", sp + ":2"
    else:
        q, k, v = (linear(g, x, C, C, rng, n, std, const_weights) for n in ("Wq", "Wk", "Wv"))
    cos, sin = g.const("rope_cos", tables[0]), g.const("rope_sin", tables[1])
    kcos, ksin = (cos, sin) if key_tables is None else (g.const("rope_cos_k", key_tables[0]),
                                                        g.const("rope_sin_k", key_tables[1]))
    q = rotate(g, _heads(g, q, S, nH, "query"), cos, sin, "query")
    k = rotate(g, _heads(g, k, S, nH, "key"), kcos, ksin, "key")
    v = _heads(g, v, S, nH, "value")
    if rotate_v:
        v = rotate(g, v, cos, sin, "value")
    w = g.node("BatchMatMulV2", "MatMul", [q, k], T=F32, adj_x=False, adj_y=True)
    w = g.node("Mul", "mul", [w, _c(g, "mul/y", 1.0 / math.sqrt(HEAD_DIM))], T=F32)
    if band is not None:
        w = g.node("AddV2", "add_window", [w, g.const("window_mask", np.asarray(band, np.float32))], T=F32)
    if adder is not None:
        w = g.node("AddV2", "add", [w, adder], T=F32)
    p = g.node("Softmax", "Softmax", [w], T=F32)
    a = g.node("BatchMatMulV2", "MatMul_1", [p, v], T=F32, adj_x=False, adj_y=False)
    a = g.node("Transpose", "transpose_out", [a, g.const("transpose_out/perm", np.array([0, 2, 1, 3], np.int32))],
               T=F32, Tperm=I32)
    return g.node("Reshape", "Reshape_out", [a, g.const("Reshape_out/shape", np.array([-1, C], np.int32))], T=F32)


def gelu_erf(g, x):
    """Keras ``gelu(approximate=False)``: 0.5 * x * (1 + erf(x / sqrt(2)))."""
    half = g.node("Mul", "gelu/mul", [_c(g, "gelu/mul/x", 0.5), x], T=F32)
    q = g.node("RealDiv", "gelu/truediv", [x, _c(g, "gelu/Cast/x", np.sqrt(2.0))], T=F32)
    a = g.node("AddV2", "gelu/add", [_c(g, "gelu/add/x", 1.0), g.node("Erf", "gelu/Erf", [q], T=F32)], T=F32)
    return g.node("Mul", "gelu/mul_1", [half, a], T=F32)


def geglu_mlp(g, x, C, F, rng, const_weights=False):
    wi = linear(g, x, C, 2 * F, rng, "Wi", math.sqrt(1.0 / C), const_weights)
    sp = g.node("Split", "split", [g.const("split/split_dim", np.array(-1, np.int32)), wi], T=F32, num_split=2)
    y = g.node("Mul", "mul", [gelu_erf(g, sp), sp + ":1"], T=F32)
    return linear(g, y, F, C, rng, "Wo", math.sqrt(2 * RESIDUAL_GAIN / F), const_weights)


def build_graph(config: str = "modernbert_base", seed: int = 0, layers: int = None, hidden: int = None,
                heads: int = None, mlp: int = None, seq_len: int = None, window: int = None, vocab: int = None,
                packed_qkv: bool = True):
    if config not in CONFIGS:
        raise ValueError(f"unknown ModernBERT config {config!r}: one of {sorted(CONFIGS)}")
    c_hidden, c_layers, c_heads, c_mlp, c_seq, c_window, c_vocab = CONFIGS[config]
    C, L, nH = hidden or c_hidden, c_layers if layers is None else layers, heads or c_heads
    F, S, V = mlp or c_mlp, seq_len or c_seq, vocab or c_vocab
    w = c_window if window is None else window
    if C != nH * HEAD_DIM or w < 0:
        raise ValueError(f"hidden {C} is not heads {nH} x {HEAD_DIM}, or window {w} < 0")
    g = GraphBuilder()
    rng = np.random.default_rng(seed)
    ids = g.placeholder("input_ids", T.DT_INT32, [-1, S])
    mask = g.placeholder("input_mask", T.DT_INT32, [-1, S])
    with g.scope("model"):
        table = g.variable("embeddings/tok_embeddings", (rng.standard_normal((V, C)) * EMBED_STD).astype(np.float32))
        flat = g.node("Reshape", "Reshape", [ids, g.const("Reshape/shape", np.array([-1], np.int32))], T=I32)
        x = g.node("GatherV2", "GatherV2", [table, flat, g.const("GatherV2/axis", np.array(0, np.int32))],
                   Tparams=F32, Tindices=I32, Taxis=I32, batch_dims=0)
        x = layer_norm(g, x, C, rng, LN_EPS, "embeddings/norm")
        m = g.node("Reshape", "Reshape_1", [mask, g.const("Reshape_1/shape", np.array([-1, 1, 1, S], np.int32))], T=I32)
        m = g.node("Cast", "Cast", [m], SrcT=I32, DstT=F32, Truncate=False)
        adder = g.node("Mul", "mul", [g.node("Sub", "sub", [_c(g, "sub/x", 1.0), m], T=F32), _c(g, "mul/y", -MASK_FILL)],
                       T=F32)
        for li in range(L):
            is_global = li % GLOBAL_EVERY == 0
            with g.scope(f"layers_{li}"):
                with g.scope("attn"):
                    h = x if li == 0 else layer_norm(g, x, C, rng, LN_EPS, "attn_norm")
                    h = attention_core(g, h, C, S, nH, rng, adder,
                                       rope_tables(S, GLOBAL_THETA if is_global else LOCAL_THETA),
                                       None if is_global else window_band(S, w), packed_qkv)
                    h = linear(g, h, C, C, rng, "Wo", math.sqrt(RESIDUAL_GAIN / C))
                    x = g.node("AddV2", "add_residual", [x, h], T=F32)
                with g.scope("mlp"):
                    h = layer_norm(g, x, C, rng, LN_EPS, "mlp_norm")
                    x = g.node("AddV2", "add_residual", [x, geglu_mlp(g, h, C, F, rng)], T=F32)
        x = layer_norm(g, x, C, rng, LN_EPS, "final_norm")
        hidden_out = g.node("Reshape", "Reshape_2", [x, g.const("Reshape_2/shape", np.array([-1, S, C], np.int32))],
                            T=F32)
        first = g.node("StridedSlice", "strided_slice",
                       [hidden_out, g.const("ss/begin", np.array([0, 0, 0], np.int32)),
                        g.const("ss/end", np.array([0, 1, 0], np.int32)),
                        g.const("ss/strides", np.array([1, 1, 1], np.int32))],
                       T=F32, Index=I32, begin_mask=5, end_mask=5, ellipsis_mask=0, new_axis_mask=0, shrink_axis_mask=0)
        cls = g.node("Squeeze", "Squeeze", [first], T=F32, squeeze_dims=[1])
    saver = g.add_saver()
    ins = {"input_ids": tensor_info(ids, T.DT_INT32, [-1, S]), "input_mask": tensor_info(mask, T.DT_INT32, [-1, S])}
    outs = {"hidden": tensor_info(hidden_out, T.DT_FLOAT, [-1, S, C]), "cls": tensor_info(cls, T.DT_FLOAT, [-1, C])}
    return g, {"serving_default": signature(ins, outs, PREDICT_METHOD)}, saver


def export(export_dir: str, config: str = "modernbert_base", seed: int = 0, **overrides) -> str:
    g, sigs, saver = build_graph(config, seed, **overrides)
    return write_saved_model(export_dir, g.graph, sigs, g.variables, g.var_dtypes, saver)
