"""T5 v1.0 encoder SavedModel exporter with random-init weights, in the op vocabulary
a TF export of the Hugging Face / Mesh-TF T5 encoder produces, at a static sequence
length.  The encoder alone is what sentence-T5, GTR and the text towers in front of
image generators serve.

* Front: ``GatherV2`` of the token table, flattened to ``[B * S, C]`` as
  models/llama.py does.  There is no position table and no embedding norm: positions
  enter through the attention bias alone.
* Position bias, computed once and read by every layer: the constant bidirectional
  bucket indices ``[S, S]`` (``relative_position_bucket`` below, T5's own function)
  gather a ``[buckets, H]`` table, ``Transpose`` to ``[H, S, S]`` and ``ExpandDims``
  to ``[1, H, S, S]``; constant folding leaves one constant.  The padding adder
  ``(1 - mask) * -1e4`` ``[B, 1, 1, S]`` is added to it ONCE (``position_bias + mask``,
  as the reference implementations do), and every layer adds that ``[B, H, S, S]`` sum
  to its scores.  ``shared_sum=False`` spells the two adds per layer instead.
* ``layers`` pre-norm blocks.  T5's LayerNorm has no mean and no beta: it is
  models/llama.py's ``rms_norm`` (eps 1e-6).  Attention: three bias-free denses, heads
  64 wide, NO score scale (T5 folds it into the initialisation), ``Softmax``, the
  context, a bias-free ``o`` and ``AddV2`` with the block's input.  FFN (v1.0):
  ``wi`` -> ``Relu`` -> ``wo``, bias-free, and ``AddV2``.
* Tail: the final norm -> ``hidden`` ``[-1, S, C]``; ``pooled`` is the mean of the real
  tokens' rows (the sentence-T5 head): ``Sum(hidden * m, 1) / Maximum(Sum(m, 1), 1)``.

Signature ``serving_default`` (predict): inputs ``input_ids``, ``input_mask``
(int32 [-1, S]); outputs ``hidden`` and ``pooled``.
"""
from __future__ import annotations

import math

import numpy as np

from ..graph.builder import PREDICT_METHOD, DType, GraphBuilder, signature, tensor_info
from ..savedmodel.saved_model import write_saved_model
from ..utils import tensors as T
from .bert import _c
from .llama import linear, rms_norm
from .modernbert import _heads

F32 = DType(T.DT_FLOAT)
I32 = DType(T.DT_INT32)
HEAD_DIM = 64
LN_EPS = 1e-6
MASK_FILL = 1e4
# The reasoning of models/modernbert.py's gains, for a block that does not scale its scores.  Every dense reads
# RMS-normed (unit) rows and is N(0, gain / fan-in).  QK_GAIN 0.25 gives q and k entries of variance 1/4 and, with
# no 1 / sqrt(64), scores of variance 64 / 16: standard deviation 2, a softmax that is neither uniform nor one-hot.
# BIAS_STD 1 puts the bias at half the scores' spread: dropping it, reading it at i - j for j - i, or taking another
# head's row moves every probability.  v has unit variance.  The two layers that write into the stream get
# RESIDUAL_GAIN: the attention output has at most v's variance 1 and relu of a unit pre-activation a second moment
# of 1/2, so 0.02 makes branches of standard deviation <= 0.14 beside the unit-scale token rows (EMBED_STD 1: T5
# has no embedding norm).
QK_GAIN = 0.25
V_GAIN = 1.0
BIAS_STD = 1.0
RESIDUAL_GAIN = 0.02
EMBED_STD = 1.0
# name -> (hidden, layers, heads, ffn, seq_len, buckets, max_distance, vocab)
CONFIGS = {"t5_base_encoder": (768, 12, 12, 3072, 512, 32, 128, 32128), "t5_tiny": (128, 3, 2, 256, 200, 32, 128, 503)}


def relative_position_bucket(rel: np.ndarray, buckets: int = 32, max_distance: int = 128) -> np.ndarray:
    """T5's bidirectional bucket of ``rel = key position - query position``: half the buckets per sign, within a
    sign the first half one bucket per distance, the rest logarithmic up to ``max_distance`` and the last bucket
    for everything beyond."""
    nb = buckets // 2
    ret = (rel > 0).astype(np.int64) * nb
    n = np.abs(rel)
    exact = nb // 2
    large = exact + (np.log(np.maximum(n, 1) / exact) / math.log(max_distance / exact) * (nb - exact)).astype(np.int64)
    return (ret + np.where(n < exact, n, np.minimum(large, nb - 1))).astype(np.int32)


def bucket_indices(S: int, buckets: int = 32, max_distance: int = 128) -> np.ndarray:
    pos = np.arange(S)
    return relative_position_bucket(pos[None, :] - pos[:, None], buckets, max_distance)


def position_bias(g, S, nH, buckets, max_distance, rng):
    """``[1, H, S, S]``: the learned ``[buckets, H]`` table gathered by the constant bucket indices."""
    table = g.variable("relative_attention_bias", (rng.standard_normal((buckets, nH)) * BIAS_STD).astype(np.float32))
    idx = g.const("relative_position_bucket", bucket_indices(S, buckets, max_distance))
    v = g.node("GatherV2", "bias/GatherV2", [table, idx, g.const("bias/GatherV2/axis", np.array(0, np.int32))],
               Tparams=F32, Tindices=I32, Taxis=I32, batch_dims=0)
    v = g.node("Transpose", "bias/transpose", [v, g.const("bias/transpose/perm", np.array([2, 0, 1], np.int32))],
               T=F32, Tperm=I32)
    return g.node("ExpandDims", "bias/ExpandDims", [v, g.const("bias/ExpandDims/dim", np.array(0, np.int32))],
                  T=F32, Tdim=I32)


def attention_core(g, x, C, S, nH, rng, bias, adder=None, bias_first=True, const_weights=False):
    """q, k, v on x [B * S, C] -> the context [B * S, C] (before o).  ``bias`` is added to the unscaled scores;
    with an ``adder`` a second AddV2 follows (``bias_first=False``: the adder is added first)."""
    q = linear(g, x, C, C, rng, "q", math.sqrt(QK_GAIN / C), const_weights)
    k = linear(g, x, C, C, rng, "k", math.sqrt(QK_GAIN / C), const_weights)
    v = linear(g, x, C, C, rng, "v", math.sqrt(V_GAIN / C), const_weights)
    q, k, v = _heads(g, q, S, nH, "query"), _heads(g, k, S, nH, "key"), _heads(g, v, S, nH, "value")
    w = g.node("BatchMatMulV2", "MatMul", [q, k], T=F32, adj_x=False, adj_y=True)
    first, second = (bias, adder) if bias_first else (adder, bias)
    w = g.node("AddV2", "add", [w, first], T=F32)
    if second is not None:
        w = g.node("AddV2", "add_1", [w, second], T=F32)
    p = g.node("Softmax", "Softmax", [w], T=F32)
    a = g.node("BatchMatMulV2", "MatMul_1", [p, v], T=F32, adj_x=False, adj_y=False)
    a = g.node("Transpose", "transpose_out", [a, g.const("transpose_out/perm", np.array([0, 2, 1, 3], np.int32))],
               T=F32, Tperm=I32)
    return g.node("Reshape", "Reshape_out", [a, g.const("Reshape_out/shape", np.array([-1, C], np.int32))], T=F32)


def relu_ffn(g, x, C, F, rng):
    h = g.node("Relu", "Relu", [linear(g, x, C, F, rng, "wi", math.sqrt(1.0 / C))], T=F32)
    return linear(g, h, F, C, rng, "wo", math.sqrt(2 * RESIDUAL_GAIN / F))


def build_graph(config: str = "t5_base_encoder", seed: int = 0, layers: int = None, hidden: int = None,
                heads: int = None, ffn: int = None, seq_len: int = None, vocab: int = None, shared_sum: bool = True):
    if config not in CONFIGS:
        raise ValueError(f"unknown T5 config {config!r}: one of {sorted(CONFIGS)}")
    c_hidden, c_layers, c_heads, c_ffn, c_seq, buckets, max_distance, c_vocab = CONFIGS[config]
    C, L, nH = hidden or c_hidden, c_layers if layers is None else layers, heads or c_heads
    F, S, V = ffn or c_ffn, seq_len or c_seq, vocab or c_vocab
    if C != nH * HEAD_DIM:
        raise ValueError(f"hidden {C} is not heads {nH} x {HEAD_DIM}")
    g = GraphBuilder()
    rng = np.random.default_rng(seed)
    ids = g.placeholder("input_ids", T.DT_INT32, [-1, S])
    mask = g.placeholder("input_mask", T.DT_INT32, [-1, S])
    with g.scope("encoder"):
        table = g.variable("shared/embedding", (rng.standard_normal((V, C)) * EMBED_STD).astype(np.float32))
        flat = g.node("Reshape", "Reshape", [ids, g.const("Reshape/shape", np.array([-1], np.int32))], T=I32)
        x = g.node("GatherV2", "GatherV2", [table, flat, g.const("GatherV2/axis", np.array(0, np.int32))],
                   Tparams=F32, Tindices=I32, Taxis=I32, batch_dims=0)
        m = g.node("Reshape", "Reshape_1", [mask, g.const("Reshape_1/shape", np.array([-1, 1, 1, S], np.int32))], T=I32)
        m = g.node("Cast", "Cast", [m], SrcT=I32, DstT=F32, Truncate=False)
        adder = g.node("Mul", "mul", [g.node("Sub", "sub", [_c(g, "sub/x", 1.0), m], T=F32), _c(g, "mul/y", -MASK_FILL)],
                       T=F32)
        bias = position_bias(g, S, nH, buckets, max_distance, rng)
        total = g.node("AddV2", "position_bias_masked", [bias, adder], T=F32) if shared_sum else None
        for li in range(L):
            with g.scope(f"block_{li}"):
                with g.scope("layer_0/SelfAttention"):
                    h = rms_norm(g, x, C, rng, LN_EPS, "layer_norm")
                    h = attention_core(g, h, C, S, nH, rng, total, None) if shared_sum else \
                        attention_core(g, h, C, S, nH, rng, bias, adder)
                    h = linear(g, h, C, C, rng, "o", math.sqrt(RESIDUAL_GAIN / C))
                    x = g.node("AddV2", "add_residual", [x, h], T=F32)
                with g.scope("layer_1/DenseReluDense"):
                    h = rms_norm(g, x, C, rng, LN_EPS, "layer_norm")
                    x = g.node("AddV2", "add_residual", [x, relu_ffn(g, h, C, F, rng)], T=F32)
        x = rms_norm(g, x, C, rng, LN_EPS, "final_layer_norm")
        hidden_out = g.node("Reshape", "Reshape_2", [x, g.const("Reshape_2/shape", np.array([-1, S, C], np.int32))],
                            T=F32)
        mf = g.node("Reshape", "Reshape_3", [mask, g.const("Reshape_3/shape", np.array([-1, S, 1], np.int32))], T=I32)
        mf = g.node("Cast", "Cast_1", [mf], SrcT=I32, DstT=F32, Truncate=False)
        axis = g.const("pool/reduction_indices", np.array([1], np.int32))
        tot = g.node("Sum", "pool/Sum", [g.node("Mul", "pool/mul", [hidden_out, mf], T=F32), axis], T=F32, Tidx=I32,
                     keep_dims=False)
        cnt = g.node("Sum", "pool/Sum_1", [mf, axis], T=F32, Tidx=I32, keep_dims=False)
        pooled = g.node("RealDiv", "pool/truediv",
                        [tot, g.node("Maximum", "pool/Maximum", [cnt, _c(g, "pool/Maximum/y", 1.0)], T=F32)], T=F32)
    saver = g.add_saver()
    ins = {"input_ids": tensor_info(ids, T.DT_INT32, [-1, S]), "input_mask": tensor_info(mask, T.DT_INT32, [-1, S])}
    outs = {"hidden": tensor_info(hidden_out, T.DT_FLOAT, [-1, S, C]), "pooled": tensor_info(pooled, T.DT_FLOAT, [-1, C])}
    return g, {"serving_default": signature(ins, outs, PREDICT_METHOD)}, saver


def export(export_dir: str, config: str = "t5_base_encoder", seed: int = 0, **overrides) -> str:
    g, sigs, saver = build_graph(config, seed, **overrides)
    return write_saved_model(export_dir, g.graph, sigs, g.variables, g.var_dtypes, saver)
