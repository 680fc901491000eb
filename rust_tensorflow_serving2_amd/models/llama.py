"""Llama-style decoder SavedModel exporter with random-init weights, in the op
vocabulary a TF export of the Hugging Face Llama block produces, at a static
sequence length.

* Front: ``GatherV2`` of the token table, flattened to ``[B * S, C]`` as
  models/gpt2.py does.  There is no position table: positions enter through
  the rotation of q and k.
* ``layers`` pre-norm blocks.  RMSNorm (eps 1e-5) is ``Square`` -> ``Mean``
  (last axis, keep_dims) -> ``AddV2`` eps -> ``Rsqrt`` -> ``Mul`` by x ->
  ``Mul`` by the weight.  Attention: three bias-free denses (``H * 64``,
  ``Hkv * 64``, ``Hkv * 64`` wide).  k and v are repeated for their G = H / Hkv
  query heads by ``Reshape [-1, S, Hkv, 1, 64]`` -> ``Tile [1, 1, 1, G, 1]`` ->
  ``Reshape [-1, S, H, 64]`` (left out when G = 1); q, k, v go to ``[B, H, S,
  64]`` by ``Transpose``; q and k are rotated (rotate-half convention)::

      x1, x2 = Split(x, 2, axis = -1)
      x~ = AddV2(Mul(x, cos), Mul(ConcatV2(Neg(x2), x1), sin))

  with cos / sin constants ``[1, 1, S, 64]`` (theta 10000; the two halves of a
  row are equal).  Scores, the causal mask ``w * b - 1e4 * (1 - b)``, the
  padding adder, ``Softmax`` and the context are spelled as in models/gpt2.py;
  then a bias-free ``o_proj`` and ``AddV2`` with the block's input.  MLP:
  RMSNorm -> ``Mul(swish(gate_proj x), up_proj x)`` (``x * Sigmoid(x)``) ->
  ``down_proj`` -> ``AddV2``; no biases.
* Tail: RMSNorm -> ``hidden`` ``[-1, S, C]``; the last position (``StridedSlice``
  + ``Squeeze``) times the untied ``lm_head`` -> ``logits`` ``[-1, vocab]``.

Signature ``serving_default`` (predict): inputs ``input_ids``, ``input_mask``
(int32 [-1, S]); outputs ``logits`` and ``hidden``.  Heads are ``head_dim`` wide: 64
(written so above) unless the config or the argument says 128.
"""
from __future__ import annotations

import math

import numpy as np

from ..graph.builder import PREDICT_METHOD, DType, GraphBuilder, signature, tensor_info
from ..savedmodel.saved_model import write_saved_model
from ..utils import tensors as T
from .bert import _c

F32 = DType(T.DT_FLOAT)
I32 = DType(T.DT_INT32)
HEAD_DIM = 64
RMS_EPS = 1e-5
ROPE_THETA = 10000.0
MASK_FILL = 1e4
# Every dense kernel is N(0, gain / fan-in) over RMSNorm'd (unit) rows, as in models/gpt2.py.  QKV_GAIN 2
# gives q and k entries of variance 2, which the rotation keeps, hence scores of standard deviation 2: a
# softmax that is neither uniform nor one-hot, in which both the causal mask and a one-position shift of
# the tables show.  The two layers that write into the residual stream (o_proj, down_proj) get
# RESIDUAL_GAIN, which has to keep each branch below the embedding's scale EMBED_STD = 0.1.  The
# attention output has v's variance 2 and the SwiGLU product swish(g) * u of two unit pre-activations a
# second moment of ~0.36, so a gain of 0.01 (GPT-2's) made branches of standard deviation 0.14 and 0.085,
# as large as the stream: the worst of 433 hidden rows then sat at 4.8 % of its spread with the kernels
# and with the ops' torch paths alike (docs/numerics.md, "Llama end to end").  0.0025 halves both.
# lm_head is N(0, 1 / C): unit logits.
QKV_GAIN = 2.0
RESIDUAL_GAIN = 0.0025
EMBED_STD = 0.1
# name -> (hidden, layers, heads, kv_heads, mlp, seq_len, vocab[, head_dim = HEAD_DIM]).  llama_8b is
# Llama-3-8B's decoder with the vocabulary cut to 32000, which keeps the export and the head small.
CONFIGS = {"llama_1b": (2048, 16, 32, 8, 8192, 1024, 32000), "llama_tiny": (256, 2, 4, 2, 512, 160, 503),
           "llama_tiny_d128": (512, 2, 4, 2, 1024, 160, 503, 128),
           "llama_8b": (4096, 32, 32, 8, 14336, 1024, 32000, 128)}


def rope_tables(S: int, theta: float = ROPE_THETA, dim: int = HEAD_DIM):
    """cos, sin as ``[1, 1, S, dim]`` float32; row p is ``cat(f, f)`` of ``f = p * theta ** (-2 i / dim)``."""
    inv = theta ** (-np.arange(0, dim, 2, dtype=np.float64) / dim)
    f = np.arange(S, dtype=np.float64)[:, None] * inv[None, :]
    full = np.concatenate([f, f], -1)[None, None]
    return np.cos(full).astype(np.float32), np.sin(full).astype(np.float32)


def linear(g, x, din, dout, rng, name, std, const_weights=False):
    with g.scope(name):
        make = g.const if const_weights else g.variable
        w = make("kernel", (rng.standard_normal((din, dout)) * std).astype(np.float32))
        return g.node("MatMul", "MatMul", [x, w], T=F32, transpose_a=False, transpose_b=False)


def rms_norm(g, x, dim, rng, eps, name, weight_std=0.05):
    with g.scope(name):
        gamma = g.variable("weight", (1.0 + weight_std * rng.standard_normal(dim)).astype(np.float32))
        sq = g.node("Square", "Square", [x], T=F32)
        ms = g.node("Mean", "Mean", [sq, g.const("Mean/reduction_indices", np.array([-1], np.int32))], T=F32,
                    Tidx=I32, keep_dims=True)
        rs = g.node("Rsqrt", "Rsqrt", [g.node("AddV2", "add", [ms, _c(g, "add/y", eps)], T=F32)], T=F32)
        return g.node("Mul", "mul_1", [g.node("Mul", "mul", [x, rs], T=F32), gamma], T=F32)


def _heads(g, x, S, nH, nKV, name, tile_axis=3, head_dim=HEAD_DIM):
    """[B * S, nKV * head_dim] -> [B, nH, S, head_dim]; each of the nKV heads repeated nH / nKV times."""
    if nH != nKV:
        mult = [1, 1, 1, 1, 1]
        mult[tile_axis] = nH // nKV
        x = g.node("Reshape", f"Reshape_{name}_kv", [x, g.const(f"Reshape_{name}_kv/shape",
                                                               np.array([-1, S, nKV, 1, head_dim], np.int32))], T=F32)
        x = g.node("Tile", f"Tile_{name}", [x, g.const(f"Tile_{name}/multiples", np.array(mult, np.int32))], T=F32,
                   Tmultiples=I32)
    x = g.node("Reshape", f"Reshape_{name}", [x, g.const(f"Reshape_{name}/shape",
                                                        np.array([-1, S, nH, head_dim], np.int32))], T=F32)
    return g.node("Transpose", f"transpose_{name}", [x, g.const(f"transpose_{name}/perm",
                                                                np.array([0, 2, 1, 3], np.int32))], T=F32, Tperm=I32)


def rotate(g, x, cos, sin, name):
    sp = g.node("Split", f"split_{name}", [g.const(f"split_{name}/split_dim", np.array(-1, np.int32)), x], T=F32,
                num_split=2)
    neg = g.node("Neg", f"Neg_{name}", [sp + ":1"], T=F32)
    rot = g.node("ConcatV2", f"concat_{name}", [neg, sp, g.const(f"concat_{name}/axis", np.array(-1, np.int32))],
                 T=F32, N=2, Tidx=I32)
    return g.node("AddV2", f"add_{name}", [g.node("Mul", f"mul_{name}_cos", [x, cos], T=F32),
                                           g.node("Mul", f"mul_{name}_sin", [rot, sin], T=F32)], T=F32)


def attention_core(g, x, C, S, nH, nKV, rng, adder, tables, rotate_v=False, tile_axis=3, const_weights=False,
                   head_dim=HEAD_DIM):
    """q / k / v denses on x [B * S, C] -> the context [B * S, nH * head_dim] (before o_proj).  ``tables`` =
    (cos, sin) arrays; ``rotate_v`` and ``tile_axis`` spell graphs that are NOT Llama's attention;
    ``const_weights`` writes the kernels as constants (a graph that needs no checkpoint)."""
    std = math.sqrt(QKV_GAIN / C)
    q = linear(g, x, C, nH * head_dim, rng, "q_proj", std, const_weights)
    k = linear(g, x, C, nKV * head_dim, rng, "k_proj", std, const_weights)
    v = linear(g, x, C, nKV * head_dim, rng, "v_proj", std, const_weights)
    cos, sin = g.const("rope_cos", tables[0]), g.const("rope_sin", tables[1])
    q = rotate(g, _heads(g, q, S, nH, nH, "query", head_dim=head_dim), cos, sin, "query")
    k = rotate(g, _heads(g, k, S, nH, nKV, "key", tile_axis, head_dim), cos, sin, "key")
    v = _heads(g, v, S, nH, nKV, "value", tile_axis, head_dim)
    if rotate_v:
        v = rotate(g, v, cos, sin, "value")
    w = g.node("BatchMatMulV2", "MatMul", [q, k], T=F32, adj_x=False, adj_y=True)
    w = g.node("Mul", "mul", [w, _c(g, "mul/y", 1.0 / math.sqrt(head_dim))], T=F32)
    b = g.const("band", np.tril(np.ones((1, 1, S, S), np.float32)))
    one_minus = g.node("Sub", "sub", [_c(g, "sub/x", 1.0), b], T=F32)
    fill = g.node("Mul", "mul_2", [_c(g, "mul_2/x", MASK_FILL), one_minus], T=F32)
    w = g.node("Sub", "sub_1", [g.node("Mul", "mul_1", [w, b], T=F32), fill], T=F32)
    if adder is not None:
        w = g.node("AddV2", "add", [w, adder], T=F32)
    p = g.node("Softmax", "Softmax", [w], T=F32)
    a = g.node("BatchMatMulV2", "MatMul_1", [p, v], T=F32, adj_x=False, adj_y=False)
    a = g.node("Transpose", "transpose_out", [a, g.const("transpose_out/perm", np.array([0, 2, 1, 3], np.int32))],
               T=F32, Tperm=I32)
    return g.node("Reshape", "Reshape_out", [a, g.const("Reshape_out/shape", np.array([-1, nH * head_dim], np.int32))],
                  T=F32)


def swiglu_mlp(g, x, C, F, rng):
    gate = linear(g, x, C, F, rng, "gate_proj", math.sqrt(1.0 / C))
    up = linear(g, x, C, F, rng, "up_proj", math.sqrt(1.0 / C))
    act = g.node("Mul", "swish", [gate, g.node("Sigmoid", "Sigmoid", [gate], T=F32)], T=F32)
    return linear(g, g.node("Mul", "mul", [act, up], T=F32), F, C, rng, "down_proj", math.sqrt(2 * RESIDUAL_GAIN / F))


def build_graph(config: str = "llama_1b", seed: int = 0, layers: int = None, hidden: int = None, heads: int = None,
                kv_heads: int = None, mlp: int = None, seq_len: int = None, vocab: int = None, head_dim: int = None):
    if config not in CONFIGS:
        raise ValueError(f"unknown Llama config {config!r}: one of {sorted(CONFIGS)}")
    c_hidden, c_layers, c_heads, c_kv, c_mlp, c_seq, c_vocab = CONFIGS[config][:7]
    D = head_dim or (CONFIGS[config][7:] or (HEAD_DIM,))[0]
    C, L, nH = hidden or c_hidden, c_layers if layers is None else layers, heads or c_heads
    nKV, F, S, V = kv_heads or c_kv, mlp or c_mlp, seq_len or c_seq, vocab or c_vocab
    if C != nH * D or nH % nKV:
        raise ValueError(f"hidden {C} is not heads {nH} x {D}, or kv_heads {nKV} does not divide heads")
    tables = rope_tables(S, dim=D)
    g = GraphBuilder()
    rng = np.random.default_rng(seed)
    ids = g.placeholder("input_ids", T.DT_INT32, [-1, S])
    mask = g.placeholder("input_mask", T.DT_INT32, [-1, S])
    with g.scope("model"):
        table = g.variable("embed_tokens", (rng.standard_normal((V, C)) * EMBED_STD).astype(np.float32))
        flat = g.node("Reshape", "Reshape", [ids, g.const("Reshape/shape", np.array([-1], np.int32))], T=I32)
        x = g.node("GatherV2", "GatherV2", [table, flat, g.const("GatherV2/axis", np.array(0, np.int32))],
                   Tparams=F32, Tindices=I32, Taxis=I32, batch_dims=0)
        m = g.node("Reshape", "Reshape_1", [mask, g.const("Reshape_1/shape", np.array([-1, 1, 1, S], np.int32))], T=I32)
        m = g.node("Cast", "Cast", [m], SrcT=I32, DstT=F32, Truncate=False)
        adder = g.node("Mul", "mul", [g.node("Sub", "sub", [_c(g, "sub/x", 1.0), m], T=F32), _c(g, "mul/y", -10000.0)],
                       T=F32)
        for li in range(L):
            with g.scope(f"layers_{li}"):
                with g.scope("self_attn"):
                    h = rms_norm(g, x, C, rng, RMS_EPS, "input_layernorm")
                    h = attention_core(g, h, C, S, nH, nKV, rng, adder, tables, head_dim=D)
                    h = linear(g, h, C, C, rng, "o_proj", math.sqrt(RESIDUAL_GAIN / C))
                    x = g.node("AddV2", "add_residual", [x, h], T=F32)
                with g.scope("mlp"):
                    h = rms_norm(g, x, C, rng, RMS_EPS, "post_attention_layernorm")
                    x = g.node("AddV2", "add_residual", [x, swiglu_mlp(g, h, C, F, rng)], T=F32)
        x = rms_norm(g, x, C, rng, RMS_EPS, "norm")
        hidden_out = g.node("Reshape", "Reshape_2", [x, g.const("Reshape_2/shape", np.array([-1, S, C], np.int32))],
                            T=F32)
        last = g.node("StridedSlice", "strided_slice",
                      [hidden_out, g.const("ss/begin", np.array([0, S - 1, 0], np.int32)),
                       g.const("ss/end", np.array([0, S, 0], np.int32)),
                       g.const("ss/strides", np.array([1, 1, 1], np.int32))],
                      T=F32, Index=I32, begin_mask=5, end_mask=5, ellipsis_mask=0, new_axis_mask=0, shrink_axis_mask=0)
        last = g.node("Squeeze", "Squeeze", [last], T=F32, squeeze_dims=[1])
        logits = linear(g, last, C, V, rng, "lm_head", math.sqrt(1.0 / C))
    saver = g.add_saver()
    ins = {"input_ids": tensor_info(ids, T.DT_INT32, [-1, S]), "input_mask": tensor_info(mask, T.DT_INT32, [-1, S])}
    outs = {"logits": tensor_info(logits, T.DT_FLOAT, [-1, V]), "hidden": tensor_info(hidden_out, T.DT_FLOAT, [-1, S, C])}
    return g, {"serving_default": signature(ins, outs, PREDICT_METHOD)}, saver


def export(export_dir: str, config: str = "llama_1b", seed: int = 0, **overrides) -> str:
    g, sigs, saver = build_graph(config, seed, **overrides)
    return write_saved_model(export_dir, g.graph, sigs, g.variables, g.var_dtypes, saver)
