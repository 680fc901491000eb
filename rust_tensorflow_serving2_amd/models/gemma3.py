"""Gemma-3-style decoder SavedModel exporter with random-init weights: models/llama.py's
graph (its and models/qwen3.py's helpers spell every piece) with what Gemma-3 changes.

* Heads are 256 wide and the attention width ``H * 256`` is not the hidden width, as in
  Qwen3; q and k go through a per-head RMSNorm (``q_norm`` / ``k_norm``, weights ``[256]``)
  before the rotation; the scores are scaled by ``256 ** -0.5``.
* Local and global layers.  Every ``GLOBAL_EVERY``-th layer (the last of each six) attends
  causally to every earlier token with rope theta 1e6.  The others attend to the last
  ``sliding_window`` tokens only: key j is open for query i iff ``0 <= i - j <
  sliding_window`` (``window = sliding_window - 1`` in the kernel's terms), spelled as the
  causal mask with that band, and their rope tables use theta 1e4.
* Sandwich norms: an RMSNorm before AND after attention and before AND after the MLP; the
  post norms act on the branch before it is added to the stream.
* The embedding is scaled by ``sqrt(hidden)`` (one ``Mul`` after the gather).
* The MLP is GeGLU with the tanh-approximate GELU over the two halves of one bias-free
  dense ``[gate | up]``, as models/modernbert.py spells its erf form.
* RMS eps 1e-6.

Signature and outputs are Llama's: ``input_ids``, ``input_mask`` (int32 [-1, S]) ->
``logits`` [-1, vocab] (last position), ``hidden`` [-1, S, C].
"""
from __future__ import annotations

import math

import numpy as np

from ..graph.builder import PREDICT_METHOD, GraphBuilder, signature, tensor_info
from ..savedmodel.saved_model import write_saved_model
from ..utils import tensors as T
from .bert import _c, gelu
from .llama import F32, I32, RESIDUAL_GAIN, linear, rms_norm, rope_tables
from .qwen3 import _reshape, attention_core

HEAD_DIM = 256
RMS_EPS = 1e-6
LOCAL_THETA = 1e4
GLOBAL_THETA = 1e6
GLOBAL_EVERY = 6
# The post norms emit branches of unit RMS whatever the denses' gains are, so what models/llama.py does with
# RESIDUAL_GAIN (keep each branch below the stream) is done here from the other side, as Gemma does it: the
# embedding times sqrt(hidden) is several times a branch.  The table is N(0, STREAM_STD^2 / hidden), so the scaled
# stream starts at STREAM_STD whatever the width.  With a stream that started at a branch's own scale, gemma3_tiny's
# worst hidden row sat at 6.5 % of its spread with the kernels and 6.4 % with the ops' torch paths alike
# (docs/numerics.md, "Gemma-3 end to end"): thirteen norms and six adds each store a row in bf16.
STREAM_STD = 4.0
# name -> (hidden, layers, heads, kv_heads, mlp, seq_len, vocab, sliding_window, global_every).  gemma3_1b is
# Gemma-3-1B's decoder with the vocabulary cut to 32000, as models/llama.py cuts llama_8b's; gemma3_tiny has one
# global layer in three so that a three-layer export holds both kinds.
CONFIGS = {"gemma3_1b": (1152, 26, 4, 1, 6912, 1024, 32000, 512, GLOBAL_EVERY),
           "gemma3_tiny": (128, 3, 4, 1, 256, 160, 503, 49, 3)}


def window_band(S: int, window: int) -> np.ndarray:
    """The 0 / 1 matrix [S, S] of open keys: 0 <= i - j <= window (window < 0: the whole triangle)."""
    d = np.arange(S)[:, None] - np.arange(S)[None, :]
    return ((d >= 0) & ((d <= window) | (window < 0))).astype(np.float32)


def geglu_tanh_mlp(g, x, C, F, rng):
    wi = linear(g, x, C, 2 * F, rng, "gate_up_proj", math.sqrt(1.0 / C))
    sp = g.node("Split", "split", [g.const("split/split_dim", np.array(-1, np.int32)), wi], T=F32, num_split=2)
    with g.scope("gelu"):
        act = gelu(g, sp)
    y = g.node("Mul", "mul", [act, sp + ":1"], T=F32)
    return linear(g, y, F, C, rng, "down_proj", math.sqrt(2 * RESIDUAL_GAIN / F))


def build_graph(config: str = "gemma3_1b", seed: int = 0, layers: int = None, hidden: int = None, heads: int = None,
                kv_heads: int = None, mlp: int = None, seq_len: int = None, vocab: int = None,
                sliding_window: int = None, global_every: int = None, select: bool = False, local_band=None):
    """``select`` spells the masks with SelectV2; ``local_band`` [S, S] replaces the local layers' band (graphs
    that are NOT a sliding window)."""
    if config not in CONFIGS:
        raise ValueError(f"unknown Gemma-3 config {config!r}: one of {sorted(CONFIGS)}")
    c_hidden, c_layers, c_heads, c_kv, c_mlp, c_seq, c_vocab, c_win, c_every = CONFIGS[config]
    C, L, nH = hidden or c_hidden, c_layers if layers is None else layers, heads or c_heads
    nKV, F, S, V = kv_heads or c_kv, mlp or c_mlp, seq_len or c_seq, vocab or c_vocab
    win, every = sliding_window or c_win, global_every or c_every
    if nH % nKV or win < 1:
        raise ValueError(f"kv_heads {nKV} does not divide heads {nH}, or sliding_window {win} < 1")
    A = nH * HEAD_DIM
    local = (rope_tables(S, LOCAL_THETA, HEAD_DIM), window_band(S, win - 1) if local_band is None else local_band)
    glob = (rope_tables(S, GLOBAL_THETA, HEAD_DIM), window_band(S, -1))
    g = GraphBuilder()
    rng = np.random.default_rng(seed)
    ids = g.placeholder("input_ids", T.DT_INT32, [-1, S])
    mask = g.placeholder("input_mask", T.DT_INT32, [-1, S])
    with g.scope("model"):
        table = g.variable("embed_tokens", (rng.standard_normal((V, C)) * STREAM_STD / math.sqrt(C)).astype(np.float32))
        flat = g.node("Reshape", "Reshape", [ids, g.const("Reshape/shape", np.array([-1], np.int32))], T=I32)
        x = g.node("GatherV2", "GatherV2", [table, flat, g.const("GatherV2/axis", np.array(0, np.int32))],
                   Tparams=F32, Tindices=I32, Taxis=I32, batch_dims=0)
        x = g.node("Mul", "embed_scale", [x, _c(g, "embed_scale/y", math.sqrt(C))], T=F32)
        m = g.node("Reshape", "Reshape_1", [mask, g.const("Reshape_1/shape", np.array([-1, 1, 1, S], np.int32))], T=I32)
        m = g.node("Cast", "Cast", [m], SrcT=I32, DstT=F32, Truncate=False)
        adder = g.node("Mul", "mul", [g.node("Sub", "sub", [_c(g, "sub/x", 1.0), m], T=F32), _c(g, "mul/y", -10000.0)],
                       T=F32)
        for li in range(L):
            tables, band = glob if (li + 1) % every == 0 else local
            with g.scope(f"layers_{li}"):
                with g.scope("self_attn"):
                    h = rms_norm(g, x, C, rng, RMS_EPS, "input_layernorm")
                    h = attention_core(g, h, C, S, nH, nKV, rng, adder, tables, head_dim=HEAD_DIM, band=band,
                                       select=select)
                    h = linear(g, h, A, C, rng, "o_proj", math.sqrt(RESIDUAL_GAIN / A))
                    h = rms_norm(g, h, C, rng, RMS_EPS, "post_attention_layernorm")
                    x = g.node("AddV2", "add_residual", [x, h], T=F32)
                with g.scope("mlp"):
                    h = rms_norm(g, x, C, rng, RMS_EPS, "pre_feedforward_layernorm")
                    h = rms_norm(g, geglu_tanh_mlp(g, h, C, F, rng), C, rng, RMS_EPS, "post_feedforward_layernorm")
                    x = g.node("AddV2", "add_residual", [x, h], T=F32)
        x = rms_norm(g, x, C, rng, RMS_EPS, "norm")
        hidden_out = _reshape(g, x, [-1, S, C], "Reshape_2")
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


def export(export_dir: str, config: str = "gemma3_1b", seed: int = 0, **overrides) -> str:
    g, sigs, saver = build_graph(config, seed, **overrides)
    return write_saved_model(export_dir, g.graph, sigs, g.variables, g.var_dtypes, saver)
