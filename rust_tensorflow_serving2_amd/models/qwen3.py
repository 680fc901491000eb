"""Qwen3-style decoder SavedModel exporter with random-init weights: models/llama.py's
graph (its helpers spell every piece) with the three things Qwen3 changes.

* The attention width is ``H * 128``, not the hidden width: q / k / v are ``H * 128``,
  ``Hkv * 128`` and ``Hkv * 128`` wide and ``o_proj`` goes ``H * 128 -> hidden``.
* QK-norm: q and k are normalised per head before the rotation.  Each dense's output is
  reshaped to ``[-1, S, n, 128]`` (n = H for q, Hkv for k) and goes through an RMSNorm over
  the 128 head dims with a learned ``[128]`` weight of its own (``q_norm`` / ``k_norm``);
  the repeat of the K heads, the transpose and the rotation follow as in Llama.  v is not
  normalised.  The weights are ``1 + 0.25 N(0, 1)``, drawn separately, so that the two can
  be told apart in the result.
* RMS eps 1e-6 and rope theta 1e6.

The norm makes q and k rows of unit RMS times their weight, so the scores have a standard
deviation near 1 whatever the q / k denses' gain is; v and the residual branches keep
Llama's gains.  Signature and outputs are Llama's: ``input_ids``, ``input_mask`` (int32
[-1, S]) -> ``logits`` [-1, vocab] (last position), ``hidden`` [-1, S, C].
"""
from __future__ import annotations

import math

import numpy as np

from ..graph.builder import PREDICT_METHOD, GraphBuilder, signature, tensor_info
from ..savedmodel.saved_model import write_saved_model
from ..utils import tensors as T
from .bert import _c
from .llama import (EMBED_STD, F32, I32, MASK_FILL, QKV_GAIN, RESIDUAL_GAIN, _heads, linear, rms_norm, rope_tables,
                    rotate, swiglu_mlp)

HEAD_DIM = 128
RMS_EPS = 1e-6
ROPE_THETA = 1e6
QK_NORM_STD = 0.25
# name -> (hidden, layers, heads, kv_heads, mlp, seq_len, vocab).  qwen3_0_6b is Qwen3-0.6B's decoder (and the
# Qwen3-Embedding / Reranker 0.6B models') with the vocabulary cut to 32000, as models/llama.py cuts llama_8b's.
CONFIGS = {"qwen3_0_6b": (1024, 28, 16, 8, 3072, 1024, 32000), "qwen3_tiny": (256, 2, 4, 2, 512, 160, 503)}
# attention_core(miss=...): graphs that are NOT Qwen3's attention, one departure each
MISSES = ("q-only", "eps", "length", "after-rope", "read-elsewhere", "residual")


def _reshape(g, x, shape, name):
    return g.node("Reshape", name, [x, g.const(name + "/shape", np.array(shape, np.int32))], T=F32)


def attention_core(g, x, C, S, nH, nKV, rng, adder, tables, miss="", const_weights=False, head_dim=HEAD_DIM,
                   band=None, select=False):
    """q / k / v denses on x [B * S, C] -> the context [B * S, nH * head_dim] (before o_proj).  ``band``: the
    0 / 1 matrix [S, S] of open keys (default: the lower triangle; models/gemma3.py passes a sliding window);
    ``select``: the mask spelled ``SelectV2(band, w, -fill)`` instead of ``w * band - fill * (1 - band)``."""
    D = head_dim
    band = np.tril(np.ones((S, S), np.float32)) if band is None else np.asarray(band, np.float32).reshape(S, S)
    if miss and miss not in MISSES:
        raise ValueError(f"unknown miss {miss!r}: one of {MISSES}")
    std = math.sqrt(QKV_GAIN / C)
    q = linear(g, x, C, nH * D, rng, "q_proj", std, const_weights)
    k = linear(g, x, C, nKV * D, rng, "k_proj", std, const_weights)
    v = linear(g, x, C, nKV * D, rng, "v_proj", std, const_weights)
    cos, sin = g.const("rope_cos", tables[0]), g.const("rope_sin", tables[1])

    def head_norm(t, n, name, eps=RMS_EPS):
        if miss == "length":          # one norm over all heads' dims at once: a weight of n * 128
            return rms_norm(g, t, n * D, rng, eps, name, QK_NORM_STD)
        t = _reshape(g, t, [-1, S, n, D], f"Reshape_{name}")
        if miss == "residual":        # the norm of a sum: fuse_rmsnorm takes the add in
            t = g.node("AddV2", f"add_{name}", [t, t], T=F32)
        return rms_norm(g, t, D, rng, eps, name, QK_NORM_STD)
    early = miss != "after-rope"
    qn = head_norm(q, nH, "q_norm") if early else q
    if early and miss != "q-only":
        k = head_norm(k, nKV, "k_norm", 1e-5 if miss == "eps" else RMS_EPS)
    q = rotate(g, _heads(g, qn, S, nH, nH, "query", head_dim=D), cos, sin, "query")
    k = rotate(g, _heads(g, k, S, nH, nKV, "key", head_dim=D), cos, sin, "key")
    if not early:
        q, k = rms_norm(g, q, D, rng, RMS_EPS, "q_norm", QK_NORM_STD), rms_norm(g, k, D, rng, RMS_EPS, "k_norm",
                                                                               QK_NORM_STD)
    v = _heads(g, v, S, nH, nKV, "value", head_dim=D)
    w = g.node("BatchMatMulV2", "MatMul", [q, k], T=F32, adj_x=False, adj_y=True)
    w = g.node("Mul", "mul", [w, _c(g, "mul/y", 1.0 / math.sqrt(D))], T=F32)
    if select:
        w = g.node("SelectV2", "SelectV2", [g.const("band", band[None, None] > 0), w, _c(g, "SelectV2/e", -MASK_FILL)],
                   T=F32)
    else:
        b = g.const("band", band[None, None])
        one_minus = g.node("Sub", "sub", [_c(g, "sub/x", 1.0), b], T=F32)
        fill = g.node("Mul", "mul_2", [_c(g, "mul_2/x", MASK_FILL), one_minus], T=F32)
        w = g.node("Sub", "sub_1", [g.node("Mul", "mul_1", [w, b], T=F32), fill], T=F32)
    if adder is not None:
        w = g.node("AddV2", "add", [w, adder], T=F32)
    p = g.node("Softmax", "Softmax", [w], T=F32)
    a = g.node("BatchMatMulV2", "MatMul_1", [p, v], T=F32, adj_x=False, adj_y=False)
    a = g.node("Transpose", "transpose_out", [a, g.const("transpose_out/perm", np.array([0, 2, 1, 3], np.int32))],
               T=F32, Tperm=I32)
    out = _reshape(g, a, [-1, nH * D], "Reshape_out")
    if miss == "read-elsewhere":      # q's norm has a second reader (which adds 0 to the context)
        tap = g.node("Mul", "tap", [_reshape(g, qn, [-1, nH * D], "Reshape_tap"), _c(g, "tap/y", 0.0)], T=F32)
        out = g.node("AddV2", "add_tap", [out, tap], T=F32)
    return out


def build_graph(config: str = "qwen3_0_6b", seed: int = 0, layers: int = None, hidden: int = None, heads: int = None,
                kv_heads: int = None, mlp: int = None, seq_len: int = None, vocab: int = None, miss: str = ""):
    if config not in CONFIGS:
        raise ValueError(f"unknown Qwen3 config {config!r}: one of {sorted(CONFIGS)}")
    c_hidden, c_layers, c_heads, c_kv, c_mlp, c_seq, c_vocab = CONFIGS[config]
    C, L, nH = hidden or c_hidden, c_layers if layers is None else layers, heads or c_heads
    nKV, F, S, V = kv_heads or c_kv, mlp or c_mlp, seq_len or c_seq, vocab or c_vocab
    if nH % nKV:
        raise ValueError(f"kv_heads {nKV} does not divide heads {nH}")
    A = nH * HEAD_DIM
    tables = rope_tables(S, ROPE_THETA, HEAD_DIM)
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
                    h = attention_core(g, h, C, S, nH, nKV, rng, adder, tables, miss)
                    h = linear(g, h, A, C, rng, "o_proj", math.sqrt(RESIDUAL_GAIN / A))
                    x = g.node("AddV2", "add_residual", [x, h], T=F32)
                with g.scope("mlp"):
                    h = rms_norm(g, x, C, rng, RMS_EPS, "post_attention_layernorm")
                    x = g.node("AddV2", "add_residual", [x, swiglu_mlp(g, h, C, F, rng)], T=F32)
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


def export(export_dir: str, config: str = "qwen3_0_6b", seed: int = 0, **overrides) -> str:
    g, sigs, saver = build_graph(config, seed, **overrides)
    return write_saved_model(export_dir, g.graph, sigs, g.variables, g.var_dtypes, saver)
