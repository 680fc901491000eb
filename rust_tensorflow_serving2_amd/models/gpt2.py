"""GPT-2 SavedModel exporter with random-init weights, in the op vocabulary of
the TF GPT-2 export (openai/gpt-2 ``model.py``) at a static sequence length.

* Front: ``GatherV2`` of the token table ``wte`` + the first S rows of the
  position table ``wpe`` (``Slice``), flattened once to ``[B * S, C]`` as
  models/bert.py does.  No LayerNorm follows the embedding.
* ``layers`` pre-LN blocks.  Attention: LayerNorm (eps 1e-5) -> one packed
  dense ``c_attn`` to 3 C -> ``Reshape [-1, S, 3 C]`` -> ``Split`` on the last
  axis -> per part ``Reshape [-1, S, H, 64]`` + ``Transpose`` ->
  ``BatchMatMulV2(adj_y)`` -> ``Mul`` by 1 / sqrt(64) -> the causal mask
  ``w * b - 1e4 * (1 - b)`` (``Mul`` + ``Sub``, b the ``[1, 1, S, S]``
  lower-triangular band; ``select_mask=True`` spells it ``SelectV2(b, w,
  -1e4)``) -> ``AddV2`` of the padding adder ``(1 - input_mask) * -10000`` as
  ``[B, 1, 1, S]`` (``input_mask=False`` leaves it out) -> ``Softmax`` ->
  ``BatchMatMulV2`` -> ``Transpose`` -> ``Reshape`` -> dense ``c_proj`` ->
  ``AddV2`` with the block's input.  ``packed_qkv=False`` writes three denses
  (query / key / value) instead of ``c_attn`` + ``Split``.  MLP: LayerNorm ->
  dense to 4 C + tanh GELU (models/bert.py's spelling) -> dense -> ``AddV2``.
* Tail: LayerNorm ``ln_f`` -> ``hidden`` ``[-1, S, C]``; the last position
  (``StridedSlice`` + ``Squeeze``) times the tied ``wte`` (``MatMul``,
  transpose_b) -> ``logits`` ``[-1, vocab]``.

Signature ``serving_default`` (predict): inputs ``input_ids``, ``input_mask``
(int32 [-1, S]; ``input_mask=False`` drops the second); outputs ``logits`` and
``hidden``.  Heads are 64 wide.
"""
from __future__ import annotations

import math

import numpy as np

from ..graph.builder import PREDICT_METHOD, DType, GraphBuilder, signature, tensor_info
from ..savedmodel.saved_model import write_saved_model
from ..utils import tensors as T
from .bert import _c, dense, layer_norm

F32 = DType(T.DT_FLOAT)
I32 = DType(T.DT_INT32)
HEAD_DIM = 64
LN_EPS = 1e-5
MASK_FILL = 1e4
# Every dense kernel is N(0, gain / fan-in) over LayerNorm'd (unit) rows.  QKV_GAIN 2 gives scores of
# standard deviation 2: a softmax that is neither uniform nor one-hot, so the causal mask shows in the
# output.  The two layers that write into the residual stream get RESIDUAL_GAIN, which keeps each branch
# below the embedding's scale (EMBED_STD, POS_STD) the way GPT-2's own 1 / sqrt(2 layers) residual init
# does: with unit branches on a 0.02 embedding every block replaced the stream, and the bf16 roundings of
# a 2-layer, 128-wide net reached 6 % of a hidden row's spread in the worst of 480 rows with or without
# the attention kernel (docs/numerics.md, "GPT-2 end to end").
QKV_GAIN = 2.0
RESIDUAL_GAIN = 0.01
EMBED_STD, POS_STD = 0.1, 0.05
# name -> (hidden, layers, heads, seq_len, vocab, max_position)
CONFIGS = {"gpt2": (768, 12, 12, 1024, 50257, 1024), "gpt2_tiny": (128, 2, 2, 160, 503, 192)}


def _heads(g, x, S, nH, name):
    y = g.node("Reshape", f"Reshape_{name}", [x, g.const(f"Reshape_{name}/shape",
                                                        np.array([-1, S, nH, HEAD_DIM], np.int32))], T=F32)
    return g.node("Transpose", f"transpose_{name}", [y, g.const(f"transpose_{name}/perm",
                                                                np.array([0, 2, 1, 3], np.int32))], T=F32, Tperm=I32)


def _attention(g, x, C, S, nH, rng, adder, packed_qkv, select_mask):
    if packed_qkv:
        qkv = dense(g, x, C, 3 * C, rng, "c_attn", std=math.sqrt(QKV_GAIN / C))
        qkv = g.node("Reshape", "Reshape", [qkv, g.const("Reshape/shape", np.array([-1, S, 3 * C], np.int32))], T=F32)
        sp = g.node("Split", "split", [g.const("split/split_dim", np.array(-1, np.int32)), qkv], T=F32, num_split=3)
        parts = [sp, sp + ":1", sp + ":2"]
    else:
        parts = [dense(g, x, C, C, rng, nm, std=math.sqrt(QKV_GAIN / C)) for nm in ("query", "key", "value")]
    q, k, v = [_heads(g, p, S, nH, nm) for p, nm in zip(parts, ("query", "key", "value"))]
    w = g.node("BatchMatMulV2", "MatMul", [q, k], T=F32, adj_x=False, adj_y=True)
    w = g.node("Mul", "mul", [w, _c(g, "mul/y", 1.0 / math.sqrt(HEAD_DIM))], T=F32)
    band = np.tril(np.ones((1, 1, S, S), np.float32))
    if select_mask:
        w = g.node("SelectV2", "SelectV2", [g.const("band", band.astype(bool)), w, _c(g, "SelectV2/e", -MASK_FILL)],
                   T=F32)
    else:
        b = g.const("band", band)
        one_minus = g.node("Sub", "sub", [_c(g, "sub/x", 1.0), b], T=F32)
        fill = g.node("Mul", "mul_2", [_c(g, "mul_2/x", MASK_FILL), one_minus], T=F32)
        w = g.node("Sub", "sub_1", [g.node("Mul", "mul_1", [w, b], T=F32), fill], T=F32)
    if adder is not None:
        w = g.node("AddV2", "add", [w, adder], T=F32)
    p = g.node("Softmax", "Softmax", [w], T=F32)
    a = g.node("BatchMatMulV2", "MatMul_1", [p, v], T=F32, adj_x=False, adj_y=False)
    a = g.node("Transpose", "transpose_out", [a, g.const("transpose_out/perm", np.array([0, 2, 1, 3], np.int32))],
               T=F32, Tperm=I32)
    a = g.node("Reshape", "Reshape_out", [a, g.const("Reshape_out/shape", np.array([-1, C], np.int32))], T=F32)
    return dense(g, a, C, C, rng, "c_proj", std=math.sqrt(RESIDUAL_GAIN / C))


def build_graph(config: str = "gpt2", seed: int = 0, layers: int = None, hidden: int = None, heads: int = None,
                seq_len: int = None, vocab: int = None, input_mask: bool = True, packed_qkv: bool = True,
                select_mask: bool = False):
    if config not in CONFIGS:
        raise ValueError(f"unknown GPT-2 config {config!r}: one of {sorted(CONFIGS)}")
    c_hidden, c_layers, c_heads, c_seq, c_vocab, max_pos = CONFIGS[config]
    C, L, nH = hidden or c_hidden, c_layers if layers is None else layers, heads or c_heads
    S, V = seq_len or c_seq, vocab or c_vocab
    if C != nH * HEAD_DIM:
        raise ValueError(f"hidden {C} is not heads {nH} x {HEAD_DIM}")
    max_pos = max(max_pos, S)
    g = GraphBuilder()
    rng = np.random.default_rng(seed)
    ids = g.placeholder("input_ids", T.DT_INT32, [-1, S])
    mask = g.placeholder("input_mask", T.DT_INT32, [-1, S]) if input_mask else None
    with g.scope("model"):
        wte = g.variable("wte", (rng.standard_normal((V, C)) * EMBED_STD).astype(np.float32))
        wpe = g.variable("wpe", (rng.standard_normal((max_pos, C)) * POS_STD).astype(np.float32))
        flat = g.node("Reshape", "Reshape", [ids, g.const("Reshape/shape", np.array([-1], np.int32))], T=I32)
        tok = g.node("GatherV2", "GatherV2", [wte, flat, g.const("GatherV2/axis", np.array(0, np.int32))],
                     Tparams=F32, Tindices=I32, Taxis=I32, batch_dims=0)
        tok = g.node("Reshape", "Reshape_1", [tok, g.const("Reshape_1/shape", np.array([-1, S, C], np.int32))], T=F32)
        pos = g.node("Slice", "Slice", [wpe, g.const("Slice/begin", np.array([0, 0], np.int32)),
                                        g.const("Slice/size", np.array([S, -1], np.int32))], T=F32, Index=I32)
        x = g.node("AddV2", "add", [tok, pos], T=F32)
        x = g.node("Reshape", "Reshape_2", [x, g.const("Reshape_2/shape", np.array([-1, C], np.int32))], T=F32)
        adder = None
        if input_mask:
            m = g.node("Reshape", "Reshape_3", [mask, g.const("Reshape_3/shape", np.array([-1, 1, 1, S], np.int32))],
                       T=I32)
            m = g.node("Cast", "Cast", [m], SrcT=I32, DstT=F32, Truncate=False)
            adder = g.node("Mul", "mul", [g.node("Sub", "sub", [_c(g, "sub/x", 1.0), m], T=F32),
                                          _c(g, "mul/y", -10000.0)], T=F32)
        for li in range(L):
            with g.scope(f"h{li}"):
                with g.scope("attn"):
                    h = layer_norm(g, x, C, rng, LN_EPS, "ln_1")
                    h = _attention(g, h, C, S, nH, rng, adder, packed_qkv, select_mask)
                    x = g.node("AddV2", "add", [x, h], T=F32)
                with g.scope("mlp"):
                    h = layer_norm(g, x, C, rng, LN_EPS, "ln_2")
                    h = dense(g, h, C, 4 * C, rng, "c_fc", act="gelu", std=math.sqrt(1.0 / C))
                    h = dense(g, h, 4 * C, C, rng, "c_proj", std=math.sqrt(2 * RESIDUAL_GAIN / (4 * C)))
                    x = g.node("AddV2", "add", [x, h], T=F32)
        x = layer_norm(g, x, C, rng, LN_EPS, "ln_f")
        hidden_out = g.node("Reshape", "Reshape_4", [x, g.const("Reshape_4/shape", np.array([-1, S, C], np.int32))],
                            T=F32)
        last = g.node("StridedSlice", "strided_slice",
                      [hidden_out, g.const("ss/begin", np.array([0, S - 1, 0], np.int32)),
                       g.const("ss/end", np.array([0, S, 0], np.int32)),
                       g.const("ss/strides", np.array([1, 1, 1], np.int32))],
                      T=F32, Index=I32, begin_mask=5, end_mask=5, ellipsis_mask=0, new_axis_mask=0, shrink_axis_mask=0)
        last = g.node("Squeeze", "Squeeze", [last], T=F32, squeeze_dims=[1])
        logits = g.node("MatMul", "logits", [last, wte], T=F32, transpose_a=False, transpose_b=True)
    saver = g.add_saver()
    ins = {"input_ids": tensor_info(ids, T.DT_INT32, [-1, S])}
    if input_mask:
        ins["input_mask"] = tensor_info(mask, T.DT_INT32, [-1, S])
    outs = {"logits": tensor_info(logits, T.DT_FLOAT, [-1, V]), "hidden": tensor_info(hidden_out, T.DT_FLOAT, [-1, S, C])}
    return g, {"serving_default": signature(ins, outs, PREDICT_METHOD)}, saver


def export(export_dir: str, config: str = "gpt2", seed: int = 0, **overrides) -> str:
    g, sigs, saver = build_graph(config, seed, **overrides)
    return write_saved_model(export_dir, g.graph, sigs, g.variables, g.var_dtypes, saver)
