"""DLRM-style ranking model exporter (Criteo layout) with random-init weights,
in the TF layout a ``tf.function`` of the open-source DLRM writes.

* Inputs: ``dense [B, 13]`` float and ``sparse [B, T]`` int64, T the sum of the
  per-feature hotness.  Both are the outputs of one ``ParseExample`` (a float
  ``[13]`` key ``dense`` and an int64 ``[T]`` key ``sparse``, both required), as
  models/half_plus_two.py builds them: Predict feeds the two ``Identity`` nodes
  behind it, Classify and Regress feed serialized ``tf.Example``s.
* Sparse side: ``SplitV(sparse, hotness, axis=1)`` -> per feature
  ``GatherV2(table_f [V_f, D], ids_f, axis 0)`` -> ``Sum(axis=1)``: a sum-pooled
  embedding bag per feature.
* Bottom MLP on ``dense``: ``bottom`` widths with ReLU, the last one D.
* Interaction: ``Pack([bottom, e_0 .. e_{F-1}], axis=1)`` -> ``BatchMatMulV2(Z, Z,
  adj_y)`` -> ``Reshape [-1, (F + 1)^2]`` -> the strict lower triangle by a
  constant ``GatherV2(axis=1)`` -> ``ConcatV2([bottom, pairs], axis=1)`` ->
  ``Pad`` up to a multiple of 8 columns (``dlrm_criteo``: 128 + 351 + 1 = 480).
* Top MLP: ``top`` widths with ReLU but on the last (one logit) -> ``logits``,
  ``Sigmoid`` -> ``probabilities``.

Signatures: ``serving_default`` (Predict: dense, sparse -> logits,
probabilities), ``classify`` (scores = probabilities) and ``regress`` (outputs =
logits) over the ``ParseExample``.

Configs (name -> vocab sizes, hotness, D, bottom, top):

* ``dlrm_tiny``: five tables of 5 .. 50 rows, hotness 1 .. 3, D = 32 (tests).
* ``dlrm_criteo``: the 26 categorical features of the Criteo Kaggle set, one-hot,
  D = 128, bottom 512-256-128, top 1024-1024-512-256-1.  The vocabularies are
  capped at ``VOCAB_CAP`` = 40000 rows (ids are taken modulo the cap upstream, as
  the open-source DLRM's ``--max-ind-range`` does): 367398 rows x 128 fp32 = 188 MB
  of tables + 10 MB of MLP weights, so the export stays below 256 MB on disk.

Init: MLP kernels N(0, 2 / fan-in) (the ReLU layers keep their scale), the last
layer N(0, 1 / fan-in), biases N(0, 0.01); tables N(0, EMB_SCALE^2) with
EMB_SCALE = 0.25, chosen with scripts/bf16_emulation.py --family dlrm so that a
batch's logits stay within a few units (batch 64, vocab cap 1000: -0.8 .. 2.4
at 0.25; at 1.0 they span -7 .. 18, which a sigmoid flattens; docs/numerics.md,
"DLRM end to end", profiles/dlrm/bf16_emulation_cpu.log).
"""
from __future__ import annotations

import numpy as np

from ..graph.builder import (CLASSIFY_METHOD, PREDICT_METHOD, REGRESS_METHOD, DType, GraphBuilder, Shape, signature,
                             tensor_info)
from ..savedmodel.saved_model import write_saved_model
from ..utils import tensors as T

F32 = DType(T.DT_FLOAT)
I32 = DType(T.DT_INT32)
I64 = DType(T.DT_INT64)
NUM_DENSE = 13
VOCAB_CAP = 40000
EMB_SCALE = 0.25
# the 26 categorical cardinalities of the Criteo Kaggle display-advertising set
CRITEO_VOCAB = (1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593, 3194, 27, 14992,
                5461306, 10, 5652, 2173, 4, 7046547, 18, 15, 286181, 105, 142572)
CONFIGS = {
    "dlrm_tiny": dict(vocab=(5, 50, 7, 23, 11), hot=(1, 3, 2, 1, 2), dim=32, bottom=(16, 32), top=(32, 16, 1)),
    "dlrm_criteo": dict(vocab=CRITEO_VOCAB, hot=(1,) * 26, dim=128, bottom=(512, 256, 128),
                        top=(1024, 1024, 512, 256, 1)),
}


def config(name: str = "dlrm_criteo", vocab_cap: int = VOCAB_CAP) -> dict:
    if name not in CONFIGS:
        raise ValueError(f"unknown DLRM config {name!r}: one of {sorted(CONFIGS)}")
    cfg = dict(CONFIGS[name])
    if vocab_cap < 1:
        raise ValueError(f"vocab_cap must be >= 1, got {vocab_cap}")
    cfg["vocab"] = tuple(min(int(v), int(vocab_cap)) for v in cfg["vocab"])
    if len(cfg["vocab"]) != len(cfg["hot"]) or cfg["bottom"][-1] != cfg["dim"] or cfg["top"][-1] != 1:
        raise ValueError(f"inconsistent DLRM config {name!r}")
    return cfg


def _mlp(g, x, din, widths, rng, name, last_relu):
    for i, dout in enumerate(widths):
        last = i == len(widths) - 1
        gain = 2.0 if (not last or last_relu) else 1.0
        with g.scope(f"{name}/dense_{i}"):
            w = g.variable("kernel", (rng.standard_normal((din, dout)) * np.sqrt(gain / din)).astype(np.float32))
            b = g.variable("bias", (0.01 * rng.standard_normal(dout)).astype(np.float32))
            x = g.node("MatMul", "MatMul", [x, w], T=F32, transpose_a=False, transpose_b=False)
            x = g.node("BiasAdd", "BiasAdd", [x, b], T=F32, data_format="NHWC")
            if not last or last_relu:
                x = g.node("Relu", "Relu", [x], T=F32)
        din = dout
    return x


def build_graph(name: str = "dlrm_criteo", seed: int = 0, vocab_cap: int = VOCAB_CAP, emb_scale: float = EMB_SCALE):
    cfg = config(name, vocab_cap)
    vocab, hot, D = cfg["vocab"], cfg["hot"], cfg["dim"]
    nf, t = len(vocab), int(sum(hot))
    rng = np.random.default_rng(seed)
    g = GraphBuilder()
    ser = g.placeholder("tf_example", T.DT_STRING, [-1])
    names = g.const("ParseExample/names", np.array([], dtype=object), T.DT_STRING)
    k_d = g.const("ParseExample/key_dense", np.array(b"dense", dtype=object), T.DT_STRING)
    k_s = g.const("ParseExample/key_sparse", np.array(b"sparse", dtype=object), T.DT_STRING)
    d_d = g.const("ParseExample/default_dense", np.zeros([0], np.float32))
    d_s = g.const("ParseExample/default_sparse", np.zeros([0], np.int64))
    pe = g.node("ParseExample", "ParseExample/ParseExample", [ser, names, k_d, k_s, d_d, d_s], Nsparse=0, Ndense=2,
                sparse_types=[], Tdense=[F32, I64], dense_shapes=[Shape([NUM_DENSE]), Shape([t])])
    dense = g.node("Identity", "dense", [pe], T=F32)
    sparse = g.node("Identity", "sparse", [pe + ":1"], T=I64)
    with g.scope("dlrm"):
        bot = _mlp(g, dense, NUM_DENSE, cfg["bottom"], rng, "bottom", last_relu=True)
        split = g.node("SplitV", "split", [sparse, g.const("split/size_splits", np.array(hot, np.int32)),
                                           g.const("split/axis", np.array(1, np.int32))],
                       T=I64, Tlen=I32, num_split=nf)
        axis0 = g.const("embedding/axis", np.array(0, np.int32))
        axis1 = g.const("embedding/reduction_indices", np.array(1, np.int32))
        rows = []
        for f, v in enumerate(vocab):
            with g.scope(f"embedding_{f}"):
                table = g.variable("table", (emb_scale * rng.standard_normal((v, D))).astype(np.float32))
                e = g.node("GatherV2", "GatherV2", [table, split if f == 0 else f"{split}:{f}", axis0], Tparams=F32,
                           Tindices=I64, Taxis=I32, batch_dims=0)
                rows.append(g.node("Sum", "Sum", [e, axis1], T=F32, Tidx=I32, keep_dims=False))
        z = g.node("Pack", "stack", [bot] + rows, N=nf + 1, T=F32, axis=1)
        zz = g.node("BatchMatMulV2", "interaction/MatMul", [z, z], T=F32, adj_x=False, adj_y=True)
        n = nf + 1
        flat = g.node("Reshape", "interaction/Reshape",
                      [zz, g.const("interaction/Reshape/shape", np.array([-1, n * n], np.int32))], T=F32, Tshape=I32)
        li, lj = np.tril_indices(n, -1)
        pairs = g.node("GatherV2", "interaction/GatherV2",
                       [flat, g.const("interaction/indices", (li * n + lj).astype(np.int32)),
                        g.const("interaction/axis", np.array(1, np.int32))],
                       Tparams=F32, Tindices=I32, Taxis=I32, batch_dims=0)
        x = g.node("ConcatV2", "interaction/concat", [bot, pairs, g.const("interaction/concat/axis",
                                                                          np.array(1, np.int32))],
                   N=2, T=F32, Tidx=I32)
        width = D + len(li)
        pad = -width % 8
        if pad:
            x = g.node("Pad", "interaction/Pad",
                       [x, g.const("interaction/Pad/paddings", np.array([[0, 0], [0, pad]], np.int32))],
                       T=F32, Tpaddings=I32)
        y = _mlp(g, x, width + pad, cfg["top"], rng, "top", last_relu=False)
    logits = g.node("Identity", "logits", [y], T=F32)
    probs = g.node("Sigmoid", "probabilities", [logits], T=F32)
    saver = g.add_saver()
    ti_ex = tensor_info(ser, T.DT_STRING, [-1])
    ti_logits = tensor_info(logits, T.DT_FLOAT, [-1, 1])
    ti_probs = tensor_info(probs, T.DT_FLOAT, [-1, 1])
    sigs = {
        "serving_default": signature({"dense": tensor_info(dense, T.DT_FLOAT, [-1, NUM_DENSE]),
                                      "sparse": tensor_info(sparse, T.DT_INT64, [-1, t])},
                                     {"logits": ti_logits, "probabilities": ti_probs}, PREDICT_METHOD),
        "classify": signature({"inputs": ti_ex}, {"scores": ti_probs}, CLASSIFY_METHOD),
        "regress": signature({"inputs": ti_ex}, {"outputs": ti_logits}, REGRESS_METHOD),
    }
    return g, sigs, saver


def random_inputs(name: str, batch: int, seed: int = 0, vocab_cap: int = VOCAB_CAP, ends: bool = False):
    """(dense [B, 13] float32, sparse [B, T] int64) for a config; ``ends``: the
    first two rows hold id 0 and id V_f - 1 of every table."""
    cfg = config(name, vocab_cap)
    rng = np.random.default_rng(seed)
    dense = rng.standard_normal((batch, NUM_DENSE)).astype(np.float32)
    cols = []
    for v, l in zip(cfg["vocab"], cfg["hot"]):
        ids = rng.integers(0, v, (batch, l), dtype=np.int64)
        if ends and batch >= 2:
            ids[0, :] = 0
            ids[1, :] = v - 1
        cols.append(ids)
    return dense, np.concatenate(cols, axis=1)


def export(export_dir: str, name: str = "dlrm_criteo", seed: int = 0, vocab_cap: int = VOCAB_CAP,
           emb_scale: float = EMB_SCALE) -> str:
    g, sigs, saver = build_graph(name, seed, vocab_cap, emb_scale)
    return write_saved_model(export_dir, g.graph, sigs, g.variables, g.var_dtypes, saver)
