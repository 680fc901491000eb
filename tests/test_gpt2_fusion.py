"""GPT-2 through the fusion passes on the CPU: the fused graph (the fp32 torch
path of _CausalAttention, which computes the matched graph's own arithmetic)
== the unfused interpreter, for both spellings of the causal mask, both
spellings of q / k / v and with and without the padding adder; every near miss
of fuse_causal_attention is left alone and still computes what the interpreter
computes; what fuse_attention took before the pass existed it still takes."""
import os

import numpy as np
import pytest

import test_mobilenet_v3_fusion as v3f
from rust_tensorflow_serving2_amd.graph.builder import DType, GraphBuilder
from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
from rust_tensorflow_serving2_amd.utils import tensors as T

F32 = DType(T.DT_FLOAT)
I32 = DType(T.DT_INT32)
OUTS = ["logits", "hidden"]
LAYERS, S = 2, 24
GONE = ("BatchMatMulV2", "Softmax", "Split", "SelectV2", "Transpose", "MatMul", "BiasAdd", "SquaredDifference")


@pytest.mark.parametrize("input_mask", [True, False], ids=["adder", "no-adder"])
@pytest.mark.parametrize("packed_qkv", [True, False], ids=["split", "three-denses"])
@pytest.mark.parametrize("select_mask", [False, True], ids=["sub", "select"])
def test_gpt2_tiny_fused_matches_interpreter(models_dir, select_mask, packed_qkv, input_mask):
    from rust_tensorflow_serving2_amd.models import gpt2
    path = os.path.join(str(models_dir), f"gpt2_{int(select_mask)}{int(packed_qkv)}{int(input_mask)}", "1")
    gpt2.export(path, "gpt2_tiny", seed=2, seq_len=S, select_mask=select_mask, packed_qkv=packed_qkv,
                input_mask=input_mask)
    rng = np.random.default_rng(1)
    feeds = {"input_ids": rng.integers(0, 503, (3, S), dtype=np.int32)}
    if input_mask:
        m = np.ones((3, S), np.int32)
        m[1, S - 5:] = 0                                        # right padding
        m[2, :4] = 0                                            # left padding: the pad rows' arithmetic is the graph's
        feeds["input_mask"] = m
    ref = Servable("m", 1, path, ServableOptions(device="cpu"))
    fused = Servable("m", 1, path, ServableOptions(device="cpu", fuse=True))
    a, b = ref.run("serving_default", feeds, OUTS), fused.run("serving_default", feeds, OUTS)
    assert a["logits"].shape == (3, 503) and a["hidden"].shape == (3, S, 128)
    np.testing.assert_allclose(a["logits"], b["logits"], atol=1e-5)
    np.testing.assert_allclose(a["hidden"], b["hidden"], atol=1e-5)
    hist = fused.runner("serving_default", list(feeds), OUTS).program.op_histogram()
    assert hist.get("_CausalAttention") == LAYERS and hist.get("_FusedQKV") == LAYERS, hist
    assert "_Attention" not in hist, hist
    for op in GONE:
        assert op not in hist, hist


def _band(kind, s):
    b = np.tril(np.ones((s, s), np.float32))
    if kind == "upper":
        b = b.T.copy()
    elif kind == "hole":
        b[s - 1, 1] = 0.0
    elif kind == "offset":
        b = np.tril(np.ones((s, s), np.float32), -1)
    return b


def _core_graph(mask="sub", band="lower", fill=1e4, c_bad=False, band_s=None, fetch_scores=False, s=5, h=2):
    """The attention core over x [B * S, H * 64] (test_vit_fusion's, constants for weights) with the causal
    mask spelled as ``mask``; one keyword makes one near miss."""
    import test_vit_fusion as vf
    from rust_tensorflow_serving2_amd.models import vit
    rng = np.random.default_rng(3)
    c = h * 64
    bs = band_s or s
    g = GraphBuilder()
    x = g.placeholder("x", T.DT_FLOAT, [-1, c])
    q = vit._heads(g, vf._dense_c(g, x, c, c, rng, "query"), s, h, "query")
    k = vit._heads(g, vf._dense_c(g, x, c, c, rng, "key"), s, h, "key")
    v = vit._heads(g, vf._dense_c(g, x, c, c, rng, "value"), s, h, "value")
    sc = g.node("BatchMatMulV2", "scores", [q, k], T=F32, adj_x=False, adj_y=True)
    sc = g.node("Mul", "scaled", [sc, g.const("c", np.array(0.125, np.float32))], T=F32)
    b = _band(band, bs).reshape(1, 1, bs, bs)
    if mask == "sub":
        kept = g.node("Mul", "kept", [sc, g.const("b", b)], T=F32)
        cv = (fill * (1 - b)).astype(np.float32)
        if c_bad:
            cv[0, 0, 1, bs - 1] *= 2                            # not one fill: c != fill * (1 - b)
        sc = g.node("Sub", "masked", [kept, g.const("fill", cv)], T=F32)
    elif mask == "select":
        sc = g.node("SelectV2", "masked", [g.const("b", b.astype(bool)), sc, g.const("fill", np.array(-fill, np.float32))],
                    T=F32)
    else:
        assert mask == "adder"
        sc = g.node("AddV2", "masked", [sc, g.const("adder", (-fill * (1 - b)).astype(np.float32))], T=F32)
    pr = g.node("Softmax", "Softmax", [sc], T=F32)
    ctx = g.node("BatchMatMulV2", "ctx", [pr, v], T=F32, adj_x=False, adj_y=False)
    ctx = g.node("Transpose", "t", [ctx, g.const("perm", np.array([0, 2, 1, 3], np.int32))], T=F32, Tperm=I32)
    g.node("Reshape", "out", [ctx, g.const("out/shape", np.array([-1, c], np.int32))], T=F32)
    return g, ["out:0"] + (["scaled:0"] if fetch_scores else []), (2 * s, c)


NEAR_MISSES = [dict(band="upper"), dict(band="hole"), dict(band="offset"), dict(fill=9e3), dict(mask="select", fill=9e3),
               dict(c_bad=True), dict(band_s=1), dict(fetch_scores=True), dict(mask="select", band="offset")]


def _ids(kw):
    return "-".join(f"{k}={v}" for k, v in kw.items()) or "plain"


@pytest.mark.parametrize("kw", [dict(), dict(mask="select"), dict(s=1)], ids=_ids)
def test_causal_core_is_matched(kw):
    g, fetches, shape = _core_graph(**kw)
    hist = v3f._run_both(g, fetches, {"x": v3f._x(shape, seed=2, scale=1.0)}, atol=1e-5)
    assert hist.get("_CausalAttention") == 1 and hist.get("_FusedQKV") == 1 and "Softmax" not in hist, hist


@pytest.mark.parametrize("kw", NEAR_MISSES, ids=_ids)
def test_causal_near_misses_are_left_alone(kw):
    g, fetches, shape = _core_graph(**kw)
    hist = v3f._run_both(g, fetches, {"x": v3f._x(shape, seed=2, scale=1.0)}, atol=1e-5)
    assert "_CausalAttention" not in hist and hist.get("Softmax") == 1, hist


def test_what_fuse_attention_took_it_still_takes(models_dir):
    """A constant causal [1, 1, S, S] adder on the scores, and BERT."""
    g, fetches, shape = _core_graph(mask="adder")
    hist = v3f._run_both(g, fetches, {"x": v3f._x(shape, seed=2, scale=1.0)}, atol=1e-5)
    assert hist.get("_Attention") == 1 and "_CausalAttention" not in hist, hist
    from rust_tensorflow_serving2_amd.models import bert
    path = os.path.join(str(models_dir), "bert_beside_gpt2", "1")
    bert.export(path, bert.BertConfig(vocab_size=99, hidden=128, layers=1, heads=2, intermediate=256, max_position=16,
                                      seq_len=8), seed=1)
    fused = Servable("m", 1, path, ServableOptions(device="cpu", fuse=True))
    hist = fused.runner("serving_default", ["input_ids", "input_mask", "segment_ids"],
                        ["probabilities"]).program.op_histogram()
    assert hist.get("_Attention") == 1 and "_CausalAttention" not in hist, hist
