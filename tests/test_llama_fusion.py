"""Llama through the fusion passes on the CPU: the fused graph (the fp32 torch
paths of _RMSNorm, _RopeGQAttention and _SwiGLU, which compute the matched
graph's own arithmetic) == the unfused interpreter; every near miss of
fuse_rope_attention is left alone and still computes what the interpreter
computes; GPT-2 still becomes _CausalAttention."""
import os

import numpy as np
import pytest

import test_mobilenet_v3_fusion as v3f
from rust_tensorflow_serving2_amd.graph.builder import GraphBuilder
from rust_tensorflow_serving2_amd.models import llama
from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
from rust_tensorflow_serving2_amd.utils import tensors as T

OUTS = ["logits", "hidden"]
LAYERS, S = 2, 24
GONE = ("BatchMatMulV2", "Softmax", "Split", "Tile", "Neg", "ConcatV2", "Transpose", "MatMul", "Square", "Rsqrt", "Mean",
        "Sigmoid", "_Swish", "AddV2")


def _serve(models_dir, module, config, name, **kw):
    path = os.path.join(str(models_dir), name, "1")
    module.export(path, config, seed=2, seq_len=S, **kw)
    rng = np.random.default_rng(1)
    mask = np.ones((3, S), np.int32)
    mask[1, S - 5:] = 0                                         # right padding
    mask[2, :4] = 0                                             # left padding: the pad rows' arithmetic is the graph's
    feeds = {"input_ids": rng.integers(0, 503, (3, S), dtype=np.int32), "input_mask": mask}
    ref = Servable("m", 1, path, ServableOptions(device="cpu"))
    fused = Servable("m", 1, path, ServableOptions(device="cpu", fuse=True))
    a, b = ref.run("serving_default", feeds, OUTS), fused.run("serving_default", feeds, OUTS)
    for o in OUTS:
        np.testing.assert_allclose(a[o], b[o], atol=1e-5)
    return a, fused.runner("serving_default", list(feeds), OUTS).program.op_histogram()


@pytest.mark.parametrize("heads,kv_heads", [(4, 2), (4, 4), (8, 1)])
def test_llama_tiny_fused_matches_interpreter(models_dir, heads, kv_heads):
    a, hist = _serve(models_dir, llama, "llama_tiny", f"llama_{heads}_{kv_heads}", heads=heads, kv_heads=kv_heads,
                     hidden=heads * 64)
    assert a["logits"].shape == (3, 503) and a["hidden"].shape == (3, S, heads * 64)
    assert hist.get("_RopeGQAttention") == LAYERS and hist.get("_FusedQKV") == LAYERS, hist
    assert hist.get("_RMSNorm") == 2 * LAYERS + 1 and hist.get("_SwiGLU") == LAYERS, hist
    for op in GONE + ("_CausalAttention", "_Attention"):
        assert op not in hist, hist


def test_gpt2_tiny_still_becomes_causal_attention(models_dir):
    from rust_tensorflow_serving2_amd.models import gpt2
    _a, hist = _serve(models_dir, gpt2, "gpt2_tiny", "gpt2_beside_llama")
    assert hist.get("_CausalAttention") == LAYERS and "_RopeGQAttention" not in hist and "_RMSNorm" not in hist, hist


def _core_graph(s=5, h=4, k=2, table="llama", table_s=None, fetch=None, **kw):
    """llama.attention_core over x [B * S, H * 64]; one keyword makes one near miss."""
    cos, sin = llama.rope_tables(table_s or s)
    if table == "halves-differ":
        cos = cos.copy()
        cos[..., 1, 40] += 0.25
    g = GraphBuilder()
    x = g.placeholder("x", T.DT_FLOAT, [-1, h * 64])
    llama.attention_core(g, x, h * 64, s, h, k, np.random.default_rng(3), None, (cos, sin), const_weights=True, **kw)
    return g, ["Reshape_out:0"] + ([fetch] if fetch else []), (2 * s, h * 64)


NEAR_MISSES = [dict(table="halves-differ"), dict(table_s=1), dict(rotate_v=True), dict(tile_axis=2),
               dict(fetch="add_key:0"), dict(fetch="Tile_value:0")]


@pytest.mark.parametrize("kw", [dict(), dict(k=4), dict(s=1), dict(h=8, k=1)], ids=str)
def test_rope_core_is_matched(kw):
    g, fetches, shape = _core_graph(**kw)
    hist = v3f._run_both(g, fetches, {"x": v3f._x(shape, seed=2, scale=1.0)}, atol=1e-5)
    assert hist.get("_RopeGQAttention") == 1 and hist.get("_FusedQKV") == 1 and "Softmax" not in hist, hist


@pytest.mark.parametrize("kw", NEAR_MISSES, ids=str)
def test_rope_near_misses_are_left_alone(kw):
    g, fetches, shape = _core_graph(**kw)
    hist = v3f._run_both(g, fetches, {"x": v3f._x(shape, seed=2, scale=1.0)}, atol=1e-5)
    assert "_RopeGQAttention" not in hist and "_CausalAttention" not in hist and hist.get("Softmax") == 1, hist
