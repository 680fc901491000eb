"""Gemma-3 through the fusion passes on the CPU, as test_qwen3_fusion does for Qwen3: the
fused graph (the ops' fp32 torch paths) == the unfused interpreter, every layer becomes a
_RopeGQAttention that carries its window, every band that is not a sliding window is left
alone, and Llama, Qwen3 and GPT-2 (whose pass must leave a window alone too) fuse as before."""
import os

import numpy as np
import pytest

from rust_tensorflow_serving2_amd.models import gemma3, gpt2, llama, qwen3
from test_llama_fusion import S, _serve

LAYERS, WINDOW = 3, 6            # gemma3_tiny: local, local, global; sliding_window 7 is window 6


def _served(models_dir, module, config, name, **kw):
    """(histogram, the fused program's _RopeGQAttention and _GeGLU impls in graph order)."""
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    _a, hist = _serve(models_dir, module, config, name, **kw)
    fused = Servable("m", 1, os.path.join(str(models_dir), name, "1"), ServableOptions(device="cpu", fuse=True))
    nodes = fused.runner("serving_default", ["input_ids", "input_mask"], ["logits", "hidden"]).program.graph.nodes
    by_layer = sorted(nodes.values(), key=lambda n: n.name)
    return hist, [n.attrs["_impl"] for n in by_layer if n.op == "_RopeGQAttention"], \
        [n.attrs["_impl"] for n in by_layer if n.op == "_GeGLU"]


@pytest.mark.parametrize("select", [False, True], ids=["sub-mul", "select"])
def test_gemma3_tiny_fused_matches_interpreter(models_dir, select):
    hist, ops, glus = _served(models_dir, gemma3, "gemma3_tiny", f"gemma3_{select}", sliding_window=WINDOW + 1,
                              select=select)
    assert hist.get("_RopeGQAttention") == LAYERS and hist.get("_FusedQKV") == LAYERS, hist
    assert hist.get("_RMSNorm") == 4 * LAYERS + 1 and hist.get("_GeGLU") == LAYERS, hist    # the sandwich norms, unchanged
    for op in ("Softmax", "BatchMatMulV2", "Tile", "Tanh", "SelectV2"):
        assert op not in hist, hist
    assert [op.window for op in ops] == [WINDOW, WINDOW, -1]
    assert all(op.d == 256 and op.qk_norm[0].shape == (256,) for op in ops) and all(g.approximate for g in glus)
    assert not np.array_equal(ops[0].cos.numpy(), ops[2].cos.numpy())                       # theta 1e4 against 1e6


def _band(kind, s=S):
    d = np.arange(s)[:, None] - np.arange(s)[None, :]
    b = (d >= 0) & (d <= WINDOW)
    if kind == "hole":
        b[s - 1, s - 3] = False
    elif kind == "off-diagonal":
        b = (d >= 1) & (d <= WINDOW + 1)
        b[0, 0] = True
    elif kind == "upper":
        b = (d <= 0) & (d >= -WINDOW)
    elif kind == "two-widths":
        b = (d >= 0) & (d <= np.where(np.arange(s) < s // 2, WINDOW, WINDOW + 1)[:, None])
    return b.astype(np.float32)


@pytest.mark.parametrize("select", [False, True], ids=["sub-mul", "select"])
@pytest.mark.parametrize("kind", ["hole", "off-diagonal", "upper", "two-widths"])
def test_bands_that_are_no_window_are_left_alone(models_dir, kind, select):
    hist, ops, _ = _served(models_dir, gemma3, "gemma3_tiny", f"gemma3_{kind}_{select}", local_band=_band(kind),
                           select=select)
    assert hist.get("_RopeGQAttention") == 1 and "_CausalAttention" not in hist and hist.get("Softmax") == 2, hist
    assert ops[0].window == -1                                                              # the global layer


def test_env_switch_leaves_windowed_cores_unfused(models_dir, monkeypatch):
    monkeypatch.setenv("TFSERVE_GEMMA", "0")
    hist, ops, _ = _served(models_dir, gemma3, "gemma3_tiny", "gemma3_switch", sliding_window=WINDOW + 1)
    assert hist.get("_RopeGQAttention") == 1 and hist.get("Softmax") == 2 and ops[0].window == -1, hist


@pytest.mark.parametrize("module,config,want", [
    (llama, "llama_tiny", {"_RopeGQAttention": 2, "_FusedQKV": 2, "_RMSNorm": 5, "_SwiGLU": 2}),
    (qwen3, "qwen3_tiny", {"_RopeGQAttention": 2, "_FusedQKV": 2, "_RMSNorm": 5, "_SwiGLU": 2}),
    (gpt2, "gpt2_tiny", {"_CausalAttention": 2, "_FusedQKV": 2})], ids=["llama", "qwen3", "gpt2"])
def test_other_decoders_fuse_as_before(models_dir, monkeypatch, module, config, want):
    monkeypatch.delenv("TFSERVE_GEMMA", raising=False)
    hist, ops, _ = _served(models_dir, module, config, f"{config}_beside_gemma")
    assert {k: hist.get(k) for k in want} == want and "Softmax" not in hist and "_GeGLU" not in hist, hist
    assert [op.window for op in ops] == [-1] * want.get("_RopeGQAttention", 0)


@pytest.mark.parametrize("mask", ["sub", "select"])
def test_gpt2_pass_leaves_a_window_alone(monkeypatch, mask):
    """GPT-2's core (no rotation) with a sliding-window band: fuse_causal_attention takes the triangle only."""
    import test_gpt2_fusion as gf
    import test_mobilenet_v3_fusion as v3f
    monkeypatch.setattr(gf, "_band", lambda kind, s: _band("window", s))
    g, fetches, shape = gf._core_graph(mask=mask, s=12)
    hist = v3f._run_both(g, fetches, {"x": v3f._x(shape, seed=2, scale=1.0)}, atol=1e-5)
    assert "_CausalAttention" not in hist and "_RopeGQAttention" not in hist and hist.get("Softmax") == 1, hist
