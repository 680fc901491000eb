"""Qwen3 through the fusion passes on the CPU, as test_llama_fusion does for Llama:
the fused graph (the ops' fp32 torch paths) == the unfused interpreter, the QK-norm
goes into _RopeGQAttention, and every near miss of that match is left alone and
still computes what the interpreter computes."""
import os

import pytest

from rust_tensorflow_serving2_amd.models import qwen3
from test_llama_fusion import LAYERS, S, _serve

HIDDEN = 256


def _rope_ops(models_dir, name, **kw):
    """(outputs, histogram, the fused program's _RopeGQAttention impls)."""
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    a, hist = _serve(models_dir, qwen3, "qwen3_tiny", name, **kw)
    fused = Servable("m", 1, os.path.join(str(models_dir), name, "1"), ServableOptions(device="cpu", fuse=True))
    program = fused.runner("serving_default", ["input_ids", "input_mask"], ["logits", "hidden"]).program
    return a, hist, [n.attrs["_impl"] for n in program.graph.nodes.values() if n.op == "_RopeGQAttention"]


@pytest.mark.parametrize("heads,kv_heads", [(4, 2), (4, 4)])
def test_qwen3_tiny_fused_matches_interpreter(models_dir, heads, kv_heads):
    a, hist, ops = _rope_ops(models_dir, f"qwen3_{heads}_{kv_heads}", heads=heads, kv_heads=kv_heads)
    assert a["logits"].shape == (3, 503) and a["hidden"].shape == (3, S, HIDDEN)
    assert hist.get("_RopeGQAttention") == LAYERS and hist.get("_FusedQKV") == LAYERS, hist
    assert hist.get("_RMSNorm") == 2 * LAYERS + 1, hist
    for op in ("Softmax", "BatchMatMulV2", "Tile"):
        assert op not in hist, hist
    assert len(ops) == LAYERS
    for op in ops:
        qg, kg, eps = op.qk_norm
        assert qg.shape == kg.shape == (128,) and not (qg == kg).all() and eps == pytest.approx(1e-6)


@pytest.mark.parametrize("miss", qwen3.MISSES)
def test_near_misses_are_left_alone(models_dir, miss):
    _a, hist = _serve(models_dir, qwen3, "qwen3_tiny", f"qwen3_miss_{miss}", miss=miss)
    assert "_RopeGQAttention" not in hist and "_CausalAttention" not in hist and hist.get("Softmax") == LAYERS, hist


def test_env_switch_leaves_the_core_unfused(models_dir, monkeypatch):
    monkeypatch.setenv("TFSERVE_QKNORM", "0")
    _a, hist = _serve(models_dir, qwen3, "qwen3_tiny", "qwen3_switch")
    assert "_RopeGQAttention" not in hist and hist.get("Softmax") == LAYERS and hist.get("_RMSNorm") == 4 * LAYERS + 1, hist
