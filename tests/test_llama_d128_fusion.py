"""Llama with 128-wide heads through the fusion passes on the CPU: llama_tiny_d128
fused == the unfused interpreter, and the exporter's head_dim argument at its
default changes nothing in the graphs of the existing configs."""
import os

import pytest

import test_llama_fusion as lf
from rust_tensorflow_serving2_amd.models import llama


@pytest.mark.parametrize("heads,kv_heads", [(4, 2), (4, 4)])
def test_llama_tiny_d128_fused_matches_interpreter(models_dir, heads, kv_heads):
    a, hist = lf._serve(models_dir, llama, "llama_tiny_d128", f"llama_d128_{heads}_{kv_heads}", heads=heads,
                        kv_heads=kv_heads)
    assert a["logits"].shape == (3, 503) and a["hidden"].shape == (3, lf.S, heads * 128)
    assert hist.get("_RopeGQAttention") == lf.LAYERS and hist.get("_FusedQKV") == lf.LAYERS, hist
    for op in lf.GONE + ("_CausalAttention", "_Attention"):
        assert op not in hist, hist


def test_default_head_dim_exports_the_same_graph(tmp_path):
    pbs = []
    for name, kw in (("plain", {}), ("explicit", {"head_dim": 64})):
        path = os.path.join(str(tmp_path), name, "1")
        llama.export(path, "llama_tiny", seed=2, **kw)
        with open(os.path.join(path, "saved_model.pb"), "rb") as f:
            pbs.append(f.read())
    assert pbs[0] == pbs[1]
    with pytest.raises(ValueError, match="heads 4 x 128"):
        llama.build_graph("llama_tiny", head_dim=128)
