"""llama_tiny (random init, 2 layers, 256 wide, 4 query heads over 2 K/V heads,
S = 160: three key blocks, batch 3) end to end on the GPU runtime vs the fp32
CPU interpreter of the same SavedModel: the last position's logits and the real
rows of ``hidden`` within 5 % of the output's spread for the worst row, the
limit every model here is held to.  Once with the HIP kernels and once with the
three ops' torch paths on the GPU (what bf16 GEMMs alone cost on this net).

Measured on an MI355X (worst row's error / spread, limit 0.05):

    HIP kernels             logits 0.0213   hidden 0.0384
    the ops' torch paths    logits 0.0153   hidden 0.0231
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

OUTS = ["logits", "hidden"]
LAYERS, S, B = 2, 160, 3
NEW_OPS = ("_RMSNorm", "_RopeGQAttention", "_SwiGLU")


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """(path, feeds, the fp32 CPU interpreter's outputs): computed once.  Rows 1 and 2 end in 40 and 7 pad tokens."""
    from rust_tensorflow_serving2_amd.models import llama
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path = os.path.join(str(tmp_path_factory.mktemp("llama_tiny")), "1")
    llama.export(path, "llama_tiny", seed=4)
    mask = np.ones((B, S), np.int32)
    mask[1, S - 40:], mask[2, S - 7:] = 0, 0
    feeds = {"input_ids": np.random.default_rng(0).integers(0, 503, (B, S), dtype=np.int32), "input_mask": mask}
    return path, feeds, Servable("llama", 1, path, ServableOptions(device="cpu")).run("serving_default", feeds, OUTS)


def worst_row(got, want):
    """max over rows of (largest error in the row / standard deviation of the row's reference)."""
    got, want = got.astype(np.float64), want.astype(np.float64)
    return float((np.abs(got - want).max(-1) / want.std(-1)).max())


@pytest.mark.parametrize("kernels", [True, False], ids=["hip-kernels", "torch-paths"])
def test_llama_tiny_gpu_matches_cpu(tiny, kernels):
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path, feeds, c = tiny
    gpu = Servable("llama", 1, path, ServableOptions(device="cuda:0", max_batch_size=4))
    program = gpu.runner("serving_default", list(feeds), OUTS).program
    hist = program.op_histogram()
    assert hist.get("_RopeGQAttention") == LAYERS and hist.get("_SwiGLU") == LAYERS, hist
    assert hist.get("_RMSNorm") == 2 * LAYERS + 1, hist
    for op in ("BatchMatMulV2", "Softmax", "Tile", "Rsqrt", "Sigmoid", "_CausalAttention"):
        assert op not in hist, hist
    if not kernels:
        for node in program.graph.nodes.values():
            if node.op in NEW_OPS:
                node.attrs["_impl"].use_hip = False
    g = gpu.run("serving_default", feeds, OUTS)
    assert g["logits"].shape == (B, 503) and g["hidden"].shape == (B, S, 256)
    real = feeds["input_mask"].astype(bool)
    e_logits, e_hidden = worst_row(g["logits"], c["logits"]), worst_row(g["hidden"][real], c["hidden"][real])
    print(f"llama_tiny kernels={kernels}: worst row's error / spread: logits {e_logits:.4f}, hidden {e_hidden:.4f}")
    assert np.isfinite(g["hidden"][real]).all()
    assert e_logits < 5e-2 and e_hidden < 5e-2, (e_logits, e_hidden)
    if kernels:                       # run again (HIP-graph replay path, another batch size)
        g2 = gpu.run("serving_default", {k: v[:2] for k, v in feeds.items()}, OUTS)
        assert worst_row(g2["logits"], c["logits"][:2]) < 5e-2
