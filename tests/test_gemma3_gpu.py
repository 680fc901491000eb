"""gemma3_tiny (3 layers, two local with window 48 and one global; 128 wide, 4 / 1 heads of
width 256 with a QK-norm, sandwich norms, tanh GeGLU; S = 160, batch 3 with right padding)
end to end on the GPU runtime vs the fp32 CPU interpreter, as test_qwen3_gpu.py does for
Qwen3; limit 0.05 for the worst row.  The measured figures are in docs/numerics.md,
"Gemma-3 end to end".
"""
import os

import numpy as np
import pytest
import torch

from test_llama_gpu import OUTS, worst_row

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

LAYERS, S, B, C = 3, 160, 3, 128
NEW_OPS = ("_RMSNorm", "_RopeGQAttention", "_GeGLU")


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """(path, feeds, the fp32 CPU interpreter's outputs): computed once.  Rows 1 and 2 end in 40 and 7 pad tokens."""
    from rust_tensorflow_serving2_amd.models import gemma3
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path = os.path.join(str(tmp_path_factory.mktemp("gemma3_tiny")), "1")
    gemma3.export(path, "gemma3_tiny", seed=4)
    mask = np.ones((B, S), np.int32)
    mask[1, S - 40:], mask[2, S - 7:] = 0, 0
    feeds = {"input_ids": np.random.default_rng(0).integers(0, 503, (B, S), dtype=np.int32), "input_mask": mask}
    return path, feeds, Servable("gemma3", 1, path, ServableOptions(device="cpu")).run("serving_default", feeds, OUTS)


@pytest.mark.parametrize("kernels", [True, False], ids=["hip-kernels", "torch-paths"])
def test_gemma3_tiny_gpu_matches_cpu(tiny, kernels):
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path, feeds, c = tiny
    gpu = Servable("gemma3", 1, path, ServableOptions(device="cuda:0", max_batch_size=4))
    program = gpu.runner("serving_default", list(feeds), OUTS).program
    hist = program.op_histogram()
    assert hist.get("_RopeGQAttention") == LAYERS and hist.get("_GeGLU") == LAYERS, hist
    assert hist.get("_RMSNorm") == 4 * LAYERS + 1, hist
    for op in ("BatchMatMulV2", "Softmax", "Tile", "Rsqrt", "Tanh", "_CausalAttention"):
        assert op not in hist, hist
    windows = []
    for node in sorted(program.graph.nodes.values(), key=lambda n: n.name):
        if node.op == "_RopeGQAttention":
            assert node.attrs["_impl"].qk_norm is not None and node.attrs["_impl"].d == 256
            windows.append(node.attrs["_impl"].window)
        if not kernels and node.op in NEW_OPS:
            node.attrs["_impl"].use_hip = False
    assert windows == [48, 48, -1]
    g = gpu.run("serving_default", feeds, OUTS)
    assert g["logits"].shape == (B, 503) and g["hidden"].shape == (B, S, C)
    real = feeds["input_mask"].astype(bool)
    e_logits, e_hidden = worst_row(g["logits"], c["logits"]), worst_row(g["hidden"][real], c["hidden"][real])
    print(f"gemma3_tiny kernels={kernels}: worst row's error / spread: logits {e_logits:.4f}, hidden {e_hidden:.4f}")
    assert np.isfinite(g["hidden"][real]).all()
    assert e_logits < 5e-2 and e_hidden < 5e-2, (e_logits, e_hidden)
    if kernels:                       # run again (HIP-graph replay path, another batch size)
        g2 = gpu.run("serving_default", {k: v[:2] for k, v in feeds.items()}, OUTS)
        assert worst_row(g2["logits"], c["logits"][:2]) < 5e-2
