"""t5_tiny (3 layers, 128 wide, 2 heads, S = 200, batch 3) end to end on the GPU
runtime vs the fp32 CPU interpreter of the same SavedModel: the real rows of
``hidden`` and ``pooled`` within 5 % of the output's spread for the worst row.  Once
with the HIP kernels and once with the new op's torch path on the GPU (what bf16
storage alone costs on this net).

Measured on an MI355X (worst row's error / spread, limit 0.05):

    HIP kernels             hidden 0.0418   pooled 0.0098
    the op's torch path     hidden 0.0411   pooled 0.0096

(the unit-scale stream stored in bf16, not the kernel: docs/numerics.md, "T5 end
to end").
"""
import os

import numpy as np
import pytest
import torch

from test_llama_gpu import worst_row

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

OUTS = ["hidden", "pooled"]
LAYERS, S, B = 3, 200, 3


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """(path, feeds, the fp32 CPU interpreter's outputs): computed once.  Rows 1 and 2 end in 50 and 7 pad tokens."""
    from rust_tensorflow_serving2_amd.models import t5
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path = os.path.join(str(tmp_path_factory.mktemp("t5_tiny")), "1")
    t5.export(path, "t5_tiny", seed=4)
    mask = np.ones((B, S), np.int32)
    mask[1, S - 50:], mask[2, S - 7:] = 0, 0
    feeds = {"input_ids": np.random.default_rng(0).integers(0, 503, (B, S), dtype=np.int32), "input_mask": mask}
    return path, feeds, Servable("t5", 1, path, ServableOptions(device="cpu")).run("serving_default", feeds, OUTS)


@pytest.mark.parametrize("kernels", [True, False], ids=["hip-kernels", "torch-path"])
def test_t5_tiny_gpu_matches_cpu(tiny, kernels):
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path, feeds, c = tiny
    gpu = Servable("t5", 1, path, ServableOptions(device="cuda:0", max_batch_size=4))
    program = gpu.runner("serving_default", list(feeds), OUTS).program
    hist = program.op_histogram()
    assert hist.get("_BiasAttention") == LAYERS and hist.get("_FusedQKV") == LAYERS, hist
    assert hist.get("_RMSNorm") == 2 * LAYERS + 1, hist
    for op in ("BatchMatMulV2", "Softmax", "_Attention"):
        assert op not in hist, hist
    if not kernels:
        for node in program.graph.nodes.values():
            if node.op == "_BiasAttention":
                node.attrs["_impl"].use_hip = False
    g = gpu.run("serving_default", feeds, OUTS)
    assert g["hidden"].shape == (B, S, 128) and g["pooled"].shape == (B, 128)
    real = feeds["input_mask"].astype(bool)
    e_hidden, e_pooled = worst_row(g["hidden"][real], c["hidden"][real]), worst_row(g["pooled"], c["pooled"])
    print(f"t5_tiny kernels={kernels}: worst row's error / spread: hidden {e_hidden:.4f}, pooled {e_pooled:.4f}")
    assert np.isfinite(g["hidden"][real]).all()
    assert e_hidden < 5e-2 and e_pooled < 5e-2, (e_hidden, e_pooled)
    if kernels:                       # run again (HIP-graph replay path, another batch size)
        g2 = gpu.run("serving_default", {k: v[:2] for k, v in feeds.items()}, OUTS)
        assert worst_row(g2["pooled"], c["pooled"][:2]) < 5e-2
