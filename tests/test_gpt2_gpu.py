"""gpt2_tiny (random init, 2 layers, 128 wide, S = 160: three key blocks, batch
3) end to end on the GPU runtime vs the fp32 CPU interpreter of the same
SavedModel: the last position's logits and the real rows of ``hidden`` within
5 % of the output's spread for the worst row, the limit every model here is
held to; then a second run through the replay path at batch 2; one
_CausalAttention per layer.

Cases: an unpadded batch, and a right-padded one (rows 1 and 2 end in 40 and 7
pad tokens).  A pad position is a query row no real token attends to and is
not compared; its logits row (the last position of a padded sequence) is.

Measured on an MI355X (worst row's error / spread, limit 0.05):

    unpadded       logits 0.0215   hidden 0.0355
    right-padded   logits 0.0166   hidden 0.0355
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
PADS = {"unpadded": (0, 0, 0), "right-padded": (0, 40, 7)}


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """(path, ids, the fp32 CPU interpreter, its outputs per case): computed once."""
    from rust_tensorflow_serving2_amd.models import gpt2
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path = os.path.join(str(tmp_path_factory.mktemp("gpt2_tiny")), "1")
    gpt2.export(path, "gpt2_tiny", seed=4)
    ids = np.random.default_rng(0).integers(0, 503, (B, S), dtype=np.int32)
    cpu = Servable("gpt2", 1, path, ServableOptions(device="cpu"))
    feeds, ref = {}, {}
    for case, pads in PADS.items():
        mask = np.ones((B, S), np.int32)
        for row, n in enumerate(pads):
            mask[row, S - n:] = 0
        feeds[case] = {"input_ids": ids, "input_mask": mask}
        ref[case] = cpu.run("serving_default", feeds[case], OUTS)
    return path, feeds, ref


def worst_row(got, want):
    """max over rows of (largest error in the row / standard deviation of the row's reference)."""
    got, want = got.astype(np.float64), want.astype(np.float64)
    return float((np.abs(got - want).max(-1) / want.std(-1)).max())


@pytest.mark.parametrize("case", list(PADS))
def test_gpt2_tiny_gpu_matches_cpu(tiny, case):
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path, feeds, ref = tiny
    gpu = Servable("gpt2", 1, path, ServableOptions(device="cuda:0", max_batch_size=4))
    g, c = gpu.run("serving_default", feeds[case], OUTS), ref[case]
    assert g["logits"].shape == (B, 503) and g["hidden"].shape == (B, S, 128)
    real = feeds[case]["input_mask"].astype(bool)
    e_logits, e_hidden = worst_row(g["logits"], c["logits"]), worst_row(g["hidden"][real], c["hidden"][real])
    print(f"gpt2_tiny {case}: worst row's error / spread: logits {e_logits:.4f}, hidden {e_hidden:.4f}")
    assert np.isfinite(g["hidden"]).all()
    assert e_logits < 5e-2 and e_hidden < 5e-2, (e_logits, e_hidden)
    hist = gpu.runner("serving_default", list(feeds[case]), OUTS).program.op_histogram()
    assert hist.get("_CausalAttention") == LAYERS and hist.get("_FusedQKV") == LAYERS, hist
    for op in ("BatchMatMulV2", "Softmax", "Split", "_Attention"):
        assert op not in hist, hist
    # run again (HIP-graph replay path, another batch size)
    g2 = gpu.run("serving_default", {k: v[:2] for k, v in feeds[case].items()}, OUTS)
    assert worst_row(g2["logits"], c["logits"][:2]) < 5e-2
