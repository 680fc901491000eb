"""dlrm_criteo (26 tables capped at 1000 rows, D = 128, batch 64) end to end on
the GPU runtime vs the fp32 CPU interpreter of the same SavedModel.  The
project's end-to-end criterion applied per batch: the worst |logit error| is at
most 5 % of the batch's logit spread (max - min of the fp32 logits), and the
``probabilities > 0.5`` decision is equal for every row whose fp32 |logit|
exceeds 3x the observed error.  Rows 0 and 1 hold id 0 and id V_f - 1 of every
table.  Then a second run through the replay path at batch 17, and the op
histogram (one _EmbeddingBag, one _DotInteraction, none of the nodes they
replace).

Measured on an MI355X (profiles/dlrm/new_gpu_tests.log): fp32 logits -1.020 ..
1.697, worst |logit error| 0.01328 = 0.49 % of the spread (limit 5 %); the
batch-17 replay gives the first 17 rows' logits bit for bit.  The bf16
emulation on the CPU (scripts/bf16_emulation.py --family dlrm --batch 64: GEMM
weights, tables and every fused op's output rounded to bf16) gives 0.49 - 0.83 %
at three input seeds and two trials (profiles/dlrm/bf16_emulation_cpu.log;
docs/numerics.md, "DLRM end to end")."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

OUTS = ["logits", "probabilities"]
GONE = ("GatherV2", "Sum", "Pack", "BatchMatMulV2", "SplitV", "ConcatV2", "Pad")
CAP, BATCH = 1000, 64


@pytest.fixture(scope="module")
def criteo(tmp_path_factory):
    """(path, inputs, the fp32 CPU interpreter's outputs): computed once."""
    from rust_tensorflow_serving2_amd.models import dlrm
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path = os.path.join(str(tmp_path_factory.mktemp("dlrm_criteo")), "1")
    dlrm.export(path, "dlrm_criteo", seed=0, vocab_cap=CAP)
    dense, sparse = dlrm.random_inputs("dlrm_criteo", BATCH, seed=0, vocab_cap=CAP, ends=True)
    cfg = dlrm.config("dlrm_criteo", CAP)
    assert (sparse[0] == 0).all() and (sparse[1] == np.array(cfg["vocab"]) - 1).all()
    cpu = Servable("dlrm", 1, path, ServableOptions(device="cpu"))
    return path, dense, sparse, cpu.run("serving_default", {"dense": dense, "sparse": sparse}, OUTS)


def _check(g, c, what):
    lg, lc = g["logits"].astype(np.float64).reshape(-1), c["logits"].astype(np.float64).reshape(-1)
    spread = lc.max() - lc.min()
    err = np.abs(lg - lc).max()
    print(f"{what}: fp32 logits {lc.min():.3f} .. {lc.max():.3f}, worst |logit error| {err:.5f} = "
          f"{100 * err / spread:.2f} % of the spread")
    assert np.isfinite(lg).all() and err <= 0.05 * spread
    clear = np.abs(lc) > 3 * err
    assert clear.sum() >= len(lc) // 2, "too few rows with a decidable sign"
    pg, pc = g["probabilities"].reshape(-1), c["probabilities"].reshape(-1)
    assert ((pg > 0.5) == (pc > 0.5))[clear].all()
    np.testing.assert_allclose(pg, 1 / (1 + np.exp(-lg)), atol=1e-5)
    return err / spread


def test_dlrm_criteo_gpu_matches_cpu(criteo):
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path, dense, sparse, c = criteo
    gpu = Servable("dlrm", 1, path, ServableOptions(device="cuda:0", max_batch_size=BATCH))
    program = gpu.runner("serving_default", ["dense", "sparse"], OUTS).program
    hist = program.op_histogram()
    print("dlrm_criteo histogram:", dict(hist))
    assert hist.get("_EmbeddingBag") == 1 and hist.get("_DotInteraction") == 1, hist
    assert hist.get("_FusedMatMul") == 8, hist
    for op in GONE:
        assert op not in hist, hist
    bag = next(node.attrs["_impl"] for _fn, node, _i, _o in program.steps if node.op == "_EmbeddingBag")
    assert bag.blob.is_cuda and bag.blob.dtype == torch.bfloat16 and bag.split == [1] * 26 and bag.lead
    g = gpu.run("serving_default", {"dense": dense, "sparse": sparse}, OUTS)
    assert g["logits"].shape == (BATCH, 1)
    _check(g, c, f"dlrm_criteo batch {BATCH}")
    # run again (HIP-graph replay path, another batch size)
    g2 = gpu.run("serving_default", {"dense": dense[:17], "sparse": sparse[:17]}, OUTS)
    print("batch 17 vs the first 17 rows: worst |logit difference|", float(np.abs(g2["logits"] - g["logits"][:17]).max()))
    np.testing.assert_allclose(g2["probabilities"], g["probabilities"][:17], atol=2e-4)
    c17 = {k: v[:17] for k, v in c.items()}
    g3 = gpu.run("serving_default", {"dense": dense[:17], "sparse": sparse[:17]}, OUTS)
    np.testing.assert_array_equal(g3["logits"], g2["logits"])                   # replays are bit-equal
    lg = g2["logits"].astype(np.float64).reshape(-1)
    assert np.abs(lg - c17["logits"].reshape(-1)).max() <= 0.05 * (c["logits"].max() - c["logits"].min())
