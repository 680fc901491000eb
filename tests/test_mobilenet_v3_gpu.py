"""MobileNetV3 Large / Small (random init, full width, 64 x 64 images) end to
end on the GPU runtime vs the fp32 CPU interpreter of the same SavedModel, as
test_mobilenet_gpu.py does for V1 / V2: the project's criterion (logit error
under 5 % of the logit spread, equal top-1 where the fp32 margin exceeds 3x the
observed error), a second run through the replay path, and the op histogram
(every hard-swish in an igemm / dwconv epilogue, every squeeze-excite block on
kernels/se.hip).

The input seed is the first of 0, 1, 2, ... at which, for BOTH models as
exported, at least 2 of the 3 rows have a top-1 / top-2 log-probability margin
above 3 x 0.05 x that row's logit spread -- rows a logit error at the 5 % limit
could not flip.  It is picked on the CPU, from the fp32 interpreter alone
(scripts/bf16_emulation.py prints these lines; the run for the committed exporter
is profiles/mobilenet_v3/input_seed_probe_cpu.log).  Seed 0 (model seed 3):

    v3_large  spread 0.100 0.092 0.092   margin 0.002 0.038 0.035   needed 0.015 0.014 0.014   2 rows
    v3_small  spread 0.063 0.065 0.064   margin 0.024 0.023 0.025   needed 0.009 0.010 0.010   3 rows

At most one of the three rows may be undecided in the GPU run.

Measured on an MI355X (logit error / logit spread per row, limit 0.05):

    v3_large  0.041 0.019 0.020   rows 1 and 2 decided, equal classes
    v3_small  0.014 0.017 0.017   all rows decided, equal classes

The same script's bf16 emulation on the CPU (fp32 arithmetic, conv weights and
every fused op's output rounded to bf16) gives 0.019-0.040 for V3-Large and
0.013-0.021 for V3-Small at this seed: what the number format alone costs these
two random nets (docs/numerics.md, "MobileNetV3 end to end")."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

OUTS = ["classes", "probabilities"]
INPUT_SEED = 0
GONE = ("Relu6", "Mul", "Mean", "AddV2", "Add", "Conv2D", "DepthwiseConv2dNative", "FusedBatchNormV3", "Pad",
        "_HardSwish", "_HardSigmoid")


def _check_logits_and_classes(g, c):
    """test_mobilenet_gpu.py's criterion, plus the cap on undecided rows."""
    lg = np.log(np.maximum(g["probabilities"], 1e-30)).astype(np.float64)
    lc = np.log(np.maximum(c["probabilities"], 1e-30)).astype(np.float64)
    lg -= lg.mean(1, keepdims=True)
    lc -= lc.mean(1, keepdims=True)
    err = np.abs(lg - lc).max(1)
    rel = err / lc.std(1)
    print("logit error / logit spread per row:", rel)
    top2 = np.sort(lc, 1)[:, -2:]
    margin = top2[:, 1] - top2[:, 0]
    print("fp32 margin per row:", margin, "logit spread per row:", lc.std(1), "error per row:", err)
    assert (margin > 3 * 0.05 * lc.std(1)).sum() >= 2, "the input seed no longer gives two decidable rows"
    assert rel.max() < 5e-2, rel
    decided = margin > 3 * err
    assert decided.sum() >= len(decided) - 1, (margin, err)
    np.testing.assert_array_equal(g["classes"][decided], c["classes"][decided])
    return rel.max()


@pytest.mark.parametrize("version", ["v3_large", "v3_small"])
def test_mobilenet_v3_gpu_matches_cpu(tmp_path_factory, version):
    from rust_tensorflow_serving2_amd.models import mobilenet
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path = os.path.join(str(tmp_path_factory.mktemp("mobilenet_" + version)), "1")
    mobilenet.export(path, version=version, image_size=64, seed=3)
    gpu = Servable("mobilenet", 1, path, ServableOptions(device="cuda:0", max_batch_size=4))
    cpu = Servable("mobilenet", 1, path, ServableOptions(device="cpu"))
    x = np.random.default_rng(INPUT_SEED).random((3, 64, 64, 3), dtype=np.float32)
    g = gpu.run("serving_default", {"input": x}, OUTS)
    c = cpu.run("serving_default", {"input": x}, OUTS)
    assert g["probabilities"].shape == (3, 1001)
    np.testing.assert_allclose(g["probabilities"].sum(1), 1.0, atol=1e-4)
    hist = next(iter(gpu._runners.values())).program.op_histogram()
    print(version, "histogram:", dict(hist))
    _check_logits_and_classes(g, c)
    # run again (HIP-graph replay path, another batch size)
    g2 = gpu.run("serving_default", {"input": x[:2]}, OUTS)
    np.testing.assert_allclose(g2["probabilities"], g["probabilities"][:2], atol=2e-4)
    for op in GONE:
        assert op not in hist, hist
    assert hist.get("_SqueezeExcite") == (8 if version == "v3_large" else 9), hist
    assert hist.get("_FusedDepthwiseConv2D") == (15 if version == "v3_large" else 11), hist
    assert hist.get("_FusedConv2D") == (33 if version == "v3_large" else 25), hist
    assert hist.get("_GlobalAvgPool") == 1, hist
