"""EfficientNet-B0 (random init, full width, 64 x 64 images, batch 3) end to end
on the GPU runtime vs the fp32 CPU interpreter of the same SavedModel, as
test_mobilenet_v3_gpu.py does for MobileNetV3: the project's criterion (logit
error under 5 % of the logit spread, equal top-1 where the fp32 margin exceeds 3x
the observed error, at most one undecided row), a second run through the replay
path, and the op histogram (every swish in an igemm / dwconv epilogue, every
squeeze-excite block on kernels/se.hip with its sigmoid gate).

The input seed is the first of 0, 1, 2, ... at which at least 2 of the 3 rows
have a top-1 / top-2 log-probability margin above 3 x 0.05 x that row's logit
spread -- rows a logit error at the 5 % limit could not flip.  It is picked on
the CPU, from the fp32 interpreter alone (scripts/bf16_emulation.py --family
efficientnet prints these lines; the run for the committed exporter is
profiles/efficientnet/input_seed_probe_cpu.log).

Model seed 3 (spread / margin / needed margin per row):

    seed 0   spread 0.084 0.084 0.087   margin 0.008 0.010 0.001   needed 0.013 0.013 0.013   0 rows
    seed 1   spread 0.085 0.088 0.083   margin 0.014 0.018 0.009   needed 0.013 0.013 0.013   2 rows

The head of this exporter is the dense one of MobileNet V1 / V2 (global mean,
MatMul, softmax / argmax), which fuse_classifier_head turns into one
_ClassifierHead with the pool inside: the one pool left outside the 16
squeeze-excite ops is counted there or as a _GlobalAvgPool.

Measured on an MI355X (logit error / logit spread per row, limit 0.05):

    efficientnet_b0  0.019 0.019 0.027   all rows decided, equal classes

The same script's bf16 emulation on the CPU (fp32 arithmetic, conv weights and
every fused op's output rounded to bf16) gives 0.015-0.022 at this seed: what the
number format alone costs this random net (docs/numerics.md, "EfficientNet-B0 end
to end")."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

OUTS = ["classes", "probabilities"]
INPUT_SEED = 1
GONE = ("Sigmoid", "Mul", "Mean", "_Swish", "AddV2", "Add", "Conv2D", "DepthwiseConv2dNative", "FusedBatchNormV3",
        "FusedBatchNorm", "Pad", "_SqueezeExcite")


def _check_logits_and_classes(g, c):
    """test_mobilenet_v3_gpu.py's criterion."""
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


def test_efficientnet_b0_gpu_matches_cpu(tmp_path_factory):
    from rust_tensorflow_serving2_amd.models import efficientnet
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path = os.path.join(str(tmp_path_factory.mktemp("efficientnet_b0")), "1")
    efficientnet.export(path, image_size=64, seed=3)
    gpu = Servable("efficientnet", 1, path, ServableOptions(device="cuda:0", max_batch_size=4))
    cpu = Servable("efficientnet", 1, path, ServableOptions(device="cpu"))
    x = np.random.default_rng(INPUT_SEED).random((3, 64, 64, 3), dtype=np.float32)
    g = gpu.run("serving_default", {"input": x}, OUTS)
    c = cpu.run("serving_default", {"input": x}, OUTS)
    assert g["probabilities"].shape == (3, 1000)
    np.testing.assert_allclose(g["probabilities"].sum(1), 1.0, atol=1e-4)
    hist = next(iter(gpu._runners.values())).program.op_histogram()
    print("efficientnet_b0 histogram:", dict(hist))
    _check_logits_and_classes(g, c)
    # run again (HIP-graph replay path, another batch size)
    g2 = gpu.run("serving_default", {"input": x[:2]}, OUTS)
    np.testing.assert_allclose(g2["probabilities"], g["probabilities"][:2], atol=2e-4)
    for op in GONE:
        assert op not in hist, hist
    assert hist.get("_SqueezeExciteSigmoid") == 16, hist
    assert hist.get("_FusedDepthwiseConv2D") == 16, hist
    assert hist.get("_FusedConv2D") == 33, hist
    assert hist.get("_GlobalAvgPool", 0) + hist.get("_ClassifierHead", 0) == 1, hist
