"""MobileNet V1 / V2 (random init, full width, 64 x 64 images) end to end on
the GPU runtime vs the fp32 CPU interpreter of the same SavedModel.  Full width
makes the 64-aligned pointwise convs meet the cgemm / halo / bgemm families;
the small image makes the depthwise layers run 32^2 down to 2^2 and keeps the
tuning short."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

OUTS = ["classes", "probabilities"]


def _check_logits_and_classes(g, c):
    """bf16 GPU vs fp32 CPU (the criterion of test_resnet_gpu.py): logits
    (recovered as centred log-probabilities) within 5 % of their spread, and
    the same top-1 class wherever the fp32 top-1 / top-2 margin exceeds 3x the
    observed logit error."""
    lg = np.log(np.maximum(g["probabilities"], 1e-30)).astype(np.float64)
    lc = np.log(np.maximum(c["probabilities"], 1e-30)).astype(np.float64)
    lg -= lg.mean(1, keepdims=True)
    lc -= lc.mean(1, keepdims=True)
    err = np.abs(lg - lc).max(1)
    rel = err / lc.std(1)
    print("logit error / logit spread per row:", rel)
    assert rel.max() < 5e-2, rel
    top2 = np.sort(lc, 1)[:, -2:]
    decided = (top2[:, 1] - top2[:, 0]) > 3 * err
    assert decided.any()
    np.testing.assert_array_equal(g["classes"][decided], c["classes"][decided])
    return rel.max()


@pytest.mark.parametrize("version", ["v1", "v2"])
def test_mobilenet_gpu_matches_cpu(tmp_path_factory, version):
    from rust_tensorflow_serving2_amd.models import mobilenet
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path = os.path.join(str(tmp_path_factory.mktemp("mobilenet_" + version)), "1")
    mobilenet.export(path, version=version, image_size=64, seed=3)
    gpu = Servable("mobilenet", 1, path, ServableOptions(device="cuda:0", max_batch_size=4))
    cpu = Servable("mobilenet", 1, path, ServableOptions(device="cpu"))
    x = np.random.default_rng(1).random((3, 64, 64, 3), dtype=np.float32)
    g = gpu.run("serving_default", {"input": x}, OUTS)
    c = cpu.run("serving_default", {"input": x}, OUTS)
    assert g["probabilities"].shape == (3, 1001)
    np.testing.assert_allclose(g["probabilities"].sum(1), 1.0, atol=1e-4)
    _check_logits_and_classes(g, c)
    # run again (HIP-graph replay path, another batch size)
    g2 = gpu.run("serving_default", {"input": x[:2]}, OUTS)
    np.testing.assert_allclose(g2["probabilities"], g["probabilities"][:2], atol=2e-4)
    hist = next(iter(gpu._runners.values())).program.op_histogram()
    for op in ("DepthwiseConv2dNative", "Relu6", "Conv2D"):
        assert op not in hist, hist
    assert hist.get("_FusedDepthwiseConv2D") == (13 if version == "v1" else 17), hist
