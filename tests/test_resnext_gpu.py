"""ResNeXt-50 32x4d (random init, full width, 64 x 64 images) end to end on the
GPU runtime vs the fp32 CPU interpreter of the same SavedModel.  Full width
makes the 1x1 convs 128 ... 2048 wide (cgemm / bgemm, the dual conv, the chain)
and the sixteen grouped 3x3s run all four group widths of kernels/gconv.hip, 4 /
8 / 16 / 32 channels per group, at 16^2 down to 2^2, three of them at stride 2
behind a Pad.

bf16 storage alone (scripts/bf16_emulation.py --family resnext: conv operands
and fused-op outputs rounded to bf16 on the CPU) costs 1.4 - 1.5 % of the logit
spread per row on these inputs, with every row decidable; docs/numerics.md has
the GPU's figure."""
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


def test_resnext50_gpu_matches_cpu(tmp_path_factory):
    from rust_tensorflow_serving2_amd.models import resnet
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path = os.path.join(str(tmp_path_factory.mktemp("resnext50")), "1")
    resnet.export(path, groups=32, width_per_group=4, image_size=64, seed=3)
    gpu = Servable("resnext", 1, path, ServableOptions(device="cuda:0", max_batch_size=4))
    cpu = Servable("resnext", 1, path, ServableOptions(device="cpu"))
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
    assert "Conv2D" not in hist, hist
    assert hist.get("_FusedGroupedConv2D") == 16, hist
    kernels = [n.attrs["_impl"].kernel for _fn, n, _i, _o in next(iter(gpu._runners.values())).program.steps
               if n.op == "_FusedGroupedConv2D"]
    assert len(kernels) == 16 and all(kernels)            # every one on kernels/gconv.hip, none on the torch path
