"""Swin-T at 224 (random init, depths 2-2-6-2, window 7, 28 M parameters,
batch 3) end to end on the GPU runtime vs the fp32 CPU interpreter of the same
SavedModel, judged by test_efficientnet_gpu.py's criterion, unchanged: logit
error under 5 % of the logit spread, equal top-1 where the fp32 margin exceeds
3x the observed error, at most one undecided row; then a second run through
the replay path at batch 2, and the op histogram (one _WindowAttention with a
grid per block, no layout op, every GELU and residual add in a GEMM epilogue).
Run with the kernel and, once, with TFSERVE_WATTN=0: the op's torch path on
the device.

The input seed is the first of 0, 1, 2, ... at which at least 2 of the 3 rows
have a top-1 / top-2 log-probability margin above 3 x 0.05 x that row's logit
spread.  It is picked on the CPU, from the fp32 interpreter alone
(scripts/bf16_emulation.py --family swin --image-size 224 prints these lines;
the run for the committed exporter is profiles/swin/bf16_emulation_cpu.log).

Model seed 3 (spread / margin / needed margin per row):

    seed 0   spread 0.988 0.991 0.990   margin 0.180 0.195 0.230   needed 0.148 0.149 0.149   3 rows

Measured on an MI355X (logit error / logit spread per row, limit 0.05;
profiles/swin/test_swin_gpu.log):

    kernel   0.026 0.022 0.023   all rows decided, equal classes
    torch    0.023 0.024 0.022   all rows decided, equal classes

The same script's bf16 emulation on the CPU (fp32 arithmetic; GEMM weights and
the output of every GEMM, LayerNorm and attention rounded to bf16) gives
0.021-0.026 at this seed: what the number format alone costs this random net
(docs/numerics.md, "Swin end to end")."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from test_efficientnet_gpu import _check_logits_and_classes  # noqa: E402

OUTS = ["classes", "probabilities"]
INPUT_SEED = 0
BLOCKS = 12
GONE = ("Roll", "Transpose", "BatchMatMulV2", "Softmax", "GatherV2", "Unpack", "Erf", "Conv2D", "MatMul", "BiasAdd",
        "AddV2", "Mul", "SquaredDifference", "ExpandDims")
GRIDS = [(56, 56, 7, 0), (56, 56, 7, 3), (28, 28, 7, 0), (28, 28, 7, 3)] + [(14, 14, 7, 0), (14, 14, 7, 3)] * 3 + \
    [(7, 7, 7, 0)] * 2


@pytest.fixture(scope="module")
def swin_tiny(tmp_path_factory):
    """(path, input, the fp32 CPU interpreter's outputs): computed once."""
    from rust_tensorflow_serving2_amd.models import swin
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path = os.path.join(str(tmp_path_factory.mktemp("swin_tiny")), "1")
    swin.export(path, config="swin_tiny", image_size=224, seed=3)
    x = np.random.default_rng(INPUT_SEED).random((3, 224, 224, 3), dtype=np.float32)
    cpu = Servable("swin", 1, path, ServableOptions(device="cpu"))
    return path, x, cpu.run("serving_default", {"input": x}, OUTS)


@pytest.mark.parametrize("kernel", [True, False], ids=["kernel", "torch"])
def test_swin_tiny_gpu_matches_cpu(swin_tiny, kernel, monkeypatch):
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path, x, c = swin_tiny
    if not kernel:
        monkeypatch.setenv("TFSERVE_WATTN", "0")
    gpu = Servable("swin", 1, path, ServableOptions(device="cuda:0", max_batch_size=4))
    program = gpu.runner("serving_default", ["input"], OUTS).program
    attn = [node.attrs["_impl"] for _fn, node, _i, _o in program.steps if node.op == "_WindowAttention"]
    assert [a.grid for a in attn] == GRIDS
    assert all(a.s == 49 and a.d == 32 for a in attn) and [a.h for a in attn] == [3] * 2 + [6] * 2 + [12] * 6 + [24] * 2
    probe = torch.zeros(56 * 56, 3 * attn[0].h * 32, dtype=torch.bfloat16, device="cuda")
    assert all(a.kernel_ok(probe) == kernel for a in attn[:1])
    g = gpu.run("serving_default", {"input": x}, OUTS)
    assert g["probabilities"].shape == (3, 1000)
    np.testing.assert_allclose(g["probabilities"].sum(1), 1.0, atol=1e-4)
    hist = program.op_histogram()
    print(f"swin_tiny kernel={kernel} histogram:", dict(hist))
    worst = _check_logits_and_classes(g, c)
    print(f"swin_tiny kernel={kernel}: worst logit error / spread {worst:.4f}")
    if kernel:
        # run again (HIP-graph replay path, another batch size)
        g2 = gpu.run("serving_default", {"input": x[:2]}, OUTS)
        np.testing.assert_allclose(g2["probabilities"], g["probabilities"][:2], atol=2e-4)
    for op in GONE:
        assert op not in hist, hist
    assert hist.get("_WindowAttention") == BLOCKS and hist.get("_FusedQKV") == BLOCKS, hist
    assert hist.get("_FusedConv2D") == 1, hist
