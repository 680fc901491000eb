"""ViT-S/16 at 224 (random init, 12 layers, S = 197, 22 M parameters, batch 3)
end to end on the GPU runtime vs the fp32 CPU interpreter of the same
SavedModel, judged by test_efficientnet_gpu.py's criterion, unchanged: logit
error under 5 % of the logit spread, equal top-1 where the fp32 margin exceeds
3x the observed error, at most one undecided row; then a second run through
the replay path at batch 2, and the op histogram (the front as one
_PatchTokens, one _Attention per layer, every GELU and residual add in a GEMM
epilogue).  Run with the attention form forced to 0 (the KV-block loop), to 1
(the register kernel at 224 padded keys) and left to ops.tuned_choice.

The input seed is the first of 0, 1, 2, ... at which at least 2 of the 3 rows
have a top-1 / top-2 log-probability margin above 3 x 0.05 x that row's logit
spread -- rows a logit error at the 5 % limit could not flip.  It is picked on
the CPU, from the fp32 interpreter alone (scripts/bf16_emulation.py --family
vit --image-size 224 prints these lines; the run for the committed exporter is
profiles/vit/input_seed_probe_cpu.log).

Model seed 3 (spread / margin / needed margin per row):

    seed 0   spread 1.014 1.020 1.018   margin 0.254 0.151 0.419   needed 0.152 0.153 0.153   2 rows

Measured on an MI355X (logit error / logit spread per row, limit 0.05):

    form 0   0.036 0.035 0.030   all rows decided, equal classes
    form 1   0.033 0.030 0.029   all rows decided, equal classes (the tuner's pick)

The same script's bf16 emulation on the CPU (fp32 arithmetic; GEMM weights and
the output of every GEMM, LayerNorm, attention and the patch tokens rounded to
bf16) gives 0.026-0.031 at this seed: what the number format alone costs this
random net (docs/numerics.md, "ViT end to end")."""
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
LAYERS = 12
GONE = ("ConcatV2", "Tile", "Pack", "BatchMatMulV2", "RealDiv", "Erf", "Softmax", "Conv2D", "MatMul", "BiasAdd", "AddV2",
        "Mul", "SquaredDifference", "Transpose")


@pytest.fixture(scope="module")
def vit_small(tmp_path_factory):
    """(path, input, the fp32 CPU interpreter's outputs): computed once."""
    from rust_tensorflow_serving2_amd.models import vit
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path = os.path.join(str(tmp_path_factory.mktemp("vit_small")), "1")
    vit.export(path, config="vit_small", patch=16, image_size=224, seed=3)
    x = np.random.default_rng(INPUT_SEED).random((3, 224, 224, 3), dtype=np.float32)
    cpu = Servable("vit", 1, path, ServableOptions(device="cpu"))
    return path, x, cpu.run("serving_default", {"input": x}, OUTS)


@pytest.mark.parametrize("form", [0, 1, None], ids=["form0", "form1", "tuned"])
def test_vit_small_gpu_matches_cpu(vit_small, form):
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path, x, c = vit_small
    gpu = Servable("vit", 1, path, ServableOptions(device="cuda:0", max_batch_size=4))
    program = gpu.runner("serving_default", ["input"], OUTS).program
    attn = [node.attrs["_impl"] for _fn, node, _i, _o in program.steps if node.op == "_Attention"]
    assert len(attn) == LAYERS and all(a.s == 197 and a.h == 6 and a.d == 64 for a in attn)
    for a in attn:
        a.form = form
    g = gpu.run("serving_default", {"input": x}, OUTS)
    assert g["probabilities"].shape == (3, 1000)
    np.testing.assert_allclose(g["probabilities"].sum(1), 1.0, atol=1e-4)
    hist = program.op_histogram()
    print(f"vit_small form {form} histogram:", dict(hist))
    worst = _check_logits_and_classes(g, c)
    print(f"vit_small form {form}: worst logit error / spread {worst:.4f}")
    # run again (HIP-graph replay path, another batch size)
    g2 = gpu.run("serving_default", {"input": x[:2]}, OUTS)
    np.testing.assert_allclose(g2["probabilities"], g["probabilities"][:2], atol=2e-4)
    for op in GONE:
        assert op not in hist, hist
    assert hist.get("_PatchTokens") == 1, hist
    assert hist.get("_Attention") == LAYERS and hist.get("_FusedQKV") == LAYERS, hist
    assert hist.get("_FusedConv2D") == 1, hist
