#!/usr/bin/env python
"""What does bf16 storage alone cost a MobileNet (or, with --family resnext, a
ResNeXt-50 32x4d; with --family efficientnet, an EfficientNet-B0; with --family
convnext, a ConvNeXt-T; with --family vit, a ViT-S/16; with --family swin, a
Swin-T) end to end?  CPU only.

Exports a random-init model, runs the fp32 interpreter, and runs the fused
CPU program a second time with the conv weights rounded to bf16 and the output of
every fused conv / grouped conv / depthwise / depthwise + LayerNorm / LayerNorm / squeeze-excite op
rounded to bf16 -- what the GPU
program stores -- with everything else in fp32.  Prints, per input seed:

* the fp32 interpreter's logit spread per row, its top-1 / top-2 margin, the
  margin a row needs to be decidable (3 x 0.05 x spread) and how many rows are
  (the rule tests/test_mobilenet_v3_gpu.py picks its input seed by);
* how far the logits follow the image: std over the batch / spread over classes;
* the emulated logit error / logit spread per row, the figure the end-to-end GPU
  tests hold under 0.05.  Trial 0 is plain rounding; further trials multiply each
  value by 1 + u * 2^-9, u uniform in (-1/2, 1/2), before rounding: another sample
  of the rounding errors, as another summation order would give.

`--gated-gain` / `--expand-gain` override models/mobilenet.py's init gains
(V3_GATED_PROJECT_GAIN / V3_EXPAND_GAIN) for the exported model, or, with
--family efficientnet, models/efficientnet.py's GATED_PROJECT_GAIN / EXPAND_GAIN.
`--layer-scale` overrides models/convnext.py's LAYER_SCALE_INIT.
`--vit-gains DENSE RESIDUAL QK` overrides models/vit.py's DENSE_GAIN, RESIDUAL_GAIN and QK_GAIN; with
--family vit the GEMMs' bf16 outputs (everything but the fp32 head), the packed QKV, the attention
output and the patch tokens are rounded as well, and --vit-config / --patch pick the model.
`--swin-gains DENSE RESIDUAL QK` does the same for models/swin.py (--family swin, Swin-T, window 7; the
same ops rounded, _WindowAttention in _Attention's place); `--swin-bias-std` overrides its BIAS_STD.

    python scripts/bf16_emulation.py --version v3_small --seeds 0 1 2 3 --trials 3
    python scripts/bf16_emulation.py --family resnext --seeds 3 4 --trials 1
    python scripts/bf16_emulation.py --family efficientnet --seeds 0 1 2 --trials 3
    python scripts/bf16_emulation.py --family convnext --seeds 0 1 2 --trials 3
    python scripts/bf16_emulation.py --family vit --image-size 224 --seeds 0 1 2 --trials 2
    python scripts/bf16_emulation.py --family swin --image-size 224 --seeds 0 1 2 --trials 2
    python scripts/bf16_emulation.py --family dlrm --batch 64 --seeds 0 1 2 --trials 2 [--emb-scale 1.0]
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rust_tensorflow_serving2_amd.models import mobilenet  # noqa: E402
from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions  # noqa: E402

OUTS = ["classes", "probabilities"]
ROUNDED = ("_FusedConv2D", "_FusedGroupedConv2D", "_FusedDepthwiseConv2D", "_SqueezeExcite", "_SqueezeExciteSigmoid",
           "_FusedDepthwiseLN", "_LayerNorm")
VIT_ROUNDED = ROUNDED + ("_FusedMatMul", "_FusedQKV", "_Attention", "_WindowAttention", "_PatchTokens")


def bf16(t):
    return t.to(torch.bfloat16).float()


def centred_logits(probs):
    lg = np.log(np.maximum(probs, 1e-30)).astype(np.float64)
    return lg - lg.mean(1, keepdims=True)


def emulate(program, trial, ops=ROUNDED):
    """Round the fused ops' weights and outputs to bf16 in place; `trial[0]` selects the noise sample."""
    steps = []
    for step, (fn, node, ins, outs) in enumerate(program.steps):
        impl = node.attrs.get("_impl")
        if node.op in ops and not getattr(impl, "out_f32", False):
            if hasattr(impl, "w_ref"):
                impl.w_ref = bf16(impl.w_ref)

            def rounded(ctx, node, vals, fn=fn, step=step):
                res = []
                for y in fn(ctx, node, vals):
                    if trial[0]:
                        # a pattern of its own per step: one pattern for every op would add up coherently
                        # over layers of equal shape (a ViT's 12 blocks), which no summation order does
                        gen = torch.Generator().manual_seed(trial[0] * 1000003 + step * 7 + len(res))
                        y = y * (1 + (torch.rand(y.shape, generator=gen) - 0.5) * 2.0 ** -9)
                    res.append(bf16(y))
                return res
            steps.append((rounded, node, ins, outs))
        else:
            steps.append((fn, node, ins, outs))
    program.steps = steps


DLRM_ROUNDED = ("_FusedMatMul", "_EmbeddingBag", "_DotInteraction")


def dlrm_main(a):
    """--family dlrm: models/dlrm.py's ``--dlrm-config`` at ``--vocab-cap`` and ``--emb-scale``; GEMM weights, the
    tables and every fused op's output rounded to bf16.  Prints, per input seed, the batch's fp32 logits'
    spread (max - min over the batch) and the worst |logit error| / spread."""
    from rust_tensorflow_serving2_amd.models import dlrm
    scale = dlrm.EMB_SCALE if a.emb_scale is None else a.emb_scale
    path = os.path.join(tempfile.mkdtemp(), "1")
    dlrm.export(path, a.dlrm_config, seed=a.model_seed, vocab_cap=a.vocab_cap, emb_scale=scale)
    ref = Servable("m", 1, path, ServableOptions(device="cpu"))
    emu = Servable("m", 1, path, ServableOptions(device="cpu", fuse=True))
    outs, trial = ["logits", "probabilities"], [0]
    program = emu.runner("serving_default", ["dense", "sparse"], outs).program
    emulate(program, trial, DLRM_ROUNDED)
    for _fn, node, _i, _o in program.steps:
        if node.op == "_EmbeddingBag":
            node.attrs["_impl"].blob = bf16(node.attrs["_impl"].blob)
    print(a.dlrm_config, "vocab cap", a.vocab_cap, "embedding scale", scale, "batch", a.batch)
    for s in a.seeds:
        dense, sparse = dlrm.random_inputs(a.dlrm_config, a.batch, seed=s, vocab_cap=a.vocab_cap, ends=True)
        lg = ref.run("serving_default", {"dense": dense, "sparse": sparse}, outs)["logits"].astype(np.float64).ravel()
        spread = lg.max() - lg.min()
        print(f"{a.dlrm_config} input seed {s} logits {lg.min():.3f} .. {lg.max():.3f} spread (max - min over the "
              f"batch) {spread:.4f}")
        for t in range(a.trials):
            trial[0] = t
            le = emu.run("serving_default", {"dense": bf16(torch.from_numpy(dense)).numpy(), "sparse": sparse},
                         outs)["logits"].astype(np.float64).ravel()
            print(f"    trial {t} emulated worst |logit error| {np.abs(le - lg).max():.5f} = "
                  f"{100 * np.abs(le - lg).max() / spread:.2f} % of the spread")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dlrm-config", default="dlrm_criteo")
    ap.add_argument("--vocab-cap", type=int, default=1000)
    ap.add_argument("--emb-scale", type=float)
    ap.add_argument("--family", default="mobilenet", choices=["mobilenet", "resnext", "efficientnet", "convnext", "vit", "swin", "dlrm"],
                    help="resnext: ResNeXt-50 32x4d at full width (tests/test_resnext_gpu.py's model); efficientnet: "
                         "EfficientNet-B0 at full width (tests/test_efficientnet_gpu.py's model); convnext: ConvNeXt-T "
                         "at full width and depth (tests/test_convnext_gpu.py's model); vit: ViT-S/16 "
                         "(tests/test_vit_gpu.py's model, at --image-size 224); swin: Swin-T (tests/test_swin_gpu.py's "
                         "model, at --image-size 224); --version is MobileNet's")
    ap.add_argument("--version", default="v3_small", choices=mobilenet.VERSIONS)
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--model-seed", type=int, default=3)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2, 3])
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--gated-gain", type=float)
    ap.add_argument("--expand-gain", type=float)
    ap.add_argument("--layer-scale", type=float)
    ap.add_argument("--vit-gains", type=float, nargs=3, metavar=("DENSE", "RESIDUAL", "QK"))
    ap.add_argument("--vit-config", default="vit_small")
    ap.add_argument("--swin-gains", type=float, nargs=3, metavar=("DENSE", "RESIDUAL", "QK"))
    ap.add_argument("--swin-bias-std", type=float)
    ap.add_argument("--patch", type=int, default=16)
    a = ap.parse_args()
    if a.family == "dlrm":
        return dlrm_main(a)
    if a.gated_gain is not None:
        mobilenet.V3_GATED_PROJECT_GAIN = dict(mobilenet.V3_GATED_PROJECT_GAIN, **{a.version: a.gated_gain})
    if a.expand_gain is not None:
        mobilenet.V3_EXPAND_GAIN = dict(mobilenet.V3_EXPAND_GAIN, **{a.version: a.expand_gain})
    if a.family == "efficientnet":
        from rust_tensorflow_serving2_amd.models import efficientnet
        a.version = "efficientnet_b0"
        if a.gated_gain is not None:
            efficientnet.GATED_PROJECT_GAIN = a.gated_gain
        if a.expand_gain is not None:
            efficientnet.EXPAND_GAIN = a.expand_gain
        print(a.version, "gated project gain", efficientnet.GATED_PROJECT_GAIN, "expand gain", efficientnet.EXPAND_GAIN)
    elif a.family == "convnext":
        from rust_tensorflow_serving2_amd.models import convnext
        a.version = "convnext_tiny"
        if a.layer_scale is not None:
            convnext.LAYER_SCALE_INIT = a.layer_scale
        print(a.version, "layer scale init", convnext.LAYER_SCALE_INIT)
    elif a.family == "vit":
        from rust_tensorflow_serving2_amd.models import vit
        a.version = f"{a.vit_config}/{a.patch}"
        gains = tuple(a.vit_gains) if a.vit_gains else (vit.DENSE_GAIN, vit.RESIDUAL_GAIN, vit.QK_GAIN)
        print(a.version, "dense / residual / qk gains", gains)
    elif a.family == "swin":
        from rust_tensorflow_serving2_amd.models import swin
        a.version = "swin_tiny"
        if a.swin_bias_std is not None:
            swin.BIAS_STD = a.swin_bias_std
        gains = tuple(a.swin_gains) if a.swin_gains else (swin.DENSE_GAIN, swin.RESIDUAL_GAIN, swin.QK_GAIN)
        print(a.version, "dense / residual / qk gains", gains, "bias std", swin.BIAS_STD)
    elif a.family == "resnext":
        a.version = "resnext50"
    elif a.version.startswith("v3"):
        print(a.version, "gated project gain", mobilenet.V3_GATED_PROJECT_GAIN[a.version], "expand gain",
              mobilenet.V3_EXPAND_GAIN[a.version])
    path = os.path.join(tempfile.mkdtemp(), "1")
    if a.family == "efficientnet":
        efficientnet.export(path, image_size=a.image_size, seed=a.model_seed)
    elif a.family == "convnext":
        convnext.export(path, image_size=a.image_size, seed=a.model_seed, layer_scale_init=convnext.LAYER_SCALE_INIT)
    elif a.family == "vit":
        vit.export(path, config=a.vit_config, patch=a.patch, image_size=a.image_size, seed=a.model_seed, gains=gains)
    elif a.family == "swin":
        swin.export(path, config="swin_tiny", image_size=a.image_size, seed=a.model_seed, gains=gains)
    elif a.family == "resnext":
        from rust_tensorflow_serving2_amd.models import resnet
        resnet.export(path, groups=32, width_per_group=4, image_size=a.image_size, seed=a.model_seed)
    else:
        mobilenet.export(path, version=a.version, image_size=a.image_size, seed=a.model_seed)
    ref = Servable("m", 1, path, ServableOptions(device="cpu"))
    emu = Servable("m", 1, path, ServableOptions(device="cpu", fuse=True))
    trial = [0]
    emulate(emu.runner("serving_default", ["input"], OUTS).program, trial, VIT_ROUNDED if a.family in ("vit", "swin") else ROUNDED)
    np.set_printoptions(precision=4, suppress=True)
    for s in a.seeds:
        x = np.random.default_rng(s).random((a.batch, a.image_size, a.image_size, 3), dtype=np.float32)
        lc = centred_logits(ref.run("serving_default", {"input": x}, OUTS)["probabilities"])
        spread = lc.std(1)
        top2 = np.sort(lc, 1)[:, -2:]
        margin = top2[:, 1] - top2[:, 0]
        print(f"{a.version} input seed {s} spread {spread} margin {margin} need {0.15 * spread} "
              f"ok rows {int((margin > 0.15 * spread).sum())}  image dependence {lc.std(0).mean() / spread.mean():.3f}")
        xb = bf16(torch.from_numpy(x)).numpy()
        for t in range(a.trials):
            trial[0] = t
            lg = centred_logits(emu.run("serving_default", {"input": xb}, OUTS)["probabilities"])
            print(f"    trial {t} emulated logit error / spread {np.abs(lg - lc).max(1) / spread}")


if __name__ == "__main__":
    main()
