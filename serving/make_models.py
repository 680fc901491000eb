"""Synthesize the model repository (``serving/fetch.sh`` equivalent, no network).

The reference downloads ``resnet_v2_fp32_savedmodel_NHWC`` and copies version
``1538687283`` into ``models/1/`` plus an ``example.jpg`` (``serving/fetch.sh:7-31``).
Offline, we write random-init SavedModels of the same architectures in the
same ``<root>/<name>/<version>/`` layout:

    python serving/make_models.py --root serving/models [--models resnet,resnet_v2,resnext50,mobilenet,mobilenet_v2,mobilenet_v3_large,mobilenet_v3_small,efficientnet_b0,convnext_tiny,vit_b16,swin_tiny,bert,gpt2,gpt2_tiny,llama,llama_tiny,llama_8b,llama_tiny_d128,qwen3,qwen3_tiny,modernbert,t5,dlrm,half_plus_two]

* ``resnet``        ResNet-50 v1.5 (NHWC, alias "input", outputs classes/probabilities)
* ``resnet_v2``     ResNet-50 v2 pre-activation (the fetch.sh model's architecture)
* ``resnext50``     ResNeXt-50 32x4d (ResNet-50 v1.5's layout, grouped 3x3 convs: 32 groups)
* ``mobilenet``     MobileNet V1 1.0 224 (slim layout: SAME depthwise convs, ReLU6)
* ``mobilenet_v2``  MobileNet V2 1.0 224 (Keras layout: Pad + VALID on stride 2, linear bottlenecks)
* ``mobilenet_v3_large`` / ``mobilenet_v3_small``  MobileNetV3 1.0 224 (Keras layout: hard-swish, squeeze-excite)
* ``efficientnet_b0``  EfficientNet-B0 224 (Keras layout: swish, sigmoid-gated squeeze-excite, 5x5 depthwise convs)
* ``convnext_tiny``  ConvNeXt-T 224 (Keras layout: 7x7 depthwise convs, LayerNorm, erf GELU, layer scale)
* ``vit_b16``       ViT-B/16 224 (TF layout: patch conv, class token by Tile + ConcatV2, 12 pre-LN blocks, S = 197)
* ``swin_tiny``     Swin-T 224 (TF layout: 4x4 patch conv, window 7, tf.roll shifted windows, packed QKV, patch merging)
* ``bert``          BERT-base seq 128 (input_ids / input_mask / segment_ids)
* ``gpt2`` / ``gpt2_tiny``  GPT-2 124M at S = 1024 (TF layout: packed c_attn + Split, w * b - 1e4 * (1 - b) causal mask,
                    tied head on the last position; input_ids / input_mask) and a 2-layer, 128-wide one at S = 160
* ``llama`` (= ``llama_1b``) / ``llama_tiny``  Llama-style decoder, 2048 wide, 16 layers, 32 query heads over 8 K/V heads, SwiGLU 8192,
                    S = 1024 (RMSNorm, rotate-half RoPE tables as constants, K / V repeated by Tile, untied head on the
                    last position; input_ids / input_mask) and a 2-layer, 256-wide one (4 / 2 heads) at S = 160
* ``llama_8b`` / ``llama_tiny_d128``  the same decoder with 128-wide heads: 4096 wide, 32 layers, 32 / 8 heads, SwiGLU 14336,
                    S = 1024, vocabulary 32000 (~13 GB of fp32 weights), and a 2-layer, 512-wide one (4 / 2 heads) at S = 160
* ``qwen3`` (= ``qwen3_0_6b``) / ``qwen3_tiny``  Qwen3-style decoder: Llama's graph with 128-wide heads whose total width is not the
                    hidden width and a per-head RMSNorm on q and k before the rotation; 1024 wide, 28 layers, 16 / 8 heads,
                    SwiGLU 3072, S = 1024, vocabulary 32000, and a 2-layer, 256-wide one (4 / 2 heads) at S = 160
* ``gemma3`` (= ``gemma3_1b``) / ``gemma3_tiny``  Gemma-3-style decoder: 256-wide heads with QK-norm, five local layers (sliding window
                    512, rope theta 1e4) to one global, sandwich norms, tanh GeGLU; 1152 wide, 26 layers, 4 / 1 heads, MLP 6912,
                    S = 1024, vocabulary 32000, and a 3-layer, 128-wide one (window 49, one global layer) at S = 160
* ``modernbert`` (= ``modernbert_base`` and ``modernbert_tiny``)  ModernBERT-style encoder, 768 wide, 22 layers, 12 heads, GeGLU 1152,
                    S = 1024, vocabulary 50368 (pre-norm, bias-free, rotate-half RoPE in every layer, two layers in three
                    local with a +-64 band adder; input_ids / input_mask -> hidden, cls) and a 3-layer, 128-wide one at
                    S = 200 with a +-24 window
* ``t5`` (= ``t5_base_encoder`` and ``t5_tiny``)  T5 v1.0 encoder, 768 wide, 12 layers, 12 heads of 64, ReLU FFN 3072, S = 512,
                    vocabulary 32128 (pre-norm RMS LayerNorm, bias-free, no score scale, the relative-position bias of 32
                    buckets up to distance 128 added with the padding adder once for all layers; input_ids / input_mask ->
                    hidden, pooled = the masked mean) and a 3-layer, 128-wide one at S = 200
* ``dlrm``          DLRM, Criteo layout (13 dense + 26 sparse features, D = 128, tables capped at 40000 rows: 198 MB;
                    Predict dense / sparse, Classify and Regress over tf.Examples)
* ``half_plus_two`` TF Serving's canonical test model

and ``example.jpg`` (a synthetic 224x224 RGB image).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
    ap.add_argument("--models", default="resnet,half_plus_two")
    ap.add_argument("--version", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    import numpy as np
    from rust_tensorflow_serving2_amd.models import half_plus_two, resnet
    names = [m.strip() for m in args.models.split(",") if m.strip()]
    # ``modernbert`` and ``t5`` stand for both of their models
    both = {"modernbert": ("modernbert_base", "modernbert_tiny"), "t5": ("t5_base_encoder", "t5_tiny")}
    names = [n for m in names for n in both.get(m, (m,))]
    for m in names:
        out = os.path.join(args.root, m, str(args.version))
        if os.path.exists(os.path.join(out, "saved_model.pb")):
            print(f"exists: {out}")
            continue
        if m == "resnet":
            resnet.export(out, seed=args.seed)
        elif m == "resnet_v2":
            resnet.export(out, seed=args.seed, version="v2")
        elif m == "resnext50":
            resnet.export(out, seed=args.seed, groups=32, width_per_group=4)
        elif m in ("mobilenet", "mobilenet_v2", "mobilenet_v3_large", "mobilenet_v3_small"):
            from rust_tensorflow_serving2_amd.models import mobilenet
            version = {"mobilenet": "v1", "mobilenet_v2": "v2"}.get(m, m[len("mobilenet_"):])
            mobilenet.export(out, version=version, seed=args.seed)
        elif m == "efficientnet_b0":
            from rust_tensorflow_serving2_amd.models import efficientnet
            efficientnet.export(out, seed=args.seed)
        elif m == "convnext_tiny":
            from rust_tensorflow_serving2_amd.models import convnext
            convnext.export(out, seed=args.seed)
        elif m == "vit_b16":
            from rust_tensorflow_serving2_amd.models import vit
            vit.export(out, config="vit_base", patch=16, image_size=224, seed=args.seed)
        elif m == "swin_tiny":
            from rust_tensorflow_serving2_amd.models import swin
            swin.export(out, config="swin_tiny", image_size=224, seed=args.seed)
        elif m == "bert":
            from rust_tensorflow_serving2_amd.models import bert
            bert.export(out, bert.BertConfig(), seed=args.seed)
        elif m in ("gpt2", "gpt2_tiny"):
            from rust_tensorflow_serving2_amd.models import gpt2
            gpt2.export(out, m, seed=args.seed)
        elif m in ("llama", "llama_1b", "llama_tiny", "llama_8b", "llama_tiny_d128"):
            from rust_tensorflow_serving2_amd.models import llama
            llama.export(out, "llama_1b" if m == "llama" else m, seed=args.seed)
        elif m in ("qwen3", "qwen3_0_6b", "qwen3_tiny"):
            from rust_tensorflow_serving2_amd.models import qwen3
            qwen3.export(out, "qwen3_0_6b" if m == "qwen3" else m, seed=args.seed)
        elif m in ("gemma3", "gemma3_1b", "gemma3_tiny"):
            from rust_tensorflow_serving2_amd.models import gemma3
            gemma3.export(out, "gemma3_1b" if m == "gemma3" else m, seed=args.seed)
        elif m in ("modernbert_base", "modernbert_tiny"):
            from rust_tensorflow_serving2_amd.models import modernbert
            modernbert.export(out, m, seed=args.seed)
        elif m in ("t5_base_encoder", "t5_tiny"):
            from rust_tensorflow_serving2_amd.models import t5
            t5.export(out, m, seed=args.seed)
        elif m == "dlrm":
            from rust_tensorflow_serving2_amd.models import dlrm
            dlrm.export(out, "dlrm_criteo", seed=args.seed)
        elif m == "half_plus_two":
            half_plus_two.export(out)
        else:
            raise SystemExit(f"unknown model {m}")
        print(f"wrote {out}")
    from PIL import Image
    rng = np.random.default_rng(args.seed)
    img = os.path.join(args.root, "example.jpg")
    Image.fromarray(rng.integers(0, 256, (224, 224, 3), dtype=np.uint8)).save(img)
    print(f"wrote {img}")


if __name__ == "__main__":
    main()
