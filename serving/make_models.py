"""Synthesize the model repository (``serving/fetch.sh`` equivalent, no network).

The reference downloads ``resnet_v2_fp32_savedmodel_NHWC`` and copies version
``1538687283`` into ``models/1/`` plus an ``example.jpg`` (``serving/fetch.sh:7-31``).
Offline, we write random-init SavedModels of the same architectures in the
same ``<root>/<name>/<version>/`` layout:

    python serving/make_models.py --root serving/models [--models resnet,resnet_v2,resnext50,mobilenet,mobilenet_v2,mobilenet_v3_large,mobilenet_v3_small,efficientnet_b0,convnext_tiny,vit_b16,swin_tiny,bert,dlrm,half_plus_two]

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
    for m in [m.strip() for m in args.models.split(",") if m.strip()]:
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
