"""What the fusion passes make of every exporter's graph, as text that two
commits can be diffed on: a refactor of graph/fused.py must leave it unchanged.

For each exporter under models/ (in the tiny configuration its fusion test
exports) the fused program is compiled on --device and printed one line per
step: op, node name, input refs, and a sha256 over the implementation -- every
tensor attribute (name, dtype, shape, bytes) and every plain field, children
and nested ops included.  A last line per model is the sha256 of the outputs
for one seeded batch.  On a GPU run it with TFSERVE_AUTOTUNE=0, so that shapes
the committed table lacks take their default configs.

    python scripts/fold_digest.py [--device cpu|cuda] [--models resnet_v1 vit ...]
"""
import argparse
import hashlib
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IMAGE_OUTS = ["classes", "probabilities"]


def exporters():
    """name -> (export(path), feeds by alias, output aliases)."""
    from rust_tensorflow_serving2_amd.models import bert, convnext, efficientnet, mobilenet, resnet, vit
    rng = np.random.default_rng(0)
    image = {"input": rng.random((3, 32, 32, 3), dtype=np.float32)}
    cfg = bert.BertConfig(vocab_size=100, hidden=64, layers=2, heads=2, intermediate=128, max_position=64, seq_len=32)
    mask = np.ones((3, 32), np.int32)
    mask[1, 20:] = 0
    tokens = {"input_ids": rng.integers(0, 100, (3, 32)).astype(np.int32), "input_mask": mask,
              "segment_ids": np.repeat(np.arange(32, dtype=np.int32)[None] // 16, 3, 0)}
    tiny = dict(image_size=32, num_classes=11)
    table = {
        "resnet_v1": lambda p: resnet.export(p, blocks=(1, 1, 1, 1), width=8, seed=1, **tiny),
        "resnet_v2": lambda p: resnet.export(p, version="v2", blocks=(2, 2, 1, 1), width=8, seed=4, **tiny),
        "resnext": lambda p: resnet.export(p, blocks=(1, 1, 1, 1), width=16, groups=4, width_per_group=16, seed=5,
                                           **tiny),
        "convnext": lambda p: convnext.export(p, depths=(1, 1, 2, 1), dims=(16, 24, 32, 40), seed=5, **tiny),
        "vit": lambda p: vit.export(p, hidden=128, heads=2, layers=2, mlp=256, patch=8, seed=5, **tiny),
    }
    for version in ("v1", "v2", "v3_large", "v3_small"):
        table["mobilenet_" + version] = lambda p, v=version: mobilenet.export(p, version=v, alpha=0.25, seed=5, **tiny)
    for form in ("plain", "beta", "identity_n"):
        table["efficientnet_" + form] = lambda p, f=form: efficientnet.export(p, width_coefficient=0.5, seed=5,
                                                                              swish_form=f, **tiny)
    out = {name: (fn, image, IMAGE_OUTS) for name, fn in table.items()}
    out["bert"] = (lambda p: bert.export(p, cfg, seed=3), tokens, ["pooled_output", "probabilities"])
    return out


def absorb(h, v, seen):
    """Feed the value of one attribute into the hash ``h``."""
    if isinstance(v, torch.Tensor):
        h.update(f"T{v.dtype}{tuple(v.shape)}".encode())
        h.update(v.detach().cpu().contiguous().flatten().view(torch.uint8).numpy().tobytes())
    elif isinstance(v, (tuple, list)):
        h.update(f"{type(v).__name__}{len(v)}(".encode())
        for x in v:
            absorb(h, x, seen)
    elif isinstance(v, dict):
        for k in sorted(v, key=repr):
            h.update(repr(k).encode())
            absorb(h, v[k], seen)
    elif v is None or isinstance(v, (bool, int, float, str, bytes, torch.dtype, torch.device, np.generic)):
        h.update(repr(v).encode())
    elif hasattr(v, "__dict__") and id(v) not in seen:        # a child op, or a record of plain fields
        seen.add(id(v))
        h.update(type(v).__name__.encode())
        for k in sorted(vars(v)):
            h.update(k.encode())
            absorb(h, getattr(v, k), seen)
    else:
        h.update(type(v).__name__.encode())


def digest(name, export, feeds, outs, device, root):
    from rust_tensorflow_serving2_amd.graph.compiler import compile_program
    from rust_tensorflow_serving2_amd.server import servable as S
    path = os.path.join(root, name, "1")
    export(path)
    sv = S.Servable(name, 1, path, S.ServableOptions(device=device, fuse=True, warmup=False))
    sig = sv.signature("serving_default")[1]
    ins, specs = S._specs(sig.inputs), S._specs(sig.outputs)
    aliases = sorted(feeds)
    prog = compile_program(sv.fresh_graph(), [ins[a].name for a in aliases], [specs[a].name for a in outs],
                           sv.options.torch_device, sv.passes(), sv.options.extra)
    for _fn, node, _ins, _outs in prog.steps:
        h = hashlib.sha256()
        absorb(h, node.attrs.get("_impl"), set())
        refs = ",".join(f"{n}:{i}" for n, i in node.inputs)
        print(f"{name} {node.op} {node.name} [{refs}] {h.hexdigest()[:24]}")
    values = prog.run([torch.from_numpy(feeds[a]).to(sv.options.torch_device) for a in aliases])
    h = hashlib.sha256()
    for v in values:
        absorb(h, torch.as_tensor(v), set())
    print(f"{name} outputs {h.hexdigest()}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--models", nargs="*", help="default: every exporter")
    args = ap.parse_args()
    table = exporters()
    with tempfile.TemporaryDirectory() as root:
        for name in args.models or sorted(table):
            digest(name, *table[name], args.device, root)


if __name__ == "__main__":
    main()
