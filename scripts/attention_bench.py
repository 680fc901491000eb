"""Attention at ViT lengths: form 1 (attention_ragged_kernel, the register
kernel padded to 32 keys by its descriptors) against form 0 (at these lengths
attention_flash_kernel, the KV-block loop) on the same tensors.

Per (B, S, H) and mask layout, each timing is the median of single cold
launches taken the way ops.tuned_choice takes them (L2 flushed, the GPU kept
busy while the host records the start event and issues the launch).  The
default shapes are ViT's S = 50 (224 / 32), 65 (128 / 16), 197 (224 / 16) at
B * H = 12 and 384, and S = 100 with BERT's [B, 1, 1, S] key adder.

    python scripts/attention_bench.py [--shapes B,S,H[,key] ...] [--reps 21] [--json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dwconv_bench import timed  # noqa: E402

SHAPES = [(b, s, 12, "none") for s in (50, 65, 197) for b in (1, 32)] + [(1, 100, 12, "key"), (32, 100, 12, "key")]


def parse(text):
    f = text.split(",")
    return int(f[0]), int(f[1]), int(f[2]), (f[3] if len(f) > 3 else "none")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", type=parse, default=SHAPES, metavar="B,S,H[,key]")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_bench needs a GPU: a timing taken anywhere else says nothing")
    from rust_tensorflow_serving2_amd import ops
    H = ops.hip()
    dev = torch.device("cuda:0")
    flush = ops._flush_buffer()
    print(f"{'B x S x H':>14} {'mask':>5} {'keys run':>8} {'form 0 us':>10} {'form 1 us':>10} {'form 0 / form 1':>15}")
    for b, s, h, mask in args.shapes:
        g = torch.Generator().manual_seed(s * 100 + b)
        qkv = torch.randn(b, s, 3 * h * 64, generator=g).to(torch.bfloat16).to(dev)
        m, bstride = None, 0
        if mask == "key":
            m = torch.zeros(b, s)
            m[:, s - s // 4:] = -10000.0
            m, bstride = m.to(dev), s
        out = [torch.empty(b, s, h * 64, dtype=torch.bfloat16, device=dev) for _ in range(2)]
        forms = H.attention_forms(s)
        t = {}
        for form in forms:
            t[form] = timed(lambda: H.attention(qkv, m, h, 0.125, out[form], bstride, 0, form), flush, args.reps)
        sp = max(64, (s + 31) // 32 * 32)
        if 1 in t:
            # the two algorithms round differently: close, not equal
            err = (out[0].float() - out[1].float()).abs().max().item()
            assert err < 0.05, err
        f1 = f"{t[1]:10.1f}" if 1 in t else f"{'-':>10}"
        ratio = f"{t[0] / t[1]:15.2f}" if 1 in t else f"{'-':>15}"
        print(f"{f'{b}x{s}x{h}':>14} {mask:>5} {sp:>8} {t[0]:10.1f} {f1} {ratio}", flush=True)
        if args.json:
            print(json.dumps({"b": b, "s": s, "h": h, "mask": mask, "padded": sp,
                              "form0_us": round(t[0], 2), "form1_us": round(t[1], 2) if 1 in t else None}), flush=True)


if __name__ == "__main__":
    main()
