"""Squeeze-and-excite: the two HIP launches (kernels/se.hip) against the op
sequence they replace and against a device-to-device copy of the same bytes,
for every distinct squeeze-excite shape of MobileNetV3-Large (224 x 224).

Timings per shape and batch size, each the median of single cold launches taken
the way ops.tuned_config takes them (L2 flushed, the GPU kept busy while the
host records the start event and issues the launch):

  * gate:    hip().se_gate (pooling + both FCs, one workgroup per image);
  * gate1:   se_gate on one pixel per image (same C and Cr): the FCs alone, so
             gate - gate1 is what the pooling costs;
  * scale:   hip().se_scale;
  * parent:  what the block ran as before the fused op: global_avgpool, two
             _FusedConv2D launches with M = batch rows (tile picks tuned first),
             then Add, Relu6, Mul and the broadcast Mul as torch launches on
             the bf16 tensors;
  * copy:    one torch copy_ of the bytes se_scale moves (it reads x once and
             writes y once): the floor of se_scale.

    python scripts/se_bench.py [--batch 1 32] [--reps 21] [--json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dwconv_bench import timed  # noqa: E402


def v3_large_se_shapes():
    """Distinct (H, W, C, Cr) of the squeeze-excite blocks, in network order."""
    from rust_tensorflow_serving2_amd.models import mobilenet
    shapes, size = {}, 112
    for i, (_k, exp, _out, se, _act, stride) in enumerate(mobilenet.V3_LARGE, 1):
        size = -(-size // stride)
        if se:
            shapes.setdefault((size, size, exp, mobilenet._make_divisible(exp / 4)), []).append(i)
    return shapes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("se_bench needs a GPU: a timing taken anywhere else says nothing")
    from rust_tensorflow_serving2_amd import ops
    from rust_tensorflow_serving2_amd.graph.fused import FusedConv
    H = ops.hip()
    dev = torch.device("cuda:0")
    flush = ops._flush_buffer()
    relu, hsig = ops.ACT["relu"], ops.ACT["hard_sigmoid"]
    print(f"{'batch':>5} {'H x W x C / Cr':>20} {'blocks':>8} {'gate us':>8} {'gate1 us':>8} {'scale us':>8} {'copy us':>8} "
          f"{'parent us':>9} {'parent/new':>10} {'scale/copy':>10}")
    for n in args.batch:
        for (h, w, c, cr), blocks in v3_large_se_shapes().items():
            g = torch.Generator().manual_seed(h * 1000 + c)
            x = torch.randn(n, h, w, c, generator=g).to(torch.bfloat16).to(dev)
            w1 = torch.randn(c, cr, generator=g) * (2.0 / c) ** 0.5
            w2 = torch.randn(cr, c, generator=g) * (2.0 / cr) ** 0.5
            b1, b2 = torch.randn(cr, generator=g) * 0.1, torch.randn(c, generator=g) * 0.1
            dw1, db1, dw2, db2 = (t.to(dev) for t in (w1, b1, w2, b2))
            gate_out = torch.empty(n, c, device=dev)
            y = torch.empty_like(x)
            x1 = x[:, :1, :1, :].contiguous()
            gate = timed(lambda: H.se_gate(x, dw1, db1, dw2, db2, relu, hsig, gate_out), flush, args.reps)
            gate1 = timed(lambda: H.se_gate(x1, dw1, db1, dw2, db2, relu, hsig, gate_out), flush, args.reps)
            scale = timed(lambda: H.se_scale(x, gate_out, y), flush, args.reps)
            conv1 = FusedConv(w1.reshape(1, 1, c, cr), b1, (1, 1), "SAME", (0, 0, 0, 0), "relu", dev, True, "fc1")
            conv2 = FusedConv(w2.reshape(1, 1, cr, c), b2, (1, 1), "SAME", (0, 0, 0, 0), "none", dev, True, "fc2")

            def parent():
                p = H.global_avgpool(x).reshape(n, 1, 1, c)
                t = conv2(None, None, [conv1(None, None, [p])[0]])[0]
                t = torch.clamp(t + 3.0, 0.0, 6.0) * (1.0 / 6.0)
                return x * t
            parent()                                     # tunes the two convs' tile picks
            par = timed(parent, flush, args.reps)
            src = torch.empty(x.numel() * 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            copy = timed(lambda: dst.copy_(src), flush, args.reps)
            row = {"n": n, "h": h, "w": w, "c": c, "cr": cr, "blocks": blocks, "gate_us": round(gate, 2),
                   "gate_one_pixel_us": round(gate1, 2), "scale_us": round(scale, 2), "copy_us": round(copy, 2),
                   "parent_us": round(par, 2), "bytes": x.numel() * 4}
            print(f"{n:>5} {f'{h}x{w}x{c} / {cr}':>20} {','.join(map(str, blocks)):>8} {gate:8.1f} {gate1:8.1f} {scale:8.1f} "
                  f"{copy:8.1f} {par:9.1f} {par / (gate + scale):10.2f} {scale / copy:10.2f}", flush=True)
            if args.json:
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
