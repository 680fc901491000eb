"""Depthwise conv: the HIP kernel (kernels/dwconv.hip) against the PyTorch path
it replaces and against a device-to-device copy of the same bytes, for every
distinct depthwise shape of MobileNet V1 and V2 (224 x 224) at one batch size.

Three timings per shape, each the median of single cold launches taken the way
ops.tuned_config takes them (L2 flushed, the GPU kept busy while the host
records the start event and issues the launch):

  * new:    hip().dwconv2d, both strip heights of the 3x3 kernels (the engine
            picks per shape with ops.tuned_choice) -- the faster one is "new";
  * parent: graph/ops.py _dwconv on the same bf16 NHWC tensor (permute -> pad ->
            F.conv2d(groups=C) -> permute -> contiguous), what a
            DepthwiseConv2dNative node ran before the fused op existed;
  * copy:   one torch copy_ of (input + output bytes) / 2, which moves the
            bytes the op must move (it reads the input once and writes the
            output once; the copy reads and writes half of their sum each):
            the floor of this op.

Prints one table row per shape and, with --json, one JSON line per shape.

``--k5`` times, instead, the distinct 5x5 depthwise shapes of EfficientNet-B0 and
MobileNetV3-Large (224 x 224) with a swish epilogue: the generic kernel, the 5x5
strip kernel at both heights (2 and 4 output rows per thread) and the copy floor.

    python scripts/dwconv_bench.py [--batch 32] [--reps 21] [--json] [--k5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def mobilenet_dw_shapes():
    """Distinct (H, W, C, stride, padding) of the depthwise layers, padding as
    the exporters write it: V1 SAME; V2 SAME at stride 1, Pad + VALID at stride 2."""
    from rust_tensorflow_serving2_amd.models import mobilenet
    shapes = {}
    size, c = 112, 32
    for filters, stride in mobilenet.V1_BLOCKS:
        shapes.setdefault((size, size, c, stride, "SAME"), []).append("v1")
        size, c = -(-size // stride), filters
    size, c = 112, 32
    for t, ch, reps, first in mobilenet.V2_BLOCKS:
        for r in range(reps):
            stride = first if r == 0 else 1
            shapes.setdefault((size, size, c * t, stride, "SAME" if stride == 1 else "PAD_VALID"), []).append("v2")
            size, c = -(-size // stride), ch
    return shapes


def k5_dw_shapes():
    """Distinct (H, W, C, stride, padding) of the 5x5 depthwise layers of
    EfficientNet-B0 and MobileNetV3-Large, padding as the exporters write it."""
    from rust_tensorflow_serving2_amd.models import efficientnet, mobilenet
    shapes = {}
    size = 112
    for k, repeats, fin, fout, ratio, first in efficientnet.BLOCKS:
        for r in range(repeats):
            stride, cin = (first, fin) if r == 0 else (1, fout)
            if k == 5:
                shapes.setdefault((size, size, cin * ratio, stride, "SAME" if stride == 1 else "PAD_VALID"), []).append("b0")
            size = -(-size // stride)
    size = 112
    for k, exp, _out, _se, _act, stride in mobilenet.V3_LARGE:
        if k == 5:
            shapes.setdefault((size, size, exp, stride, "SAME" if stride == 1 else "PAD_VALID"), []).append("v3l")
        size = -(-size // stride)
    return shapes


def bench_k5(args, H, ops, O, dev, flush):
    n = args.batch
    print(f"{'H x W x C':>16} {'s':>2} {'pad':>9} {'models':>6} {'generic us':>10} {'strip2 us':>9} {'strip4 us':>9} "
          f"{'copy us':>8} {'generic/best':>12} {'best/copy':>9}")
    for (h, w, c, s, padding), users in sorted(k5_dw_shapes().items(), key=lambda kv: (-kv[0][0], kv[0][2])):
        g = torch.Generator().manual_seed(h * 1000 + c)
        x = torch.randn(n, h, w, c, generator=g).to(torch.bfloat16).to(dev)
        w25 = (torch.randn(25, c, generator=g) / 5).to(dev)
        b = torch.randn(c, generator=g).to(dev)
        if padding == "SAME":
            pads = O.tf_same_pads(h, 5, s) + O.tf_same_pads(w, 5, s)
        else:                                           # Keras correct_pad in front of a VALID conv
            pads = (2 - (1 - h % 2), 2, 2 - (1 - w % 2), 2)
        ho, wo = (h + pads[0] + pads[1] - 5) // s + 1, (w + pads[2] + pads[3] - 5) // s + 1
        out = torch.empty(n, ho, wo, c, dtype=torch.bfloat16, device=dev)
        forms = H.dwconv_forms(n, ho, wo, c, 5, 5, s, s)
        assert forms == [0, 2, 4], forms
        outs = {}
        t = {}
        for strip in forms:
            t[strip] = timed(lambda strip=strip: H.dwconv2d(x, w25, b, 5, 5, s, s, pads[0], pads[2], ho, wo,
                                                            ops.ACT["swish"], out, strip), flush, args.reps)
            outs[strip] = out.clone()
        assert all(torch.equal(outs[0].view(torch.int16), outs[f].view(torch.int16)) for f in forms)   # bit-equal forms
        nbytes = (x.numel() + out.numel()) * 2           # what the op reads + writes
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy = timed(lambda: dst.copy_(src), flush, args.reps)
        best = min(t, key=t.get)
        row = {"n": n, "h": h, "w": w, "c": c, "k": 5, "stride": s, "padding": padding,
               "models": "+".join(sorted(set(users))), "generic_us": round(t[0], 2), "strip2_us": round(t[2], 2),
               "strip4_us": round(t[4], 2), "best": best, "copy_us": round(copy, 2), "bytes": nbytes}
        print(f"{f'{h}x{w}x{c}':>16} {s:>2} {padding:>9} {row['models']:>6} {t[0]:10.1f} {t[2]:9.1f} {t[4]:9.1f} "
              f"{copy:8.1f} {t[0] / t[best]:12.2f} {t[best] / copy:9.2f}", flush=True)
        if args.json:
            print(json.dumps(row), flush=True)


def timed(fn, flush, reps):
    from rust_tensorflow_serving2_amd import ops
    fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(reps):
        flush.zero_()
        torch.cuda._sleep(ops._HOST_SHADOW_CYCLES)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        samples.append(start.elapsed_time(end) * 1e3)
    samples.sort()
    return samples[len(samples) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--k5", action="store_true", help="the 5x5 shapes of EfficientNet-B0 and MobileNetV3-Large: generic "
                                                      "kernel vs both strip heights vs the copy floor")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dwconv_bench needs a GPU: a timing taken anywhere else says nothing")
    from rust_tensorflow_serving2_amd import ops
    from rust_tensorflow_serving2_amd.graph import ops as O
    from rust_tensorflow_serving2_amd.graph.ir import Node
    H = ops.hip()
    dev = torch.device("cuda:0")
    flush = ops._flush_buffer()
    if args.k5:
        return bench_k5(args, H, ops, O, dev, flush)
    n = args.batch
    print(f"{'H x W x C':>16} {'s':>2} {'pad':>9} {'models':>6} {'new us':>8} {'strip':>5} {'parent us':>10} "
          f"{'copy us':>8} {'parent/new':>10} {'new/copy':>8} {'GB/s':>7}")
    for (h, w, c, s, padding), users in sorted(mobilenet_dw_shapes().items(), key=lambda kv: (-kv[0][0], kv[0][2])):
        g = torch.Generator().manual_seed(h * 1000 + c)
        x = torch.randn(n, h, w, c, generator=g).to(torch.bfloat16).to(dev)
        wt = (torch.randn(3, 3, c, generator=g) / 3).to(dev)
        b = torch.randn(c, generator=g).to(dev)
        if padding == "SAME":
            pads = O.tf_same_pads(h, 3, s) + O.tf_same_pads(w, 3, s)
        else:                                           # Keras correct_pad in front of a VALID conv
            pads = (1 - (1 - h % 2), 1, 1 - (1 - w % 2), 1)
        ho, wo = (h + pads[0] + pads[1] - 3) // s + 1, (w + pads[2] + pads[3] - 3) // s + 1
        out = torch.empty(n, ho, wo, c, dtype=torch.bfloat16, device=dev)
        w9 = wt.reshape(9, c).contiguous()
        new = {strip: timed(lambda strip=strip: H.dwconv2d(x, w9, b, 3, 3, s, s, pads[0], pads[2], ho, wo,
                                                           ops.ACT["relu6"], out, strip), flush, args.reps)
               for strip in (2, 8)}
        strip = min(new, key=new.get)
        # the parent's op: an EXPLICIT-padding DepthwiseConv2dNative node on the bf16 NHWC tensor, then the
        # separate Relu6 launch (the BatchNorm between them is left out: in the parent's favour)
        node = Node(name="dw", op="DepthwiseConv2dNative", inputs=[],
                    attrs={"strides": [1, s, s, 1], "padding": b"EXPLICIT", "data_format": b"NHWC",
                           "explicit_paddings": [0, 0, pads[0], pads[1], pads[2], pads[3], 0, 0]})
        w4 = wt.reshape(3, 3, c, 1).to(torch.bfloat16)
        y_parent = O.OPS["DepthwiseConv2dNative"](None, node, [x, w4])[0]
        assert y_parent.shape == out.shape, (y_parent.shape, out.shape)
        parent = timed(lambda: torch.clamp(O.OPS["DepthwiseConv2dNative"](None, node, [x, w4])[0], 0, 6), flush,
                       args.reps)
        nbytes = (x.numel() + out.numel()) * 2           # what the op reads + writes
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy = timed(lambda: dst.copy_(src), flush, args.reps)
        row = {"n": n, "h": h, "w": w, "c": c, "stride": s, "padding": padding, "models": "+".join(sorted(set(users))),
               "new_us": round(new[strip], 2), "strip": strip, "new_us_by_strip": {k: round(v, 2) for k, v in new.items()},
               "parent_us": round(parent, 2), "copy_us": round(copy, 2), "bytes": nbytes}
        print(f"{f'{h}x{w}x{c}':>16} {s:>2} {padding:>9} {row['models']:>6} {new[strip]:8.1f} {strip:>5} {parent:10.1f} "
              f"{copy:8.1f} {parent / new[strip]:10.2f} {new[strip] / copy:8.2f} {nbytes / new[strip] / 1e3:7.0f}",
              flush=True)
        if args.json:
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
