"""Grouped conv: the HIP kernel (kernels/gconv.hip) against torch's grouped conv on
the same bf16 tensors and against a device-to-device copy of the same bytes,
for every distinct grouped-conv shape of ResNeXt-50 32x4d (224 x 224): four
stride-1 shapes and three stride-2 ones, at each batch size asked for.

Three timings per shape, each the median of single cold launches taken the way
ops.tuned_config takes them (L2 flushed, the GPU kept busy while the host
records the start event and issues the launch):

  * kernel: hip().gconv2d (one form);
  * torch:  F.conv2d(groups=) + bias + ReLU on the bf16 NHWC tensor seen as
            channels-last NCHW, the filter converted once outside the timing:
            the library's grouped conv;
  * copy:   one torch copy_ of (input + output bytes) / 2, which moves the
            bytes the op must move (it reads the input once and writes the
            output once; the copy reads and writes half of their sum each):
            the floor of this op.

Prints one table row per shape and, with --json, one JSON line per shape.

    python scripts/gconv_bench.py [--batch 1 32] [--reps 21] [--json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def resnext50_gconv_shapes(groups=32, width_per_group=4, image_size=224):
    """Distinct (H, W, C, Cg, stride) of the grouped 3x3s, as models/resnet.py lays them out."""
    from rust_tensorflow_serving2_amd.models import resnet
    shapes = {}
    size = image_size // 4                                  # behind the stem conv and the max-pool
    for si, n in enumerate(resnet.BLOCKS_50):
        inner = 64 * 2 ** si * width_per_group // 64 * groups
        for bi in range(n):
            stride = 2 if (bi == 0 and si > 0) else 1
            key = (size, size, inner, inner // groups, stride)
            shapes[key] = shapes.get(key, 0) + 1
            size //= stride
    return shapes


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
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gconv_bench needs a GPU: a timing taken anywhere else says nothing")
    from rust_tensorflow_serving2_amd import ops
    from rust_tensorflow_serving2_amd.graph.fused import pack_grouped_filter
    H = ops.hip()
    dev = torch.device("cuda:0")
    flush = ops._flush_buffer()
    print(f"{'N':>3} {'H x W x C':>14} {'Cg':>3} {'s':>2} {'layers':>6} {'kernel us':>9} {'torch us':>9} {'copy us':>8} "
          f"{'torch/kernel':>12} {'kernel/copy':>11} {'GB/s':>7}")
    for n in args.batch:
        for (h, w, c, cg, s), layers in sorted(resnext50_gconv_shapes().items(), key=lambda kv: (-kv[0][0], kv[0][2])):
            g = torch.Generator().manual_seed(h * 1000 + c)
            x = torch.randn(n, h, w, c, generator=g).to(torch.bfloat16).to(dev)
            wt = torch.randn(3, 3, cg, c, generator=g) * (9 * cg) ** -0.5
            b = torch.randn(c, generator=g).to(dev)
            pads = (1, 1, 1, 1)                            # SAME at stride 1, the exporter's Pad at stride 2
            ho, wo = (h + 2 - 3) // s + 1, (w + 2 - 3) // s + 1
            out = torch.empty(n, ho, wo, c, dtype=torch.bfloat16, device=dev)
            wp = pack_grouped_filter(wt, cg).to(dev)
            kernel = timed(lambda: H.gconv2d(x, wp, b, cg, s, pads[0], pads[2], ho, wo, ops.ACT["relu"], out), flush,
                           args.reps)
            # the library: channels-last NCHW view of the same tensor, OIHW bf16 filter in channels-last too
            xc = x.permute(0, 3, 1, 2)
            wo_ihw = wt.permute(3, 2, 0, 1).to(torch.bfloat16).to(dev).contiguous(memory_format=torch.channels_last)
            bb = b.to(torch.bfloat16)

            def lib():
                return torch.relu_(F.conv2d(xc, wo_ihw, bb, stride=s, padding=1, groups=c // cg))
            y = lib()
            assert y.shape == (n, c, ho, wo), (y.shape, out.shape)
            torch.testing.assert_close(y.permute(0, 2, 3, 1).float(), out.float(), atol=0.1, rtol=0.05)
            lib_us = timed(lib, flush, args.reps)
            nbytes = (x.numel() + out.numel()) * 2           # what the op reads + writes
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            copy = timed(lambda: dst.copy_(src), flush, args.reps)
            row = {"n": n, "h": h, "w": w, "c": c, "cg": cg, "stride": s, "layers": layers,
                   "kernel_us": round(kernel, 2), "torch_us": round(lib_us, 2), "copy_us": round(copy, 2),
                   "bytes": nbytes}
            print(f"{n:>3} {f'{h}x{w}x{c}':>14} {cg:>3} {s:>2} {layers:>6} {kernel:9.1f} {lib_us:9.1f} {copy:8.1f} "
                  f"{lib_us / kernel:12.2f} {kernel / copy:11.2f} {nbytes / kernel / 1e3:7.0f}", flush=True)
            if args.json:
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
