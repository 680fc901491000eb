"""Windowed attention: the HIP kernel (kernels/wattn.hip) against the op's own
torch path on the same tensors, for Swin-T's four stage shapes at 224 x 224
(56 x 56 x 3 heads, 28 x 28 x 6, 14 x 14 x 12, 7 x 7 x 24; window 7, S = 49) at
batch 1 and batch 32, in image order with the shifted grid (shift 3 and the
mask; the 7 x 7 stage is one window: shift 0, no mask).

Three timings per shape, each the median of single cold launches taken the way
ops.tuned_config takes them (L2 flushed, the GPU kept busy while the host
records the start event and issues the launch):

  * kernel: hip().window_attention with grid = (Hf, Wf, 7, shift);
  * torch:  WindowAttentionOp's torch path on the device (TFSERVE_WATTN=0):
            roll, partition, batched matmuls, softmax, reverse, roll;
  * copy:   one torch copy_ of (qkv + output bytes) / 2: the bytes the op must
            move, the floor of this op.

Prints one table row per shape and, with --json, one JSON line per shape.

    python scripts/wattn_bench.py [--batch 1 32] [--reps 21] [--json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dwconv_bench import timed  # noqa: E402

SHAPES = ((56, 3), (28, 6), (14, 12), (7, 24))      # (Hf = Wf, heads) of Swin-T's stages at 224 x 224
WS = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wattn_bench needs a GPU: a timing taken anywhere else says nothing")
    from rust_tensorflow_serving2_amd import ops
    from rust_tensorflow_serving2_amd.graph.patterns import WindowAttentionOp
    from rust_tensorflow_serving2_amd.models.swin import shift_mask
    H = ops.hip()
    dev = torch.device("cuda:0")
    flush = ops._flush_buffer()
    S = WS * WS
    print(f"{'N x H x W x heads':>18} {'wgs':>6} {'kernel us':>9} {'torch us':>9} {'copy us':>8} {'torch/kernel':>12} "
          f"{'kernel/copy':>11} {'GB/s':>7}")
    for n in args.batch:
        for hw, heads in SHAPES:
            shift = WS // 2 if hw > WS else 0
            g = torch.Generator().manual_seed(hw * 100 + heads)
            rows = n * hw * hw
            qkv = torch.randn(rows, 3 * heads * 32, generator=g).to(torch.bfloat16).to(dev)
            bias = torch.randn(heads, S, S, generator=g)
            mask = torch.from_numpy(shift_mask(hw, hw, WS, shift)) if shift else None
            op = WindowAttentionOp(heads, 32, S, 32 ** -0.5, bias, mask, dev, True)
            op.grid = (hw, hw, WS, shift)
            out = torch.empty(rows, heads * 32, dtype=torch.bfloat16, device=dev)
            kernel = timed(lambda: H.window_attention(qkv, op.bias, op.mask, heads, op.scale, out, list(op.grid)),
                           flush, args.reps)
            os.environ["TFSERVE_WATTN"] = "0"
            try:
                y_torch = op(None, None, [qkv])[0]
                torch_us = timed(lambda: op(None, None, [qkv]), flush, args.reps)
            finally:
                del os.environ["TFSERVE_WATTN"]
            err = (out.float() - y_torch.float()).abs().max().item()
            assert err < 0.1, err
            nbytes = (qkv.numel() + out.numel()) * 2
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            copy = timed(lambda: dst.copy_(src), flush, args.reps)
            wgs = n * (hw // WS) ** 2 * heads
            row = {"n": n, "h": hw, "w": hw, "heads": heads, "shift": shift, "workgroups": wgs,
                   "kernel_us": round(kernel, 2), "torch_us": round(torch_us, 2), "copy_us": round(copy, 2),
                   "bytes": nbytes}
            print(f"{f'{n}x{hw}x{hw}x{heads}':>18} {wgs:>6} {kernel:9.1f} {torch_us:9.1f} {copy:8.1f} "
                  f"{torch_us / kernel:12.2f} {kernel / copy:11.2f} {nbytes / kernel / 1e3:7.0f}", flush=True)
            if args.json:
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
