"""Depthwise 7x7 + LayerNorm: the fused HIP kernel (kernels/dwln.hip) against
the pair of launches it replaces, on the same tensors, for ConvNeXt-T's four
block shapes (224 x 224: 56 x 56 x 96, 28 x 28 x 192, 14 x 14 x 384, 7 x 7 x 768)
at batch 1 and batch 32.

Three timings per shape, each the median of single cold launches taken the way
ops.tuned_config takes them (L2 flushed, the GPU kept busy while the host
records the start event and issues the launch):

  * fused: hip().dwconv_ln;
  * pair:  hip().dwconv2d (7x7: the generic kernel) into a bf16 tensor, then
           hip().layernorm on it -- what _FusedDepthwiseConv2D + _LayerNorm run
           (both launches inside one pair of events);
  * copy:  one torch copy_ of (input + output bytes) / 2: the bytes the fused op
           must move, the floor of this op.

Prints one table row per shape and, with --json, one JSON line per shape.

    python scripts/dwln_bench.py [--batch 1 32] [--reps 21] [--json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dwconv_bench import timed  # noqa: E402

SHAPES = ((56, 96), (28, 192), (14, 384), (7, 768))      # (H = W, C) of ConvNeXt-T's stages at 224 x 224
EPS = 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dwln_bench needs a GPU: a timing taken anywhere else says nothing")
    from rust_tensorflow_serving2_amd import ops
    H = ops.hip()
    dev = torch.device("cuda:0")
    flush = ops._flush_buffer()
    print(f"{'N x H x W x C':>18} {'wgs':>5} {'fused us':>9} {'pair us':>8} {'dw us':>7} {'ln us':>7} {'copy us':>8} "
          f"{'pair/fused':>10} {'fused/copy':>10} {'GB/s':>7}")
    for n in args.batch:
        for hw, c in SHAPES:
            g = torch.Generator().manual_seed(hw * 1000 + c)
            x = torch.randn(n, hw, hw, c, generator=g).to(torch.bfloat16).to(dev)
            w = (torch.randn(49, c, generator=g) / 7).to(dev)
            b = torch.randn(c, generator=g).to(dev)
            gamma = (1 + 0.2 * torch.randn(c, generator=g)).to(dev)
            beta = (0.2 * torch.randn(c, generator=g)).to(dev)
            out = torch.empty(n, hw, hw, c, dtype=torch.bfloat16, device=dev)
            mid = torch.empty_like(out)
            out2 = torch.empty_like(out)

            def dw():
                return H.dwconv2d(x, w, b, 7, 7, 1, 1, 3, 3, hw, hw, 0, mid, 0)

            def ln():
                return H.layernorm(mid, None, gamma, beta, EPS, out2)
            fused = timed(lambda: H.dwconv_ln(x, w, b, gamma, beta, EPS, 3, 3, hw, hw, out), flush, args.reps)
            pair = timed(lambda: (dw(), ln()), flush, args.reps)
            t_dw = timed(dw, flush, args.reps)
            t_ln = timed(ln, flush, args.reps)
            y_pair = ln().float()
            err = (out.float() - y_pair).abs().max().item()
            assert err < 0.25, err                          # (the pair rounds in between: close, not equal)
            nbytes = (x.numel() + out.numel()) * 2          # what the fused op reads + writes
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            copy = timed(lambda: dst.copy_(src), flush, args.reps)
            wgs = H.dwconv_ln_grid(n, hw, hw, c)
            row = {"n": n, "h": hw, "w": hw, "c": c, "workgroups": wgs, "fused_us": round(fused, 2),
                   "pair_us": round(pair, 2), "dwconv_us": round(t_dw, 2), "layernorm_us": round(t_ln, 2),
                   "copy_us": round(copy, 2), "bytes": nbytes}
            print(f"{f'{n}x{hw}x{hw}x{c}':>18} {wgs:>5} {fused:9.1f} {pair:8.1f} {t_dw:7.1f} {t_ln:7.1f} {copy:8.1f} "
                  f"{pair / fused:10.2f} {fused / copy:10.2f} {nbytes / fused / 1e3:7.0f}", flush=True)
            if args.json:
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
