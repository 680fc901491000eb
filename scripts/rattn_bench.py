"""Bidirectional RoPE attention with a local window: rope_attention
(kernels/rattn.hip: q and k rotated at load, only the key blocks a query block's
window touches are walked) against what runs without it -- on the same tensors:

(a) "op torch path": what the graph runs for this subgraph before the kernel
    existed, RopeAttentionOp with use_hip = False on the device (fp32, the
    [B, H, S, S] scores materialised, the fill added outside the window);
(b) "torch sdpa": the rotation in fp32 rounded to bf16, then
    torch.nn.functional.scaled_dot_product_attention with the same boolean mask.

Each local row also prints local / global of the kernel next to the block-count
ceiling (S / 64 blocks against 3 at window 64).  (The two design variants that
were measured with this script and taken out again, 128 query rows per workgroup
and a resident key range, had a column each: profiles/modernbert/ keeps the logs.)

Per (B, S, H, window), each timing is the median of single cold runs taken the
way ops.tuned_choice takes them (dwconv_bench.timed), and the whole measurement
is repeated ``--rounds`` times, alternating the candidates: the table shows the
median of the rounds' medians and their spread (max - min over the rounds, as a
share of the median), which is what a ratio has to beat.

    python scripts/rattn_bench.py [--shapes B,S,H,W ...] [--reps 21] [--rounds 5] [--json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dwconv_bench import timed  # noqa: E402
from gqattn_bench import parse, rotated  # noqa: E402

SHAPES = [(b, s, 12, w) for s in (512, 1024, 2048, 4096) for b in (1, 8) for w in (-1, 64)]
NAMES = ["rope_attention", "op torch path", "torch sdpa"]


def sdpa(qkv, cos, sin, h, scale, mask, out):
    b, s, _ = qkv.shape
    q, k, v = qkv.split([h * 64] * 3, -1)
    q, k = rotated(q, h, 64, cos, sin).transpose(1, 2), rotated(k, h, 64, cos, sin).transpose(1, 2)
    y = torch.nn.functional.scaled_dot_product_attention(q, k, v.reshape(b, s, h, 64).transpose(1, 2), attn_mask=mask,
                                                         scale=scale)
    out.copy_(y.transpose(1, 2).reshape(b, s, h * 64))


def candidates(H, qkv, cos, sin, h, w, out):
    from rust_tensorflow_serving2_amd.graph.patterns import RopeAttentionOp
    b, s, _ = qkv.shape
    scale = 0.125
    op = RopeAttentionOp(h, 64, s, scale, w, -10000.0, cos, sin, qkv.device, False)
    flat = qkv.reshape(b * s, -1)
    pos = torch.arange(s, device=qkv.device)
    mask = None if w < 0 else (pos[:, None] - pos[None, :]).abs() <= w
    return {"rope_attention": lambda: H.rope_attention(qkv, cos, sin, None, h, scale, w, out["rope_attention"]),
            "op torch path": lambda: out["op torch path"].copy_(op(None, None, [flat])[0].reshape(b, s, h * 64)),
            "torch sdpa": lambda: sdpa(qkv, cos, sin, h, scale, mask, out["torch sdpa"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", type=parse, default=None, metavar="B,S,H,W")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rattn_bench needs a GPU: a timing taken anywhere else says nothing")
    from rust_tensorflow_serving2_amd import ops
    from rust_tensorflow_serving2_amd.models import llama
    H = ops.hip()
    dev = torch.device("cuda:0")
    flush = ops._flush_buffer()
    kernel_us = {}
    for b, s, h, w in args.shapes or SHAPES:
        g = torch.Generator().manual_seed(s * 100 + b)
        qkv = torch.randn(b, s, 3 * h * 64, generator=g).to(torch.bfloat16).to(dev)
        cos, sin = (torch.from_numpy(t[0, 0, :, :32].copy()).to(dev) for t in llama.rope_tables(s))
        out = {n: torch.empty(b, s, h * 64, dtype=torch.bfloat16, device=dev) for n in NAMES}
        runs = candidates(H, qkv, cos, sin, h, w, out)
        rounds = {n: [] for n in runs}
        for _ in range(args.rounds):
            for n, fn in runs.items():                       # alternating: every round times every candidate once
                rounds[n].append(timed(fn, flush, args.reps))
        err = (out["rope_attention"].float() - out["op torch path"].float()).abs().max().item()
        assert err < 0.05, err
        med = {n: statistics.median(v) for n, v in rounds.items()}
        spread = {n: (max(v) - min(v)) / med[n] for n, v in rounds.items()}
        kernel_us[(b, s, h, w)] = med["rope_attention"]
        cells = " ".join(f"{n} {med[n]:.1f} us (spread {spread[n]:.1%})" for n in NAMES)
        ratios = " ".join(f"{n} / rope_attention {med[n] / med['rope_attention']:.2f}" for n in NAMES[1:])
        line = f"{f'{b}x{s}x{h} w={w}':>18}  {cells}  {ratios}"
        if w >= 0 and (b, s, h, -1) in kernel_us:
            line += f"  global / local {kernel_us[(b, s, h, -1)] / med['rope_attention']:.2f} (blocks {s // 64} : 3)"
        print(line, flush=True)
        if args.json:
            print(json.dumps({"b": b, "s": s, "h": h, "window": w, "rounds": args.rounds,
                              "us": {n: [round(x, 2) for x in v] for n, v in rounds.items()}}), flush=True)


if __name__ == "__main__":
    main()
