"""Attention with a relative-position bias: bias_attention (kernels/battn.hip: the
bias read as a [H, 2 S - 1] table, 127 entries per block pair) against what runs
without it -- on the same tensors:

(a) "op torch path": what the graph runs for this subgraph before the kernel
    existed, AttentionOp's torch path on the device with the [B, H, S, S] adder
    (position bias + padding adder, materialised once per forward as the graph
    does; fp32 scores, softmax and context);
(b) "torch sdpa": torch.nn.functional.scaled_dot_product_attention in bf16 with
    that adder as attn_mask;
(c) "attention": this repository's ``attention`` at the same shape with the key
    adder and NO bias -- not an alternative, the bias's cost.

Per (B, S, H), each timing is the median of single cold runs taken the way
ops.tuned_choice takes them (dwconv_bench.timed), and the whole measurement is
repeated ``--rounds`` times, alternating the candidates: the table shows the
median of the rounds' medians and their spread (max - min over the rounds, as a
share of the median), which is what a ratio has to beat.

    python scripts/battn_bench.py [--shapes B,S,H ...] [--reps 21] [--rounds 5] [--json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dwconv_bench import timed  # noqa: E402
from gqattn_bench import parse  # noqa: E402

SHAPES = [(b, s, 12) for s in (128, 512, 2048) for b in (1, 8, 32)]
NAMES = ["bias_attention", "op torch path", "torch sdpa", "attention"]


def sdpa(qkv, h, scale, mask, out):
    b, s, _ = qkv.shape
    q, k, v = (t.reshape(b, s, h, 64).transpose(1, 2) for t in qkv.split([h * 64] * 3, -1))
    y = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=scale)
    out.copy_(y.transpose(1, 2).reshape(b, s, h * 64))


def candidates(H, qkv, table, key_adder, h, out):
    from rust_tensorflow_serving2_amd.graph.patterns import AttentionOp, BiasAttentionOp
    b, s, _ = qkv.shape
    scale = 1.0                                                  # T5 does not scale its scores
    dense = BiasAttentionOp(h, 64, s, scale, table, qkv.device, False).dense_bias(qkv.device)
    adder = (dense + key_adder[:, None, None, :]).contiguous()   # [B, H, S, S] f32: the graph's shared sum
    adder16 = adder.to(torch.bfloat16)
    op = AttentionOp(h, 64, s, scale, False)
    flat = qkv.reshape(b * s, -1)
    ka4 = key_adder.reshape(b, 1, 1, s).contiguous()
    return {"bias_attention": lambda: H.bias_attention(qkv, table, key_adder, h, scale, out["bias_attention"]),
            "op torch path": lambda: out["op torch path"].copy_(op(None, None, [flat, adder])[0].reshape(b, s, h * 64)),
            "torch sdpa": lambda: sdpa(qkv, h, scale, adder16, out["torch sdpa"]),
            "attention": lambda: H.attention(qkv, ka4, h, scale, out["attention"], s, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", type=parse, default=None, metavar="B,S,H")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("battn_bench needs a GPU: a timing taken anywhere else says nothing")
    from rust_tensorflow_serving2_amd import ops
    H = ops.hip()
    dev = torch.device("cuda:0")
    flush = ops._flush_buffer()
    for b, s, h in args.shapes or SHAPES:
        g = torch.Generator().manual_seed(s * 100 + b)
        # q and k at a quarter of unit variance: unscaled scores of standard deviation 2 (models/t5.py)
        qkv = torch.randn(b, s, 3 * h * 64, generator=g)
        qkv[..., :2 * h * 64] *= 0.5
        qkv = qkv.to(torch.bfloat16).to(dev)
        table = torch.randn(h, 2 * s - 1, generator=g).to(dev)
        key_adder = torch.zeros(b, s)
        key_adder[:, s - s // 8:] = -10000.0
        key_adder = key_adder.to(dev)
        out = {n: torch.empty(b, s, h * 64, dtype=torch.bfloat16, device=dev) for n in NAMES}
        runs = candidates(H, qkv, table, key_adder, h, out)
        rounds = {n: [] for n in runs}
        for _ in range(args.rounds):
            for n, fn in runs.items():                       # alternating: every round times every candidate once
                rounds[n].append(timed(fn, flush, args.reps))
        err = (out["bias_attention"].float() - out["op torch path"].float()).abs().max().item()
        assert err < 0.05, err
        med = {n: statistics.median(v) for n, v in rounds.items()}
        spread = {n: (max(v) - min(v)) / med[n] for n, v in rounds.items()}
        cells = " ".join(f"{n} {med[n]:.1f} us (spread {spread[n]:.1%})" for n in NAMES)
        ratios = " ".join(f"{n} / bias_attention {med[n] / med['bias_attention']:.2f}" for n in NAMES[1:])
        print(f"{f'{b}x{s}x{h}':>12}  {cells}  {ratios}", flush=True)
        if args.json:
            print(json.dumps({"b": b, "s": s, "h": h, "rounds": args.rounds,
                              "us": {n: [round(x, 2) for x in v] for n, v in rounds.items()}}), flush=True)
        del runs, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
