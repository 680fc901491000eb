"""Causal attention: causal_attention (kernels/cattn.hip, the mask from indices,
key blocks above the diagonal skipped) against the only way to compute the same
thing without it: attention(form 0) given a materialised [1, 1, S, S] -inf
upper-triangular adder (mask_qstride = S), on the same tensors.

Per (B, S, H), each timing is the median of single cold launches taken the way
ops.tuned_choice takes them (dwconv_bench.timed: L2 flushed, the GPU kept busy
while the host records the start event and issues the launch), and the whole
measurement is repeated ``--rounds`` times, alternating the two kernels: the
table shows the median of the rounds' medians and their spread (max - min over
the rounds, as a share of the median), which is what a ratio has to beat.  Both
query-block heights of the new kernel are timed (qb 64, qb 128) besides the
launcher's own choice.  At S = 128 and 256 form 0 is the register kernel; a
ragged S <= 256 also times form 1 (the register kernel padded to 32 keys).

    python scripts/cattn_bench.py [--shapes B,S,H ...] [--reps 21] [--rounds 5] [--json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dwconv_bench import timed  # noqa: E402

SHAPES = [(b, s, 12) for s in (128, 256, 512, 1024, 2048) for b in (1, 32)]


def parse(text):
    f = text.split(",")
    return int(f[0]), int(f[1]), int(f[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", type=parse, default=SHAPES, metavar="B,S,H")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cattn_bench needs a GPU: a timing taken anywhere else says nothing")
    from rust_tensorflow_serving2_amd import ops
    H = ops.hip()
    dev = torch.device("cuda:0")
    flush = ops._flush_buffer()
    names = ["masked form 0", "masked form 1", "causal", "causal qb64", "causal qb128"]
    print(f"{'B x S x H':>14} " + " ".join(f"{n + ' us':>16} {'spread':>6}" for n in names) + f" {'form 0 / causal':>15}")
    for b, s, h in args.shapes:
        g = torch.Generator().manual_seed(s * 100 + b)
        qkv = torch.randn(b, s, 3 * h * 64, generator=g).to(torch.bfloat16).to(dev)
        mask = torch.triu(torch.full((s, s), float("-inf")), 1).reshape(1, 1, s, s).to(dev)
        out = {n: torch.empty(b, s, h * 64, dtype=torch.bfloat16, device=dev) for n in names}
        runs = {"masked form 0": lambda: H.attention(qkv, mask, h, 0.125, out["masked form 0"], 0, s, 0),
                "causal": lambda: H.causal_attention(qkv, None, h, 0.125, out["causal"]),
                "causal qb64": lambda: H.causal_attention(qkv, None, h, 0.125, out["causal qb64"], 64),
                "causal qb128": lambda: H.causal_attention(qkv, None, h, 0.125, out["causal qb128"], 128)}
        # the register kernel: form 1 at ragged lengths, form 0 itself at S in {64, 128, 192, 256}
        if 1 in H.attention_forms(s):
            runs["masked form 1"] = lambda: H.attention(qkv, mask, h, 0.125, out["masked form 1"], 0, s, 1)
        rounds = {n: [] for n in runs}
        for _ in range(args.rounds):
            for n, fn in runs.items():                       # alternating: every round times every kernel once
                rounds[n].append(timed(fn, flush, args.reps))
        # the two algorithms round differently: close, not equal
        err = (out["masked form 0"].float() - out["causal"].float()).abs().max().item()
        assert err < 0.05, err
        med = {n: statistics.median(v) for n, v in rounds.items()}
        spread = {n: (max(v) - min(v)) / med[n] for n, v in rounds.items()}
        cells = " ".join(f"{med[n]:16.1f} {spread[n]:6.1%}" if n in med else f"{'-':>16} {'-':>6}" for n in names)
        print(f"{f'{b}x{s}x{h}':>14} {cells} {med['masked form 0'] / med['causal']:15.2f}", flush=True)
        if args.json:
            print(json.dumps({"b": b, "s": s, "h": h, "rounds": args.rounds,
                              "us": {n: [round(x, 2) for x in v] for n, v in rounds.items()}}), flush=True)


if __name__ == "__main__":
    main()
