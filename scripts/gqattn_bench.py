"""RoPE + grouped-query causal attention: rope_gqa_attention (kernels/gqattn.hip: q
and k rotated at load, each K / V block staged once for the G query heads of its
group) against the best composition without it: torch rotates q and k, repeats
K / V for their groups and packs a [B, S, 3 * H * 64] buffer (``compose``), then
causal_attention (kernels/cattn.hip) runs over it -- on the same tensors.

Per (B, S, H, Hkv), each timing is the median of single cold runs taken the way
ops.tuned_choice takes them (dwconv_bench.timed: L2 flushed, the GPU kept busy
while the host records the start event and issues the work), and the whole
measurement is repeated ``--rounds`` times, alternating the candidates: the table
shows the median of the rounds' medians and their spread (max - min over the
rounds, as a share of the median), which is what a ratio has to beat.  The
composition is timed whole and its attention launch alone ("cattn only": what the
composition would cost if the rotation and the repeat were free).

    python scripts/gqattn_bench.py [--shapes B,S,H,Hkv ...] [--reps 21] [--rounds 5] [--json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dwconv_bench import timed  # noqa: E402

SHAPES = [(b, s, 32, k) for k in (8, 4) for s in (128, 512, 1024, 2048) for b in (1, 8)]


def parse(text):
    return tuple(int(v) for v in text.split(","))


def compose(qkv, cos, sin, h, k):
    """[B, S, (H + 2 Hkv) 64] -> [B, S, 3 H 64]: q and k rotated in fp32 and rounded once, K / V repeated per group."""
    b, s, _ = qkv.shape
    q, kk, v = qkv.split([h * 64, k * 64, k * 64], -1)

    def rot(t, n):
        t = t.reshape(b, s, n, 64).float()
        t1, t2 = t[..., :32], t[..., 32:]
        c, sn = cos[None, :, None, :], sin[None, :, None, :]
        return torch.cat([t1 * c - t2 * sn, t2 * c + t1 * sn], -1).to(torch.bfloat16)
    kr = rot(kk, k).repeat_interleave(h // k, 2)
    vr = v.reshape(b, s, k, 64).repeat_interleave(h // k, 2)
    return torch.cat([rot(q, h), kr, vr], 2).reshape(b, s, 3 * h * 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", type=parse, default=SHAPES, metavar="B,S,H,Hkv")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gqattn_bench needs a GPU: a timing taken anywhere else says nothing")
    from rust_tensorflow_serving2_amd import ops
    from rust_tensorflow_serving2_amd.models import llama
    H = ops.hip()
    dev = torch.device("cuda:0")
    flush = ops._flush_buffer()
    names = ["rope_gqa", "composition", "cattn only"]
    print(f"{'B x S x H/Hkv':>16} " + " ".join(f"{n + ' us':>15} {'spread':>6}" for n in names) +
          f" {'composition / rope_gqa':>23}")
    for b, s, h, k in args.shapes:
        g = torch.Generator().manual_seed(s * 100 + b)
        qkv = torch.randn(b, s, (h + 2 * k) * 64, generator=g).to(torch.bfloat16).to(dev)
        cos, sin = (torch.from_numpy(t[0, 0, :, :32].copy()).to(dev) for t in llama.rope_tables(s))
        out = {n: torch.empty(b, s, h * 64, dtype=torch.bfloat16, device=dev) for n in names}
        packed = compose(qkv, cos, sin, h, k)
        runs = {"rope_gqa": lambda: H.rope_gqa_attention(qkv, cos, sin, None, h, k, 0.125, out["rope_gqa"]),
                "composition": lambda: H.causal_attention(compose(qkv, cos, sin, h, k), None, h, 0.125,
                                                          out["composition"]),
                "cattn only": lambda: H.causal_attention(packed, None, h, 0.125, out["cattn only"])}
        rounds = {n: [] for n in runs}
        for _ in range(args.rounds):
            for n, fn in runs.items():                       # alternating: every round times every candidate once
                rounds[n].append(timed(fn, flush, args.reps))
        # the same roundings in the same order: the two paths agree to the last bit or nearly
        err = (out["rope_gqa"].float() - out["composition"].float()).abs().max().item()
        assert err < 0.05, err
        med = {n: statistics.median(v) for n, v in rounds.items()}
        spread = {n: (max(v) - min(v)) / med[n] for n, v in rounds.items()}
        cells = " ".join(f"{med[n]:15.1f} {spread[n]:6.1%}" for n in names)
        print(f"{f'{b}x{s}x{h}/{k}':>16} {cells} {med['composition'] / med['rope_gqa']:23.2f}", flush=True)
        if args.json:
            print(json.dumps({"b": b, "s": s, "h": h, "hkv": k, "rounds": args.rounds,
                              "us": {n: [round(x, 2) for x in v] for n, v in rounds.items()}}), flush=True)


if __name__ == "__main__":
    main()
