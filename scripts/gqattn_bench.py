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

A shape with a fifth field D = 128 runs kernels/gqattn128.hip.  causal_attention
has no 128-wide form, so there the baselines are (a) "op torch path": what the
graph op ran before the kernel existed, RopeGQAttentionOp with use_hip = False on
the device (fp32, K / V repeated, [B, H, S, S] scores materialised), and (b)
"torch sdpa": the rotation in fp32 rounded to bf16, then
torch.nn.functional.scaled_dot_product_attention(is_causal=True) over K / V
repeated for their groups.  ``--d128`` runs the D = 128 shape list.  ``--qk-norm``
(D = 128 shapes) gives the kernel a QK-norm and times it against the op's torch
path, the norm-less kernel and two rmsnorm launches plus the norm-less kernel.

A shape with D = 256 and a sixth field, the window, runs kernels/gqattn256.hip
(rope_gqa_attention256) with a QK-norm against the same two baselines; sdpa takes
no norm and gets a window as a boolean mask.  ``--d256`` runs Gemma's shape list.

    python scripts/gqattn_bench.py [--shapes B,S,H,Hkv[,D[,window]] ...] [--d128] [--d256] [--qk-norm] [--reps 21] [--rounds 5] [--json]
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
SHAPES_D128 = [(b, s, 32, k, 128) for k in (8, 32) for s in (128, 512, 1024, 2048) for b in (1, 8)]
SHAPES_D256 = [(b, s, h, k, 256, w) for h, k in ((4, 1), (8, 4)) for s in (512, 1024, 2048, 4096) for b in (1, 8)
               for w in (-1, 511)]


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


def rotated(t, n, d, cos, sin):
    """[B, S, n d] -> [B, S, n, d]: rotate-half in fp32, one rounding to bf16."""
    b, s, _ = t.shape
    t = t.reshape(b, s, n, d).float()
    t1, t2 = t[..., :d // 2], t[..., d // 2:]
    c, sn = cos[None, :, None, :], sin[None, :, None, :]
    return torch.cat([t1 * c - t2 * sn, t2 * c + t1 * sn], -1).to(torch.bfloat16)


def sdpa(qkv, cos, sin, h, k, d, scale, out):
    """Baseline (b): torch rotation, K / V repeated, torch's fused causal attention."""
    b, s, _ = qkv.shape
    q, kk, v = qkv.split([h * d, k * d, k * d], -1)
    q = rotated(q, h, d, cos, sin).transpose(1, 2)
    kk = rotated(kk, k, d, cos, sin).repeat_interleave(h // k, 2).transpose(1, 2)
    v = v.reshape(b, s, k, d).repeat_interleave(h // k, 2).transpose(1, 2)
    y = torch.nn.functional.scaled_dot_product_attention(q, kk, v, is_causal=True, scale=scale)
    out.copy_(y.transpose(1, 2).reshape(b, s, h * d))


def candidates256(H, qkv, cos, sin, h, k, window, out, qk_norm):
    """D = 256 (kernels/gqattn256.hip): the kernel with the QK-norm and this window, the op's torch path doing the
    same, and torch rotation + sdpa (no norm; a window goes in as a boolean mask, which costs sdpa its causal path)."""
    from rust_tensorflow_serving2_amd.graph.patterns import RopeGQAttentionOp
    d, (b, s, _) = 256, qkv.shape
    scale = d ** -0.5
    op = RopeGQAttentionOp(h, k, d, s, scale, -10000.0, cos, sin, qkv.device, False, qk_norm, window)
    flat = qkv.reshape(b * s, -1)
    band = None
    if 0 <= window < s - 1:
        i = torch.arange(s, device=qkv.device)
        band = ((i[:, None] - i[None, :]) >= 0) & ((i[:, None] - i[None, :]) <= window)

    def torch_sdpa():
        q, kk, v = qkv.split([h * d, k * d, k * d], -1)
        q = rotated(q, h, d, cos, sin).transpose(1, 2)
        kk = rotated(kk, k, d, cos, sin).repeat_interleave(h // k, 2).transpose(1, 2)
        v = v.reshape(b, s, k, d).repeat_interleave(h // k, 2).transpose(1, 2)
        y = torch.nn.functional.scaled_dot_product_attention(q, kk, v, attn_mask=band, is_causal=band is None,
                                                             scale=scale)
        out["torch sdpa"].copy_(y.transpose(1, 2).reshape(b, s, h * d))
    return {"rope_gqa": lambda: H.rope_gqa_attention256(qkv, cos, sin, None, h, k, scale, window, out["rope_gqa"],
                                                        *qk_norm),
            "op torch path": lambda: out["op torch path"].copy_(op(None, None, [flat])[0].reshape(b, s, h * d)),
            "torch sdpa": torch_sdpa}


def candidates(H, qkv, cos, sin, h, k, d, out, qk_norm=None):
    """name -> callable writing out[name]; the first is the kernel, the second what it is checked against."""
    scale = d ** -0.5
    if qk_norm is not None:
        from rust_tensorflow_serving2_amd.graph.patterns import RopeGQAttentionOp
        b, s, _ = qkv.shape
        qg, kg, eps = qk_norm
        op = RopeGQAttentionOp(h, k, d, s, scale, -10000.0, cos, sin, qkv.device, False, qk_norm)
        flat = qkv.reshape(b * s, -1)
        # what the graph can launch without the fused norm: rmsnorm over q's and k's [B S n, 128] rows, then the
        # norm-less kernel (its packed input taken as given: the copies that would pack it are not charged)
        q_rows = qkv[..., :h * d].reshape(-1, d).contiguous()
        k_rows = qkv[..., h * d:(h + k) * d].reshape(-1, d).contiguous()
        qn, kn = torch.empty_like(q_rows), torch.empty_like(k_rows)

        def unfused():
            H.rmsnorm(q_rows, qg, eps, None, qn)
            H.rmsnorm(k_rows, kg, eps, None, kn)
            H.rope_gqa_attention(qkv, cos, sin, None, h, k, scale, out["rmsnorm x2 + no norm"])
        return {"rope_gqa": lambda: H.rope_gqa_attention(qkv, cos, sin, None, h, k, scale, out["rope_gqa"], qg, kg, eps),
                "op torch path": lambda: out["op torch path"].copy_(op(None, None, [flat])[0].reshape(b, s, h * d)),
                "no norm": lambda: H.rope_gqa_attention(qkv, cos, sin, None, h, k, scale, out["no norm"]),
                "rmsnorm x2 + no norm": unfused}
    runs = {"rope_gqa": lambda: H.rope_gqa_attention(qkv, cos, sin, None, h, k, scale, out["rope_gqa"])}
    if d == 64:
        packed = compose(qkv, cos, sin, h, k)
        runs["composition"] = lambda: H.causal_attention(compose(qkv, cos, sin, h, k), None, h, scale,
                                                         out["composition"])
        runs["cattn only"] = lambda: H.causal_attention(packed, None, h, scale, out["cattn only"])
    else:
        from rust_tensorflow_serving2_amd.graph.patterns import RopeGQAttentionOp
        b, s, _ = qkv.shape
        op = RopeGQAttentionOp(h, k, d, s, scale, -10000.0, cos, sin, qkv.device, False)
        flat = qkv.reshape(b * s, -1)
        runs["op torch path"] = lambda: out["op torch path"].copy_(op(None, None, [flat])[0].reshape(b, s, h * d))
        runs["torch sdpa"] = lambda: sdpa(qkv, cos, sin, h, k, d, scale, out["torch sdpa"])
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", type=parse, default=None, metavar="B,S,H,Hkv[,D]")
    ap.add_argument("--d128", action="store_true", help="the D = 128 shape list instead of the D = 64 one")
    ap.add_argument("--d256", action="store_true", help="the D = 256 shape list (Gemma: QK-norm, window -1 and 511)")
    ap.add_argument("--qk-norm", action="store_true",
                    help="D = 128 with the QK-norm in the kernel, against the op's torch path, the norm-less kernel "
                         "(the cost of the norm) and two rmsnorm launches followed by the norm-less kernel")
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
    for shape in args.shapes or (SHAPES_D256 if args.d256 else SHAPES_D128 if args.d128 else SHAPES):
        b, s, h, k = shape[:4]
        d = shape[4] if len(shape) > 4 else 64
        g = torch.Generator().manual_seed(s * 100 + b)
        qkv = torch.randn(b, s, (h + 2 * k) * d, generator=g).to(torch.bfloat16).to(dev)
        cos, sin = (torch.from_numpy(t[0, 0, :, :d // 2].copy()).to(dev) for t in llama.rope_tables(s, dim=d))
        names = ["rope_gqa", "composition", "cattn only"] if d == 64 else ["rope_gqa", "op torch path", "torch sdpa"]
        qk_norm = None
        if args.qk_norm:
            if d != 128:
                raise SystemExit("--qk-norm needs D = 128 shapes")
            names = ["rope_gqa", "op torch path", "no norm", "rmsnorm x2 + no norm"]
            qk_norm = tuple((1 + 0.25 * torch.randn(d, generator=g)).to(dev) for _ in range(2)) + (1e-6,)
        window = shape[5] if len(shape) > 5 else -1
        if d == 256:
            names = ["rope_gqa", "op torch path", "torch sdpa"]
            qk_norm = tuple((1 + 0.25 * torch.randn(d, generator=g)).to(dev) for _ in range(2)) + (1e-6,)
        out = {n: torch.empty(b, s, h * d, dtype=torch.bfloat16, device=dev) for n in names}
        runs = candidates256(H, qkv, cos, sin, h, k, window, out, qk_norm) if d == 256 else \
            candidates(H, qkv, cos, sin, h, k, d, out, qk_norm)
        rounds = {n: [] for n in runs}
        for _ in range(args.rounds):
            for n, fn in runs.items():                       # alternating: every round times every candidate once
                rounds[n].append(timed(fn, flush, args.reps))
        # the same roundings in the same order (D = 64) or an fp32 computation of the same thing (D = 128)
        err = (out["rope_gqa"].float() - out[names[1]].float()).abs().max().item()
        assert err < 0.05, err
        med = {n: statistics.median(v) for n, v in rounds.items()}
        spread = {n: (max(v) - min(v)) / med[n] for n, v in rounds.items()}
        cells = " ".join(f"{n} {med[n]:.1f} us (spread {spread[n]:.1%})" for n in names)
        ratios = " ".join(f"{n} / rope_gqa {med[n] / med['rope_gqa']:.2f}" for n in names[1:])
        tag = f"{b}x{s}x{h}/{k} D={d}" + (f" w={window}" if d == 256 else "")
        print(f"{tag:>22}  {cells}  {ratios}", flush=True)
        if args.json:
            print(json.dumps({"b": b, "s": s, "h": h, "hkv": k, "d": d, "rounds": args.rounds,
                              "us": {n: [round(x, 2) for x in v] for n, v in rounds.items()}}), flush=True)


if __name__ == "__main__":
    main()
