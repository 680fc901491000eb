"""ResNet-50's identity-block expand convs (1x1, cout = 4 cin, + shortcut +
ReLU) on the row-panel kernel (kernels/panel.hip) against the tile-config path
the graph runs for them, and against a device-to-device copy of the bytes the
op has to move -- the stage-2, -3 and -4 shapes at each batch size asked for.

Timings are medians of single cold launches taken the way ops.tuned_config
takes them (L2 flushed, the GPU kept busy while the host records the start
event and issues the launch):

  * tiled: hip().conv2d with the committed table's pick for the conv's key
           (or, for a key the table lacks, the untuned cgemm config);
  * panel: hip().conv1x1_panel, every (bm, nsplit) of conv1x1_panel_forms;
  * copy:  one torch copy_ of (A + residual + output bytes) / 2: the op reads
           A and the residual once and writes the output once.

Prints one table row per (shape, form) and, with --json, one JSON line per
shape.  --only-form I (0 = tiled, -1 = the copy) launches that form alone
--launches times, the L2 flushed before each: the run to put under a counter
pass (--stage 2 / 3 / 4 keeps one shape, so a kernel name is one shape).

    python scripts/panel_bench.py [--batch 32 16 8] [--reps 21] [--json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EXPAND = [(28, 128, 512), (14, 256, 1024), (7, 512, 2048)]     # (H = W, cin, cout) of stages 2-4


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
    ap.add_argument("--batch", type=int, nargs="+", default=[32, 16, 8])
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--only-form", type=int, default=None)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--stage", type=int, default=0, choices=[0, 2, 3, 4], help="only this stage's shape")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("panel_bench needs a GPU: a timing taken anywhere else says nothing")
    from rust_tensorflow_serving2_amd import ops
    H = ops.hip()
    dev = torch.device("cuda:0")
    relu = ops.ACT["relu"]
    ops._ensure_cache()
    flush = ops._flush_buffer()
    if args.only_form is None:
        print(f"{'N':>3} {'M x N x K':>18} {'form':>12} {'wgs':>5} {'us':>7} {'vs tiled':>8} {'vs copy':>7}")
    for n in args.batch:
        for hw, cin, cout in (EXPAND if not args.stage else EXPAND[args.stage - 2:args.stage - 1]):
            g = torch.Generator().manual_seed(hw * 1000 + cin)
            x = torch.randn(n, hw, hw, cin, generator=g).to(torch.bfloat16).to(dev)
            w = (torch.randn(cout, cin, generator=g) * cin ** -0.5).to(torch.bfloat16).to(dev)
            b = torch.randn(cout, generator=g).to(dev)
            res = torch.randn(n, hw, hw, cout, generator=g).to(torch.bfloat16).to(dev)
            out = torch.empty(n, hw, hw, cout, dtype=torch.bfloat16, device=dev)
            m = n * hw * hw
            key = ("conv", tuple(x.shape), x.dtype, cout, 1, 1, 1, True, "relu", None)
            cfg, splits = ops._TUNED.get(key) or (ops.UNTUNED_CGEMM, 1)

            def tiled():
                return H.conv2d(x, w, b, res, 1, 1, 1, 1, 0, 0, 0, 0, relu, cfg=cfg, out=out, splits=splits)
            forms = [tuple(f) for f in H.conv1x1_panel_forms(m, cout, cin)]
            runs = [(f"cfg {cfg} x{splits}", -(-m // 64) * (cout // 64), tiled)]
            for bm, ns in forms:
                runs.append((f"bm {bm} ns {ns}", -(-m // bm) * ns,
                             lambda bm=bm, ns=ns: H.conv1x1_panel(x, w, b, res, relu, bm, ns, out=out)))
            nbytes = (x.numel() + res.numel() + out.numel()) * 2
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            if args.only_form is not None:
                if args.only_form < len(runs):
                    name, _wgs, fn = runs[args.only_form] if args.only_form >= 0 else \
                        (f"copy of {nbytes // 2} bytes", 0, lambda: dst.copy_(src))
                    for _ in range(args.launches):
                        flush.zero_()
                        fn()
                    torch.cuda.synchronize()
                    print(f"launched {name} x{args.launches}: {n} {m}x{cout}x{cin}", flush=True)
                continue
            ref = tiled().float()
            copy = timed(lambda: dst.copy_(src), flush, args.reps)
            row = {"n": n, "m": m, "cout": cout, "cin": cin, "bytes": nbytes, "copy_us": round(copy, 2), "forms": []}
            base = None
            for name, wgs, fn in runs:
                if base is not None:
                    out.zero_()
                    torch.testing.assert_close(fn().float(), ref, atol=0.1, rtol=0.05)
                us = timed(fn, flush, args.reps)
                base = us if base is None else base
                row["forms"].append({"form": name, "wgs": wgs, "us": round(us, 2)})
                print(f"{n:>3} {f'{m}x{cout}x{cin}':>18} {name:>12} {wgs:>5} {us:7.1f} {us / base:8.2f} {us / copy:7.2f}",
                      flush=True)
            print(f"{n:>3} {f'{m}x{cout}x{cin}':>18} {'copy':>12} {'':>5} {copy:7.1f}", flush=True)
            if args.json:
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
