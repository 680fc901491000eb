"""DLRM's two kernels (kernels/embag.hip, kernels/interact.hip) at dlrm_criteo's
shapes (26 one-hot tables, D = 128, F = 27 rows per sample, 128 + 351 + 1 = 480
output columns), batch 1 / 64 / 2048, each against three baselines on the same
tensors:

  * torch:   the op's own torch path on the device (EmbeddingBagOp /
             DotInteractionOp with the kernel switched off);
  * unfused: the replaced nodes as a program compiled with no passes (SplitV, 26 x
             GatherV2 -> Sum, Pack; BatchMatMulV2, Reshape, GatherV2, ConcatV2, Pad);
  * copy:    one torch copy_ of (bytes read + bytes written) / 2: the bytes the
             op must move, the floor of this op.

Every figure is the median of single cold launches taken the way ops.tuned_config
takes them (L2 flushed, the GPU kept busy while the host records the start event
and issues the launch; scripts/dwconv_bench.py timed); the four candidates of a
shape are timed one after another in one process on one GPU.  With --engine the
whole forward is timed through the serving runtime (HIP-graph replay, host wall
clock per request, requests interleaved) with the two passes on and off
(TFSERVE_DLRM=0).

    python scripts/dlrm_bench.py [--batch 1 64 2048] [--reps 21] [--vocab-cap 40000] [--engine] [--json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dwconv_bench import timed  # noqa: E402


def _subgraphs(vocab, d, tables):
    """(embedding-bag graph, interaction graph) as GraphBuilders over placeholders."""
    from rust_tensorflow_serving2_amd.graph.builder import DType, GraphBuilder
    from rust_tensorflow_serving2_amd.utils import tensors as T
    f32, i32, i64 = DType(T.DT_FLOAT), DType(T.DT_INT32), DType(T.DT_INT64)
    nf = len(vocab)
    g = GraphBuilder()
    x0 = g.placeholder("x0", T.DT_FLOAT, [-1, d])
    sparse = g.placeholder("sparse", T.DT_INT64, [-1, nf])
    sp = g.node("SplitV", "split", [sparse, g.const("sizes", np.ones(nf, np.int32)), g.const("axis", np.array(1, np.int32))],
                T=i64, Tlen=i32, num_split=nf)
    rows = []
    for f in range(nf):
        e = g.node("GatherV2", f"gather{f}", [g.const(f"table{f}", tables[f]), sp if f == 0 else f"{sp}:{f}",
                                             g.const(f"ga{f}", np.array(0, np.int32))],
                   Tparams=f32, Tindices=i64, Taxis=i32, batch_dims=0)
        rows.append(g.node("Sum", f"sum{f}", [e, g.const(f"sa{f}", np.array(1, np.int32))], T=f32, Tidx=i32, keep_dims=False))
    g.node("Pack", "out", [x0] + rows, N=nf + 1, T=f32, axis=1)
    n = nf + 1
    h = GraphBuilder()
    z = h.placeholder("z", T.DT_FLOAT, [-1, n, d])
    dense = h.placeholder("dense", T.DT_FLOAT, [-1, d])
    zz = h.node("BatchMatMulV2", "zz", [z, z], T=f32, adj_x=False, adj_y=True)
    flat = h.node("Reshape", "flat", [zz, h.const("shape", np.array([-1, n * n], np.int32))], T=f32, Tshape=i32)
    li, lj = np.tril_indices(n, -1)
    pairs = h.node("GatherV2", "pairs", [flat, h.const("idx", (li * n + lj).astype(np.int32)),
                                         h.const("axis", np.array(1, np.int32))],
                   Tparams=f32, Tindices=i32, Taxis=i32, batch_dims=0)
    cat = h.node("ConcatV2", "cat", [dense, pairs, h.const("caxis", np.array(1, np.int32))], N=2, T=f32, Tidx=i32)
    pad = -(d + len(li)) % 8
    h.node("Pad", "out", [cat, h.const("paddings", np.array([[0, 0], [0, pad]], np.int32))], T=f32, Tpaddings=i32)
    return g, h, pad


def _copy_us(nbytes, dev, flush, reps):
    src = torch.empty(max(nbytes // 2, 16), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src), flush, reps)


def kernels(args):
    from rust_tensorflow_serving2_amd import ops
    from rust_tensorflow_serving2_amd.graph.compiler import compile_program
    from rust_tensorflow_serving2_amd.graph.fused import default_passes
    from rust_tensorflow_serving2_amd.graph.ir import from_graph_def
    from rust_tensorflow_serving2_amd.models import dlrm
    dev = torch.device("cuda:0")
    flush = ops._flush_buffer()
    cfg = dlrm.config("dlrm_criteo", args.vocab_cap)
    vocab, d = cfg["vocab"], cfg["dim"]
    rng = np.random.default_rng(0)
    tables = [(0.25 * rng.standard_normal((v, d))).astype(np.float32) for v in vocab]
    bag_g, dot_g, pad = _subgraphs(vocab, d, tables)
    progs = {}
    for name, g, feeds in (("bag", bag_g, ["x0:0", "sparse:0"]), ("dot", dot_g, ["z:0", "dense:0"])):
        progs[name, "fused"] = compile_program(from_graph_def(g.graph), feeds, ["out:0"], device=dev, passes=default_passes())
        progs[name, "unfused"] = compile_program(from_graph_def(g.graph), feeds, ["out:0"], device=dev)
    bag = next(n.attrs["_impl"] for _f, n, _i, _o in progs["bag", "fused"].steps if n.op == "_EmbeddingBag")
    dot = next(n.attrs["_impl"] for _f, n, _i, _o in progs["dot", "fused"].steps if n.op == "_DotInteraction")
    print(f"dlrm_criteo tables: {sum(vocab)} rows x {d} bf16 = {sum(vocab) * d * 2 / 2 ** 20:.1f} MiB (vocab cap {args.vocab_cap})")
    print(f"{'op':>16} {'B':>5} {'kernel us':>9} {'torch us':>9} {'unfused us':>10} {'copy us':>8} {'torch/kernel':>12} "
          f"{'unfused/kernel':>14} {'kernel/copy':>11}")
    for b in args.batch:
        _dense, sparse = dlrm.random_inputs("dlrm_criteo", b, seed=1, vocab_cap=args.vocab_cap)
        ids = torch.from_numpy(sparse).to(dev)
        x0 = torch.randn(b, d, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(dev)
        for name, op, ins, nbytes in (
                ("embedding_bag", bag, [x0, ids], ids.numel() * 8 + 2 * (len(vocab) + 1) * b * d * 2),
                ("dot_interaction", dot, None, 0)):
            if name == "dot_interaction":
                z = bag(None, None, [x0, ids])[0]
                ins = [z, x0]
                nbytes = (z.numel() + x0.numel() + b * (d + dot.idx.numel() + pad)) * 2
            node = type("N", (), {"name": name})()
            y = op(None, node, ins)[0]
            kernel = timed(lambda: op(None, node, ins), flush, args.reps)
            op.use_hip = False
            try:
                y_torch = op(None, node, ins)[0]
                torch_us = timed(lambda: op(None, node, ins), flush, args.reps)
            finally:
                op.use_hip = True
            err = (y.float() - y_torch.float()).abs().max().item()
            assert err < 0.5, err
            fins = [t.float() if t.is_floating_point() else t for t in ins]
            unfused = timed(lambda: progs["bag" if op is bag else "dot", "unfused"].run(fins), flush, args.reps)
            copy = _copy_us(nbytes, dev, flush, args.reps)
            row = {"op": name, "batch": b, "kernel_us": round(kernel, 2), "torch_us": round(torch_us, 2),
                   "unfused_us": round(unfused, 2), "copy_us": round(copy, 2), "bytes": nbytes}
            print(f"{name:>16} {b:>5} {kernel:9.1f} {torch_us:9.1f} {unfused:10.1f} {copy:8.1f} {torch_us / kernel:12.2f} "
                  f"{unfused / kernel:14.2f} {kernel / copy:11.2f}", flush=True)
            if args.json:
                print(json.dumps(row), flush=True)


def engine(args):
    from rust_tensorflow_serving2_amd.models import dlrm
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    path = os.path.join(tempfile.mkdtemp(), "1")
    dlrm.export(path, "dlrm_criteo", seed=0, vocab_cap=args.vocab_cap)
    outs = ["logits", "probabilities"]
    servables = {}
    for mode in ("fused", "unfused"):
        os.environ["TFSERVE_DLRM"] = "1" if mode == "fused" else "0"
        try:
            s = Servable("dlrm", 1, path, ServableOptions(device="cuda:0", max_batch_size=max(args.batch),
                                                          allowed_batch_sizes=tuple(sorted(args.batch))))
            hist = s.runner("serving_default", ["dense", "sparse"], outs).program.op_histogram()
        finally:
            del os.environ["TFSERVE_DLRM"]
        servables[mode] = s
        print(f"engine {mode}: {sum(hist.values())} steps {dict(hist)}")
    print(f"{'B':>5} {'fused ms':>9} {'unfused ms':>10} {'unfused/fused':>13}")
    for b in args.batch:
        dense, sparse = dlrm.random_inputs("dlrm_criteo", b, seed=1, vocab_cap=args.vocab_cap)
        feeds = {"dense": dense, "sparse": sparse}
        samples = {"fused": [], "unfused": []}
        for mode, s in servables.items():
            for _ in range(3):
                s.run("serving_default", feeds, outs)
        for _ in range(args.reps):
            for mode, s in servables.items():                 # interleaved
                t0 = time.perf_counter()
                s.run("serving_default", feeds, outs)
                samples[mode].append((time.perf_counter() - t0) * 1e3)
        med = {m: sorted(v)[len(v) // 2] for m, v in samples.items()}
        print(f"{b:>5} {med['fused']:9.3f} {med['unfused']:10.3f} {med['unfused'] / med['fused']:13.2f}", flush=True)
        if args.json:
            print(json.dumps({"engine_batch": b, "fused_ms": round(med["fused"], 4), "unfused_ms": round(med["unfused"], 4)}),
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 64, 2048])
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--vocab-cap", type=int, default=40000)
    ap.add_argument("--engine", action="store_true", help="also time the whole forward through the serving runtime")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dlrm_bench needs a GPU: a timing taken anywhere else says nothing")
    kernels(args)
    if args.engine:
        engine(args)


if __name__ == "__main__":
    main()
