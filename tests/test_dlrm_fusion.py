"""DLRM through the fusion passes on the CPU: dlrm_tiny fused == the reference
interpreter with exactly one _EmbeddingBag and one _DotInteraction and none of
the nodes they replace; every spelling the two passes take; every near miss
stays unfused (and still computes what the interpreter computes); an id outside
its table raises on the CPU; both ops can be built from meta tensors; the
exporter's defaults are pinned."""
import hashlib
import os

import numpy as np
import pytest
import torch

import test_mobilenet_v3_fusion as v3f
from rust_tensorflow_serving2_amd.graph.builder import DType, GraphBuilder
from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
from rust_tensorflow_serving2_amd.utils import tensors as T

OUTS = ["logits", "probabilities"]
F32, I32, I64 = DType(T.DT_FLOAT), DType(T.DT_INT32), DType(T.DT_INT64)
GONE = ("GatherV2", "Sum", "Pack", "BatchMatMulV2", "SplitV", "ConcatV2", "Pad", "Reshape", "MatMul", "BiasAdd", "Relu")


@pytest.fixture(scope="module")
def tiny_dlrm(models_dir):
    from rust_tensorflow_serving2_amd.models import dlrm
    path = os.path.join(str(models_dir), "dlrm_tiny", "1")
    dlrm.export(path, "dlrm_tiny", seed=5)
    ref = Servable("m", 1, path, ServableOptions(device="cpu"))
    fused = Servable("m", 1, path, ServableOptions(device="cpu", fuse=True))
    return ref, fused, fused.runner("serving_default", ["dense", "sparse"], OUTS).program


def test_dlrm_fused_matches_interpreter(tiny_dlrm):
    from rust_tensorflow_serving2_amd.models import dlrm
    ref, fused, _program = tiny_dlrm
    dense, sparse = dlrm.random_inputs("dlrm_tiny", 9, seed=1, ends=True)
    a = ref.run("serving_default", {"dense": dense, "sparse": sparse}, OUTS)
    b = fused.run("serving_default", {"dense": dense, "sparse": sparse}, OUTS)
    assert a["logits"].shape == (9, 1) and np.ptp(a["logits"]) > 0.1          # (the inputs reach the output)
    np.testing.assert_allclose(a["logits"], b["logits"], atol=1e-5)
    np.testing.assert_allclose(a["probabilities"], b["probabilities"], atol=1e-6)
    # the sparse ids alone move the logit
    c = ref.run("serving_default", {"dense": dense, "sparse": np.roll(sparse, 1, axis=0)}, OUTS)
    assert np.abs(c["logits"] - a["logits"]).max() > 1e-3


def test_dlrm_fully_fused(tiny_dlrm):
    _ref, _fused, program = tiny_dlrm
    hist = program.op_histogram()
    assert hist.get("_EmbeddingBag") == 1 and hist.get("_DotInteraction") == 1, hist
    assert hist.get("_FusedMatMul") == 5, hist
    for op in GONE:
        assert op not in hist, hist
    bag = next(node for _fn, node, _i, _o in program.steps if node.op == "_EmbeddingBag")
    impl = bag.attrs["_impl"]
    assert impl.vocab == [5, 50, 7, 23, 11] and impl.split == [1, 3, 2, 1, 2] and impl.d == 32 and impl.lead
    assert len(bag.inputs) == 2 and bag.inputs[1][0] == "sparse"             # the op reads `sparse` itself
    assert tuple(impl.blob.shape) == (96, 32)
    dot = next(node.attrs["_impl"] for _fn, node, _i, _o in program.steps if node.op == "_DotInteraction")
    assert (dot.f, dot.self_interaction, dot.pad) == (6, False, 1)


# ------------------------------------------------------------------ fuse_embedding_bag on small graphs
def _bag_graph(spelling="split", lead=True, vocab=(4, 6), hot=(2, 2), dims=(8, 8), gather_axis=0, batch_dims=0,
               keep_dims=False, sum_axis=1, second_reader=False, fetch_sum=False, pack_axis=1):
    """x0 [-1, D] and sparse [-1, T] -> [x0?, e_0 ..] stacked on axis 1; one keyword makes one near miss."""
    rng = np.random.default_rng(7)
    g = GraphBuilder()
    feeds = {}
    x0 = g.placeholder("x0", T.DT_FLOAT, [-1, dims[0]])
    if spelling == "separate":
        id_refs = [g.placeholder(f"ids{f}", T.DT_INT64, [-1, l]) for f, l in enumerate(hot)]
    else:
        sparse = g.placeholder("sparse", T.DT_INT64, [-1, sum(hot)])
        sp = g.node("SplitV", "split", [sparse, g.const("sizes", np.array(hot, np.int32)),
                                        g.const("split/axis", np.array(1, np.int32))], T=I64, Tlen=I32, num_split=len(hot))
        id_refs = [sp if f == 0 else f"{sp}:{f}" for f in range(len(hot))]
    rows = []
    fetches = ["out:0"]
    for f, (v, d) in enumerate(zip(vocab, dims)):
        table = g.const(f"table{f}", rng.standard_normal((v, d)).astype(np.float32))
        e = g.node("GatherV2", f"gather{f}", [table, id_refs[f], g.const(f"gaxis{f}", np.array(gather_axis, np.int32))],
                   Tparams=F32, Tindices=I64, Taxis=I32, batch_dims=batch_dims)
        s = g.node("Sum", f"sum{f}", [e, g.const(f"saxis{f}", np.array(sum_axis, np.int32))], T=F32, Tidx=I32,
                   keep_dims=keep_dims)
        rows.append(s)
    parts = ([x0] if lead else []) + rows
    if spelling == "concat":
        cat = g.node("ConcatV2", "concat", parts + [g.const("caxis", np.array(1, np.int32))], N=len(parts), T=F32, Tidx=I32)
        g.node("Reshape", "out", [cat, g.const("shape", np.array([-1, len(parts), sum(dims) // len(dims)], np.int32))],
               T=F32, Tshape=I32)
    else:
        g.node("Pack", "out", parts, N=len(parts), T=F32, axis=pack_axis)
    if second_reader:
        g.node("Neg", "reader", [rows[0]], T=F32)
        fetches.append("reader:0")
    if fetch_sum:
        fetches.append(rows[1] + ":0")
    b = 3
    ids = np.stack([rng.integers(0, min(vocab[f], min(dims)), b) for f in range(len(hot)) for _ in range(hot[f])], 1)
    if lead:
        feeds["x0"] = v3f._x((b, dims[0]), seed=2)
    if spelling == "separate":
        first = 0
        for f, l in enumerate(hot):
            feeds[f"ids{f}"] = ids[:, first:first + l].astype(np.int64)
            first += l
    else:
        feeds["sparse"] = ids.astype(np.int64)
    return g, fetches, feeds


def _ids(kw):
    return "-".join(f"{k}={v}" for k, v in kw.items()) or "plain"


BAG_MATCHES = [dict(), dict(lead=False), dict(spelling="separate"), dict(spelling="separate", lead=False),
               dict(spelling="concat"), dict(spelling="concat", lead=False), dict(hot=(1, 3)),
               dict(vocab=(1, 6), hot=(1, 2))]
BAG_NEAR_MISSES = [
    dict(lead=False, gather_axis=1, vocab=(5, 5)),                # a gather on axis 1
    dict(spelling="concat", lead=False, dims=(8, 24)),            # tables of different D
    dict(lead=False, keep_dims=True),                             # keep_dims=True
    dict(lead=False, sum_axis=2),                                 # a Sum over axis 2
    dict(second_reader=True),                                     # an embedding term with a second reader
    dict(fetch_sum=True),                                         # ... or fetched
    dict(lead=False, pack_axis=0),                                # stacked on axis 0
]


@pytest.mark.parametrize("kw", BAG_MATCHES, ids=_ids)
def test_embedding_bag_is_matched(kw):
    g, fetches, feeds = _bag_graph(**kw)
    hist = v3f._run_both(g, fetches, feeds)
    assert hist.get("_EmbeddingBag") == 1, hist
    for op in ("GatherV2", "Sum", "Pack", "ConcatV2", "SplitV", "Reshape"):
        assert op not in hist, hist


@pytest.mark.parametrize("kw", BAG_NEAR_MISSES, ids=_ids)
def test_embedding_bag_near_misses_are_left_alone(kw):
    g, fetches, feeds = _bag_graph(**kw)
    hist = v3f._run_both(g, fetches, feeds)
    assert "_EmbeddingBag" not in hist and hist.get("GatherV2") == 2 and hist.get("Sum") == 2, hist


def test_batch_dims_stays_unfused():
    """(The interpreter does not implement batch_dims: both programs keep the GatherV2 and reject it alike.)"""
    from rust_tensorflow_serving2_amd.graph import ops as O
    from rust_tensorflow_serving2_amd.graph.compiler import compile_program
    from rust_tensorflow_serving2_amd.graph.fused import default_passes
    from rust_tensorflow_serving2_amd.graph.ir import from_graph_def
    g, fetches, feeds = _bag_graph(batch_dims=1)
    names = [f"{k}:0" for k in feeds]
    vals = [torch.from_numpy(v) for v in feeds.values()]
    ref = compile_program(from_graph_def(g.graph), names, fetches)
    fused = compile_program(from_graph_def(g.graph), names, fetches, passes=default_passes())
    hist = fused.op_histogram()
    assert "_EmbeddingBag" not in hist and hist.get("GatherV2") == 2, hist
    for program in (ref, fused):
        with pytest.raises(O.Unsupported, match="batch_dims"):
            program.run(vals)


def _programs(g, fetches, feeds):
    from rust_tensorflow_serving2_amd.graph.compiler import compile_program
    from rust_tensorflow_serving2_amd.graph.fused import default_passes
    from rust_tensorflow_serving2_amd.graph.ir import from_graph_def
    names = [f"{k}:0" for k in feeds]
    return (compile_program(from_graph_def(g.graph), names, fetches),
            compile_program(from_graph_def(g.graph), names, fetches, passes=default_passes()))


@pytest.mark.parametrize("spelling", ["split", "separate"])
@pytest.mark.parametrize("bad", [-1, 6, 2 ** 32 + 1])
def test_out_of_range_id_raises_on_the_cpu(spelling, bad):
    from rust_tensorflow_serving2_amd.graph import ops as O
    g, fetches, feeds = _bag_graph(spelling=spelling)
    key = "sparse" if spelling == "split" else "ids1"
    feeds[key] = feeds[key].copy()
    feeds[key][1, -1] = bad                                   # table 1 has 6 rows
    ref, fused = _programs(g, fetches, feeds)
    assert fused.op_histogram().get("_EmbeddingBag") == 1
    vals = [torch.from_numpy(v) for v in feeds.values()]
    for program in (ref, fused):
        with pytest.raises(O.OpError, match=r"out of range \[0, 6\)"):
            program.run(vals)


def test_embedding_bag_op_keeps_the_nodes_semantics_for_other_inputs():
    """A sparse tensor of another width fails as the SplitV did; rank-3 ids are summed over axis 1 as the nodes did."""
    from rust_tensorflow_serving2_amd.graph import ops as O
    g, fetches, feeds = _bag_graph()
    ref, fused = _programs(g, fetches, feeds)
    x0 = torch.from_numpy(feeds["x0"])
    wide = torch.zeros(3, 5, dtype=torch.int64)
    for program in (ref, fused):
        with pytest.raises(O.OpError):
            program.run([x0, wide])
    g, fetches, feeds = _bag_graph(spelling="separate", lead=False)
    ref, fused = _programs(g, fetches, feeds)
    ids = [torch.randint(0, 4, (3, 2, 5), generator=torch.Generator().manual_seed(f)) for f in range(2)]
    a, b = ref.run(ids)[0], fused.run(ids)[0]
    assert tuple(a.shape) == (3, 2, 5, 8)
    np.testing.assert_allclose(np.asarray(a), np.asarray(b), atol=1e-6)


# ------------------------------------------------------------------ fuse_dot_interaction on small graphs
def _tril(f, k):
    i, j = np.tril_indices(f, k)
    return (i * f + j).astype(np.int32)


def _interact_graph(f=5, d=8, dd=8, k=-1, idx=None, adj_x=False, adj_y=True, two_operands=False, pad=1, pad_value=None,
                    pad_batch=False, gather_axis=1, concat_axis=1, second_reader=False, fetch_inner=False, ff=None,
                    dense_last=False):
    rng = np.random.default_rng(5)
    g = GraphBuilder()
    z = g.placeholder("z", T.DT_FLOAT, [-1, f, d])
    dense = g.placeholder("dense", T.DT_FLOAT, [-1, dd])
    feeds = {"z": v3f._x((3, f, d), seed=1, scale=1.0), "dense": v3f._x((3, dd), seed=2)}
    other = z
    if two_operands:
        other = g.placeholder("z2", T.DT_FLOAT, [-1, f, d])
        feeds["z2"] = v3f._x((3, f, d), seed=3, scale=1.0)
    zz = g.node("BatchMatMulV2", "zz", [z, other], T=F32, adj_x=adj_x, adj_y=adj_y)
    flat = g.node("Reshape", "flat", [zz, g.const("flat/shape", np.array([-1, ff or f * f], np.int32))], T=F32, Tshape=I32)
    idx = _tril(f, k) if idx is None else np.asarray(idx, np.int32)
    pairs = g.node("GatherV2", "pairs", [flat, g.const("idx", idx), g.const("gaxis", np.array(gather_axis, np.int32))],
                   Tparams=F32, Tindices=I32, Taxis=I32, batch_dims=0)
    parts = [pairs, dense] if dense_last else [dense, pairs]
    out = g.node("ConcatV2", "cat" if pad or pad_batch else "out",
                 parts + [g.const("caxis", np.array(concat_axis, np.int32))], N=2, T=F32, Tidx=I32)
    fetches = ["out:0"]
    if pad_batch:
        g.node("Pad", "out", [out, g.const("paddings", np.array([[0, 1], [0, 1]], np.int32))], T=F32, Tpaddings=I32)
    elif pad and pad_value is not None:
        g.node("PadV2", "out", [out, g.const("paddings", np.array([[0, 0], [0, pad]], np.int32)),
                                g.const("value", np.array(pad_value, np.float32))], T=F32, Tpaddings=I32)
    elif pad:
        g.node("Pad", "out", [out, g.const("paddings", np.array([[0, 0], [0, pad]], np.int32))], T=F32, Tpaddings=I32)
    if second_reader:
        g.node("Neg", "reader", [pairs], T=F32)
        fetches.append("reader:0")
    if fetch_inner:
        fetches.append("flat:0")
    return g, fetches, feeds


def _upper(f):
    i, j = np.triu_indices(f, 1)
    return i * f + j


DOT_MATCHES = [dict(), dict(k=0), dict(pad=0), dict(pad=7), dict(f=2), dict(f=17, d=4), dict(pad_value=0.0)]
DOT_NEAR_MISSES = [
    dict(idx=_upper(5)),                                          # the upper triangle
    dict(idx=_tril(5, -1)[::-1].copy()),                          # a permutation
    dict(idx=_tril(4, -1)),                                       # another F's triangle
    dict(idx=_tril(5, -1)[:-1].copy()),                           # one pair short
    dict(f=4, d=4, adj_x=True),                                   # adj_x
    dict(f=4, d=4, adj_y=False),                                  # no adj_y
    dict(two_operands=True),                                      # two different operands
    dict(gather_axis=0, idx=[0, 1, 2], pad=0, dd=25, concat_axis=0),   # a gather of rows
    dict(second_reader=True),                                     # the pairs read twice
    dict(fetch_inner=True),                                       # the reshape fetched
    dict(dense_last=True),                                        # pairs before dense
]


@pytest.mark.parametrize("kw", DOT_MATCHES, ids=_ids)
def test_dot_interaction_is_matched(kw):
    g, fetches, feeds = _interact_graph(**kw)
    hist = v3f._run_both(g, fetches, feeds)
    assert hist.get("_DotInteraction") == 1, hist
    for op in ("BatchMatMulV2", "GatherV2", "ConcatV2", "Pad", "PadV2", "Reshape"):
        assert op not in hist, hist


@pytest.mark.parametrize("kw", DOT_NEAR_MISSES, ids=lambda kw: "-".join(kw))
def test_dot_interaction_near_misses_are_left_alone(kw):
    g, fetches, feeds = _interact_graph(**kw)
    hist = v3f._run_both(g, fetches, feeds)
    assert "_DotInteraction" not in hist and hist.get("BatchMatMulV2") == 1 and hist.get("GatherV2") == 1, hist


@pytest.mark.parametrize("kw", [dict(pad_value=1.0), dict(pad_batch=True)], ids=lambda kw: "-".join(kw))
def test_a_pad_that_is_not_a_zero_column_tail_stays(kw):
    """The concat still becomes the op; the Pad it cannot absorb stays a node."""
    g, fetches, feeds = _interact_graph(**kw)
    ref, fused = _programs(g, fetches, feeds)
    vals = [torch.from_numpy(v) for v in feeds.values()]
    np.testing.assert_allclose(np.asarray(ref.run(vals)[0]), np.asarray(fused.run(vals)[0]), atol=1e-5)
    hist = fused.op_histogram()
    assert hist.get("_DotInteraction") == 1 and hist.get("Pad", 0) + hist.get("PadV2", 0) == 1, hist
    impl = next(node.attrs["_impl"] for _fn, node, _i, _o in fused.steps if node.op == "_DotInteraction")
    assert impl.pad == 0


def test_dot_interaction_op_keeps_the_nodes_semantics_for_other_inputs():
    """Another feature count cannot be reshaped to [-1, F F] unless the counts divide: both programs
    fail alike, or agree."""
    from rust_tensorflow_serving2_amd.graph import ops as O
    g, fetches, feeds = _interact_graph()
    ref, fused = _programs(g, fetches, feeds)
    dense = torch.from_numpy(feeds["dense"])
    for program in (ref, fused):
        with pytest.raises(O.OpError):
            program.run([torch.zeros(3, 4, 8), dense])
    z10 = torch.from_numpy(v3f._x((3, 10, 8), seed=4, scale=1.0))          # 100 = 4 x 25: [12, 25]
    dense12 = torch.from_numpy(v3f._x((12, 8), seed=5))
    np.testing.assert_allclose(np.asarray(ref.run([z10, dense12])[0]), np.asarray(fused.run([z10, dense12])[0]), atol=1e-5)


# ------------------------------------------------------------------ meta tensors, the exporter
def test_ops_are_constructible_from_meta_tensors():
    """A follower GPU compiles on shape-only weights: neither op computes with a table's values."""
    from rust_tensorflow_serving2_amd.graph.patterns import DotInteractionOp, EmbeddingBagOp
    tables = [torch.empty(v, 16, device="meta") for v in (3, 9)]
    for use_hip in (False, True):
        op = EmbeddingBagOp(tables, [1, 2], True, False, torch.device("cpu"), use_hip, "bag")
        assert tuple(op.blob.shape) == (12, 16) and not op.blob.is_meta
        assert op.blob.dtype == (torch.bfloat16 if use_hip else torch.float32)
        assert op.features([1, 2], "cpu")[0] == [0, 3, 0, 1, 3, 9, 1, 2]
    dot = DotInteractionOp(6, False, 1, torch.device("cpu"), False, "dot")
    assert dot.idx.tolist() == _tril(6, -1).tolist()


def test_table_blob_travels_with_the_weights(tiny_dlrm):
    from rust_tensorflow_serving2_amd.graph.placement import weight_refs
    _ref, _fused, program = tiny_dlrm
    refs = weight_refs(program)
    shapes = [tuple(t.shape) for (holder, k, _i), t in refs if k == "blob"]
    assert shapes == [(96, 32)]                                   # the table blob travels with the weights


def test_follower_compiles_the_same_program_from_a_shape_only_bundle(tiny_dlrm):
    """What a follower GPU does (parallel/weights.py): every float variable a meta tensor.  The program has the
    leader's steps and the leader's weight manifest, so the broadcast blob binds."""
    from rust_tensorflow_serving2_amd.graph.compiler import bind_variables, compile_program
    from rust_tensorflow_serving2_amd.graph.fused import default_passes
    from rust_tensorflow_serving2_amd.graph.ir import from_graph_def
    from rust_tensorflow_serving2_amd.graph.placement import manifest_of, weight_refs
    from rust_tensorflow_serving2_amd.parallel.weights import MemoryBundle
    _ref, fused, program = tiny_dlrm
    b = fused.bundle.bundle
    names = sorted(b.keys())
    meta = MemoryBundle({n: torch.empty(list(b.shape(n)), dtype=torch.float32, device="meta") for n in names},
                        {n: b.dtype(n) for n in names})
    g = from_graph_def(fused.bundle.graph_def)
    bind_variables(g, meta)
    follower = compile_program(g, ["dense:0", "sparse:0"], ["logits:0", "probabilities:0"], passes=default_passes())
    assert follower.op_histogram() == program.op_histogram()
    assert manifest_of(weight_refs(follower)) == manifest_of(weight_refs(program))


def test_dlrm_configs():
    from rust_tensorflow_serving2_amd.models import dlrm
    cfg = dlrm.config("dlrm_criteo")
    assert len(cfg["vocab"]) == 26 and max(cfg["vocab"]) == dlrm.VOCAB_CAP == 40000 and cfg["dim"] == 128
    assert sum(cfg["vocab"]) == 367398
    # fp32 tables + MLP weights stay below 256 MB
    mlp = 13 * 512 + 512 * 256 + 256 * 128 + 480 * 1024 + 1024 * 1024 + 1024 * 512 + 512 * 256 + 256
    assert (sum(cfg["vocab"]) * 128 + mlp) * 4 < 256 * 2 ** 20
    tiny = dlrm.config("dlrm_tiny")
    assert 5 <= min(tiny["vocab"]) and max(tiny["vocab"]) <= 50 and set(tiny["hot"]) == {1, 2, 3} and tiny["dim"] == 32
    g, sigs, _saver = dlrm.build_graph("dlrm_criteo", vocab_cap=10)
    ops = [n.op for n in g.graph.node]
    assert ops.count("GatherV2") == 27 and ops.count("Sum") == 26 and ops.count("SplitV") == 1
    assert ops.count("Pack") == 1 and ops.count("BatchMatMulV2") == 1 and ops.count("Pad") == 1
    assert ops.count("MatMul") == 8 and ops.count("ParseExample") == 1 and ops.count("Sigmoid") == 1
    assert set(sigs) == {"serving_default", "classify", "regress"}
    assert g.variables["dlrm/top/dense_0/kernel"].shape == (480, 1024)
    with pytest.raises(ValueError, match="unknown DLRM config"):
        dlrm.build_graph("dlrm_huge")


# sha256 of the GraphDef (deterministic serialization) and of the variables (sorted by name: name bytes, then
# the array's bytes) of build_graph()'s defaults (dlrm_criteo at the 40000-row cap), and the number of variables
PINNED = ("a30cdef2f079f18a295cfdcde7a0119ac38f9c525ef1e1730ea75569c6b58238",
          "4d417b6bdde9db9fc1ce2e83cdbc712516f62570476e4abcd286c34c22bb619c", 42)


def test_default_export_is_pinned():
    from rust_tensorflow_serving2_amd.models import dlrm
    g, _sigs, _saver = dlrm.build_graph()
    h = hashlib.sha256()
    for name in sorted(g.variables):
        h.update(name.encode())
        h.update(np.ascontiguousarray(g.variables[name]).tobytes())
    got = (hashlib.sha256(g.graph.SerializeToString(deterministic=True)).hexdigest(), h.hexdigest(), len(g.variables))
    assert got == PINNED, got
