"""T5 through the fusion passes on the CPU: the fused graph (the fp32 torch path of
_BiasAttention, which computes the matched graph's own arithmetic from the table) ==
the unfused interpreter, in both nestings of the two adds; every near miss of
fuse_bias_attention is left to fuse_attention and still computes what the interpreter
computes; TFSERVE_T5=0 removes the pass."""
import os

import numpy as np
import pytest

import test_mobilenet_v3_fusion as v3f
from rust_tensorflow_serving2_amd.graph.builder import DType, GraphBuilder
from rust_tensorflow_serving2_amd.models import t5
from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
from rust_tensorflow_serving2_amd.utils import tensors as T

F32 = DType(T.DT_FLOAT)
OUTS = ["hidden", "pooled"]
LAYERS = 3


def _serve(models_dir, name, shared_sum=True):
    path = os.path.join(str(models_dir), name, "1")
    t5.export(path, "t5_tiny", seed=2, shared_sum=shared_sum)
    S = t5.CONFIGS["t5_tiny"][4]
    mask = np.ones((3, S), np.int32)
    mask[1, S - 40:] = 0                                        # right padding
    mask[2, :9] = 0                                             # left padding: the pad rows' arithmetic is the graph's
    feeds = {"input_ids": np.random.default_rng(1).integers(0, 503, (3, S), dtype=np.int32), "input_mask": mask}
    ref = Servable("m", 1, path, ServableOptions(device="cpu"))
    fused = Servable("m", 1, path, ServableOptions(device="cpu", fuse=True))
    a, b = ref.run("serving_default", feeds, OUTS), fused.run("serving_default", feeds, OUTS)
    return a, b, fused.runner("serving_default", list(feeds), OUTS).program


@pytest.mark.parametrize("shared_sum", [True, False], ids=["shared-sum", "two-adds"])
def test_t5_tiny_fused_matches_interpreter(models_dir, shared_sum):
    a, b, prog = _serve(models_dir, f"t5_tiny_{int(shared_sum)}", shared_sum)
    S = t5.CONFIGS["t5_tiny"][4]
    assert a["hidden"].shape == (3, S, 128) and a["pooled"].shape == (3, 128)
    # fp32 against fp32 in another summation order (one 3 C wide GEMM, one softmax over S = 200): a 256-deep dot
    # product reordered moves a unit-scale value by up to 256 * 2^-24 = 1.5e-5, and each of the three blocks stacks a
    # few of those under an RMS norm; 1e-4 of the outputs' unit scale is far below what a wrong table does (order 0.1)
    for o in OUTS:
        np.testing.assert_allclose(a[o], b[o], atol=1e-4)
    hist = prog.op_histogram()
    assert hist.get("_BiasAttention") == LAYERS and hist.get("_FusedQKV") == LAYERS, hist
    assert hist.get("_RMSNorm") == 2 * LAYERS + 1, hist
    for op in ("BatchMatMulV2", "Softmax", "_Attention", "Rsqrt"):
        assert op not in hist, hist
    # the [B, H, S, S] sum of the bias and the padding adder is read by nothing once every layer is rewritten
    assert not [n.name for _f, n, _i, _o in prog.steps if n.name.endswith("position_bias_masked")]
    assert [n.attrs["_impl"].sum_first for _f, n, _i, _o in prog.steps if n.op == "_BiasAttention"] == [shared_sum] * LAYERS


def test_without_the_pass_fuse_attention_takes_the_layers(models_dir, monkeypatch):
    monkeypatch.setenv("TFSERVE_T5", "0")
    a, b, prog = _serve(models_dir, "t5_tiny_off")
    hist = prog.op_histogram()
    assert hist.get("_Attention") == LAYERS and "_BiasAttention" not in hist, hist
    np.testing.assert_allclose(a["hidden"], b["hidden"], atol=1e-4)


def _toeplitz(s, h, seed=7):
    table = v3f._x((h, 2 * s - 1), seed=seed, scale=1.0)
    pos = np.arange(s)
    return np.ascontiguousarray(table[:, pos[None, :] - pos[:, None] + s - 1][None])


def _core_graph(s=9, h=2, bias=None, adder=True, bias_first=True, shared=False, second_const=False, fed_bias=False,
                fetch=None):
    """t5.attention_core over x [B * S, H * 64]; one keyword makes one spelling or one near miss."""
    g = GraphBuilder()
    feeds = {"x": v3f._x((2 * s, h * 64), seed=2, scale=1.0)}
    x = g.placeholder("x", T.DT_FLOAT, [-1, h * 64])
    if fed_bias:
        b = g.placeholder("fed_bias", T.DT_FLOAT, [1, h, s, s])
        feeds["fed_bias"] = _toeplitz(s, h)
    else:
        b = g.const("position_bias", _toeplitz(s, h) if bias is None else bias)
    a = None
    if second_const:
        a = g.const("second_bias", _toeplitz(s, h, seed=8))
    elif adder:
        a = g.placeholder("key_adder", T.DT_FLOAT, [-1, 1, 1, s])
        feeds["key_adder"] = np.where(np.arange(2 * s).reshape(2, 1, 1, s) % 5 == 4, -1e4, 0.0).astype(np.float32)
    if shared:
        b, a = g.node("AddV2", "shared_sum", [b, a], T=F32), None
    t5.attention_core(g, x, h * 64, s, h, np.random.default_rng(3), b, a, bias_first, const_weights=True)
    return g, ["Reshape_out:0"] + ([fetch] if fetch else []), feeds


@pytest.mark.parametrize("kw", [dict(), dict(bias_first=False), dict(shared=True), dict(adder=False),
                                dict(bias=_toeplitz(9, 2)[0]), dict(s=1), dict(s=70)], ids=str)
def test_bias_core_is_matched(kw):
    """(A table read backwards or at another head would show: the op's torch path rebuilds the bias from ITS table.)"""
    g, fetches, feeds = _core_graph(**kw)
    hist = v3f._run_both(g, fetches, feeds, atol=1e-5)
    assert hist.get("_BiasAttention") == 1 and hist.get("_FusedQKV") == 1 and "Softmax" not in hist, hist


_BENT = _toeplitz(9, 2)
_BENT[0, 1, 4, 6] += 1e-6 * abs(_BENT[0, 1, 4, 6]) + 1e-7       # one entry off its diagonal by a few ulps
NEAR_MISSES = [dict(bias=_BENT), dict(bias=_BENT, adder=False), dict(second_const=True), dict(bias=_toeplitz(9, 1)),
               dict(fed_bias=True), dict(fetch="add:0"), dict(fetch="MatMul:0")]


@pytest.mark.parametrize("kw", NEAR_MISSES, ids=["not-toeplitz", "not-toeplitz-alone", "two-constants", "other-H",
                                                 "fed-bias", "fetched-sum", "fetched-scores"])
def test_near_misses_are_left_to_fuse_attention(kw):
    g, fetches, feeds = _core_graph(**kw)
    hist = v3f._run_both(g, fetches, feeds, atol=1e-5)
    assert "_BiasAttention" not in hist, hist
    if kw.get("adder") is False:                                # one adder under the Softmax: fuse_attention's pattern
        assert hist.get("_Attention") == 1, hist
