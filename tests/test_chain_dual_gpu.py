"""The dual-source form of the chain kernel (kernels/chain.hip): a stride-1
dual conv (a projecting bottleneck's expand conv + projection shortcut as one
K-concatenated GEMM over two A sources) chained with the next block's 1x1
reduce -- ResNet-50 stage 1's first block.

Kernel level: every element under the kernel_bounds.py bounds (y1 against
fp64 over the concatenated rows, y2 against the reference computed from the
kernel's own bf16 y1).  Graph level: the pass turns the dual conv and the
reduce into one _ChainConv, and both forms of the op agree with the fp32 CPU
program."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import kernel_bounds as kb  # noqa: E402
from kernel_bounds import BF, rnd  # noqa: E402
from rust_tensorflow_serving2_amd.ops import ACT, hip  # noqa: E402

DEV = torch.device("cuda:0")
C1, C2, N1, N2 = 64, 64, 256, 64


def dev(t):
    return t.to(DEV)


def inputs(m):
    h = rnd(m, C1, seed=81).to(BF)
    x = rnd(m, C2, seed=82).to(BF)
    w1 = rnd(N1, C1 + C2, scale=1 / math.sqrt(C1 + C2), seed=83).to(BF)
    b1 = rnd(N1, scale=0.3, seed=84)
    w2 = rnd(N2, N1, scale=1 / math.sqrt(N1), seed=85).to(BF)
    b2 = rnd(N2, scale=0.3, seed=86)
    return h, x, w1, b1, w2, b2


def launch(h, x, w1, b1, w2, b2, act1, act2):
    m = h.shape[0]
    return hip().conv_chain(dev(h.reshape(1, 1, m, -1)), dev(w1), dev(b1), None, ACT[act1], dev(w2), dev(b2),
                            ACT[act2], x2=dev(x.reshape(1, 1, m, -1)))


@pytest.mark.parametrize("m", [77, 200])
def test_conv_chain_dual_two_step_within_bound(m):
    """M = 77: one full 64-row tile plus a partial one; M = 200: several
    tiles, the last one partial."""
    assert hip().conv_chain_supported(C1 + C2, N1, N2, True)
    h, x, w1, b1, w2, b2 = inputs(m)
    parts1 = kb.gemm_parts(torch.cat([h, x], 1), w1, b1)
    for act1, act2 in (("relu", "relu"), ("none", "relu")):
        y1, y2 = launch(h, x, w1, b1, w2, b2, act1, act2)
        assert y1.shape == (1, 1, m, N1) and y2.shape == (1, 1, m, N2)
        ref1, bound1 = kb.epilogue(*parts1, C1 + C2, 1, act1)
        kb.assert_within(y1.reshape(m, N1), ref1, bound1, f"conv_chain dual y1: {act1} m={m}")
        ref2, bound2 = kb.epilogue(*kb.gemm_parts(y1.reshape(m, N1).cpu(), w2, b2), N1, 1, act2)
        kb.assert_within(y2.reshape(m, N2), ref2, bound2, f"conv_chain dual y2: {act2} m={m}")


def test_conv_chain_dual_is_deterministic():
    h, x, w1, b1, w2, b2 = inputs(200)
    outs = [launch(h, x, w1, b1, w2, b2, "relu", "relu") for _ in range(4)]
    for y1, y2 in outs[1:]:
        assert torch.equal(y1, outs[0][0]) and torch.equal(y2, outs[0][1])


def test_conv_chain_dual_rejects_unbuilt_shapes():
    h, x, w1, b1, w2, b2 = inputs(77)
    with pytest.raises(RuntimeError):                        # c2 = 32: not a whole k-tile
        launch(h, x[:, :32].contiguous(), w1, b1, w2, b2, "relu", "relu")
    with pytest.raises(RuntimeError):                        # x2 with other rows than x
        hip().conv_chain(dev(h.reshape(1, 1, 77, C1)), dev(w1), dev(b1), None, ACT["relu"], dev(w2), dev(b2),
                         ACT["relu"], x2=dev(x[:64].reshape(1, 1, 64, C2)))
    with pytest.raises(RuntimeError):                        # w1 narrower than c1 + c2
        launch(h, x, w1[:, :C1].contiguous(), b1, w2, b2, "relu", "relu")
    assert not hip().conv_chain_supported(C1 + C2, N1, 128, True)
    assert not hip().conv_chain_supported(C1 + C2, N1, N2)    # as a single source it is not built


# ------------------------------------------------------------------ graph level
@pytest.fixture(scope="module")
def small_resnet(tmp_path_factory):
    from rust_tensorflow_serving2_amd.models import resnet
    path = os.path.join(str(tmp_path_factory.mktemp("chain_dual")), "1")
    resnet.export(path, blocks=(2, 1, 1, 1), width=64, num_classes=10, image_size=32)
    return path


@pytest.fixture(scope="module")
def cpu_outputs(small_resnet):
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    x = np.random.default_rng(4).random((5, 32, 32, 3), dtype=np.float32)
    cpu = Servable("resnet", 1, small_resnet, ServableOptions(device="cpu"))
    return x, cpu.run("serving_default", {"input": x}, ["classes", "probabilities"])


def gpu_run(path, x):
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    gpu = Servable("resnet", 1, path, ServableOptions(device="cuda:0", max_batch_size=8))
    out = gpu.run("serving_default", {"input": x}, ["classes", "probabilities"])
    prog = next(iter(gpu._runners.values())).program
    return out, (prog.op_histogram(), prog.op_histogram(flat=True))


def close_to_cpu(g, c):
    """The comparison of test_resnet_gpu.py (bf16 GPU program against the fp32
    CPU program): probabilities within 5e-3, centred logits within 5 % of
    their spread."""
    assert np.abs(g["probabilities"] - c["probabilities"]).max() < 5e-3
    lg = np.log(np.maximum(g["probabilities"], 1e-30)).astype(np.float64)
    lc = np.log(np.maximum(c["probabilities"], 1e-30)).astype(np.float64)
    lg -= lg.mean(1, keepdims=True)
    lc -= lc.mean(1, keepdims=True)
    assert (np.abs(lg - lc).max(1) / lc.std(1)).max() < 5e-2


def test_pass_chains_the_stride1_dual_conv(small_resnet, cpu_outputs, monkeypatch):
    """Stage 1's projecting block: its dual conv and block 2's reduce become
    one _ChainConv (one chain more, one dual conv fewer than with the pass
    off); the projecting blocks of stages 2-4 sample x at stride 2 and stay."""
    from rust_tensorflow_serving2_amd import ops
    x, c = cpu_outputs
    monkeypatch.setattr(ops, "AUTOTUNE", False)              # the untuned picks: nothing is timed here
    monkeypatch.setenv("TFSERVE_CONV_CHAIN", "0")
    g0, (hist0, flat0) = gpu_run(small_resnet, x)
    monkeypatch.setenv("TFSERVE_CONV_CHAIN", "1")
    g1, (hist1, flat1) = gpu_run(small_resnet, x)
    assert hist0.get("_FusedDualConv") == 4 and "_ChainConv" not in hist0, hist0
    assert hist1.get("_FusedDualConv") == 3, hist1
    # block 1's dual conv -> block 2's reduce, and block 2's expand -> stage 2's reduce
    assert hist1.get("_ChainConv") == 2, hist1
    assert hist1["_FusedConv2D"] == hist0["_FusedConv2D"] - 3       # two reduces and block 2's expand
    # the flat histogram lists the dual chain's three convs as its members (a
    # dual conv and a conv), so 2 per dual conv + 2 per chain counts every conv
    assert flat0 == hist0 and flat1.get("_FusedDualConv") == 4 and flat1.get("_ChainConv") == 1, flat1
    convs = [h["_FusedConv2D"] + 2 * h["_FusedDualConv"] + 2 * h.get("_ChainConv", 0) for h in (flat0, flat1)]
    assert convs[0] == convs[1]
    monkeypatch.setenv("TFSERVE_CONV_CHAIN_SHAPES", "stage1")
    _g, (hist_s1, _flat) = gpu_run(small_resnet, x)
    assert hist_s1 == hist1
    close_to_cpu(g0, c)
    close_to_cpu(g1, c)


def test_both_forms_of_the_dual_chain_agree(small_resnet, cpu_outputs, monkeypatch):
    """The tuned choice of the dual chain forced to the chain kernel (1) and to
    the two convs (0): the op asks with a key of its own, defaults to the
    chain, and both programs match the fp32 CPU program and each other."""
    from rust_tensorflow_serving2_amd import ops
    x, c = cpu_outputs
    monkeypatch.setattr(ops, "AUTOTUNE", False)
    real = ops.tuned_choice
    outs = {}
    for forced in (1, 0):
        asked = []

        def choice(key, options, default, forced=forced, asked=asked):
            if key[0] == "chain" and key[4] == ("dual", C2):
                asked.append((key, sorted(options), default))
                return forced
            return real(key, options, default)
        monkeypatch.setattr(ops, "tuned_choice", choice)
        outs[forced], _hist = gpu_run(small_resnet, x)
        assert asked and all(k[0] == "chain" and o == [0, 1] and d == 1 for k, o, d in asked), asked
        close_to_cpu(outs[forced], c)
    assert np.abs(outs[1]["probabilities"] - outs[0]["probabilities"]).max() < 5e-3
