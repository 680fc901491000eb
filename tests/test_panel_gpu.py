"""The row-panel 1x1 conv kernel (kernels/panel.hip): a workgroup owns bm rows
x N / nsplit columns, keeps its A rows in registers and walks the n-tiles over
one W ring that never drains.

Kernel level: every element under the kernel_bounds.py bound of the fp64
reference, for every depth, both panel heights, spans of 1, 2 and 4 n-tiles
(K = 128 with 4 n-tiles: 8 ring slots across three n-tile boundaries; K = 512:
the ring wraps inside one n-tile), full, partial and several panels.  The tile
kernel the graph runs today (config 42) is held to the same bound on the same
operands.  Graph level: each option of the op's tuned choice forced in turn
matches the fp32 CPU program."""
import functools
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
from test_chain_dual_gpu import close_to_cpu  # noqa: E402

DEV = torch.device("cuda:0")


def dev(t):
    return None if t is None else t.to(DEV)


@functools.lru_cache(maxsize=None)
def operands(m, n, k):
    """(x, w, bias, res) on the host and the fp64 (pre, mag) with and without
    the residual: computed once per shape, shared by every case over it."""
    x = rnd(m, k, seed=91).to(BF)
    w = rnd(n, k, scale=1 / math.sqrt(k), seed=92).to(BF)
    b = rnd(n, scale=0.3, seed=93)
    r = rnd(m, n, seed=94).to(BF)
    return (x, w, b, r), kb.gemm_parts(x, w, b, r), kb.gemm_parts(x, w, b)


def panel(x, w, b, r, act, bm, nsplit):
    m = x.shape[0]
    y = hip().conv1x1_panel(dev(x.reshape(1, 1, m, -1)), dev(w), dev(b),
                            None if r is None else dev(r.reshape(1, 1, m, -1)), ACT[act], bm, nsplit)
    return y.reshape(m, -1)


def tiled(x, w, b, r, act):
    """The same conv on the tile kernel the graph picks today: cgemm<64,64,2,2,2>, one K slice."""
    m = x.shape[0]
    y = hip().conv2d(dev(x.reshape(1, 1, m, -1)), dev(w), dev(b), None if r is None else dev(r.reshape(1, 1, m, -1)),
                     1, 1, 1, 1, 0, 0, 0, 0, ACT[act], cfg=42, splits=1)
    return y.reshape(m, -1)


CASES = [(k, n, ns, bm, m) for k in (128, 256, 512) for n, ns in ((256, 1), (512, 2), (512, 4))
         for bm in ((64, 128) if k <= 256 else (64,)) for m in (77, 200)]


@pytest.mark.parametrize("k,n,nsplit,bm,m", CASES)
def test_panel_within_bound(k, n, nsplit, bm, m):
    """M = 77: one full and one partial 64-row panel, a single partial 128-row
    panel; M = 200: several panels, the last one partial."""
    assert hip().conv1x1_panel_supported(m, n, k, bm, nsplit)
    (x, w, b, r), with_res, without = operands(m, n, k)
    for res, act, parts in ((r, "relu", with_res), (None, "none", without)):
        ref, bound = kb.epilogue(*parts, k, 1, act)
        y = panel(x, w, b, res, act, bm, nsplit)
        worst = kb.assert_within(y, ref, bound, f"panel K={k} N={n} nsplit={nsplit} bm={bm} m={m} {act}")
        y42 = tiled(x, w, b, res, act)
        kb.assert_within(y42, ref, bound, f"cfg 42 K={k} N={n} m={m} {act}")
        print(f"panel K={k} N={n} nsplit={nsplit} bm={bm} m={m} {act}: worst err/bound {worst:.3f}, "
              f"bit-equal to cfg 42: {torch.equal(y, y42)}")


def test_panel_is_deterministic():
    (x, w, b, r), _, _ = operands(200, 512, 128)
    outs = [panel(x, w, b, r, "relu", 64, 1) for _ in range(4)]
    for y in outs[1:]:
        assert torch.equal(y, outs[0])


def test_panel_rejects_what_it_was_not_built_for():
    def raises(m, n, k, bm, nsplit, act="relu", res_cols=None):
        x = rnd(m, k, seed=1).to(BF)
        w = rnd(n, k, seed=2).to(BF)
        b = rnd(n, seed=3)
        r = None if res_cols is None else rnd(m, res_cols, seed=4).to(BF)
        with pytest.raises(RuntimeError):
            hip().conv1x1_panel(dev(x.reshape(1, 1, m, k)), dev(w), dev(b),
                                None if r is None else dev(r.reshape(1, 1, m, res_cols)), ACT[act], bm, nsplit)
        kw = {} if res_cols is None else {"res_stride": res_cols}
        assert not hip().conv1x1_panel_supported(m, n, k, bm, nsplit, act=ACT[act], **kw)

    raises(77, 256, 96, 64, 1)                    # K = 96
    raises(77, 1024, 576, 64, 1)                  # K = 576
    raises(77, 100, 128, 64, 1)                   # N = 100
    raises(77, 192, 128, 64, 2)                   # spans of 96 columns: not whole n-tiles
    raises(77, 256, 128, 64, 3)                   # nsplit = 3
    raises(77, 1024, 512, 128, 1)                 # bm = 128 with K = 512
    raises(77, 256, 128, 64, 1, act="relu6")      # an igemm-only activation
    raises(77, 256, 128, 64, 1, res_cols=320)     # a residual of another row stride
    assert hip().conv1x1_panel_supported(77, 256, 128, 64, 1, act=ACT["relu"], res_stride=256)


# ------------------------------------------------------------------ graph level
@pytest.fixture(scope="module")
def small_resnet(tmp_path_factory):
    from rust_tensorflow_serving2_amd.models import resnet
    path = os.path.join(str(tmp_path_factory.mktemp("panel")), "1")
    resnet.export(path, blocks=(1, 2, 1, 1), width=64, num_classes=10, image_size=32)
    return path


def test_every_option_of_the_panel_choice_agrees(small_resnet, monkeypatch):
    """The op asks ops.tuned_choice with a "panel" key, options 0 (the tile
    path), 1, 2, ... (the kernel's forms) and default 0; each option forced
    across the whole program matches the fp32 CPU program, and the programs
    agree with each other."""
    from rust_tensorflow_serving2_amd import ops
    from rust_tensorflow_serving2_amd.server.servable import Servable, ServableOptions
    x = np.random.default_rng(4).random((5, 32, 32, 3), dtype=np.float32)
    fetch = ["classes", "probabilities"]
    c = Servable("resnet", 1, small_resnet, ServableOptions(device="cpu")).run("serving_default", {"input": x}, fetch)
    monkeypatch.setattr(ops, "AUTOTUNE", False)
    real = ops.tuned_choice
    outs, most = {}, 1
    forced = 0
    while forced <= most:
        asked = []

        def choice(key, options, default, forced=forced, asked=asked):
            if key[0] == "panel":
                asked.append((key, sorted(options), default))
                return forced if forced in options else max(options)
            return real(key, options, default)
        monkeypatch.setattr(ops, "tuned_choice", choice)
        gpu = Servable("resnet", 1, small_resnet, ServableOptions(device="cuda:0", max_batch_size=8))
        outs[forced] = gpu.run("serving_default", {"input": x}, fetch)
        assert asked, "no conv asked for a panel choice"
        for key, opts, default in asked:
            assert opts == list(range(len(opts))) and len(opts) >= 2 and default == 0, (key, opts, default)
        most = max(len(o) - 1 for _k, o, _d in asked)
        close_to_cpu(outs[forced], c)
        forced += 1
    assert len(outs) >= 2
    for o in outs.values():
        assert np.abs(o["probabilities"] - outs[0]["probabilities"]).max() < 5e-3
