"""The grouped conv kernel (kernels/gconv.hip) under its elementwise bound.

fp64 reference and bound from gconv_bounds.py (docs/numerics.md, "Grouped
conv"); EVERY output element is checked and every output buffer is pre-filled
with NaN (an element the kernel skips fails).

The grid: every channels-per-group the kernel takes, each at one 32-channel
slab (or two), at three slabs and at a channel count whose groups do not fill
the last slab evenly; images smaller than the pixel tile (8 x 16 outputs at
stride 1, 4 x 16 at stride 2), and images larger than it in both directions and
a multiple of it in neither; stride 2 with the exporter's explicit (1, 1, 1, 1)
padding on odd and even heights and with SAME's (0, 1, 0, 1) on even inputs."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import gconv_bounds as gb  # noqa: E402
import kernel_bounds as kb  # noqa: E402
from kernel_bounds import BF, rnd  # noqa: E402
from rust_tensorflow_serving2_amd.graph.fused import pack_grouped_filter  # noqa: E402
from rust_tensorflow_serving2_amd.ops import ACT, hip  # noqa: E402

DEV = torch.device("cuda:0")
CUS = torch.cuda.get_device_properties(0).multi_processor_count
NAN = float("nan")
N = 3
GROUPS = [(4, 32), (4, 96), (8, 32), (8, 96), (16, 32), (16, 96), (32, 64), (32, 96)]       # (Cg, C)
# (h, w), stride, pads (top, bottom, left, right)
GEOMETRIES = (
    [((h, w), 1, (1, 1, 1, 1)) for h, w in ((7, 7), (9, 5), (17, 20))] +
    # 19 x 35 -> 10 x 18 outputs: past the stride-2 tile (4 x 16) both ways
    [((h, w), 2, (1, 1, 1, 1)) for h, w in ((7, 7), (9, 5), (17, 20), (8, 7), (19, 35))] +
    [((h, w), 2, (0, 1, 0, 1)) for h, w in ((8, 6), (18, 20), (20, 36))])


def out_size(hw, stride, pads):
    return ((hw[0] + pads[0] + pads[1] - 3) // stride + 1, (hw[1] + pads[2] + pads[3] - 3) // stride + 1)


@functools.lru_cache(maxsize=None)
def operands(cg, c, n, hw, seed=0):
    """bf16 input, bf16-valued filter (HWIO, in-depth cg), fp32 bias: pre ~ N(0.3, 1)."""
    x = rnd(n, hw[0], hw[1], c, seed=seed + 1).to(BF)
    w = rnd(3, 3, cg, c, scale=(9 * cg) ** -0.5, seed=seed + 2).to(BF)
    b = 0.3 + rnd(c, scale=0.3, seed=seed + 3)
    return x, w, b, pack_grouped_filter(w.float(), cg).to(DEV), b.to(DEV)


def launch(x, wp, b, cg, stride, pads, act, **kw):
    n, h, w, c = x.shape
    ho, wo = out_size((h, w), stride, pads)
    out = torch.full((n, ho, wo, c), NAN, dtype=BF, device=DEV)
    y = hip().gconv2d(x.to(DEV), wp, b, cg, stride, pads[0], pads[2], ho, wo, ACT[act], out, **kw)
    assert y.data_ptr() == out.data_ptr()
    return y


@pytest.mark.parametrize("cg,c", GROUPS)
def test_gconv_within_bound(cg, c):
    worst = 0.0
    for hw, stride, pads in GEOMETRIES:
        x, w, b, wp, bd = operands(cg, c, N, hw)
        pre, mag = gb.gconv_parts(x, w, b, stride, pads)
        assert pre.shape[1:3] == out_size(hw, stride, pads)
        for act in ("none", "relu"):
            ref, bound = kb.epilogue(pre, mag, gb.k_slots(cg), splits=1, act=act)
            r = kb.assert_within(launch(x, wp, bd, cg, stride, pads, act), ref, bound,
                                 f"gconv Cg {cg} C {c} {hw} s{stride} pads {pads} {act}")
            worst = max(worst, r)
    print(f"gconv Cg {cg} C {c}: worst err / bound = {worst:.3f}")


@pytest.mark.parametrize("cg,c", [(4, 32), (8, 96)])
@pytest.mark.parametrize("which", ["first", "middle", "last"])
@pytest.mark.parametrize("stride", [1, 2])
def test_group_isolation(cg, c, which, stride):
    """+Inf in every input element of one group: that group's outputs alone are
    non-finite, and every other output is within the bound of the reference
    with that group zeroed.  (A block-diagonal filter, or an MFMA that pairs
    one group's activations with another's zero weights, gives 0 x Inf = NaN.)"""
    groups = c // cg
    g = {"first": 0, "middle": groups // 2, "last": groups - 1}[which]
    hw, pads = (17, 20), (1, 1, 1, 1)
    x, w, b, wp, bd = operands(cg, c, N, hw)
    sl = slice(g * cg, (g + 1) * cg)
    xi, xz = x.clone(), x.clone()
    xi[..., sl] = float("inf")
    xz[..., sl] = 0
    for act in ("none", "relu"):
        y = launch(xi, wp, bd, cg, stride, pads, act).float().cpu()
        # (the kernel's ReLU is x > 0 ? x : 0, as every epilogue's here: NaN and -Inf leave it as 0, and a
        # window of Infs under weights of both signs sums to NaN)
        hit = y[..., sl]
        assert not torch.isfinite(hit[hit != 0] if act == "relu" else hit).any(), f"{which} {act}"
        keep = torch.ones(c, dtype=torch.bool)
        keep[sl] = False
        assert torch.isfinite(y[..., keep]).all(), f"{which} {act}"
        ref, bound = gb.gconv_ref(xz, w, b, stride, pads, act)
        kb.assert_within(y[..., keep], ref[..., keep], bound[..., keep], f"gconv group isolation {which} {act}")


@pytest.mark.parametrize("cg,c", [(4, 32), (32, 64)])
@pytest.mark.parametrize("stride", [1, 2])
def test_image_isolation(cg, c, stride):
    """Image 1 of 3 is all Inf: images 0 and 2 are untouched (no tap leaks
    across the batch or row seams of a flattened pixel index)."""
    hw, pads = (9, 5), (1, 1, 1, 1)
    x, w, b, wp, bd = operands(cg, c, N, hw)
    xi = x.clone()
    xi[1] = float("inf")
    y = launch(xi, wp, bd, cg, stride, pads, "none").float().cpu()
    ref, bound = gb.gconv_ref(x, w, b, stride, pads, "none")
    assert not torch.isfinite(y[1]).any()
    for i in (0, 2):
        kb.assert_within(y[i], ref[i], bound[i], f"gconv image isolation, image {i}")


def test_many_tiles_stage1():
    """ResNeXt-50 32x4d stage 1 itself, 56 x 56 x 128 with 4 channels per group,
    at a batch that gives more workgroups than the device has CUs."""
    per_image = 7 * 4 * 4                       # 8 x 16 pixel tiles x 32-channel slabs
    n = max(8, CUS // per_image + 1)
    assert n * per_image > CUS
    x, w, b, wp, bd = operands(4, 128, n, (56, 56), seed=50)
    ref, bound = gb.gconv_ref(x, w, b, 1, (1, 1, 1, 1), "relu")
    r = kb.assert_within(launch(x, wp, bd, 4, 1, (1, 1, 1, 1), "relu"), ref, bound, "gconv stage 1")
    print(f"gconv stage 1, batch {n}: worst err / bound = {r:.3f}")


def test_many_tiles_stride_2():
    """The first block of stage 2: 56 x 56 x 256 behind the exporter's Pad, 8
    channels per group, stride 2 -> 28 x 28 x 256."""
    x, w, b, wp, bd = operands(8, 256, 4, (56, 56), seed=60)
    ref, bound = gb.gconv_ref(x, w, b, 2, (1, 1, 1, 1), "relu")
    assert ref.shape == (4, 28, 28, 256) and 4 * 7 * 2 * 8 > CUS
    r = kb.assert_within(launch(x, wp, bd, 8, 2, (1, 1, 1, 1), "relu"), ref, bound, "gconv stage 2 stride 2")
    print(f"gconv stage 2 / 2: worst err / bound = {r:.3f}")


@pytest.mark.parametrize("cg,c,stride", [(4, 96, 1), (16, 96, 2), (32, 64, 1)])
def test_gconv_is_deterministic(cg, c, stride):
    x, _w, _b, wp, bd = operands(cg, c, N, (17, 20))
    a = launch(x, wp, bd, cg, stride, (1, 1, 1, 1), "relu")
    b = launch(x, wp, bd, cg, stride, (1, 1, 1, 1), "relu")
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("what,cg,kw", [
    ("Cg 2", 2, {}), ("Cg 64", 64, {}), ("unequal group widths", 4, dict(cg_out=8)),
    ("stride (1, 2)", 4, dict(sw=2)), ("a 5 x 5 filter", 4, dict(kh=5, kw=5)), ("ReLU6", 4, dict(act="relu6"))])
def test_launcher_rejects(what, cg, kw):
    """What the kernel does not take is an error, and nothing is written."""
    kw = dict(kw)
    act = kw.pop("act", "relu")
    x = torch.ones(1, 12, 12, 64, dtype=BF, device=DEV)
    good = pack_grouped_filter(torch.zeros(3, 3, 4, 64), 4).to(DEV)
    # (a shape the kernel takes must come with its packed filter: the ReLU6 call has it, so that the
    # activation alone is what the launcher refuses)
    wp = good if not kw and cg == 4 else torch.zeros(64 * 1024, dtype=BF, device=DEV)
    b = torch.zeros(64, device=DEV)
    wo = 12 // kw.get("sw", 1)
    out = torch.full((1, 12, wo, 64), NAN, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="gconv2d: invalid argument"):
        hip().gconv2d(x, wp, b, cg, 1, 1, 1, 12, wo, ACT[act], out, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), what
    # the same call in a shape the kernel takes writes every element
    out = torch.full((1, 12, 12, 64), NAN, dtype=BF, device=DEV)
    hip().gconv2d(x, good, b, 4, 1, 1, 1, 12, 12, ACT["relu"], out)
    assert (out == 0).all()
