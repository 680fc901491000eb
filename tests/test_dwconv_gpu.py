"""The depthwise conv kernel (kernels/dwconv.hip) under its elementwise bound.

fp64 reference and bound from dwconv_bounds.py (docs/numerics.md, "Depthwise
conv"); EVERY output element is checked, every output buffer is pre-filled with
NaN (an element the kernel skips fails), and the inputs are scaled so that
about a quarter of the pre-activations fall below 0 and a quarter above 6 --
asserted on the reference, so ReLU and ReLU6 really clamp on both sides."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import dwconv_bounds as db  # noqa: E402
import kernel_bounds as kb  # noqa: E402
from kernel_bounds import BF, rnd  # noqa: E402
from rust_tensorflow_serving2_amd.graph.ops import tf_same_pads  # noqa: E402
from rust_tensorflow_serving2_amd.ops import ACT, hip  # noqa: E402

DEV = torch.device("cuda:0")
ACTS = ["none", "relu", "relu6"]

# (n, h, w, c), (kh, kw), (sh, sw), padding: "SAME" | "VALID" | (top, bottom, left, right)
CASES = {
    "centre_tap_only": ((1, 1, 1, 8), (3, 3), (1, 1), "SAME"),          # every tap but the centre is masked
    "h_ne_w_3_chunks": ((2, 7, 5, 24), (3, 3), (1, 1), "SAME"),         # strip taller than the image, batch stride
    "s2_same_odd_even": ((1, 9, 12, 8), (3, 3), (2, 2), "SAME"),        # pads (1, 1) and (0, 1)
    "s2_same_even_odd": ((1, 10, 11, 8), (3, 3), (2, 2), "SAME"),       # pads (0, 1) and (1, 1)
    "valid": ((1, 8, 8, 16), (3, 3), (1, 1), "VALID"),
    "explicit": ((1, 6, 6, 8), (3, 3), (1, 1), (2, 0, 0, 2)),
    "generic_5x5": ((1, 9, 9, 8), (5, 5), (1, 1), "SAME"),
    "generic_stride_2_1": ((1, 9, 9, 8), (3, 3), (2, 1), "SAME"),
    "many_blocks_s1": ((3, 40, 40, 64), (3, 3), (1, 1), "SAME"),        # 2 blocks per row, 120 output rows
    "partial_wave_s2": ((2, 33, 33, 136), (3, 3), (2, 2), "SAME"),      # 17 chunks, 289 = 256 + 33 threads per row
}


def geometry(shape, k, s, padding):
    _n, h, w, _c = shape
    if padding == "SAME":
        pads = tf_same_pads(h, k[0], s[0]) + tf_same_pads(w, k[1], s[1])
    elif padding == "VALID":
        pads = (0, 0, 0, 0)
    else:
        pads = tuple(padding)
    ho = (h + pads[0] + pads[1] - k[0]) // s[0] + 1
    wo = (w + pads[2] + pads[3] - k[1]) // s[1] + 1
    return pads, ho, wo


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs (on the device) and the fp64 (pre, mag) of a case, computed once.
    pre ~ N(3, 4.45^2): quartiles at 0 and 6."""
    shape, k, s, padding = CASES[name]
    pads, ho, wo = geometry(shape, k, s, padding)
    c = shape[3]
    seed = sorted(CASES).index(name) * 10
    x = rnd(*shape, seed=seed + 1).to(BF)
    w = rnd(k[0], k[1], c, scale=4.45 / math.sqrt(k[0] * k[1]), seed=seed + 2)
    b = 3.0 + rnd(c, scale=0.3, seed=seed + 3)
    pre, mag = db.dw_parts(x, w, b, s, pads)
    assert pre.shape == (shape[0], ho, wo, c)
    return (x.to(DEV), w.reshape(k[0] * k[1], c).contiguous().to(DEV), b.to(DEV)), (pre, mag), (pads, ho, wo)


def launch(name, act, strip=0, x=None):
    shape, k, s, _padding = CASES[name]
    (x0, w, b), _parts, (pads, ho, wo) = case(name)
    out = torch.full((shape[0], ho, wo, shape[3]), float("nan"), dtype=BF, device=DEV)
    y = hip().dwconv2d(x0 if x is None else x, w, b, k[0], k[1], s[0], s[1], pads[0], pads[2], ho, wo, ACT[act], out,
                       strip)
    assert y.data_ptr() == out.data_ptr()
    return y


def strips_of(name):
    shape, k, s, _padding = CASES[name]
    _pads, ho, wo = case(name)[2]
    auto = hip().dwconv_strip(shape[0], ho, wo, shape[3], k[0], k[1], s[0], s[1])
    return (0,) if auto == 0 else (0, 2, 8)


@pytest.mark.parametrize("name", sorted(CASES))
def test_dwconv_within_bound(name):
    _k = CASES[name][1]
    _ins, (pre, mag), _geo = case(name)
    taps = _k[0] * _k[1]
    if pre.numel() >= 500:
        # the clamp is exercised on both sides
        lo, hi = (pre < 0).double().mean().item(), (pre > 6).double().mean().item()
        assert 0.12 < lo < 0.38 and 0.12 < hi < 0.38, (lo, hi)
    for act in ACTS:
        ref = db.act64x(act, pre)
        bound = kb.out_bound(ref, (taps + 2) * kb.E * mag, out_f32=False)
        for strip in strips_of(name):
            kb.assert_within(launch(name, act, strip), ref, bound, f"dwconv {name} {act} strip={strip}")


def test_generic_and_strip_cases_take_their_kernels():
    """The case list reaches all three code paths."""
    assert strips_of("generic_5x5") == (0,) and strips_of("generic_stride_2_1") == (0,)
    assert strips_of("many_blocks_s1") == (0, 2, 8) and strips_of("partial_wave_s2") == (0, 2, 8)


@pytest.mark.parametrize("name,pixel", [("h_ne_w_3_chunks", (0, 0, 0)), ("s2_same_odd_even", (0, 0, 0)),
                                        ("explicit", (0, 0, 0)), ("generic_5x5", (0, 0, 0)),
                                        ("generic_stride_2_1", (0, 0, 0)), ("generic_stride_2_1", (0, 4, 5)),
                                        ("many_blocks_s1", (0, 0, 0))])
def test_dwconv_inf_pixel_stays_in_its_windows(name, pixel):
    """+Inf in one input pixel: the outputs whose window does not contain it are
    finite and within the bound (a tap masked by a product with 0 instead of a
    select would turn the clamped neighbour's Inf into NaN)."""
    shape, k, s, _padding = CASES[name]
    (x, _w, _b), (pre, mag), (pads, ho, wo) = case(name)
    xi = x.clone()
    xi[pixel] = float("inf")
    ind = torch.zeros(shape)
    ind[pixel] = 1.0
    touched, _ = db.dw_parts(ind, torch.ones(k[0], k[1], shape[3]), torch.zeros(shape[3]), s, pads)
    clean = touched == 0
    assert clean.any() and (~clean).any()
    for act in ACTS:
        ref = db.act64x(act, pre)
        bound = kb.out_bound(ref, (k[0] * k[1] + 2) * kb.E * mag, out_f32=False)
        for strip in strips_of(name):
            y = launch(name, act, strip, x=xi).float().cpu()
            assert torch.isfinite(y[clean]).all(), f"{name} {act} strip={strip}"
            kb.assert_within(y[clean], ref[clean], bound[clean], f"dwconv inf {name} {act} strip={strip}")


@pytest.mark.parametrize("name", ["h_ne_w_3_chunks", "partial_wave_s2", "generic_5x5"])
def test_dwconv_is_deterministic(name):
    for strip in strips_of(name):
        a, b = launch(name, "relu6", strip), launch(name, "relu6", strip)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_dwconv_binding_rejects_what_the_kernel_does_not_take():
    def call(c=8, k=3, act=0, **kw):
        x = torch.zeros(1, 12, 12, c, dtype=BF, device=DEV)
        w = torch.zeros(k * k, c, device=DEV)
        b = torch.zeros(c, device=DEV)
        p = k // 2
        return hip().dwconv2d(x, w, b, k, k, 1, 1, p, p, 12, 12, act, **kw)
    assert call().shape == (1, 12, 12, 8)
    with pytest.raises(RuntimeError, match="C % 8"):
        call(c=12)
    with pytest.raises(RuntimeError, match="7 x 7"):
        call(k=9)
    for act in (2, 3, 4, 6, -1, 17):            # GELU / tanh are not depthwise epilogues; 6+ are no codes at all
        with pytest.raises(RuntimeError, match="activation"):
            call(act=act)
    with pytest.raises(RuntimeError, match="strip"):
        call(strip=3)
