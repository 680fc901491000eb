"""The 5x5 strip depthwise kernel (kernels/dwconv.hip dwconv5x5_kernel) for
every activation the depthwise kernels take and both strip heights, next to the
generic kernel it replaces on request.

* every case is within the elementwise bound of dwconv_bounds / se_bounds /
  swish_bounds with taps = 25 (EVERY output element, NaN-prefilled buffers);
* its accumulation order is the generic kernel's, so the int16 view of every
  strip form equals the generic kernel's output exactly, for every activation
  (which is what makes switching a model's 5x5 layers to it no change);
* a +Inf pixel stays in the windows that contain it; two launches are bit-equal;
* dwconv_forms answers [0, 2, 4] for these shapes, dwconv_strip still 0, and
  strip 4 on a 3x3 / strip 3 anywhere are rejected.

The shapes are the smallest that reach each path: one live tap; an image smaller
than the filter and the strip with a batch stride; both SAME paddings of stride
2 with Ho = 5 (no multiple of either strip height); VALID; Keras' correct_pad;
two workgroups per output row; 17 chunks (34 half chunks) per pixel with a
partial last workgroup."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import dwconv_bounds as db  # noqa: E402
import kernel_bounds as kb  # noqa: E402
import se_bounds as sb  # noqa: E402
import swish_bounds as wb  # noqa: E402
from kernel_bounds import BF, rnd  # noqa: E402
from rust_tensorflow_serving2_amd.graph.ops import tf_same_pads  # noqa: E402
from rust_tensorflow_serving2_amd.ops import ACT, hip  # noqa: E402

DEV = torch.device("cuda:0")
ACTS = ("none", "relu", "relu6", "hard_swish", "swish")
STRIPS = (0, 2, 4)
SPREAD = 3.0
TAPS = 25

# (n, h, w, c), stride, padding
CASES = {
    "centre_tap_only": ((1, 1, 1, 8), 1, "SAME"),
    "smaller_than_filter": ((2, 3, 2, 24), 1, "SAME"),
    "s2_same_odd_even": ((1, 9, 12, 8), 2, "SAME"),
    "s2_same_even_odd": ((1, 10, 11, 8), 2, "SAME"),
    "valid": ((1, 8, 8, 16), 1, "VALID"),
    "s2_correct_pad": ((1, 12, 12, 8), 2, (1, 2, 1, 2)),
    "two_workgroups_s1": ((3, 20, 20, 64), 1, "SAME"),
    "partial_workgroup_s2": ((2, 17, 17, 136), 2, "SAME"),
}


def geometry(shape, s, padding):
    _n, h, w, _c = shape
    if padding == "SAME":
        pads = tf_same_pads(h, 5, s) + tf_same_pads(w, 5, s)
    elif padding == "VALID":
        pads = (0, 0, 0, 0)
    else:
        pads = tuple(padding)
    return pads, (h + pads[0] + pads[1] - 5) // s + 1, (w + pads[2] + pads[3] - 5) // s + 1


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs (on the device) and the fp64 (pre, mag) of a case, computed once;
    pre ~ N(0, 3^2) over the whole output (test_hard_swish_gpu's scaling)."""
    shape, s, padding = CASES[name]
    pads, ho, wo = geometry(shape, s, padding)
    c = shape[3]
    seed = sorted(CASES).index(name) * 10 + 900
    x = rnd(*shape, seed=seed + 1).to(BF)
    w = rnd(5, 5, c, scale=SPREAD / 5.0, seed=seed + 2)
    b = rnd(c, scale=0.3, seed=seed + 3)
    if shape[1] * shape[2] > 1:
        w = w * (SPREAD / max(db.dw_parts(x, w, 0 * b, s, pads)[0].std().item(), 1e-3))
    pre, mag = db.dw_parts(x, w, b, s, pads)
    assert pre.shape == (shape[0], ho, wo, c)
    return (x.to(DEV), w.reshape(25, c).contiguous().to(DEV), b.to(DEV)), (pre, mag), (pads, ho, wo)


def ref_bound(act, pre, mag):
    if act == "hard_swish":
        return sb.hard_swish_dw(pre, mag, TAPS)
    if act == "swish":
        return wb.swish_dw(pre, mag, TAPS)
    ref = db.act64x(act, pre)
    return ref, kb.out_bound(ref, (TAPS + 2) * kb.E * mag, out_f32=False)


def launch(name, act, strip, x=None):
    shape, s, _padding = CASES[name]
    (x0, w, b), _parts, (pads, ho, wo) = case(name)
    out = torch.full((shape[0], ho, wo, shape[3]), float("nan"), dtype=BF, device=DEV)
    y = hip().dwconv2d(x0 if x is None else x, w, b, 5, 5, s, s, pads[0], pads[2], ho, wo, ACT[act], out, strip)
    assert y.data_ptr() == out.data_ptr()
    return y


def test_geometries_are_the_ones_meant():
    assert geometry(*CASES["s2_same_odd_even"]) == ((2, 2, 1, 2), 5, 6)
    assert geometry(*CASES["s2_same_even_odd"]) == ((1, 2, 2, 2), 5, 6)
    assert geometry(*CASES["s2_correct_pad"]) == ((1, 2, 1, 2), 6, 6)
    assert geometry(*CASES["partial_workgroup_s2"])[1:] == (9, 9) and 9 * (136 // 4) == 306      # 256 + 50
    assert geometry(*CASES["two_workgroups_s1"])[1:] == (20, 20) and 20 * (64 // 4) == 320


@pytest.mark.parametrize("name", sorted(CASES))
def test_dwconv5x5_within_bound_and_bit_equal_to_the_generic_kernel(name):
    _ins, (pre, mag), _geo = case(name)
    if pre.numel() >= 500:
        lo, hi = (pre < -3).double().mean().item(), (pre > 3).double().mean().item()
        assert 0.10 < lo < 0.25 and 0.10 < hi < 0.25, (lo, hi)
    worst = 0.0
    for act in ACTS:
        ref, bound = ref_bound(act, pre, mag)
        generic = launch(name, act, 0)
        for strip in STRIPS:
            y = generic if strip == 0 else launch(name, act, strip)
            worst = max(worst, kb.assert_within(y, ref, bound, f"dwconv5x5 {name} {act} strip={strip}"))
            assert torch.equal(y.view(torch.int16), generic.view(torch.int16)), f"{name} {act} strip={strip}"
    print(f"dwconv5x5 {name}: worst err / bound = {worst:.3f}")


@pytest.mark.parametrize("name,pixel", [("smaller_than_filter", (0, 0, 0)), ("s2_same_odd_even", (0, 0, 0)),
                                        ("s2_same_even_odd", (0, 9, 10)), ("s2_correct_pad", (0, 5, 6)),
                                        ("two_workgroups_s1", (1, 10, 0)), ("partial_workgroup_s2", (1, 16, 16))])
def test_dwconv5x5_inf_pixel_stays_in_its_windows(name, pixel):
    """+Inf in one input pixel: the outputs whose window does not contain it are
    finite and within the bound (a tap masked by a product with 0 instead of a
    select would turn the clamped neighbour's Inf into NaN)."""
    shape, s, _padding = CASES[name]
    (x, _w, _b), (pre, mag), (pads, _ho, _wo) = case(name)
    xi = x.clone()
    xi[pixel] = float("inf")
    ind = torch.zeros(shape)
    ind[pixel] = 1.0
    touched, _ = db.dw_parts(ind, torch.ones(5, 5, shape[3]), torch.zeros(shape[3]), s, pads)
    clean = touched == 0
    assert clean.any() and (~clean).any()
    for act in ACTS:
        ref, bound = ref_bound(act, pre, mag)
        for strip in STRIPS:
            y = launch(name, act, strip, x=xi).float().cpu()
            assert torch.isfinite(y[clean]).all(), f"{name} {act} strip={strip}"
            kb.assert_within(y[clean], ref[clean], bound[clean], f"dwconv5x5 inf {name} {act} strip={strip}")


@pytest.mark.parametrize("name", ["smaller_than_filter", "two_workgroups_s1", "partial_workgroup_s2"])
def test_dwconv5x5_is_deterministic(name):
    for strip in STRIPS:
        a, b = launch(name, "swish", strip), launch(name, "swish", strip)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_forms_and_the_auto_rule():
    H = hip()
    for name, (shape, s, padding) in CASES.items():
        _pads, ho, wo = geometry(shape, s, padding)
        assert H.dwconv_forms(shape[0], ho, wo, shape[3], 5, 5, s, s) == [0, 2, 4], name
        assert H.dwconv_strip(shape[0], ho, wo, shape[3], 5, 5, s, s) == 0, name
    assert H.dwconv_forms(1, 12, 12, 8, 3, 3, 1, 1) == [0, 2, 8] and H.dwconv_forms(2, 17, 17, 136, 3, 3, 2, 2) == [0, 2, 8]
    for k, s in (((5, 5), (2, 1)), ((5, 5), (3, 3)), ((5, 3), (1, 1)), ((7, 7), (1, 1)), ((3, 3), (1, 2)), ((1, 1), (1, 1))):
        assert H.dwconv_forms(1, 12, 12, 8, k[0], k[1], s[0], s[1]) == [0], (k, s)


def test_strip_values_the_binding_rejects():
    def call(k=5, s=1, **kw):
        x = torch.zeros(1, 12, 12, 8, dtype=BF, device=DEV)
        p = k // 2
        ho = (12 + 2 * p - k) // s + 1
        return hip().dwconv2d(x, torch.zeros(k * k, 8, device=DEV), torch.zeros(8, device=DEV), k, k, s, s, p, p, ho, ho,
                              0, **kw)
    for strip in (0, 2, 4, 8):                  # (8 on a 5x5 has always meant the generic kernel)
        assert call(strip=strip).shape == (1, 12, 12, 8)
    assert call(s=2, strip=4).shape == (1, 6, 6, 8)
    for kw in (dict(k=3, strip=4), dict(k=7, strip=4), dict(k=5, s=3, strip=4), dict(strip=3), dict(k=3, strip=3),
               dict(strip=1), dict(strip=5)):
        with pytest.raises(RuntimeError, match="strip"):
            call(**kw)
