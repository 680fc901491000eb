"""The fused depthwise 7x7 + bias + LayerNorm kernel (kernels/dwln.hip) against
the elementwise bound of dwln_bounds, EVERY output element, NaN-prefilled
buffers.  test_dwln_bounds_cpu.py shows that the bound rejects a conv result
rounded to bf16 before the statistics.

The shapes are the smallest that reach each path: every channel count class (one
chunk; chunk counts that are no power of two; the four ConvNeXt-T widths; the
most the kernel takes, two columns per workgroup), maps smaller than the
filter's reach, maps that are no multiple of the column tile or of either tile
height, the three paddings, both tile heights (the launcher picks 4 rows from
1024 workgroups on, else 2)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import dwln_bounds as lb  # noqa: E402
import kernel_bounds as kb  # noqa: E402
from kernel_bounds import BF, rnd  # noqa: E402
from rust_tensorflow_serving2_amd.ops import hip  # noqa: E402

DEV = torch.device("cuda:0")
MAXC = int(hip().dwconv_ln_max_c)

# (n, h, w, c), pads (top, bottom, left, right), eps
CASES = {f"c{c}_9x11": ((2, 9, 11, c), lb.SAME, 1e-6) for c in (8, 40, 96, 104, 192, 384, 768, MAXC)}
CASES.update({
    "c768_7x7": ((1, 7, 7, 768), lb.SAME, 1e-6),
    "map_1x1": ((2, 1, 1, 96), lb.SAME, 1e-6),
    "map_2x2": ((2, 2, 2, 768), lb.SAME, 1e-6),
    "map_3x5": ((2, 3, 5, 8), lb.SAME, 1e-6),
    "map_7x7": ((2, 7, 7, 192), lb.SAME, 1e-6),
    "c96_20x23": ((1, 20, 23, 96), lb.SAME, 1e-6),
    "c384_15x13": ((1, 15, 13, 384), lb.SAME, 1e-6),
    "valid": ((2, 10, 9, 40), lb.VALID, 1e-6),
    "valid_c96": ((1, 13, 12, 96), lb.VALID, 1e-6),
    "explicit_2_1": ((1, 11, 12, 96), (2, 1, 2, 1), 1e-6),
    "eps_1e-3": ((1, 14, 14, 384), lb.SAME, 1e-3),
    "tall_tiles": ((171, 9, 11, 192), lb.SAME, 1e-6),            # 1026 workgroups: 4-row tiles, 9 rows = 2 1/4 tiles
})


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs (on the device) and the fp64 (ref, bound) of a case, computed once."""
    shape, pads, eps = CASES[name]
    c = shape[3]
    seed = sorted(CASES).index(name) * 10 + 1500
    x = rnd(*shape, seed=seed + 1).to(BF)
    w = rnd(7, 7, c, scale=1.0 / 7.0, seed=seed + 2)
    b = rnd(c, scale=0.3, seed=seed + 3)
    gamma = 1.0 + rnd(c, scale=0.2, seed=seed + 4)
    beta = rnd(c, scale=0.2, seed=seed + 5)
    ref, bound = lb.dwln_ref(x, w, b, gamma, beta, eps, pads)
    ho, wo = lb.out_hw(shape[1], shape[2], pads)
    assert ref.shape == (shape[0], ho, wo, c)
    dev = tuple(t.to(DEV) for t in (x, w.reshape(49, c).contiguous(), b, gamma, beta))
    return dev, (ref, bound), (ho, wo)


def launch(name, x=None):
    shape, pads, eps = CASES[name]
    (x0, w, b, gamma, beta), _rb, (ho, wo) = case(name)
    out = torch.full((shape[0], ho, wo, shape[3]), float("nan"), dtype=BF, device=DEV)
    y = hip().dwconv_ln(x0 if x is None else x, w, b, gamma, beta, eps, pads[0], pads[2], ho, wo, out)
    assert y.data_ptr() == out.data_ptr()
    return y


def test_geometries_are_the_ones_meant():
    """Workgroup counts: 256 / (C / 8) columns at most per workgroup, in equal
    tiles; 4 rows per workgroup from 1024 workgroups on, else 2."""
    H = hip()
    assert MAXC >= 768 and MAXC % 8 == 0
    assert H.dwconv_ln_grid(2, 9, 11, 8) == 2 * 5 * 1                 # 32 columns fit: one tile, 2-row tiles
    assert H.dwconv_ln_grid(2, 9, 11, 104) == 2 * 5 * 1               # 19 columns fit
    assert H.dwconv_ln_grid(2, 9, 11, 192) == 2 * 5 * 2               # 10 columns fit: tiles of 6 and 5
    assert H.dwconv_ln_grid(2, 9, 11, MAXC) == 2 * 5 * -(-11 // (2048 // MAXC))
    assert H.dwconv_ln_grid(1, 20, 23, 96) == 10 * 2                  # 21 fit: tiles of 12 and 11
    assert H.dwconv_ln_grid(1, 15, 13, 384) == 8 * 3                  # 5 fit: tiles of 5, 5 and 3
    assert H.dwconv_ln_grid(170, 9, 11, 192) == 170 * 5 * 2           # 4-row tiles would be 1020 workgroups
    assert H.dwconv_ln_grid(171, 9, 11, 192) == 171 * 3 * 2           # 1026: 4-row tiles
    assert H.dwconv_ln_grid(1, 7, 7, 768) == 4 * 4
    assert H.dwconv_ln_grid(0, 7, 7, 768) == 0 and H.dwconv_ln_grid(1, 7, 7, 12) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_dwln_within_bound(name):
    _ins, (ref, bound), _geo = case(name)
    y = launch(name)
    worst = kb.assert_within(y, ref, bound, f"dwconv_ln {name}")
    print(f"dwconv_ln {name}: worst err / bound = {worst:.3f}")


def test_constant_pixels_give_beta_exactly():
    """x = 0 and a constant bias: every channel of every pixel is equal after the
    conv, the centred values are exactly 0, and the output is bf16(beta)
    whatever eps (rstd is 1000 at eps 1e-6) and gamma are."""
    c = 96
    x = torch.zeros(2, 5, 6, c, dtype=BF, device=DEV)
    w = rnd(49, c, seed=1).to(DEV)
    gamma, beta = rnd(c, seed=2).to(DEV), rnd(c, seed=3).to(DEV)
    for eps in (1e-6, 1e-3):
        out = torch.full((2, 5, 6, c), float("nan"), dtype=BF, device=DEV)
        y = hip().dwconv_ln(x, w, torch.full((c,), 0.75, device=DEV), gamma, beta, eps, 3, 3, 5, 6, out)
        assert torch.equal(y.view(torch.int16), beta.to(BF).expand(2, 5, 6, c).contiguous().view(torch.int16)), eps


@pytest.mark.parametrize("name,pixel", [("c96_20x23", (0, 0, 0)), ("c96_20x23", (0, 9, 12)),
                                        ("tall_tiles", (1, 0, 0)), ("tall_tiles", (1, 4, 5)),
                                        ("c384_15x13", (0, 14, 12)), ("c384_15x13", (0, 7, 6))])
def test_inf_pixel_stays_in_its_windows(name, pixel):
    """+Inf in one channel of one pixel: every output pixel more than 3 rows or
    columns away, and every other image, equals the clean run bit for bit (a
    tap masked by a product with 0 instead of a select would turn the clamped
    neighbour's Inf into NaN; a statistic shared between pixels would spread
    it).  The pixels within reach may be NaN."""
    shape, _pads, _eps = CASES[name]
    (x, *_rest), _rb, _geo = case(name)
    clean = launch(name)
    xi = x.clone()
    xi[pixel + (5,)] = float("inf")
    y = launch(name, x=xi)
    n, h, w = pixel
    hh = torch.arange(shape[1]).view(-1, 1)
    ww = torch.arange(shape[2]).view(1, -1)
    far = ((hh - h).abs() > 3) | ((ww - w).abs() > 3)
    mask = torch.ones(shape[:3], dtype=torch.bool)
    mask[n] = far
    assert mask.any() and (~mask).any()
    mask = mask.to(DEV)
    assert torch.equal(y.view(torch.int16)[mask], clean.view(torch.int16)[mask])
    assert not torch.isfinite(y.float()[~mask]).all()          # (the Inf did arrive)


@pytest.mark.parametrize("name", ["c40_9x11", "c384_15x13", "tall_tiles"])
def test_no_stray_writes(name):
    """`out` is a slice of a larger NaN-filled buffer: the guard elements before
    and after it stay NaN, and every element of `out` is written."""
    shape, pads, eps = CASES[name]
    (x, w, b, gamma, beta), (ref, bound), (ho, wo) = case(name)
    numel = shape[0] * ho * wo * shape[3]
    guard = 4096
    buf = torch.full((numel + 2 * guard,), float("nan"), dtype=BF, device=DEV)
    out = buf[guard:guard + numel].view(shape[0], ho, wo, shape[3])
    y = hip().dwconv_ln(x, w, b, gamma, beta, eps, pads[0], pads[2], ho, wo, out)
    kb.assert_within(y, ref, bound, f"dwconv_ln guarded {name}")
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + numel:]).all()


@pytest.mark.parametrize("name", ["c104_9x11", "c768_7x7", "tall_tiles"])
def test_two_runs_are_bit_equal(name):
    a, b = launch(name), launch(name)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("rows", [2, 4])
def test_more_workgroups_than_the_machine_holds_at_once(rows):
    """N x 48 x 48 x 96: 16-column tiles, 3 per row.  A workgroup is one wave on
    each of a CU's 4 SIMDs, so a CU holds as many workgroups as a SIMD holds
    waves of the kernel (profiles/convnext/resources.txt):

    * 2-row tiles (72 workgroups per image): 239 VGPRs, 2 waves of the 512 /
      240, 4 KB of LDS (40 per 160 KB): 2 per CU, 512 on 256 CUs.  N = 8 is
      the smallest batch beyond that (576 workgroups);
    * 4-row tiles (36 per image, from 1024 workgroups on): 123 VGPRs, 4 waves
      of the 512 / 128, 8 KB of LDS (20): 4 per CU, 1024.  N = 29 is the first
      batch with 4-row tiles (1044 workgroups), and already beyond it.

    Either way the last workgroups start only when earlier ones have left."""
    H = hip()
    per_image = {2: 72, 4: 36}
    resident = {2: 256 * 2, 4: 256 * 4}

    def rows_of(n):
        return next(r for r in (2, 4) if H.dwconv_ln_grid(n, 48, 48, 96) == n * per_image[r])
    n = next(n for n in range(1, 64) if rows_of(n) == rows and H.dwconv_ln_grid(n, 48, 48, 96) > resident[rows])
    assert (n, H.dwconv_ln_grid(n, 48, 48, 96)) == {2: (8, 576), 4: (29, 1044)}[rows]
    c = 96
    x = rnd(n, 48, 48, c, seed=11).to(BF)
    w = rnd(7, 7, c, scale=1.0 / 7.0, seed=12)
    b, gamma, beta = rnd(c, scale=0.3, seed=13), 1.0 + rnd(c, scale=0.2, seed=14), rnd(c, scale=0.2, seed=15)
    ref, bound = lb.dwln_ref(x, w, b, gamma, beta, 1e-6, lb.SAME)
    out = torch.full((n, 48, 48, c), float("nan"), dtype=BF, device=DEV)
    y = H.dwconv_ln(x.to(DEV), w.reshape(49, c).to(DEV), b.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-6, 3, 3, 48, 48,
                    out)
    worst = kb.assert_within(y, ref, bound, f"dwconv_ln {n} x 48 x 48 x 96")
    print(f"dwconv_ln {n}x48x48x96: worst err / bound = {worst:.3f}")


def test_what_the_binding_rejects():
    H = hip()

    def call(c=96, k=7, s=1, x=None, glen=None, **kw):
        x = torch.zeros(1, 8, 8, c, dtype=BF, device=DEV) if x is None else x
        g = torch.ones(c if glen is None else glen, device=DEV)
        return H.dwconv_ln(x, torch.zeros(k * k, c, device=DEV), torch.zeros(c, device=DEV), g,
                           torch.zeros(c, device=DEV), 1e-6, 3, 3, 8, 8, kh=k, kw=k, sh=s, sw=s, **kw)
    assert call().shape == (1, 8, 8, 96)
    with pytest.raises(RuntimeError, match="C % 8 == 0 and 8 <= C <="):
        call(c=12)
    with pytest.raises(RuntimeError, match=f"8 <= C <= {MAXC}"):
        call(c=MAXC + 8)
    with pytest.raises(RuntimeError, match="the filter is 7 x 7"):
        call(k=5)
    with pytest.raises(RuntimeError, match="the stride is 1"):
        call(s=2)
    with pytest.raises(RuntimeError, match="16-B aligned"):
        call(x=torch.zeros(8 * 8 * 96 + 8, dtype=BF, device=DEV)[4:4 + 8 * 8 * 96].view(1, 8, 8, 96))
    with pytest.raises(RuntimeError, match="gamma and beta must have C entries"):
        call(glen=48)
    assert not H.dwconv_ln_supported(1, 8, 8, 12, 7, 7, 1, 1) and not H.dwconv_ln_supported(1, 8, 8, MAXC + 8, 7, 7, 1, 1)
    assert not H.dwconv_ln_supported(1, 8, 8, 96, 5, 5, 1, 1) and not H.dwconv_ln_supported(1, 4, 4, 96, 7, 7, 2, 2)
    assert H.dwconv_ln_supported(32, 56, 56, 96, 7, 7, 1, 1) and H.dwconv_ln_supported(1, 7, 7, MAXC, 7, 7, 1, 1)
