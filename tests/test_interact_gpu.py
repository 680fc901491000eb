"""dot_interaction (kernels/interact.hip) against the fp64 reference and bound of
tests/interact_bounds.py.  Z and out are views into NaN-filled buffers with
guard bands; the guards must still be NaN afterwards and every column of out,
the zero tail included, must have been written."""
import pytest
import torch

import interact_bounds as ib
import kernel_bounds as kb

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

BF = torch.bfloat16
NAN = float("nan")
GUARD = 1024


def hip():
    from rust_tensorflow_serving2_amd.ops import hip as _hip
    return _hip()


def launch(z, dense=None, k=-1, pad=0):
    """-> (y [B, Wp], guards intact); Z and out are views into NaN-filled buffers."""
    b, f, _d = z.shape
    dd = 0 if dense is None else dense.shape[1]
    wp = ib.width(f, dd, pad, k)
    assert hip().dot_interaction_width(f, dd, pad, k == 0) == wp
    big_z = torch.full((GUARD + z.numel() + GUARD,), NAN, dtype=BF, device="cuda")
    big_z[GUARD:GUARD + z.numel()] = z.cuda().reshape(-1)
    n = b * wp
    big_y = torch.full((GUARD + n + GUARD,), NAN, dtype=BF, device="cuda")
    out = big_y[GUARD:GUARD + n].view(b, wp)
    y = hip().dot_interaction(big_z[GUARD:GUARD + z.numel()].view(z.shape), None if dense is None else dense.cuda(),
                              k == 0, pad, out)
    assert y.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return y, bool(torch.isnan(big_y[:GUARD]).all() and torch.isnan(big_y[GUARD + n:]).all())


def check(z, dense, k, pad, what):
    y, intact = launch(z, dense, k, pad)
    assert intact, f"{what}: a guard element was written"
    ref, bound = ib.interact_ref(z, dense, k, pad)
    worst = ib.assert_within_where_finite(y, ref, bound, what)
    dd = 0 if dense is None else dense.shape[1]
    tail = y[:, dd + ib.pair_count(z.shape[1], k):].cpu()
    assert torch.equal(tail.view(torch.int16), torch.zeros_like(tail).view(torch.int16)), f"{what}: the tail is not +0"
    if dense is not None:
        assert torch.equal(y[:, :dd].cpu().view(torch.int16), dense.view(torch.int16))
    return y, worst


@pytest.mark.parametrize("k", [-1, 0])
@pytest.mark.parametrize("d", [32, 128, 256])
@pytest.mark.parametrize("f", [2, 15, 16, 17, 27, 32])
def test_dot_interaction_within_bound(f, d, k):
    """B = 3; without dense and pad, and with a 24-wide dense at pad 1 and 7."""
    z = kb.rnd(3, f, d, seed=f * 7 + d).to(BF)
    dense = kb.rnd(3, 24, seed=f).to(BF)
    assert hip().dot_interaction_supported(3, f, d, 24, 7, k == 0)
    for dn, pad in ((None, 0), (dense, 1), (dense, 7)):
        _y, worst = check(z, dn, k, pad, f"dot_interaction F={f} D={d} k={k} pad={pad}")
        print(f"dot_interaction F={f} D={d} k={k} dense={dn is not None} pad={pad}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("b", [1, 1025])
@pytest.mark.parametrize("f,d,dd", [(27, 128, 128), (16, 32, 8)])
def test_batches(b, f, d, dd):
    """One sample, and 257 workgroups with a last one of a single live wave."""
    z = kb.rnd(b, f, d, seed=b + f).to(BF)
    dense = kb.rnd(b, dd, seed=3).to(BF)
    check(z, dense, -1, 1, f"dot_interaction B={b} F={f} D={d}")


@pytest.mark.parametrize("poison", [float("inf"), NAN])
@pytest.mark.parametrize("f", [5, 27])
def test_non_finite_rows_stay_in_their_own_pairs(f, poison):
    """A feature row of +Inf / NaN in sample 1 and all of sample 3, beside clean samples: the output
    is non-finite exactly where the reference is."""
    z = kb.rnd(5, f, 64, seed=f).to(BF)
    z[1, f // 2] = poison
    z[3] = poison
    dense = kb.rnd(5, 8, seed=2).to(BF)
    y, _ = check(z, dense, -1, 3, f"poisoned F={f}")
    clean, _ = check(kb.rnd(5, f, 64, seed=f).to(BF), dense, -1, 3, "clean")
    for s in (0, 2, 4):
        assert torch.equal(y[s].view(torch.int16), clean[s].view(torch.int16))
    bad = sum(1 for i, j in ib.tril_pairs(f, -1) if f // 2 in (i, j))
    assert int((~torch.isfinite(y[1].float())).sum()) == bad


def test_reruns_are_bit_equal():
    z = kb.rnd(130, 27, 128, seed=1).to(BF)
    dense = kb.rnd(130, 128, seed=2).to(BF)
    runs = [launch(z, dense, -1, 1)[0].view(torch.int16).clone() for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def test_dot_interaction_rejections():
    H = hip()
    z = torch.zeros(2, 4, 32, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError, match="2 <= F <= 32"):
        H.dot_interaction(torch.zeros(2, 33, 32, dtype=BF, device="cuda"))
    with pytest.raises(RuntimeError, match="2 <= F <= 32"):
        H.dot_interaction(torch.zeros(2, 1, 32, dtype=BF, device="cuda"))
    with pytest.raises(RuntimeError, match="D must be a multiple of 32"):
        H.dot_interaction(torch.zeros(2, 4, 48, dtype=BF, device="cuda"))
    with pytest.raises(RuntimeError, match="D must be a multiple of 32"):
        H.dot_interaction(torch.zeros(2, 4, 288, dtype=BF, device="cuda"))
    with pytest.raises(RuntimeError, match="Dd % 8"):
        H.dot_interaction(z, torch.zeros(2, 12, dtype=BF, device="cuda"))
    with pytest.raises(RuntimeError, match=r"dense must be \[2, Dd\]"):
        H.dot_interaction(z, torch.zeros(3, 8, dtype=BF, device="cuda"))
    with pytest.raises(RuntimeError, match="pad must be"):
        H.dot_interaction(z, None, False, -1)
    with pytest.raises(RuntimeError, match="exceed"):
        H.dot_interaction(z, None, False, 2000)
    with pytest.raises(RuntimeError, match="expected"):
        H.dot_interaction(z.float())
    with pytest.raises(RuntimeError, match="z must be 16-byte aligned"):
        big = torch.zeros(z.numel() + 8, dtype=BF, device="cuda")
        H.dot_interaction(big[1:1 + z.numel()].view(2, 4, 32))
    with pytest.raises(RuntimeError, match="wrong size"):
        H.dot_interaction(z, None, False, 0, torch.zeros(2, 6, dtype=BF, device="cuda"))
    with pytest.raises(RuntimeError, match="out must be 16-byte aligned"):
        big = torch.zeros(2 * 8 + 8, dtype=BF, device="cuda")
        H.dot_interaction(z, None, False, 0, big[1:17].view(2, 8))
    assert not H.dot_interaction_supported(2, 33, 32)
    assert not H.dot_interaction_supported(2, 4, 48)
    assert not H.dot_interaction_supported(2, 4, 32, 12)
    assert H.dot_interaction_supported(2, 4, 32, 8, 1, True)
