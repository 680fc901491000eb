"""The DLRM kernels' bounds (tests/interact_bounds.py) on the CPU: the kernels'
arithmetic emulated in torch meets them; three wrong schemes do not (a bf16
rounding of every hot row's partial sum, the upper-triangle order, a clamped and
zeroed invalid id next to an Inf row); the index formula is np.tril_indices."""
import numpy as np
import pytest
import torch

import interact_bounds as ib
import kernel_bounds as kb

BF = torch.bfloat16
VOCAB, HOT = (1, 9, 40, 5), (1, 2, 5, 64)


@pytest.mark.parametrize("d", [8, 24, 128])
@pytest.mark.parametrize("with_dense", [False, True])
def test_embag_emulation_meets_the_bound(d, with_dense):
    ids, tables = ib.embag_inputs(5, VOCAB, HOT, d, seed=d)
    dense = kb.rnd(5, d, seed=3).to(BF) if with_dense else None
    ref, bound = ib.embag_ref(ids, tables, HOT, dense)
    y = ib.embag_emulate(ids, tables, HOT, dense)
    assert y.shape == (5, len(VOCAB) + int(with_dense), d)
    worst = kb.assert_within(y, ref, bound, f"embag emulation D={d}")
    assert 0.5 < worst <= 1.0                                    # the rounding itself comes close to 2^-8 |ref|
    if with_dense:
        assert torch.equal(y[:, 0], dense)
    # L = 1 (feature 0, a one-row table): the table row itself
    assert torch.equal(y[:, int(with_dense)], tables[0][0].expand(5, d))


def test_embag_invalid_ids_add_zeros():
    ids, tables = ib.embag_inputs(6, VOCAB, HOT, 16, seed=1)
    ids[1, 0] = -1
    ids[2, 1] = VOCAB[1]
    ids[3, 3] = 2 ** 32 + 1
    ids[4, 8:] = -7                                              # a bag of invalid ids only
    ref, bound = ib.embag_ref(ids, tables, HOT)
    assert torch.equal(ref[1, 0], torch.zeros(16, dtype=torch.float64))
    assert torch.equal(ref[4, 3], torch.zeros(16, dtype=torch.float64))
    kb.assert_within(ib.embag_emulate(ids, tables, HOT), ref, bound, "invalid ids")


def test_rounding_every_partial_sum_violates_the_bound():
    ids, tables = ib.embag_inputs(32, VOCAB, HOT, 64, seed=2)
    ref, bound = ib.embag_ref(ids, tables, HOT)
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within(ib.embag_emulate(ids, tables, HOT, round_partials=True), ref, bound, "rounded partial sums")


def test_clamped_and_zeroed_id_next_to_inf_is_nan():
    """Row 0 and row V - 1 of a table hold +Inf; ids -1 and V select nothing.  Reading the clamped
    row and multiplying by 0 gives NaN, which the checker rejects; the select gives zeros."""
    ids, tables = ib.embag_inputs(4, (6, 6), (2, 1), 8, seed=4)
    for t in tables:
        t[0] = float("inf")
        t[-1] = float("inf")
    ids[:, 0] = torch.tensor([1, 2, 3, 4])
    ids[:, 1] = torch.tensor([-1, 6, 2 ** 32 + 1, 2])
    ids[:, 2] = torch.tensor([-1, 6, 3, 2 ** 40])
    ref, bound = ib.embag_ref(ids, tables, (2, 1))
    assert torch.isfinite(ref).all()
    kb.assert_within(ib.embag_emulate(ids, tables, (2, 1)), ref, bound, "select")
    bad = ib.embag_emulate(ids, tables, (2, 1), clamp_and_zero=True)
    assert torch.isnan(bad.float()).any()
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within(bad, ref, bound, "clamp and zero")


@pytest.mark.parametrize("f", [2, 15, 16, 17, 27, 32])
@pytest.mark.parametrize("k", [-1, 0])
def test_index_formula_is_tril_indices(f, k):
    ii, jj = np.tril_indices(f, k)
    assert ib.tril_pairs(f, k) == list(zip(ii.tolist(), jj.tolist()))
    assert ib.pair_count(f, k) == len(ii)
    from rust_tensorflow_serving2_amd.graph.patterns import tril_pairs
    assert tril_pairs(f, k) == (ii * f + jj).tolist()


@pytest.mark.parametrize("f,d", [(2, 32), (17, 128), (27, 128), (32, 256)])
@pytest.mark.parametrize("k", [-1, 0])
def test_interact_emulation_meets_the_bound(f, d, k):
    z = kb.rnd(3, f, d, seed=f + d).to(BF)
    dense = kb.rnd(3, 16, seed=5).to(BF)
    for dn, pad in ((None, 0), (dense, 1), (dense, 7)):
        ref, bound = ib.interact_ref(z, dn, k, pad)
        y = ib.interact_emulate(z, dn, k, pad)
        assert y.shape == ref.shape and ref.shape[1] % 8 == 0
        worst = kb.assert_within(y, ref, bound, f"interaction emulation F={f} D={d} k={k}")
        assert worst <= 1.0
        dd = 0 if dn is None else 16
        assert torch.equal(y[:, dd + ib.pair_count(f, k):].float(), torch.zeros(3, ref.shape[1] - dd - ib.pair_count(f, k)))


def test_upper_triangle_order_violates_the_bound():
    z = kb.rnd(3, 6, 32, seed=9).to(BF)
    ref, bound = ib.interact_ref(z, None, -1, 0)
    with pytest.raises(AssertionError, match="outside the bound"):
        kb.assert_within(ib.interact_emulate(z, None, -1, 0, upper=True), ref, bound, "upper triangle")


def test_inf_row_reaches_its_own_pairs_only():
    z = kb.rnd(2, 5, 32, seed=10).to(BF)
    z[1, 2] = float("inf")
    ref, bound = ib.interact_ref(z, None, -1, 0)
    bad = {p for p, (i, j) in enumerate(ib.tril_pairs(5, -1)) if 2 in (i, j)}
    assert torch.isfinite(ref[0]).all()
    assert {int(p) for p in (~torch.isfinite(ref[1])).nonzero().reshape(-1)} == bad
    ib.assert_within_where_finite(ib.interact_emulate(z, None, -1, 0), ref, bound, "Inf row")
