"""embedding_bag (kernels/embag.hip) against the fp64 reference and bound of
tests/interact_bounds.py.  Every output is a view into a NaN-filled buffer with
guard bands, which must still be NaN afterwards."""
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
VOCAB, HOT = (1, 9, 40, 70), (1, 2, 5, 64)          # mixed hotness in one launch, a one-row table


def hip():
    from rust_tensorflow_serving2_amd.ops import hip as _hip
    return _hip()


def features(vocab, hot):
    flat, base, first = [], 0, 0
    for v, l in zip(vocab, hot):
        flat += [base, v, first, l]
        base += v
        first += l
    return flat


def launch(ids, tables, hot, dense=None, flat=None):
    """-> (y, guards intact) with y a view into a NaN-filled buffer."""
    b, d = ids.shape[0], tables[0].shape[1]
    flat = features([t.shape[0] for t in tables], hot) if flat is None else flat
    n = b * (len(tables) + (dense is not None)) * d
    big = torch.full((GUARD + n + GUARD,), NAN, dtype=BF, device="cuda")
    out = big[GUARD:GUARD + n].view(b, -1, d)
    feat = torch.tensor(flat, dtype=torch.int64).view(-1, 4).cuda()
    y = hip().embedding_bag(ids.cuda(), torch.cat(tables).cuda(), feat, flat, None if dense is None else dense.cuda(), out)
    assert y.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return y, bool(torch.isnan(big[:GUARD]).all() and torch.isnan(big[GUARD + n:]).all())


@pytest.mark.parametrize("with_dense", [False, True])
@pytest.mark.parametrize("b", [1, 3, 257])
@pytest.mark.parametrize("d", [8, 24, 128, 1024])
def test_embedding_bag_within_bound(d, b, with_dense):
    ids, tables = ib.embag_inputs(b, VOCAB, HOT, d, seed=d + b)
    dense = kb.rnd(b, d, seed=5).to(BF) if with_dense else None
    assert hip().embedding_bag_supported(b, ids.shape[1], d, features(VOCAB, HOT), sum(VOCAB), with_dense, True)
    y, intact = launch(ids, tables, HOT, dense)
    assert intact, "a guard element was written"
    ref, bound = ib.embag_ref(ids, tables, HOT, dense)
    worst = kb.assert_within(y, ref, bound, f"embedding_bag B={b} D={d} dense={with_dense}")
    print(f"embedding_bag B={b} D={d} dense={with_dense}: worst err/bound {worst:.3f}")
    if with_dense:
        assert torch.equal(y[:, 0].cpu(), dense)


def test_int32_ids_equal_int64_ids():
    ids, tables = ib.embag_inputs(3, VOCAB, HOT, 24, seed=1)
    ids[1, 2] = -1
    ids[2, 5] = 40
    a, ok_a = launch(ids, tables, HOT)
    b, ok_b = launch(ids.to(torch.int32), tables, HOT)
    assert ok_a and ok_b and torch.equal(a.view(torch.int16), b.view(torch.int16))
    ref, bound = ib.embag_ref(ids, tables, HOT)
    kb.assert_within(b, ref, bound, "int32 ids")


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_invalid_ids_give_zeros_next_to_inf_rows(dtype):
    """Ids -1, V_f and 2^32 + 1 add nothing, although row 0 and row V_f - 1 of that table and of
    its neighbours hold +Inf (a clamped row times 0 would be NaN, an offset past the table the
    neighbour's row)."""
    vocab, hot = (6, 4, 6), (2, 1, 3)
    ids, tables = ib.embag_inputs(4, vocab, hot, 16, seed=2)
    for t in tables:
        t[0] = float("inf")
        t[-1] = float("inf")
    big = 2 ** 32 + 1 if dtype == torch.int64 else -(2 ** 31)
    ids[:, 0:2] = torch.tensor([[1, 2], [-1, 3], [6, 4], [big, 1]])
    ids[:, 2] = torch.tensor([-1, 4, big, 2])
    ids[:, 3:6] = torch.tensor([[1, -1, 6], [big, 2, 3], [-1, -1, -1], [4, 3, 2]])
    y, intact = launch(ids.to(dtype), tables, hot)
    ref, bound = ib.embag_ref(ids, tables, hot)
    assert intact and torch.isfinite(ref).all()
    kb.assert_within(y, ref, bound, "invalid ids")
    assert torch.equal(y[2, 2].cpu().float(), torch.zeros(16))                 # a bag of invalid ids only
    assert torch.equal(y[:3, 1].cpu().float(), torch.zeros(3, 16))


def test_hotness_one_is_a_bit_copy():
    d, v = 24, 9
    ids, tables = ib.embag_inputs(5, (v,), (1,), d, seed=3)
    tables[0][2, :4] = torch.tensor([-0.0, 0.0, 2.0 ** -126, -3.0e38]).to(BF)  # -0, the smallest normal, near the maximum
    ids[:, 0] = torch.tensor([2, 0, 8, 2, 5])
    y, intact = launch(ids, tables, (1,))
    assert intact
    assert torch.equal(y[:, 0].cpu().view(torch.int16), tables[0][ids[:, 0]].view(torch.int16))


def test_reruns_are_bit_equal():
    ids, tables = ib.embag_inputs(65, VOCAB, HOT, 128, seed=4)
    runs = [launch(ids, tables, HOT)[0].view(torch.int16).clone() for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def test_more_workgroups_than_the_machine_holds():
    """129 x 24 = 3096 workgroups of 256 threads (256 CUs hold at most 8 each)."""
    vocab, hot = tuple(range(3, 27)), (1,) * 24
    ids, tables = ib.embag_inputs(257, vocab, hot, 1024, seed=6)
    y, intact = launch(ids, tables, hot)
    assert intact
    want = torch.stack([t[ids[:, f]] for f, t in enumerate(tables)], 1)
    assert torch.equal(y.cpu().view(torch.int16), want.view(torch.int16))


def test_embedding_bag_rejections():
    H = hip()
    ids, tables = ib.embag_inputs(2, (4, 5), (1, 2), 16, seed=7)
    blob, flat = torch.cat(tables).cuda(), features((4, 5), (1, 2))
    feat = torch.tensor(flat, dtype=torch.int64).view(-1, 4).cuda()
    idc = ids.cuda()
    with pytest.raises(RuntimeError, match="D must be a multiple of 8"):
        H.embedding_bag(idc, torch.zeros(9, 12, dtype=BF, device="cuda"), feat, flat)
    with pytest.raises(RuntimeError, match="D must be a multiple of 8"):
        H.embedding_bag(idc, torch.zeros(9, 1032, dtype=BF, device="cuda"), feat, flat)
    with pytest.raises(RuntimeError, match="hotness 65"):
        H.embedding_bag(torch.zeros(2, 66, dtype=torch.int64, device="cuda"), blob, feat, [0, 4, 0, 1, 4, 5, 1, 65])
    with pytest.raises(RuntimeError, match="does not fit"):
        H.embedding_bag(idc, blob, feat, [0, 4, 0, 1, 4, 6, 1, 2])              # the blob has 9 rows
    with pytest.raises(RuntimeError, match="does not fit"):
        H.embedding_bag(idc, blob, feat, [0, 4, 0, 1, 4, 5, 2, 2])              # slots 2 .. 3 of 3
    with pytest.raises(RuntimeError, match="features has"):
        H.embedding_bag(idc, blob, feat, flat[:4])
    with pytest.raises(RuntimeError, match="int32 or int64"):
        H.embedding_bag(idc.float(), blob, feat, flat)
    with pytest.raises(RuntimeError, match="expected"):
        H.embedding_bag(idc, blob.float(), feat, flat)
    with pytest.raises(RuntimeError, match="dense must be"):
        H.embedding_bag(idc, blob, feat, flat, torch.zeros(2, 8, dtype=BF, device="cuda"))
    with pytest.raises(RuntimeError, match="ids must be 16-byte aligned"):
        big = torch.zeros(7, dtype=torch.int64, device="cuda")
        H.embedding_bag(big[1:7].view(2, 3), blob, feat, flat)
    with pytest.raises(RuntimeError, match="out must be 16-byte aligned"):
        big = torch.zeros(2 * 2 * 16 + 8, dtype=BF, device="cuda")
        H.embedding_bag(idc, blob, feat, flat, None, big[1:1 + 64].view(2, 2, 16))
    with pytest.raises(RuntimeError, match="wrong size"):
        H.embedding_bag(idc, blob, feat, flat, None, torch.zeros(2, 3, 16, dtype=BF, device="cuda"))
    assert not H.embedding_bag_supported(2, 3, 12, flat, 9)
    assert not H.embedding_bag_supported(2, 3, 16, [0, 4, 0, 1, 4, 5, 1, 65], 9)
    assert H.embedding_bag_supported(2, 3, 16, flat, 9, True, False)
