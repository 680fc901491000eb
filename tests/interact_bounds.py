"""fp64 references and elementwise error bounds for the DLRM kernels
(kernels/embag.hip, kernels/interact.hip), in tests/kernel_bounds.py's error
model (U_BF16 = 2^-8 per rounding to bf16, E = 2^-23 per fp32 operation).  A
plain helper module; docs/numerics.md ("DLRM kernels") derives the constants.

embedding_bag   y = bf16(r_0 + r_1 + .. + r_{L-1}), fp32, in slot order, from
                the first row's value.  L - 1 additions, each off by at most E
                times its partial sum, and every partial sum is at most
                sum_l |r_l|:
                    acc   = (L - 1) E sum_l |r_l|
                    bound = 2^-8 (|ref| + acc) + acc        (kernel_bounds.out_bound)
                L = 1: acc = 0 and the value is a copy (the GPU test also
                compares the bits).  An id outside [0, V_f) adds nothing; the
                dense row is a copy (bound 0).
dot_interaction y = bf16(z_i . z_j): D exact bf16 x bf16 products summed in
                fp32 on the matrix cores, kernel_bounds.acc_bound with K = D,
                one slab and no activation:
                    acc   = (D + 5) E (|z_i| . |z_j|)
                    bound = 2^-8 (|ref| + acc) + acc
                The dense columns are copies and the tail is zero (bound 0).
"""
import numpy as np
import torch

import kernel_bounds as kb

BF = torch.bfloat16


def tril_pairs(f, k):
    """[(i, j)] in the kernels' order: position i (i + 1 + 2k) / 2 + j holds (i, j), j <= i + k."""
    out = [None] * (f * (f + 1 + 2 * k) // 2)
    for i in range(f):
        for j in range(0, i + k + 1):
            out[i * (i + 1 + 2 * k) // 2 + j] = (i, j)
    return out


def pair_count(f, k):
    return f * (f + 1 + 2 * k) // 2


def width(f, dd, pad, k):
    return (dd + pair_count(f, k) + pad + 7) // 8 * 8


# ---------------------------------------------------------------- embedding bag
def embag_ref(ids, tables, hot, dense=None):
    """ids [B, T] (any integer dtype), tables: bf16 [V_f, D] each, hot: L_f each, dense: bf16
    [B, D] or None -> (ref, bound) [B, F0 + F, D] in fp64.  Tables may hold non-finite rows as
    long as no valid id selects them."""
    ids = ids.long()
    b = ids.shape[0]
    d = tables[0].shape[1]
    refs, bounds = [], []
    if dense is not None:
        refs.append(kb.d(dense))
        bounds.append(torch.zeros(b, d, dtype=torch.float64))
    first = 0
    for t, l in zip(tables, hot):
        t64 = kb.d(t)
        v = t64.shape[0]
        idx = ids[:, first:first + l]
        ok = (idx >= 0) & (idx < v)
        rows = torch.where(ok[..., None], t64[idx.clamp(0, v - 1)], torch.zeros((), dtype=torch.float64))   # [B, L, D]
        ref = rows.sum(1)
        acc = (l - 1) * kb.E * rows.abs().sum(1)
        refs.append(ref)
        bounds.append(kb.out_bound(ref, acc, False))
        first += l
    return torch.stack(refs, 1), torch.stack(bounds, 1)


def embag_emulate(ids, tables, hot, dense=None, round_partials=False, clamp_and_zero=False):
    """The kernel's arithmetic in torch (fp32 adds in slot order from the first row, one rounding).
    Two wrong schemes for the bound to catch: ``round_partials`` rounds every partial sum to bf16;
    ``clamp_and_zero`` reads the clamped row of an invalid id and multiplies it by 0."""
    ids = ids.long()
    outs = [] if dense is None else [dense.clone()]
    first = 0
    for t, l in zip(tables, hot):
        tf = t.float()
        v = tf.shape[0]
        acc = None
        for s in range(l):
            idx = ids[:, first + s]
            ok = (idx >= 0) & (idx < v)
            r = tf[idx.clamp(0, v - 1)]
            r = r * ok[:, None].float() if clamp_and_zero else torch.where(ok[:, None], r, torch.zeros(()))
            acc = r if acc is None else acc + r
            if round_partials:
                acc = acc.to(BF).float()
        outs.append(acc.to(BF))
        first += l
    return torch.stack(outs, 1)


def embag_inputs(b, vocab, hot, d, seed=0, scale=1.0):
    """(ids [B, T] int64 with ids 0 and V_f - 1 in the first rows, tables bf16)."""
    g = torch.Generator().manual_seed(seed)
    tables = [(torch.randn(v, d, generator=g) * scale).to(BF) for v in vocab]
    cols = []
    for v, l in zip(vocab, hot):
        c = torch.randint(0, v, (b, l), generator=g)
        c[0, :] = 0
        c[-1, :] = v - 1
        cols.append(c)
    return torch.cat(cols, 1), tables


# ---------------------------------------------------------------- dot interaction
def interact_ref(z, dense=None, k=-1, pad=0):
    """z bf16 [B, F, D], dense bf16 [B, Dd] or None -> (ref, bound) [B, Wp] in fp64, Wp =
    ceil8(Dd + pairs + pad); non-finite where a pair's exact result is."""
    z64 = kb.d(z)
    b, f, d = z64.shape
    ii, jj = zip(*tril_pairs(f, k))
    zi, zj = z64[:, list(ii)], z64[:, list(jj)]
    ref = (zi * zj).sum(-1)
    mag = (zi.abs() * zj.abs()).sum(-1)
    acc = kb.acc_bound(ref, mag, d, 1, "none")
    bound = kb.out_bound(ref, acc, False)
    dd = 0 if dense is None else dense.shape[1]
    wp = width(f, dd, pad, k)
    out = torch.zeros(b, wp, dtype=torch.float64)
    bnd = torch.zeros(b, wp, dtype=torch.float64)
    if dense is not None:
        out[:, :dd] = kb.d(dense)
    out[:, dd:dd + ref.shape[1]] = ref
    bnd[:, dd:dd + ref.shape[1]] = bound
    return out, bnd


def interact_emulate(z, dense=None, k=-1, pad=0, upper=False):
    """fp32 Z Z^T of the bf16 values, one rounding, tril order.  ``upper``: the wrong scheme, the
    same pairs in np.triu_indices order (Z Z^T is symmetric: only the order differs, from F = 4 on)."""
    zf = z.float()
    b, f, _d = zf.shape
    zz = zf @ zf.transpose(1, 2)
    if upper:
        ii, jj = np.triu_indices(f, -k)
    else:
        ii, jj = zip(*tril_pairs(f, k))
    pairs = zz[:, list(ii), list(jj)].to(BF)
    dd = 0 if dense is None else dense.shape[1]
    out = torch.zeros(b, width(f, dd, pad, k), dtype=BF)
    if dense is not None:
        out[:, :dd] = dense
    out[:, dd:dd + pairs.shape[1]] = pairs
    return out


def assert_within_where_finite(y, ref, bound, what=""):
    """y is non-finite exactly where ref is; elsewhere |y - ref| <= bound.  Returns the worst err / bound."""
    y64 = kb.d(y)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(y64), fin), \
        f"{what}: non-finite at {(~torch.isfinite(y64)).nonzero().tolist()[:8]}, reference at {(~fin).nonzero().tolist()[:8]}"
    zero = torch.zeros((), dtype=torch.float64)
    return kb.assert_within(torch.where(fin, y64, zero), torch.where(fin, ref, zero),
                            torch.where(fin & torch.isfinite(bound), bound, zero), what)
