"""The fused graph ops (graph/fused.py, graph/patterns.py) on the kernels, under
the elementwise bounds of kernel_bounds.py (MI355X).

test_kernel_bounds_gpu.py calls the kernels with weights, tile configs and
split-K values of its own.  Here the op classes do the packing, the TF padding,
the dispatch and the pick:

 (a) every op class on every dispatch branch with the UNTUNED pick (what
     ops.tuned_config returns with autotuning off and an empty table);
 (b) every (config, split-K) pair ops.candidates() lists for the op's recorded
     (M, N, K, flags), each forced in turn -- the list the tuner would time;
 (c) the tuned-pick keys of ops that must not share a pick;
 (d) three tiny graphs through the fusion passes: folded weights elementwise,
     then the output.

ops.tuned_config / ops.tuned_choice are replaced by the `picks` fixture (the op
classes import them inside __call__), so no timing loop runs and neither the
committed nor a remote pick table is read.

Set FUSED_OPS_REPORT=<path> for the worst err / bound per op class and the
candidates each case rejected, as JSON (the table in docs/numerics.md)."""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import fused_op_refs as fr  # noqa: E402
import kernel_bounds as kb  # noqa: E402
from kernel_bounds import BF, rnd  # noqa: E402
from rust_tensorflow_serving2_amd import ops  # noqa: E402
from rust_tensorflow_serving2_amd.graph import fused as FU  # noqa: E402
from rust_tensorflow_serving2_amd.graph import patterns as PT  # noqa: E402
from rust_tensorflow_serving2_amd.ops import hip  # noqa: E402

DEV = torch.device("cuda:0")
WORST = {}
REJECTED = {}
REAL_TUNED_CONFIG = ops.tuned_config
REAL_TUNED_CHOICE = ops.tuned_choice


def within(family, y, ref, bound, what):
    r = kb.assert_within(y, ref, bound, f"{family}: {what}")
    WORST[family] = max(WORST.get(family, 0.0), r)
    return r


def dev(t):
    return None if t is None else t.to(DEV)


def _never(*_a, **_k):
    raise AssertionError("the tuner launched a candidate: no test here may time anything")


class Picks:
    """Stands in for ops.tuned_config / ops.tuned_choice.  Every call is
    recorded with the pick the real tuned_config returns when autotuning is
    off (the fixture turns it off over an empty table, so that is the
    heuristic pick -- or an entry a test put into ops._TUNED itself);
    `force` / `choice` override what the op is given."""

    def __init__(self):
        self.calls = []
        self.choices = []
        self.force = None
        self.choice = None

    def tuned_config(self, key, M, N, launch, K=64, dma=True, aligned64=False, cgemm_only=False, halo=False,
                     no_split=False, stem=False, ln=False, relu6=False):
        flags = dict(dma=dma, aligned64=aligned64, cgemm_only=cgemm_only, halo=halo, no_split=no_split, stem=stem,
                     ln=ln, relu6=relu6)
        offered = REAL_TUNED_CONFIG(key, M, N, _never, K, **flags)
        self.calls.append(dict(key=key, M=M, N=N, K=K, flags=flags, offered=offered))
        return self.force if self.force is not None else offered

    def tuned_choice(self, key, options, default):
        offered = REAL_TUNED_CHOICE(key, {o: _never for o in options}, default)
        self.choices.append(dict(key=key, options=sorted(options), default=default, offered=offered))
        return self.choice if self.choice is not None else offered

    def last(self):
        return self.calls[-1]


@pytest.fixture
def picks(monkeypatch):
    monkeypatch.setattr(ops, "AUTOTUNE", False)
    monkeypatch.setattr(ops, "_TUNED", {})
    monkeypatch.setattr(ops, "_REMOTE", {})
    monkeypatch.setitem(ops._CACHE_STATE, "loaded", True)      # the committed table is not read
    p = Picks()
    monkeypatch.setattr(ops, "tuned_config", p.tuned_config)
    monkeypatch.setattr(ops, "tuned_choice", p.tuned_choice)
    return p


def untuned_pick(call):
    """tuned_config's answer with AUTOTUNE off, written out."""
    f = call["flags"]
    c = (36 if f["no_split"] else 42) if f["cgemm_only"] else ops.heuristic_config(call["M"], call["N"])
    return c, 1 if f["no_split"] else ops.heuristic_splits(call["M"], call["N"], call["K"], c)


# ================================================================== (a) FusedConv
def conv_x(case, x):
    """What the serving path hands the op: the fp32 request on the thin-channel branches, bf16 activations else."""
    return dev(x if fr.conv_branch(*case[0]) in ("c4", "f32") else x.to(BF))


def make_conv(case, wt, b, act="none"):
    _shape, (_tag, _even, strides, padding, pads) = case
    return FU.FusedConv(wt, b, strides, padding, pads, act, DEV, True, "conv")


def expected_flags(case, x):
    (kh, kw, cin, cout), (_tag, _even, (sh, sw), padding, pads) = case
    br = fr.conv_branch(kh, kw, cin, cout)
    p = fr.tf_pads(x.shape[1], x.shape[2], kh, kw, sh, sw, padding, pads)
    return dict(dma=br in ("bf16", "aligned"), aligned64=br in ("aligned", "c4"), stem=br == "c4",
                halo=br == "aligned" and (kh, kw, sh, sw) == (3, 3, 1, 1) and p[0] <= 2 and p[2] <= 2)


@pytest.mark.parametrize("case", fr.CONV_CASES, ids=fr.conv_case_id)
def test_fused_conv_untuned_pick_within_bound(picks, case):
    (kh, kw, cin, cout), (tag, even, strides, padding, pads) = case
    x, wt, b, r, sc, sf = fr.conv_case_inputs(case)
    op = make_conv(case, wt, b)
    assert op.c4 == (fr.conv_branch(kh, kw, cin, cout) == "c4")
    xd, rd = conv_x(case, x), dev(r)
    fam = "FusedConv " + fr.conv_branch(kh, kw, cin, cout)
    for res in (r, None):
        pre, mag, k = fr.conv_parts_tf(x, wt, b, strides, padding, pads, res)
        for act in ("relu", "none"):
            op.act = act
            outs = op(None, None, [xd] + ([rd] if res is not None else []))
            call = picks.last()
            assert call["offered"] == untuned_pick(call) and (call["M"], call["N"]) == (pre[..., 0].numel(), cout)
            want = expected_flags(case, x)
            assert {f: call["flags"][f] for f in want} == want and not call["flags"]["cgemm_only"]
            assert len(outs) == 1 and outs[0].dtype == BF
            ref, bound = kb.epilogue(pre, mag, k, call["offered"][1], act, False)
            within(fam, outs[0], ref, bound, f"{fr.conv_case_id(case)} res={res is not None} {act} {call['offered']}")
    if not op.post_ok():
        assert cin % 64 != 0
        return
    assert cin % 64 == 0 and cout % 8 == 0
    for mode in ("dual", "only"):
        op = make_conv(case, wt, b)
        op.set_post(sc, sf, "relu", mode)
        outs = op(None, None, [xd, rd])
        call = picks.last()
        assert call["flags"]["cgemm_only"] and call["offered"] == untuned_pick(call) and call["offered"][0] == 42
        want = fr.conv_ref(x, wt, b, strides, padding, pads, r, "none", call["offered"][1], (sc, sf, "relu", mode))
        assert len(outs) == len(want)
        for i, (y, (ref, bound)) in enumerate(zip(outs, want)):
            within("FusedConv post", y, ref, bound, f"{fr.conv_case_id(case)} post {mode} output {i}")


def test_fused_conv_casts_an_fp32_activation_itself(picks):
    """The bf16 branches take an fp32 tensor too (hip().cast_bf16 in front)."""
    case = ((3, 3, 64, 72), ("same-odd-s1", False, (1, 1), "SAME", (0, 0, 0, 0)))
    x, wt, b, r, _sc, _sf = fr.conv_case_inputs(case)
    op = make_conv(case, wt, b, "relu")
    (ref, bound), = fr.conv_ref(x, wt, b, (1, 1), "SAME", res=r, act="relu")
    y32 = op(None, None, [dev(x), dev(r.float())])[0]
    y16 = op(None, None, [dev(x.to(BF)), dev(r)])[0]
    within("FusedConv aligned", y32, ref, bound, "fp32 input and residual")
    assert torch.equal(y32, y16)


# ================================================================== (a) FusedDualConv
def make_dual(case, w1, w2, b1, b2, act):
    s = case[6]
    ch = FU.FusedConv(w1, b1, (1, 1), "SAME", (0, 0, 0, 0), "none", DEV, True, "h")
    cx = FU.FusedConv(w2, b2, (s, s), "SAME", (0, 0, 0, 0), "none", DEV, True, "x")
    return FU.FusedDualConv(ch, cx, act, DEV, True, "dual")


@pytest.mark.parametrize("case", fr.DUAL_CASES)
def test_fused_dual_conv_untuned_pick_within_bound(picks, case):
    n, ho, wo, c1, c2, cout, s = case
    h, x, w1, w2, b1, b2, sc, sf = fr.dual_case_inputs(case)
    for act in ("relu", "none"):
        op = make_dual(case, w1, w2, b1, b2, act)
        outs = op(None, None, [dev(h), dev(x)])
        call = picks.last()
        assert call["offered"] == untuned_pick(call) and call["offered"][0] == 42 and call["flags"]["cgemm_only"]
        assert (call["M"], call["N"], call["K"]) == (n * ho * wo, cout, c1 + c2)
        (ref, bound), = fr.dual_ref(h, x, w1, w2, b1, b2, (s, s), act, call["offered"][1])
        within("FusedDualConv", outs[0], ref, bound, f"{case} {act}")
    op = make_dual(case, w1, w2, b1, b2, "none")
    assert op.post_ok()
    op.set_post(sc, sf, "relu", "dual")
    outs = op(None, None, [dev(h), dev(x)])
    want = fr.dual_ref(h, x, w1, w2, b1, b2, (s, s), "none", picks.last()["offered"][1], (sc, sf, "relu", "dual"))
    assert len(outs) == 2
    for i, (y, (ref, bound)) in enumerate(zip(outs, want)):
        within("FusedDualConv post", y, ref, bound, f"{case} post dual output {i}")


# ================================================================== (a) FusedMatMul
def run_matmul(picks, op, x, w, b, res, fam, what, base_cols=None):
    y = op(None, None, [x] + ([dev(res)] if res is not None else []))[0]
    splits = 1
    if op.use_hip:
        call = picks.last()
        assert call["offered"] == untuned_pick(call)
        splits = call["offered"][1]
    ref, bound = fr.matmul_ref(x.cpu(), w, b, res, op.act, op.out_f32, splits)
    assert y.dtype == (torch.float32 if op.out_f32 else BF) and tuple(y.shape) == tuple(ref.shape)
    within(fam, y, ref, bound, what)
    return y


@pytest.mark.parametrize("out_f32", [False, True])
def test_fused_matmul_branches_within_bound(picks, out_f32):
    m = fr.MATMUL_M
    fam = "FusedMatMul" + (" f32" if out_f32 else "")
    # K % 64 == 0, N = 13: igemm without pad_n; the padded buffer with it
    x, w, b, r = fr.matmul_inputs(m, 64, 13)
    op = FU.FusedMatMul(w, b, "none", out_f32, DEV, True, "mm")
    assert op.np == 13
    run_matmul(picks, op, dev(x), w, b, None, fam, "k=64 n=13")
    run_matmul(picks, op, dev(x), w, b, r, fam, "k=64 n=13 residual")
    opp = FU.FusedMatMul(w, b, "relu", out_f32, DEV, True, "mm", pad_n=True)
    assert opp.np == 16
    y = run_matmul(picks, opp, dev(x), w, b, None, fam, "pad_n: the [:, :13] view")
    assert picks.last()["N"] == 16 and picks.last()["flags"]["aligned64"]
    assert tuple(y.shape) == (m, 13) and y.stride() == (16, 1) and y._base is not None and tuple(y._base.shape) == (m, 16)
    # the whole padded buffer: its tail columns are act(0 + 0) = 0 exactly
    wp, bp = torch.cat([w, torch.zeros(64, 3)], 1), torch.cat([b, torch.zeros(3)])
    ref, bound = fr.matmul_ref(x, wp, bp, None, "relu", out_f32, picks.last()["offered"][1])
    assert not bound[:, 13:].any()
    within(fam, y._base, ref, bound, "pad_n: the padded buffer")
    # pad_n with a residual: the w[:n] / b[:n] slice, a contiguous [M, 13]
    y = run_matmul(picks, opp, dev(x), w, b, r, fam, "pad_n with a residual")
    assert picks.last()["N"] == 13 and y.is_contiguous()
    # a 3-D input
    y = run_matmul(picks, opp, dev(x).reshape(2, m // 2, 64), w, b, None, fam, "3-D input")
    assert tuple(y.shape) == (2, m // 2, 13) and picks.last()["M"] == m
    # a row-strided 2-D view (stride a multiple of 8) is read in place; with a residual it is copied first
    big = torch.full((m, 3, 64), 1e4, dtype=BF)
    big[:, 1] = x
    view = dev(big)[:, 1, :]
    assert view.stride() == (192, 1) and not view.is_contiguous()
    run_matmul(picks, op, view, w, b, None, fam, "row-strided view")
    assert picks.last()["key"][-1] == 192
    run_matmul(picks, op, view, w, b, r, fam, "row-strided view with a residual")
    assert picks.last()["key"][-1] != 192
    # K % 64 != 0: no pad_n
    x2, w2, b2, r2 = fr.matmul_inputs(m, 72, 13)
    op2 = FU.FusedMatMul(w2, b2, "tanh", out_f32, DEV, True, "mm", pad_n=True)
    assert op2.use_hip and op2.np == 13
    run_matmul(picks, op2, dev(x2), w2, b2, None, fam, "k=72 n=13")
    assert not picks.last()["flags"]["aligned64"]
    # K % 8 != 0: fp32 torch, at most one bf16 store
    x3, w3, b3, r3 = fr.matmul_inputs(m, 20, 13)
    op3 = FU.FusedMatMul(w3, b3, "gelu_erf", out_f32, DEV, True, "mm", pad_n=True)
    assert not op3.use_hip
    n_calls = len(picks.calls)
    run_matmul(picks, op3, dev(x3), w3, b3, r3, fam + " fallback", "k=20 n=13 residual")
    assert len(picks.calls) == n_calls


@pytest.mark.parametrize("b,n,k", [(32, 2, 768), (5, 3, 1024)])
def test_dense_softmax_op_within_bound(picks, b, n, k):
    x = rnd(b, k, seed=31)
    w = rnd(k, n, scale=1 / math.sqrt(k), seed=32).to(BF).float()
    bias = fr.q6(rnd(n, scale=0.5, seed=33))
    op = FU.DenseSoftmax(FU.FusedMatMul(w, bias, "none", True, DEV, True, "mm"))
    p, bound = kb.dense_softmax_ref(x, w.t(), bias, n)
    within("DenseSoftmax", op(None, None, [dev(x)])[0], p, bound, f"{(b, n, k)}")
    assert not picks.calls                                          # one kernel, no GEMM pick
    # a bf16 input takes the GEMM + torch softmax path: the fp32 logits' bound feeds the softmax bound
    xb = x.to(BF)
    y = op(None, None, [dev(xb)])[0]
    pre, mag, _k = fr.matmul_parts(xb, w, bias)
    p, bound = kb.softmax_ref(pre, kb.epilogue(pre, mag, k, picks.last()["offered"][1], "none", True)[1])
    within("DenseSoftmax fallback", y, p, bound, f"{(b, n, k)} bf16 input")


# ================================================================== (a) ClassifierHead
# (m, h, w, k, n, seed, classes dtype): seeds at which the reference alone leaves every row comparable
HEAD_OP_CASES = [(3, 2, 2, 512, 13, 50, torch.int64), (5, 1, 1, 512, 13, 51, torch.int32),
                 (3, 2, 2, 576, 13, 52, torch.int32), (4, 3, 1, 2048, 1001, 55, torch.int64)]


@pytest.mark.parametrize("m,h,w,k,n,seed,cdt", HEAD_OP_CASES)
def test_classifier_head_op_within_bound(picks, m, h, w, k, n, seed, cdt):
    np_ = -(-n // 8) * 8
    x, wt, b = kb.head_inputs(m, h * w, k, n, seed)
    x = x.reshape(m, h, w, k)
    b = fr.q6(b)
    mm = FU.FusedMatMul(wt.float().t().contiguous(), b, "none", True, DEV, True, "mm", pad_n=True)
    assert mm.np == (np_ if k % 64 == 0 else n)
    op = FU.ClassifierHead(mm, cdt, True)
    assert op.use_hip == (k in (512, 1024, 2048, 4096))
    probs, cls = op(None, None, [dev(x)])
    p, bound, logits, dlogit = kb.head_ref(x, wt, b, n)
    assert tuple(probs.shape) == (m, n) and cls.dtype == cdt and tuple(cls.shape) == (m,)
    within("ClassifierHead" + ("" if op.use_hip else " fallback"), probs, p, bound, f"{(m, h, w, k, n)}")
    assert kb.argmax_checked(cls.long(), logits, dlogit) == 1.0
    assert not picks.calls


# ================================================================== (a) StemPool, ChainConv, pools
@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("pool_padding", ["SAME", "VALID"])
@pytest.mark.parametrize("even", [True, False])
def test_stem_pool_op_within_bound(picks, even, pool_padding, post):
    case = ((7, 7, 3, 16), ("same-s2", even, (2, 2), "SAME", (0, 0, 0, 0)))
    x, wt, b, _r, sc, sf = fr.conv_case_inputs(case)
    conv = make_conv(case, wt, b, "relu")
    pool = FU.MaxPool((3, 3), (2, 2), pool_padding, True)
    if post:
        pool.set_post(sc, sf, "relu", "only", device=DEV)
    op = FU.StemPool(conv, pool)
    assert op.use_hip and op.accepts_bf16_input(0)
    ref, bound = fr.stem_pool_ref(x, wt, b, "SAME", "relu", pool_padding, (sc, sf, "relu") if post else None)
    y = op(None, None, [dev(x)])[0]
    within("StemPool", y, ref, bound, f"even={even} pool {pool_padding} post={post}")
    assert torch.equal(op(None, None, [dev(x.to(BF))])[0], y) and not picks.calls


@pytest.mark.parametrize("k1,n1,n2", [(64, 256, 64), (128, 512, 256)])
@pytest.mark.parametrize("choice", [1, 0])
@pytest.mark.parametrize("with_res", [True, False])
def test_chain_conv_both_choices_within_bound(picks, k1, n1, n2, choice, with_res):
    """y1 under the single-GEMM bound; y2 against the reference computed from
    the op's own bf16 y1 (as the kernel test does)."""
    n, h, w = 1, 7, 11
    x = rnd(n, h, w, k1, seed=61).to(BF)
    w1 = rnd(1, 1, k1, n1, scale=1 / math.sqrt(k1), seed=62).to(BF).float()
    w2 = rnd(1, 1, n1, n2, scale=1 / math.sqrt(n1), seed=63).to(BF).float()
    b1, b2 = fr.q6(rnd(n1, scale=0.3, seed=64)), fr.q6(rnd(n2, scale=0.3, seed=65))
    res = rnd(n, h, w, n1, seed=66).to(BF) if with_res else None
    a = FU.FusedConv(w1, b1, (1, 1), "SAME", (0, 0, 0, 0), "relu" if with_res else "none", DEV, True, "a")
    b = FU.FusedConv(w2, b2, (1, 1), "VALID", (0, 0, 0, 0), "relu", DEV, True, "b")
    op = FU.ChainConv(a, b)
    picks.choice = choice
    y1, y2 = op(None, None, [dev(x)] + ([dev(res)] if with_res else []))
    ch = picks.choices[-1]
    assert ch["options"] == [0, 1] and ch["offered"] == ch["default"] == (1 if n1 == 256 else 0)
    assert len(picks.calls) == (0 if choice == 1 else 2)
    s1, s2 = (1, 1) if choice == 1 else (picks.calls[0]["offered"][1], picks.calls[1]["offered"][1])
    (ref1, bound1), = fr.conv_ref(x, w1, b1, (1, 1), "SAME", res=res, act=a.act, splits=s1)
    within("ChainConv y1", y1, ref1, bound1, f"{(k1, n1, n2)} choice {choice} res={with_res}")
    (ref2, bound2), = fr.conv_ref(y1.cpu(), w2, b2, (1, 1), "VALID", act="relu", splits=s2)
    within("ChainConv y2", y2, ref2, bound2, f"{(k1, n1, n2)} choice {choice} res={with_res}")


def pow2_scale(c, seed):
    """+-2^j per channel: y * scale is exact, so scale-and-shift rounds once whether fused or not."""
    j = torch.randint(-2, 3, (c,), generator=torch.Generator().manual_seed(seed))
    sign = torch.where(rnd(c, seed=seed + 1) > -0.5, 1.0, -1.0)
    return sign * torch.pow(2.0, j.float())


@pytest.mark.parametrize("padding", ["SAME", "VALID"])
@pytest.mark.parametrize("c", [8, 72])
def test_maxpool_op_bit_exact(picks, padding, c):
    x = rnd(2, 10, 13, c, seed=c).to(BF)
    pp = fr.tf_pads(10, 13, 3, 3, 2, 2, padding)
    ref = kb.maxpool_ref(x, 3, 3, 2, 2, *pp)
    op = FU.MaxPool((3, 3), (2, 2), padding, True)
    y = op(None, None, [dev(x)])[0]
    assert y.dtype == BF and torch.equal(y.double().cpu(), ref)
    # post `only` on the kernel: exact with power-of-two scales (one rounding to fp32, one to bf16) ...
    sc, sf = pow2_scale(c, c), fr.q6(rnd(c, seed=c + 2) * 0.2)
    want32 = torch.relu(ref.float() * sc + sf)
    op.set_post(sc, sf, "relu", "only", device=DEV)
    z = op(None, None, [dev(x)])[0]
    assert z.dtype == BF and torch.equal(z.cpu(), want32.to(BF))
    # ... and within the affine's bound with general ones
    sc2 = fr.q6(rnd(c, seed=c + 3) * 0.5 + 1.0)
    op.set_post(sc2, sf, "relu", "only", device=DEV)
    ref2, bound2 = fr.affine_after(ref, torch.zeros_like(ref), sc2, sf)
    within("MaxPool post", op(None, None, [dev(x)])[0], ref2, bound2, f"{padding} c={c}")
    # post `dual` runs on the torch path: the pooled map beside its affine
    op.set_post(sc, sf, "relu", "dual", device=DEV)
    y2, z2 = op(None, None, [dev(x)])
    assert torch.equal(y2.double().cpu(), ref) and torch.equal(z2.float().cpu(), want32)
    # C % 8 != 0: the torch path, still exact
    x5 = rnd(2, 10, 13, 5, seed=5).to(BF)
    y5 = FU.MaxPool((3, 3), (2, 2), padding, True)(None, None, [dev(x5)])[0]
    assert torch.equal(y5.double().cpu(), kb.maxpool_ref(x5, 3, 3, 2, 2, *pp))


@pytest.mark.parametrize("c,keep", [(72, False), (72, True), (12, False), (12, True)])
def test_global_avgpool_op_within_bound(picks, c, keep):
    g = rnd(3, 3, 5, c, seed=c).to(BF)
    ref, bound, _ = kb.gap_ref(g)
    y = FU.GlobalAvgPool(keep, True)(None, None, [dev(g)])[0]
    assert tuple(y.shape) == ((3, 1, 1, c) if keep else (3, c))
    within("GlobalAvgPool" + ("" if c % 8 == 0 else " fallback"), y.reshape(3, c), ref, bound, f"c={c} keep={keep}")


@pytest.mark.parametrize("cols", [10, 1001])
@pytest.mark.parametrize("bf16", [False, True])
def test_softmax_argmax_op_views(picks, cols, bf16):
    lg = rnd(3, cols, scale=4, seed=cols + 7)
    lg = lg.to(BF) if bf16 else lg
    ref, bound = kb.softmax_ref(lg)
    op = FU.SoftmaxArgMax(True, torch.int32)
    ld = -(-cols // 8) * 8 + 8
    full = torch.full((3, ld), 1e4, dtype=lg.dtype)
    full[:, :cols] = lg
    inter = torch.full((3, 2 * cols), 1e4, dtype=lg.dtype)
    inter[:, ::2] = lg
    for name, view in (("contiguous", dev(lg)), ("row-strided", dev(full)[:, :cols]), ("last stride 2", dev(inter)[:, ::2])):
        p, c = op(None, None, [view])
        assert c.dtype == torch.int32
        within("SoftmaxArgMax", p, ref, bound, f"cols={cols} bf16={bf16} {name}")
        assert kb.argmax_checked(c.long(), lg, 0.0) == 1.0


# ================================================================== (a) patterns.py ops
@pytest.mark.parametrize("cols", [64, 52])
def test_layernorm_op_within_bound(picks, cols):
    x = (rnd(37, cols, seed=41) * 3 + 5).to(BF)
    gm, bt = rnd(cols, seed=43), rnd(cols, seed=44)
    op = PT.LayerNormOp(gm, bt, 1e-5, DEV, True)
    ref, bound = kb.layernorm_ref(x.double(), gm, bt, 1e-5)
    y = op(None, None, [dev(x)])[0]
    assert y.dtype == BF
    within("LayerNormOp" + ("" if cols % 8 == 0 else " fallback"), y, ref, bound, f"cols={cols}")


def test_key_mask_adder_op(picks):
    op = PT.KeyMaskAdderOp(1.0, -10000.0)
    for m in (torch.tensor([[[1, 1, 0, 1, 0]], [[0, 1, 1, 1, 1]]], dtype=torch.int32),
              torch.tensor([[[1.0, 0.5, 0.0, 0.25]]])):
        y = op(None, None, [dev(m)])[0]
        assert tuple(y.shape) == (m.shape[0], 1, 1, m.shape[2]) and y.dtype == torch.float32
        ref = (1.0 - m.double()) * -10000.0
        # (one - m) * scale or m * -scale + one * scale: two fp32 operations on values of that size
        bound = 2 * kb.E * (m.double().abs() * 10000.0 + 10000.0)
        within("KeyMaskAdderOp", y.reshape(m.shape), ref, bound, f"{m.dtype}")
        assert torch.equal(y.cpu().reshape(m.shape)[m == 1], torch.zeros(int((m == 1).sum())))


@pytest.mark.parametrize("s", [1, 33, 100])
@pytest.mark.parametrize("d", [64, 32])
def test_attention_op_with_key_mask_within_bound(picks, s, d):
    b, h = 2, 3
    qkv = rnd(b, s, 3 * h * d, seed=21 + s).to(BF)
    keep = torch.ones(b, 1, s, dtype=torch.int32)
    keep[b - 1, 0, s // 2 + 1:] = 0
    adder = PT.KeyMaskAdderOp(1.0, -10000.0)(None, None, [dev(keep)])[0]
    op = PT.AttentionOp(h, d, s, 1 / math.sqrt(d), True)
    y = op(None, None, [dev(qkv).reshape(b * s, 3 * h * d), adder])[0]
    assert tuple(y.shape) == (b * s, h * d) and y.dtype == BF
    ref, bound = kb.attention_ref(qkv, h, 1 / math.sqrt(d), (1.0 - keep[:, 0].double()) * -10000.0)
    within("AttentionOp" + ("" if d == 64 else " fallback"), y.reshape(b, s, h * d), ref, bound, f"S={s} D={d}")
    y0 = op(None, None, [dev(qkv)])[0]
    ref0, bound0 = kb.attention_ref(qkv, h, 1 / math.sqrt(d), None)
    within("AttentionOp" + ("" if d == 64 else " fallback"), y0.reshape(b, s, h * d), ref0, bound0, f"S={s} D={d} no mask")


@pytest.mark.parametrize("hd", [64, 520])
def test_embedding_ln_op_within_bound(picks, hd):
    S = 16
    gen = torch.Generator().manual_seed(hd)
    ids = torch.randint(0, 50, (2, S), dtype=torch.int32, generator=gen)
    tt = torch.randint(0, 3, (2, S), dtype=torch.int32, generator=gen)
    word, typ, pos = (rnd(50, hd, seed=31).to(BF).float(), rnd(3, hd, seed=32).to(BF).float(),
                      rnd(1, S, hd, seed=33).to(BF).float())
    gm, bt = rnd(hd, seed=34), rnd(hd, seed=35)
    op = PT.EmbeddingLNOp([word, typ], pos, S, gm, bt, 1e-6, DEV, True)
    assert op.hip_ok
    y = op(None, None, [dev(ids), dev(tt)])[0]
    assert tuple(y.shape) == (2, S, hd)
    ref, bound = kb.layernorm_ref(kb.embed_sum(ids, tt, word, pos[0], typ, S), gm, bt, 1e-6)
    within("EmbeddingLNOp", y.reshape(2 * S, hd), ref, bound, f"hd={hd}")
    op1 = PT.EmbeddingLNOp([word], None, S, gm, bt, 1e-6, DEV, True)
    ref1, bound1 = kb.layernorm_ref(kb.embed_sum(ids, None, word, None, None, S), gm, bt, 1e-6)
    within("EmbeddingLNOp", op1(None, None, [dev(ids)])[0].reshape(2 * S, hd), ref1, bound1, f"hd={hd} word only")


# ================================================================== (a) LayerNorm around GEMMs
def lnx_setup(m=77, C=64, F4=128):
    """producer GEMM (+ residual) -> LayerNorm -> {A of a GELU GEMM, residual of
    another GEMM}, rewritten by defer_layernorm (as test_fusion.py drives it)."""
    from rust_tensorflow_serving2_amd.graph.ir import Graph, Node
    w0 = rnd(C, C, scale=1 / 8, seed=1).to(BF).float()
    w1 = rnd(C, F4, scale=1 / 8, seed=2).to(BF).float()
    w2 = rnd(F4, C, scale=1 / 11, seed=3).to(BF).float()
    b0, b1, b2 = fr.q6(rnd(C, scale=0.2, seed=4)), fr.q6(rnd(F4, scale=0.2, seed=5)), fr.q6(rnd(C, scale=0.2, seed=6))
    gam, bet = 1 + rnd(C, scale=0.1, seed=7), rnd(C, scale=0.1, seed=8)
    mm0 = FU.FusedMatMul(w0, b0, "none", False, DEV, True, "p")
    mm1 = FU.FusedMatMul(w1, b1, "gelu_tanh", False, DEV, True, "a")
    mm2 = FU.FusedMatMul(w2, b2, "none", False, DEV, True, "r")
    ln = PT.LayerNormOp(gam, bet, 1e-6, DEV, True)
    g = Graph()
    g.add(Node(name="x", op="Placeholder"))
    g.add(Node(name="p", op="_FusedMatMul", inputs=[("x", 0), ("x", 0)], attrs={"_impl": mm0}))
    g.add(Node(name="ln", op="_LayerNorm", inputs=[("p", 0)], attrs={"_impl": ln}))
    g.add(Node(name="a", op="_FusedMatMul", inputs=[("ln", 0)], attrs={"_impl": mm1}))
    g.add(Node(name="r", op="_FusedMatMul", inputs=[("a", 0), ("ln", 0)], attrs={"_impl": mm2}))
    order = ["x", "p", "ln", "a", "r"]
    os.environ["TFSERVE_DEFER_LN"] = "1"
    try:
        FU.defer_layernorm(g, order, set(), [("r", 0)], DEV, None)
    finally:
        del os.environ["TFSERVE_DEFER_LN"]
    assert "ln" not in g.nodes
    P, A, R = (g.nodes[k].attrs["_impl"] for k in "par")
    x = (rnd(m, C, seed=9) * 1.5 + 0.3).to(BF)
    return dict(g=g, P=P, A=A, R=R, x=x, w=(w0, w1, w2), b=(b0, b1, b2), gam=gam, bet=bet, eps=1e-6, m=m, C=C, F4=F4)


def lnx_check_producer(picks, t):
    """P: z = x @ w0 + b0 + x and z's row partials."""
    z, st = t["P"](None, t["g"].nodes["p"], [dev(t["x"]), dev(t["x"])])
    ref, bound = kb.lnx_ref(t["x"], t["w"][0].t(), t["b"][0], "none", zr=t["x"])
    within("DeferredLNMatMul producer", z, ref, bound, f"{picks.last()['offered']}")
    assert st.shape[0] == t["m"] and st.shape[2] == 2
    sums, sbound = kb.stats_bound(z, st.shape[1])
    within("DeferredLNMatMul row statistics", st.double().sum(1), sums, sbound, f"{picks.last()['offered']}")
    return z.cpu()


def lnx_input_side_ref(t, z, parts):
    """A: act(LN(z) @ w1 + b1) computed as rstd (z @ W' - mean colsum) + b'.
    The reference folds in fp64; the op's fp32 fold is checked against it
    first, then its own rounded bias and colsum enter the kernel's bound: the
    op's colsum is an fp32 sum of K bf16 values on the device (K roundings,
    where lnx_ref assumes one), so |mean| rstd K 2^-24 sum|W'| is added."""
    A, (w1, b1), gam, bet, C = t["A"], (t["w"][1], t["b"][1]), t["gam"], t["bet"], t["C"]
    wf = (w1 * gam[:, None]).t().contiguous().to(BF)                       # folded in fp32, rounded once
    assert fr.same_bits(A.w.cpu()[:, :C].contiguous(), wf), "gamma fold"
    b64 = b1.double() + bet.double() @ w1.double()
    slack = (C + 2) * kb.E * (b1.double().abs() + bet.double().abs() @ w1.double().abs())
    kb.assert_within(A.b, b64, slack, "beta fold")
    colsum64 = wf.double().sum(1)
    cs_slack = C * kb.U_F32 * wf.double().abs().sum(1)
    kb.assert_within(A.colsum, colsum64, cs_slack, "colsum")
    ref, bound = kb.lnx_ref(z, wf, A.b.cpu(), "gelu_tanh", a_parts=parts, a_eps=t["eps"], colsum=A.colsum.cpu())
    mean, rstd, _dm, _rel = kb.ln_stats_err(z.double(), parts, t["eps"])
    extra = kb.L_ACT["gelu_tanh"] * rstd * mean.abs() * cs_slack
    return ref, bound + (1 + kb.U_BF16) * extra


def test_deferred_layernorm_matmuls_untuned_pick_within_bound(picks):
    t = lnx_setup()
    z = lnx_check_producer(picks, t)
    call = picks.last()
    assert call["offered"] == (36, 1) and call["flags"]["ln"] and call["flags"]["no_split"]
    st = kb.row_partials(z, 2)                     # statistics as the bounds assume them: off by 2^-24
    a = t["A"](None, t["g"].nodes["a"], [dev(z), dev(st)])[0]
    ref, bound = lnx_input_side_ref(t, z, 2)
    within("DeferredLNMatMul input side", a, ref, bound, "untuned")
    r = t["R"](None, t["g"].nodes["r"], [a, dev(z), dev(st)])[0]
    ref, bound = kb.lnx_ref(a.cpu(), t["w"][2].t(), t["b"][2], "none", zr=z, r_parts=2, r_gamma=t["gam"],
                            r_beta=t["bet"], r_eps=t["eps"])
    within("DeferredLNMatMul residual side", r, ref, bound, "untuned")


@pytest.mark.parametrize("choice", [0, 1, 2, 3])
def test_matmul_layernorm_op_every_choice_within_bound(picks, choice):
    m, k, n = 33, 128, 512
    x, w, b, r = fr.matmul_inputs(m, k, n)
    r = (r.float() * 2 + 3).to(BF)
    gm, bt = rnd(n, seed=65), rnd(n, seed=66)
    mm = FU.FusedMatMul(w, b, "none", False, DEV, True, "mm")
    ln = PT.LayerNormOp(gm, bt, 1e-12, DEV, True)
    assert FU.MatMulLN.fusable(mm, ln)
    op = FU.MatMulLN(mm, ln)
    picks.choice = choice
    y = op(None, None, [dev(x), dev(r)])[0]
    ch = picks.choices[-1]
    assert choice in ch["options"] and ch["offered"] == ch["default"] == 0
    pre, mag, _k = fr.matmul_parts(x, w, b, r)
    if choice == 0:
        # two launches: the GEMM's bf16 output (its whole elementwise bound) is the LayerNorm's input error
        dz = kb.epilogue(pre, mag, k, picks.last()["offered"][1], "none", False)[1]
    else:
        assert not picks.calls
        dz = (k + 5) * kb.E * mag
    ref, bound = kb.layernorm_ref(pre, gm, bt, 1e-12, dz=dz)
    within("MatMulLN", y, ref, bound, f"choice {choice}")


# ================================================================== (b) every candidate the tuner would time
def cand_conv(kh, kw, cin, cout, tag, even, strides, padding, pads, act="relu", with_res=True, post=None):
    case = ((kh, kw, cin, cout), (tag, even, strides, padding, pads))
    x, wt, b, r, sc, sf = fr.conv_case_inputs(case)
    res = r if with_res else None
    op = make_conv(case, wt, b, act)
    pargs = None
    if post:
        pargs = (sc, sf, "relu", post)
        op.set_post(*pargs)
    pre, mag, k = fr.conv_parts_tf(x, wt, b, strides, padding, pads, res)
    ins = [conv_x(case, x)] + ([dev(r)] if with_res else [])
    return (lambda: op(None, None, ins)), (lambda s: fr.with_post(pre, mag, k, s, act, pargs))


def cand_dual(case):
    h, x, w1, w2, b1, b2, sc, sf = fr.dual_case_inputs(case)
    op = make_dual(case, w1, w2, b1, b2, "relu")
    pre, mag, k = fr.dual_parts(h, x, w1, w2, b1, b2, (case[6], case[6]))
    ins = [dev(h), dev(x)]
    return (lambda: op(None, None, ins)), (lambda s: fr.with_post(pre, mag, k, s, "relu", None))


def cand_matmul(m, k, n, act, out_f32, with_res, pad_n=False):
    x, w, b, r = fr.matmul_inputs(m, k, n)
    res = r if with_res else None
    op = FU.FusedMatMul(w, b, act, out_f32, DEV, True, "mm", pad_n=pad_n)
    pre, mag, _k = fr.matmul_parts(x, w, b, res)
    ins = [dev(x)] + ([dev(r)] if with_res else [])
    return (lambda: op(None, None, ins)), (lambda s: [kb.epilogue(pre, mag, k, s, act, out_f32)])


def cand_lnx():
    t = lnx_setup(m=130)
    x = t["x"]
    z64, _b = kb.lnx_ref(x, t["w"][0].t(), t["b"][0], "none", zr=x)
    z = z64.to(BF)                                   # a bf16 pre-LayerNorm sum (any will do: it is the input here)
    st = kb.row_partials(z, 2)
    ref, bound = lnx_input_side_ref(t, z, 2)
    ins = [dev(z), dev(st)]
    return (lambda: t["A"](None, t["g"].nodes["a"], ins)), (lambda s: [(ref, bound)])


CANDIDATE_CASES = {
    "conv halo 3x3x64x72": lambda: cand_conv(3, 3, 64, 72, "same-odd-s1", False, (1, 1), "SAME", (0, 0, 0, 0)),
    "conv halo 3x3x128x72 explicit": lambda: cand_conv(3, 3, 128, 72, "explicit-s1", False, (1, 1), "EXPLICIT",
                                                        fr.EXPLICIT_PADS, "none", False),
    "conv halo 3x3x64x64 persist": lambda: cand_conv(3, 3, 64, 64, "same-even-s1", True, (1, 1), "SAME", (0, 0, 0, 0),
                                                      "relu", False),
    "conv halo post dual": lambda: cand_conv(3, 3, 64, 72, "same-even-s1", True, (1, 1), "SAME", (0, 0, 0, 0), "none",
                                             True, "dual"),
    "conv 3x3x64x72 top pad 3": lambda: cand_conv(3, 3, 64, 72, "explicit-p3", False, (1, 1), "EXPLICIT", (3, 0, 1, 2)),
    "conv aligned 3x3x64x72 s2": lambda: cand_conv(3, 3, 64, 72, "same-even-s2", True, (2, 2), "SAME", (0, 0, 0, 0)),
    "conv aligned 3x3x64x72 s12": lambda: cand_conv(3, 3, 64, 72, "same-s12", True, (1, 2), "SAME", (0, 0, 0, 0)),
    "conv aligned 1x1x64x72 dense": lambda: cand_conv(1, 1, 64, 72, "valid", False, (1, 1), "VALID", (0, 0, 0, 0)),
    "conv aligned 1x1x64x72 s2": lambda: cand_conv(1, 1, 64, 72, "same-odd-s2", False, (2, 2), "SAME", (0, 0, 0, 0)),
    "conv bf16 3x3x24x40": lambda: cand_conv(3, 3, 24, 40, "same-even-s2", True, (2, 2), "SAME", (0, 0, 0, 0)),
    "conv f32 3x3x12x8": lambda: cand_conv(3, 3, 12, 8, "same-odd-s1", False, (1, 1), "SAME", (0, 0, 0, 0)),
    "conv c4 7x7x3x16": lambda: cand_conv(7, 7, 3, 16, "same-even-s2", True, (2, 2), "SAME", (0, 0, 0, 0)),
    "conv c4 5x8x1x8": lambda: cand_conv(5, 8, 1, 8, "same-odd-s1", False, (1, 1), "SAME", (0, 0, 0, 0)),
    "dual s1": lambda: cand_dual(fr.DUAL_CASES[0]),
    "dual s2": lambda: cand_dual(fr.DUAL_CASES[1]),
    "matmul 88x72x64": lambda: cand_matmul(88, 64, 72, "gelu_tanh", False, True),
    "matmul 88x13x64 pad_n f32": lambda: cand_matmul(88, 64, 13, "none", True, False, pad_n=True),
    "matmul 88x13x72": lambda: cand_matmul(88, 72, 13, "tanh", False, False),
    "matmul deep 40x72x2048": lambda: cand_matmul(40, 2048, 72, "relu", False, True),
    "deferred-LN matmul": cand_lnx,
}


@pytest.mark.parametrize("name", list(CANDIDATE_CASES))
def test_every_candidate_the_tuner_would_time(picks, name):
    run, refs = CANDIDATE_CASES[name]()
    run()                                            # the untuned pick, recorded
    call = picks.last()
    untuned = call["offered"]
    assert untuned == untuned_pick(call)
    cands = ops.candidates(call["M"], call["N"], call["K"], **call["flags"])
    assert cands and len(set(cands)) == len(cands)
    if call["flags"]["no_split"]:
        assert all(s == 1 for _c, s in cands)
    accepted, rejected = [], []
    prev = hip().get_splitk_fixup()
    try:
        for pair in [untuned] + cands:
            want = None
            for fixup in ((1, 0) if pair[1] > 1 else (prev,)):
                hip().set_splitk_fixup(fixup)
                picks.force = pair
                try:
                    outs = run()
                except RuntimeError as e:
                    torch.cuda.synchronize()         # a launch rejection leaves the device fine; a fault would raise here
                    assert "needs" in str(e) or "launch failed" in str(e) or "config" in str(e), str(e)
                    rejected.append(pair)
                    break
                want = want or refs(pair[1])
                assert len(outs) == len(want)
                for i, (y, (ref, bound)) in enumerate(zip(outs, want)):
                    within("candidates: " + name.split(" ")[0], y, ref, bound,
                           f"{name}: pair {pair} fixup {fixup} output {i}")
            else:
                accepted.append(pair)
    finally:
        hip().set_splitk_fixup(prev)
        picks.force = None
    REJECTED[name] = dict(pairs=len(cands), max_splits=max(s for _c, s in cands),
                          rejected_configs=sorted({c for c, _s in rejected}))
    assert accepted, f"{name}: no candidate launched"
    assert untuned in accepted, f"{name}: the untuned pick {untuned} was rejected"
    bad = sorted({c for c, _s in rejected if c not in ops.BGEMM and c != ops.HALO_PERSIST})
    assert not bad, f"{name}: configs {bad} are listed by ops.candidates() but rejected at launch"
    # a config is taken or rejected whole, whatever the split
    assert not {c for c, _s in rejected} & {c for c, _s in accepted}
    if "deep" in name:
        assert {8, 16} <= {s for _c, s in accepted}


# ================================================================== (c) keys
def test_convs_that_differ_in_column_stride_do_not_share_a_pick(picks):
    """3x3, 64 channels, the same input: (sh, sw) = (1, 1) may run a halo
    config, (1, 2) may not.  A pick recorded for the first must not be what
    the second is offered."""
    shape = (3, 3, 64, 72)
    c11 = (shape, ("same-even-s1", True, (1, 1), "SAME", (0, 0, 0, 0)))
    c12 = (shape, ("same-s12", True, (1, 2), "SAME", (0, 0, 0, 0)))
    x, wt, b, _r, _sc, _sf = fr.conv_case_inputs(c11)
    op11, op12 = make_conv(c11, wt, b), make_conv(c12, wt, b)
    xd = dev(x.to(BF))
    op11(None, None, [xd])
    k11 = picks.last()["key"]
    assert picks.last()["flags"]["halo"]
    ops._TUNED[k11] = (48, 1)                       # a halo pick, as the tuner would record it
    y = op11(None, None, [xd])[0]
    assert picks.last()["offered"] == (48, 1)
    (ref, bound), = fr.conv_ref(x, wt, b, (1, 1), "SAME")
    within("FusedConv aligned", y, ref, bound, "forced halo pick")
    y = op12(None, None, [xd])[0]
    call = picks.last()
    assert call["key"] != k11 and not call["flags"]["halo"]
    assert call["offered"] == untuned_pick(call) and call["offered"] != (48, 1)
    (ref, bound), = fr.conv_ref(x, wt, b, (1, 2), "SAME", splits=call["offered"][1])
    within("FusedConv aligned", y, ref, bound, "(1, 2) beside a recorded (1, 1) pick")
    # and the other way round
    ops._TUNED.clear()
    ops._TUNED[call["key"]] = (36, 2)
    op11(None, None, [xd])
    assert picks.last()["offered"] == untuned_pick(picks.last())
    # a top pad beyond the halo kernel's reach: same input shape, its own key
    c3 = (shape, ("explicit-p3", True, (1, 1), "EXPLICIT", (3, 0, 1, 2)))
    ops._TUNED.clear()
    ops._TUNED[k11] = (48, 1)
    make_conv(c3, wt, b)(None, None, [xd])
    assert picks.last()["key"] != k11 and not picks.last()["flags"]["halo"]
    assert picks.last()["offered"] == untuned_pick(picks.last())


def test_square_stride_keys_are_the_committed_table_s(picks):
    """Every key of the committed table parses and has the layout the ops
    build today; a square-stride conv / dual conv / matmul builds exactly it."""
    with open(os.path.join(os.path.dirname(ops.__file__), "tuned_mi355x.json")) as f:
        doc = json.load(f)
    arity = {"conv": 10, "dual": 7, "mm": (7, 8), "chain": 7, "mmx": 10, "mmln": 5}
    for text, v in doc["picks"].items():
        key = eval(text, {"torch": torch, "__builtins__": {}})
        assert isinstance(key, tuple) and key[0] in arity and repr(key) == text
        want = arity[key[0]]
        assert len(key) in (want if isinstance(want, tuple) else (want,)), text
        assert len(v) == 2 and int(v[0]) in ops.TILES or key[0] in ("chain", "mmln")
    case = ((3, 3, 64, 72), ("same-even-s2", True, (2, 2), "SAME", (0, 0, 0, 0)))
    x, wt, b, r, _sc, _sf = fr.conv_case_inputs(case)
    make_conv(case, wt, b, "relu")(None, None, [dev(x.to(BF)), dev(r)])
    assert picks.last()["key"] == ("conv", (5, 8, 10, 64), BF, 72, 3, 3, 2, True, "relu", None)
    h, x2, w1, w2, b1, b2, _sc, _sf = fr.dual_case_inputs(fr.DUAL_CASES[1])
    make_dual(fr.DUAL_CASES[1], w1, w2, b1, b2, "relu")(None, None, [dev(h), dev(x2)])
    assert picks.last()["key"] == ("dual", tuple(h.shape), tuple(x2.shape), 72, 2, "relu", None)


# ================================================================== (d) tiny graphs through the passes
def _builder():
    from rust_tensorflow_serving2_amd.graph.builder import DType, GraphBuilder
    from rust_tensorflow_serving2_amd.utils import tensors as T
    return GraphBuilder(), DType(T.DT_FLOAT), T


def _conv_node(g, f32, x, name, w, stride=1):
    return g.node("Conv2D", name, [x, g.const(name + "/w", w.numpy())], T=f32, strides=[1, stride, stride, 1],
                  padding="SAME", data_format="NHWC", dilations=[1, 1, 1, 1], use_cudnn_on_gpu=True,
                  explicit_paddings=[])


BN_EPS = 1e-3


def _bn_params(c, seed):
    """Distinct per-channel parameters: a fold along the wrong axis of a 64 x 64 filter still type-checks."""
    gamma = 1.0 + 0.5 * torch.sin(torch.arange(c) * 0.37 + seed)
    beta = 0.3 * torch.cos(torch.arange(c) * 0.91 + seed)
    mean = 0.2 * torch.sin(torch.arange(c) * 1.7 + seed)
    var = 0.5 + (torch.arange(c) % 7).float() * 0.25 + 0.01 * seed
    return gamma, beta, mean, var


def _bn_node(g, f32, x, name, params):
    cs = [g.const(f"{name}/{n}", p.numpy()) for n, p in zip(("gamma", "beta", "mean", "var"), params)]
    return g.node("FusedBatchNormV3", name, [x] + cs, T=f32, U=f32, epsilon=BN_EPS, data_format="NHWC",
                  is_training=False, exponential_avg_factor=1.0)


def _fold64(w, bias, params):
    """The test's own fp64 fold: w' = w scale, b' = (bias - mean) scale + beta."""
    gamma, beta, mean, var = (p.double() for p in params)
    scale = gamma / torch.sqrt(var + BN_EPS)
    prod = (bias.double() - mean) * scale
    # b' in fp32: the subtraction, the scale (var + eps, rsqrt, times gamma: 3.5 roundings), the product
    # and the final addition -> 6.5 2^-24 |prod| + 2^-24 |beta|
    return w.double() * scale, prod + beta, 7 * kb.U_F32 * (prod.abs() + beta.abs()), scale, beta - mean * scale


def _check_folded(op_w_hwio, op_b, w64, b64, bslack, what):
    err = (op_w_hwio.double().cpu() - w64).abs()
    assert (err <= kb.U_BF16 * w64.abs()).all(), f"{what}: folded weights off by up to {(err / w64.abs()).max():.3g} relative"
    kb.assert_within(op_b, b64, bslack, f"{what}: folded bias")


def _compile(g, feeds, fetch):
    from rust_tensorflow_serving2_amd.graph.compiler import compile_program
    from rust_tensorflow_serving2_amd.graph.ir import from_graph_def
    return compile_program(from_graph_def(g.graph), [f + ":0" for f in feeds], [fetch + ":0"], device=DEV,
                           passes=FU.default_passes())


def _impls(prog, op):
    return [node.attrs["_impl"] for _fn, node, _i, _o in prog.steps if node.op == op]


def test_graph_conv_bias_bn_add_relu(picks):
    g, f32, T = _builder()
    c = 64
    w = rnd(3, 3, c, c, scale=1 / 24, seed=1)
    bias = rnd(c, scale=0.3, seed=2)
    params = _bn_params(c, 1)
    x = g.placeholder("x", T.DT_FLOAT, [-1, 7, 9, c])
    r = g.placeholder("r", T.DT_FLOAT, [-1, 7, 9, c])
    y = _conv_node(g, f32, x, "conv", w)
    y = g.node("BiasAdd", "bias", [y, g.const("b", bias.numpy())], T=f32, data_format="NHWC")
    y = _bn_node(g, f32, y, "bn", params)
    y = g.node("AddV2", "add", [y, r], T=f32)
    out = g.node("Relu", "relu", [y], T=f32)
    prog = _compile(g, ["x", "r"], out)
    assert prog.op_histogram() == {"_FusedConv2D": 1}
    op, = _impls(prog, "_FusedConv2D")
    assert (op.act, op.padding, (op.sh, op.sw), op.post) == ("relu", "SAME", (1, 1), None)
    w64, b64, bslack, _s, _t = _fold64(w, bias, params)
    wu, pad = fr.unpack_dense(op.w.cpu(), 3, 3, c)
    assert not pad.numel() or not pad.float().any()
    _check_folded(wu, op.b, w64, b64, bslack, "conv + bias + BN")
    xs, rs = rnd(5, 7, 9, c, seed=3).to(BF), rnd(5, 7, 9, c, seed=4).to(BF)
    yv = prog.run([dev(xs), dev(rs)])[0]
    (ref, bound), = fr.conv_ref(xs, wu.float(), op.b.cpu(), (1, 1), "SAME", res=rs, act="relu",
                                splits=picks.last()["offered"][1])
    within("graph conv+bias+BN+add+relu", yv, ref, bound, "output")


def test_graph_v2_preactivation_pair_gets_a_dual_post_output(picks):
    """conv1's sum feeds BN -> Relu -> conv2 AND conv2's shortcut add: conv1
    writes [sum, relu(bn(sum))] in one launch."""
    g, f32, T = _builder()
    c = 64
    w1, w2 = rnd(3, 3, c, c, scale=1 / 24, seed=1), rnd(1, 1, c, c, scale=1 / 8, seed=2)
    params = _bn_params(c, 2)
    x = g.placeholder("x", T.DT_FLOAT, [-1, 8, 10, c])
    y1 = _conv_node(g, f32, x, "conv1", w1)
    pre = g.node("Relu", "relu", [_bn_node(g, f32, y1, "bn", params)], T=f32)
    y2 = _conv_node(g, f32, pre, "conv2", w2)
    out = g.node("AddV2", "add", [y2, y1], T=f32)
    prog = _compile(g, ["x"], out)
    assert prog.op_histogram() == {"_FusedConv2D": 2}
    op1, op2 = _impls(prog, "_FusedConv2D")
    assert (op1.kh, op1.post_mode, op1.act, op2.kh, op2.post, op2.act) == (3, "dual", "none", 1, None, "none")
    sc, sf, act2 = op1.post
    assert act2 == "relu"
    _w, _b, _bs, scale64, shift64 = _fold64(w1, torch.zeros(c), params)
    kb.assert_within(sc, scale64, 4 * kb.U_F32 * scale64.abs(), "post scale")
    kb.assert_within(sf, shift64, 7 * kb.U_F32 * ((params[2].double() * scale64).abs() + params[1].double().abs()),
                     "post shift")
    wu1, _p = fr.unpack_dense(op1.w.cpu(), 3, 3, c)
    wu2, _p = fr.unpack_dense(op2.w.cpu(), 1, 1, c)
    assert fr.same_bits(wu1.contiguous(), w1.to(BF)) and fr.same_bits(wu2.contiguous(), w2.to(BF))
    assert not op1.b.any() and not op2.b.any()
    xs = rnd(5, 8, 10, c, seed=3).to(BF)
    yv = prog.run([dev(xs)])[0]
    s1, s2 = picks.calls[-2]["offered"][1], picks.calls[-1]["offered"][1]
    (r1, d1), (rz, dz) = fr.conv_ref(xs, wu1.float(), op1.b.cpu(), (1, 1), "SAME", splits=s1,
                                     post=(sc.cpu(), sf.cpu(), "relu", "dual"))
    # conv2 reads the stored z and adds the stored y1: their elementwise bounds propagate through |W2| and the add
    pre2, mag2, k2 = fr.conv_parts_tf(rz, wu2.float(), op2.b.cpu(), (1, 1), "SAME", res=r1)
    acc = kb.acc_bound(pre2, mag2, k2, s2, "none") + (dz.reshape(-1, c) @ wu2.double().reshape(c, c).abs()).reshape(d1.shape) + d1
    within("graph v2 pre-activation pair", yv, pre2, kb.out_bound(pre2, acc, False), "output")
    # and the two outputs of conv1 themselves
    o1, oz = op1(None, None, [dev(xs)])
    within("graph v2 pre-activation pair", o1, r1, d1, "conv1 sum")
    within("graph v2 pre-activation pair", oz, rz, dz, "conv1 post output")


def test_graph_projecting_block_becomes_a_dual_conv(picks):
    g, f32, T = _builder()
    c = 64
    wa, wb = rnd(1, 1, c, c, scale=1 / 8, seed=1), rnd(1, 1, c, c, scale=1 / 8, seed=2)
    pa, pb = _bn_params(c, 3), _bn_params(c, 4)
    h = g.placeholder("h", T.DT_FLOAT, [-1, 4, 5, c])
    x = g.placeholder("x", T.DT_FLOAT, [-1, 8, 9, c])
    ya = _bn_node(g, f32, _conv_node(g, f32, h, "expand", wa), "bn_a", pa)
    yb = _bn_node(g, f32, _conv_node(g, f32, x, "project", wb, stride=2), "bn_b", pb)
    out = g.node("Relu", "relu", [g.node("AddV2", "add", [ya, yb], T=f32)], T=f32)
    prog = _compile(g, ["h", "x"], out)
    assert prog.op_histogram() == {"_FusedDualConv": 1}
    op, = _impls(prog, "_FusedDualConv")
    assert (op.c1, op.c2, op.cout, op.sh, op.sw, op.act) == (c, c, c, 2, 2, "relu")
    wa64, ba64, sa, _s, _t = _fold64(wa, torch.zeros(c), pa)
    wb64, bb64, sb, _s, _t = _fold64(wb, torch.zeros(c), pb)
    g1, g2, pad = fr.unpack_dual(op.w.cpu(), c, c)
    assert not pad.numel()
    _check_folded(g1.reshape(1, 1, c, c), op.b, wa64, ba64 + bb64, sa + sb + kb.U_F32 * (ba64 + bb64).abs(),
                  "expand + BN (bias: both folds summed)")
    _check_folded(g2.reshape(1, 1, c, c), op.b, wb64, ba64 + bb64, sa + sb + kb.U_F32 * (ba64 + bb64).abs(),
                  "project + BN")
    hs, xs = rnd(5, 4, 5, c, seed=5).to(BF), rnd(5, 8, 9, c, seed=6).to(BF)
    yv = prog.run([dev(hs), dev(xs)])[0]
    zero = torch.zeros(c)
    (ref, bound), = fr.dual_ref(hs, xs, g1.float().reshape(1, 1, c, c), g2.float().reshape(1, 1, c, c), op.b.cpu(), zero,
                                (2, 2), "relu", picks.last()["offered"][1])
    within("graph projecting block", yv, ref, bound, "output")


def test_zz_report_worst_ratios():
    """Not a check: writes the worst err / bound per op class and the
    candidates each case rejected when asked to."""
    path = os.environ.get("FUSED_OPS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"worst": dict(sorted(WORST.items())), "rejected": REJECTED}, f, indent=1)
    assert all(v <= 1.0 for v in WORST.values())
