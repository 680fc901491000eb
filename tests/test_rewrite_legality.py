"""The fusion passes on graphs that are not the zoo's (CPU).

Every case of rewrite_cases.py, and 200 seeded random graphs, are compiled
twice -- without passes (the interpreter) and with default_passes() -- and run:

* every fetch has the same shape and dtype in both programs;
* the fused program's op histogram is the case's;
* a graph the passes must leave alone equals the interpreter bit for bit;
* a rewritten graph is within the fp32 folding error of the ORIGINAL graph's
  fp64 value -- and so is the interpreter, which checks the reference itself.
  The bound is kernel_bounds.acc_bound per rewrite_cases.Aff, with no
  tolerance of its own;
* a program that raises fails (except where the case says the graph cannot be
  served, and then both must refuse it).
"""
import math
import random

import numpy as np
import pytest
import torch

import kernel_bounds as kb
import rewrite_cases as rc
from kernel_bounds import E


def compile_both(g, feeds, fetches, device=torch.device("cpu")):
    from rust_tensorflow_serving2_amd.graph.compiler import compile_program
    from rust_tensorflow_serving2_amd.graph.fused import default_passes
    from rust_tensorflow_serving2_amd.graph.ir import from_graph_def
    plain = compile_program(from_graph_def(g.graph), feeds, fetches, device=device)
    fused = compile_program(from_graph_def(g.graph), feeds, fetches, device=device, passes=default_passes())
    return plain, fused


def same_bits(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_floating_point():
        return torch.equal(a.contiguous().view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                           b.contiguous().view(torch.int32 if b.dtype == torch.float32 else torch.int16))
    return torch.equal(a, b)


def check_histogram(case, hist, gpu=False):
    must = case.must_gpu if gpu else case.must
    for op, count in must.items():
        assert hist.get(op, 0) == count, f"{op}: {hist.get(op, 0)} != {count} in {hist}"
    extra = set(hist) - set(must) - set(case.maybe)
    assert not extra, f"unexpected ops {sorted(extra)} in {hist}"


def check_same_signature(a, b, fetches):
    for name, u, v in zip(fetches, a, b):
        u, v = torch.as_tensor(u), torch.as_tensor(v)
        assert tuple(u.shape) == tuple(v.shape), f"{name}: fused shape {tuple(v.shape)} != {tuple(u.shape)}"
        assert u.dtype == v.dtype, f"{name}: fused dtype {v.dtype} != {u.dtype}"


@pytest.mark.parametrize("entry", rc.CASES, ids=lambda e: e.id)
def test_case(entry):
    from rust_tensorflow_serving2_amd.graph import ops as O
    case = entry.build()
    plain, fused = compile_both(case.b.g, case.b.feeds, case.fetches)
    if case.raises:
        texts = []
        for prog in (plain, fused):
            with pytest.raises(O.OpError if case.raises == "OpError" else O.Unsupported) as refusal:
                prog.run(list(case.b.inputs))
            texts.append(str(refusal.value))
        if case.raises == "OpError":
            check_histogram(case, fused.op_histogram())
            assert texts[0] == texts[1], f"the fused program's error differs: {texts}"
        return
    a, b = plain.run(list(case.b.inputs)), fused.run(list(case.b.inputs))
    check_same_signature(a, b, case.fetches)
    check_histogram(case, fused.op_histogram())
    if case.exact:
        for name, u, v in zip(case.fetches, a, b):
            assert same_bits(u, v), f"{name}: the fused program differs from the interpreter"
    if case.ref is not None:
        for name, u, v, rb in zip(case.fetches, a, b, case.ref(False)):
            ref, bound = rb
            assert tuple(ref.shape) == tuple(torch.as_tensor(u).shape), f"{name}: reference shape {tuple(ref.shape)}"
            kb.assert_within(u, ref, bound, f"{entry.id} {name} (interpreter)")
            kb.assert_within(v, ref, bound, f"{entry.id} {name} (fused)")


def test_every_pass_has_a_positive_control():
    """A guard tightened until nothing fuses would pass every leave-alone case."""
    seen = set()
    for entry in rc.CASES:
        seen |= {op for op in entry.build().must if op.startswith("_")}
    cpu_ops = set(rc.FUSED_OPS) - {"_FusedDualConv", "_ChainConv", "_FusedMatMulLN"}     # device-only passes
    assert cpu_ops <= seen, sorted(cpu_ops - seen)


# ================================================================== seeded random graphs
# The generator builds the GraphDef and, in the same pass, its fp64 value with a
# running error bound that holds for fp32 arithmetic in either association
# order (rewrite_cases' model, per tensor instead of per chain):
#
#   val   the exact value of the original graph
#   mag   an envelope of the magnitudes the value is summed from
#         (|x| |w| |scales| + |addends|), >= |val|
#   err   the bound so far; a K-deep dot product adds kb.acc_bound (K + 4
#         roundings of mag) to the error its operand carries through |w|, an
#         elementwise step adds rc.STEP roundings of mag, a max-pool passes the
#         largest error in its window on, a mean adds kb.gap_ref's cnt + 2
#         roundings, tanh and softmax add kb.act_abs / kb.softmax_ref.
N_GRAPHS = 200
# a tap counts as "inside a would-be chain" when the tapped tensor has a conv / GEMM upstream with only chain
# links since (CHAIN_LINKS), and the op that reads it next is another link or the closing activation
CHAIN_ROOTS = ("Conv2D", "DepthwiseConv2dNative", "MatMul")
CHAIN_LINKS = ("BiasAdd", "FusedBatchNormV3", "Mul", "AddV2")
CHAIN_ENDS = ("Relu", "Relu6")
WATCHED = ("_FusedConv2D", "_FusedDepthwiseConv2D", "_FusedMatMul", "_GlobalAvgPool", "_MaxPool", "_SoftmaxArgMax")


class Val:
    def __init__(self, name, val, mag=None, err=None, op="Placeholder"):
        self.name, self.val, self.op = name, val, op
        self.mag = val.abs() if mag is None else mag
        self.err = torch.zeros_like(val) if err is None else err

    @property
    def shape(self):
        return list(self.val.shape)


class Gen:
    def __init__(self, seed):
        self.r = random.Random(seed)
        self.seed = seed
        self.b = rc.GB()
        self.fetches, self.checks = [], []          # checks: Val, or ("argmax", Val, axis)
        self.last_tap = None
        self.n = 0

    def uid(self, stem):
        self.n += 1
        return f"{stem}{self.n}"

    def data(self, shape, scale=1.0):
        self.n += 1
        return rc.bfv(kb.rnd(*shape, scale=scale, seed=1000 * self.seed + self.n)) if shape else \
            rc.bfv(kb.rnd(1, seed=1000 * self.seed + self.n)[0] * scale)

    def feed(self, shape, dyn=True):
        v = self.data(shape)
        return Val(self.b.ph(self.uid("in"), v, dyn_batch=dyn), kb.d(v))

    # ---- ops: each returns the new Val
    def linear(self, t, op, name, fn, k):
        val, mag = fn(t.val), fn(t.mag, True)
        err = fn(t.err, True) + kb.acc_bound(val, mag, k, 1, "none")
        return Val(name, val, mag, err, op)

    def conv(self, t, depthwise=False):
        import torch.nn.functional as F
        import fused_op_refs as fr
        r = self.r
        _b, h, w, c = t.shape
        k = r.choice([1, 3]) if not depthwise else 3
        s = r.choice([1, 1, 2]) if min(h, w) >= 4 else 1
        padding = r.choice(["SAME", "SAME", "VALID"]) if min(h, w) > k else "SAME"
        pre_pad = padding == "VALID" and k == 3 and r.random() < 0.5
        if pre_pad:
            t = self.maybe_tap(self.pad(t))
            _b, h, w, c = t.shape
        cout = c if depthwise else r.choice([4, 8, 8, 16])
        wt = self.data([k, k, c, 1 if depthwise else cout], 1.0 / math.sqrt(k * k * (1 if depthwise else c)))
        p = fr.tf_pads(h, w, k, k, s, s, padding)
        w64 = kb.d(wt)

        def fn(x, absolute=False):
            ww = w64.abs() if absolute else w64
            xx = F.pad(x.permute(0, 3, 1, 2), [p[2], p[3], p[0], p[1]])
            if depthwise:
                y = F.conv2d(xx, ww.permute(2, 3, 0, 1).reshape(c, 1, k, k), stride=s, groups=c)
            else:
                y = F.conv2d(xx, ww.permute(3, 2, 0, 1), stride=s)
            return y.permute(0, 2, 3, 1)
        nm = self.uid("dw" if depthwise else "conv")
        node = self.b.dw(t.name, wt, s, padding, nm) if depthwise else self.b.conv(t.name, wt, s, padding, nm)
        return self.linear(t, "DepthwiseConv2dNative" if depthwise else "Conv2D", node, fn, k * k * (1 if depthwise else c))

    def pad(self, t):
        import torch.nn.functional as F
        f = lambda x: F.pad(x, [0, 0, 1, 1, 1, 1])  # noqa: E731
        return Val(self.b.pad(t.name, [0, 0, 1, 1, 1, 1, 0, 0], self.uid("pad")), f(t.val), f(t.mag), f(t.err), "Pad")

    def matmul(self, t):
        k = t.shape[1]
        n = self.r.choice([4, 8, 10, 16])
        wt = self.data([k, n], 1.6 / math.sqrt(k))
        w64 = kb.d(wt)
        return self.linear(t, "MatMul", self.b.matmul(t.name, wt, self.uid("mm")),
                           lambda x, absolute=False: x @ (w64.abs() if absolute else w64), k)

    def bias(self, t):
        v = self.data([t.shape[-1]], 0.3)
        return self.addv(t, kb.d(v), self.b.bias(t.name, v, self.uid("bias")), "BiasAdd")

    def addv(self, t, v, node, op, vmag=None, verr=0.0):
        nt = Val(node, t.val + v, t.mag + (v.abs() if vmag is None else vmag), None, op)
        nt.err = t.err + verr + rc.STEP * E * nt.mag
        return nt

    def mulv(self, t, v, node):
        nt = Val(node, t.val * v, t.mag * v.abs(), None, "Mul")
        nt.err = t.err * v.abs() + rc.STEP * E * nt.mag
        return nt

    def bn(self, t):
        c = t.shape[-1]
        params = rc.bn_params(c, self.r.randrange(9))
        gamma, beta, mean, var = (kb.d(p) for p in params)
        inv = gamma / torch.sqrt(var + rc.BN_EPS)
        node = self.b.bn(t.name, params, self.uid("bn"))
        m = self.mulv(t, inv, node)
        out = self.addv(m, beta - mean * inv, node, "FusedBatchNormV3", beta.abs() + (mean * inv).abs())
        return out

    def const_shape(self, shape):
        r = self.r
        if len(shape) == 4:
            _b, h, w, c = shape
            return r.choice([[c], [c], [1, 1, 1, c], [], [w, 1], [1, w, 1], [h, 1, 1], [1, h, w, 1], [1, 1, w, c]])
        m, n = shape
        return r.choice([[n], [n], [1, n], [], [m, 1]])

    def scale(self, t):
        v = rc.wave(self.const_shape(t.shape), self.r.randrange(9))
        c = self.b.c(v, self.uid("k"))
        ins = (c, t.name) if self.r.random() < 0.3 else (t.name, c)
        return self.mulv(t, kb.d(v), self.b.bi("Mul", *ins, self.uid("mul")))

    def shift(self, t):
        v = rc.wave(self.const_shape(t.shape), self.r.randrange(9), -1.0, 1.0)
        return self.addv(t, kb.d(v), self.b.bi("AddV2", t.name, self.b.c(v, self.uid("k")), self.uid("add")), "AddV2")

    def add_live(self, t, live):
        same = [u for u in live if u.shape == t.shape and u is not t]
        if same and self.r.random() < 0.6:
            u = self.r.choice(same)
        else:
            shape = self.const_shape(t.shape) if self.r.random() < 0.4 else t.shape
            if len(t.shape) == 4 and self.r.random() < 0.3:
                shape = [t.shape[0], 1, 1, t.shape[3]]
            u = self.feed(shape, dyn=shape == t.shape or (len(shape) == 4 and shape[0] == t.shape[0]))
        ins = (u.name, t.name) if self.r.random() < 0.3 else (t.name, u.name)
        return self.addv(t, u.val, self.b.bi("AddV2", *ins, self.uid("res")), "AddV2", u.mag, u.err)

    def act(self, t):
        op = self.r.choice(["Relu", "Relu", "Relu6", "Tanh"])
        node = self.b.un(op, t.name, self.uid(op.lower()))
        if op == "Tanh":
            val = torch.tanh(t.val)
            return Val(node, val, val.abs(), t.err + kb.act_abs("tanh", t.val) + E * val.abs(), op)
        val = t.val.clamp(0.0, 6.0) if op == "Relu6" else torch.relu(t.val)
        return Val(node, val, t.mag, t.err, op)

    def maxpool(self, t):
        import torch.nn.functional as F
        import fused_op_refs as fr
        _b, h, w, _c = t.shape
        k, s = self.r.choice([(2, 2), (3, 2), (3, 1), (2, 1)])
        padding = self.r.choice(["SAME", "VALID", "EXPLICIT"]) if min(h, w) >= k else "SAME"
        ep = [0, 0, 1, 0, 0, 1, 0, 0] if padding == "EXPLICIT" else []
        p = fr.tf_pads(h, w, k, k, s, s, padding, (1, 0, 0, 1))

        def pool(x, fill):
            xp = F.pad(x.permute(0, 3, 1, 2), [p[2], p[3], p[0], p[1]], value=fill)
            return F.max_pool2d(xp, k, s).permute(0, 2, 3, 1)
        node = self.b.maxpool(t.name, k, s, padding, ep, name=self.uid("pool"))
        return Val(node, pool(t.val, float("-inf")), pool(t.mag, 0.0), pool(t.err, 0.0), "MaxPool")

    def mean(self, t):
        axes, keep = self.r.choice([[1, 2], [1, 2], [2, 1], [-3, -2]]), self.r.random() < 0.4
        ax = sorted(a % len(t.shape) for a in axes)
        cnt = int(np.prod([t.shape[a] for a in ax]))
        f = lambda x: x.mean(ax, keepdim=keep)  # noqa: E731
        node = self.b.mean(t.name, axes, keep, self.uid("mean"))
        return Val(node, f(t.val), f(t.mag), f(t.err) + (cnt + 2) * E * f(t.mag), "Mean")

    def reshape(self, t, shape):
        f = lambda x: x.reshape(shape)  # noqa: E731
        node = self.b.reshape(t.name, shape, self.uid("reshape"))
        return Val(node, f(t.val), f(t.mag), f(t.err), "Reshape")

    def softmax_argmax(self, t):
        axis = self.r.choice([-1, 1] if len(t.shape) == 2 else [-1, 1, 2])
        p, bound = kb.softmax_ref(t.val, t.err)
        sm = self.b.un("Softmax", t.name, self.uid("softmax"))
        am = self.b.argmax(t.name, axis, self.r.choice(["int64", "int32"]), self.uid("argmax"))
        self.fetches += [sm, am]
        self.checks += [Val(sm, p, p, bound), ("argmax", t, axis)]

    def maybe_tap(self, t, p=0.45):
        """Fetch t, or give it a second reader, and remember it: if the next
        op continues a chain the tap sits inside a would-be fused chain."""
        self.last_tap = None
        if self.r.random() < p and t.op != "Placeholder":
            if self.r.random() < 0.5:
                self.fetches.append(t.name)
                self.checks.append(t)
            else:
                u = Val(self.b.un("Tanh", t.name, self.uid("side")), torch.tanh(t.val))
                u.err = t.err + kb.act_abs("tanh", t.val) + E * u.val.abs()
                self.fetches.append(u.name)
                self.checks.append(u)
            self.last_tap = t.op
        return t

    def build(self):
        r = self.r
        h = r.choice([4, 6, 8])
        t = self.feed([2, h, r.choice([4, 6, 8]) if r.random() < 0.5 else h, r.choice([4, 8, 16])])
        live = [t]
        in_chain = rooted = False
        for _ in range(r.randrange(3, 9)):
            rank = len(t.shape)
            if rank == 4:
                ops = ["conv"] * 5 + ["dw"] * 4 + ["bias", "bn", "bn", "scale", "shift", "add_live", "add_live", "act",
                                                  "act", "maxpool", "maxpool", "mean", "mean", "flat"]
            elif rank == 2:
                ops = ["matmul"] * 5 + ["bias", "scale", "shift", "add_live", "act", "sa", "sa"]
            else:
                ops = ["sa"]
            kind = r.choice(ops)
            if kind in ("bias", "bn", "scale", "shift", "act") and t.op in ("Placeholder", "Reshape", "Mean", "MaxPool") \
                    and r.random() < 0.7:
                kind = "conv" if rank == 4 else "matmul"      # elementwise ops mostly follow a conv / GEMM
            tapped_in_chain = self.last_tap is not None and rooted
            if kind == "sa":
                self.softmax_argmax(t)
                break
            if kind == "flat":
                b_, hh, ww, cc = t.shape
                shape = r.choice([[-1, cc], [b_, hh * ww * cc], [b_, hh * ww, cc]])
                nt = self.reshape(t, [t.val.numel() // cc, cc] if shape[0] == -1 else shape)
            elif kind == "conv":
                nt = self.conv(t)
            elif kind == "dw":
                nt = self.conv(t, depthwise=True)
            elif kind == "add_live":
                nt = self.add_live(t, live)
            else:
                nt = getattr(self, kind)(t)
            if tapped_in_chain and nt.op in CHAIN_LINKS + CHAIN_ENDS:
                in_chain = True
            rooted = nt.op in CHAIN_ROOTS or (rooted and nt.op in CHAIN_LINKS)
            t = self.maybe_tap(nt)
            live.append(t)
        if not self.fetches or self.fetches[-1] != t.name:
            if len(t.shape) <= 3 and t.name not in self.fetches and r.random() < 0.5 and not any(
                    isinstance(c, tuple) for c in self.checks):
                self.softmax_argmax(t)
            if t.name not in self.fetches:
                self.fetches.append(t.name)
                self.checks.append(t)
        self.in_chain = in_chain
        return self


def run_generated(seed):
    gen = Gen(seed).build()
    fetches = [f + ":0" for f in gen.fetches]
    plain, fused = compile_both(gen.b.g, gen.b.feeds, fetches)
    a, b = plain.run(list(gen.b.inputs)), fused.run(list(gen.b.inputs))
    check_same_signature(a, b, fetches)
    for name, u, v, chk in zip(fetches, a, b, gen.checks):
        if isinstance(chk, tuple):
            _tag, t, axis = chk
            # classes are compared where the top-2 gap clears twice the logits' error bound
            top2 = t.val.topk(2, axis).values
            clear = (top2.select(axis, 0) - top2.select(axis, 1)) > 2 * t.err.amax(axis)
            want = t.val.argmax(axis)
            for who, got in (("interpreter", u), ("fused", v)):
                got = torch.as_tensor(got).long()
                assert got.shape == want.shape, f"seed {seed} {name} ({who}): shape {tuple(got.shape)}"
                assert torch.equal(got[clear], want[clear]), f"seed {seed} {name} ({who}): classes differ"
            continue
        bound = chk.err + kb.U_F32 * chk.val.abs()
        kb.assert_within(u, chk.val, bound, f"seed {seed} {name} (interpreter)")
        kb.assert_within(v, chk.val, bound, f"seed {seed} {name} (fused)")
    return fused.op_histogram(), gen.in_chain


@pytest.fixture(scope="module")
def generated():
    """The 200 programs, run once: per seed (histogram, tap inside a chain) or the failure."""
    out = {}
    for seed in range(N_GRAPHS):
        try:
            out[seed] = run_generated(seed)
        except Exception as e:       # noqa: BLE001  (reported per seed below, and as a failure)
            out[seed] = e
    return out


@pytest.mark.parametrize("seed", range(N_GRAPHS))
def test_generated_graph(generated, seed):
    if isinstance(generated[seed], Exception):
        raise generated[seed]


def test_generator_covers_the_passes(generated):
    """The generator cannot silently test nothing."""
    ok = [v for v in generated.values() if not isinstance(v, Exception)]
    assert len(ok) == N_GRAPHS, f"{N_GRAPHS - len(ok)} generated graphs failed"
    fused = sum(1 for h, _c in ok if any(op.startswith("_") for op in h))
    assert fused >= N_GRAPHS // 2, f"only {fused} programs hold a fused op"
    for op in WATCHED:
        n = sum(1 for h, _c in ok if op in h)
        assert n >= 10, f"{op} appears in {n} programs only"
    tapped = sum(1 for _h, c in ok if c)
    assert tapped >= 40, f"only {tapped} programs have a fetched or doubly-read intermediate inside a chain"
