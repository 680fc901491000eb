"""Small graphs that resemble, or are, the patterns the fusion passes rewrite.

A plain helper module like kernel_bounds.py (no fixtures, nothing at import
time).  Each case builds a GraphDef with GraphBuilder and says what the passes
must make of it and what the fetches must be:

    case.b         the builder (case.b.g.graph is the GraphDef), with its
                   feeds (case.b.feeds) and their arrays (case.b.inputs)
    case.fetches   tensor names
    case.must      {op: count} the fused program's histogram must hold
    case.maybe     ops it may hold besides (every other op must be absent)
    case.exact     the fused program equals the interpreter bit for bit (a
                   graph the passes leave alone, or whose rewritten part does
                   the interpreter's own arithmetic)
    case.ref(gpu)  [(fp64 reference, elementwise bound), ...] per fetch, from
                   the ORIGINAL graph's constants; gpu=False: fp32 arithmetic
                   in any association order (both CPU programs must sit inside
                   it), gpu=True: the HIP kernels' bounds (kernel_bounds.py)
    case.gpu       the device leg runs it (its reference is one fused op, or
                   fused ops whose stored intermediates the reference rounds)
    case.raises    both programs must refuse the graph with ops.Unsupported; "OpError": both must
                   refuse the batch with ops.OpError and the same text (case.must still holds)

Inputs and weights are bf16-valued, so one table serves both legs.  Constants
that a pass could apply along the wrong axis are distinct along every axis and
the sizes are chosen so that the wrong fold type-checks (Wo == H == Cout == 8,
batch == N == 4, S == cols == 16): a wrong fold then gives wrong numbers, not
an exception.

Bounds.  A fused chain is a K-deep dot product followed by per-element
multiplies and adds (bias, the BatchNorm affine, a scale, a residual).  `Aff`
tracks its value and its magnitude |x| |w| |scales| + |addends| in fp64; every
step costs either program at most 8 fp32 roundings of that magnitude (the
BatchNorm affine is the longest: var + eps, rsqrt, times gamma, mean times
that, beta minus, x times, plus = 7), whether it is applied to the
accumulator (the interpreter) or folded into the weights and the bias (the
pass), so the fp32 error is kb.acc_bound with K + 8 steps products.  On the
device the folded weights are rounded to bf16 once more, 2^-8 |x| |w'|, which
is added to the kernel's bound; the kernel's own terms are kb's, unchanged.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import fused_op_refs as fr
import gconv_bounds as gb
import kernel_bounds as kb
from kernel_bounds import BF, E, rnd

FUSED_OPS = ("_FusedConv2D", "_FusedDepthwiseConv2D", "_FusedGroupedConv2D", "_FusedDualConv", "_FusedMatMul",
             "_GlobalAvgPool", "_MaxPool",
             "_SoftmaxArgMax", "_LayerNorm", "_FusedQKV", "_Attention", "_EmbeddingLN", "_KeyMaskAdder",
             "_DenseSoftmax", "_ClassifierHead", "_StemPool", "_ChainConv", "_FusedMatMulLN")
BN_EPS = 1e-3
STEP = 8            # fp32 roundings per folded elementwise step (see the module docstring)


def bfv(t):
    """bf16-valued fp32."""
    return t.to(BF).float()


def wave(shape, seed, lo=0.5, hi=1.5):
    """A bf16-valued constant that differs along every axis (no two entries of
    a row, column or plane agree), positive."""
    n = int(np.prod(shape))
    i = torch.arange(n, dtype=torch.float32)
    return bfv(lo + (hi - lo) * (0.5 + 0.5 * torch.sin(i * 0.737 + seed))).reshape(shape)


def bn_params(c, seed):
    """Distinct per channel (test_fused_ops_gpu._bn_params explains why)."""
    i = torch.arange(c)
    return (1.0 + 0.5 * torch.sin(i * 0.37 + seed), 0.3 * torch.cos(i * 0.91 + seed),
            0.2 * torch.sin(i * 1.7 + seed), 0.5 + (i % 7).float() * 0.25 + 0.01 * seed)


# ---------------------------------------------------------------- the builder
class GB:
    """GraphBuilder with the feeds' arrays and one-line TF ops."""

    def __init__(self):
        from rust_tensorflow_serving2_amd.graph.builder import DType, GraphBuilder
        from rust_tensorflow_serving2_amd.utils import tensors as T
        self.g, self.T = GraphBuilder(), T
        self.f32, self.i32, self.i64 = DType(T.DT_FLOAT), DType(T.DT_INT32), DType(T.DT_INT64)
        self.feeds, self.inputs = [], []

    def ph(self, name, value, dyn_batch=True):
        shape = list(value.shape)
        if dyn_batch and shape:
            shape[0] = -1
        dt = self.T.DT_FLOAT if value.is_floating_point() else self.T.DT_INT32
        n = self.g.placeholder(name, dt, shape)
        self.feeds.append(n + ":0")
        self.inputs.append(value)
        return n

    def c(self, value, name="c"):
        a = value.detach().numpy() if torch.is_tensor(value) else np.asarray(value, np.float32)
        return self.g.const(name, a)

    def ints(self, v, name="i"):
        return self.g.const(name, np.asarray(v, np.int32))

    def n(self, op, name, ins, **attrs):
        return self.g.node(op, name, list(ins), T=self.f32, **attrs)

    def conv(self, x, w, stride=1, padding="SAME", name="conv", fmt="NHWC", dil=1, ep=()):
        w = w if isinstance(w, str) else self.c(w, name + "/w")
        s = [1, stride, stride, 1] if fmt == "NHWC" else [1, 1, stride, stride]
        dl = [1, dil, dil, 1] if fmt == "NHWC" else [1, 1, dil, dil]
        return self.n("Conv2D", name, [x, w], strides=s, padding=padding, data_format=fmt, dilations=dl,
                      use_cudnn_on_gpu=True, explicit_paddings=list(ep))

    def dw(self, x, w, stride=1, padding="SAME", name="dw", fmt="NHWC", dil=1, ep=()):
        w = w if isinstance(w, str) else self.c(w, name + "/w")
        s = [1, stride, stride, 1] if fmt == "NHWC" else [1, 1, stride, stride]
        dl = [1, dil, dil, 1] if fmt == "NHWC" else [1, 1, dil, dil]
        return self.n("DepthwiseConv2dNative", name, [x, w], strides=s, padding=padding, data_format=fmt,
                      dilations=dl, explicit_paddings=list(ep))

    def bias(self, x, b, name="bias"):
        return self.n("BiasAdd", name, [x, b if isinstance(b, str) else self.c(b, name + "/b")], data_format="NHWC")

    def bn(self, x, params, name="bn", training=False):
        cs = [p if isinstance(p, str) else self.c(p, f"{name}/{k}")
              for k, p in zip(("gamma", "beta", "mean", "var"), params)]
        return self.g.node("FusedBatchNormV3", name, [x] + cs, T=self.f32, U=self.f32, epsilon=BN_EPS,
                           data_format="NHWC", is_training=training, exponential_avg_factor=1.0)

    def pad(self, x, pads, name="pad"):
        return self.n("Pad", name, [x, self.ints(np.asarray(pads).reshape(-1, 2), name + "/p")], Tpaddings=self.i32)

    def matmul(self, x, w, name="mm", ta=False, tb=False):
        return self.n("MatMul", name, [x, w if isinstance(w, str) else self.c(w, name + "/w")], transpose_a=ta,
                      transpose_b=tb)

    def mean(self, x, axes, keep=False, name="mean"):
        return self.n("Mean", name, [x, self.ints(axes, name + "/axes")], Tidx=self.i32, keep_dims=keep)

    def maxpool(self, x, k=3, s=2, padding="SAME", ep=(), fmt="NHWC", ksize=None, name="pool"):
        ks = ksize or ([1, k, k, 1] if fmt == "NHWC" else [1, 1, k, k])
        st = [1, s, s, 1] if fmt == "NHWC" else [1, 1, s, s]
        return self.n("MaxPool", name, [x], ksize=ks, strides=st, padding=padding, data_format=fmt,
                      explicit_paddings=list(ep))

    def argmax(self, x, axis, out="int64", name="argmax"):
        dt = self.i64 if out == "int64" else self.i32
        return self.n("ArgMax", name, [x, self.ints(axis, name + "/axis")], Tidx=self.i32, output_type=dt)

    def reshape(self, x, shape, name="reshape"):
        return self.n("Reshape", name, [x, self.ints(shape, name + "/shape")], Tshape=self.i32)

    def un(self, op, x, name=None):
        return self.n(op, name or op.lower(), [x])

    def bi(self, op, a, b, name=None):
        return self.n(op, name or op.lower(), [a, b])


# ---------------------------------------------------------------- references
class Aff:
    """A K-deep dot product and the elementwise steps after it, in fp64."""

    def __init__(self, pre, dot, k, bf16_w=True, k_gpu=None):
        self.pre, self.mag, self.dot, self.k = pre, dot, dot, k
        self.steps, self.wfold = 0, False
        self.bf16_w = bf16_w          # the kernel's weights are bf16 (the depthwise filter stays fp32)
        self.k_gpu = k_gpu or k       # the additions the kernel performs, where it pads K (gconv_bounds.k_slots)

    @classmethod
    def conv(cls, x, w_hwio, strides=(1, 1), padding="SAME", pads=(0, 0, 0, 0)):
        pre, mag, k = fr.conv_parts_tf(x, w_hwio, None, strides, padding, pads)
        return cls(pre, mag, k)

    @classmethod
    def dwconv(cls, x, w_hwc, strides=(1, 1), padding="SAME", pads=(0, 0, 0, 0)):
        kh, kw, c = w_hwc.shape
        pt, pb, pl, pr = fr.tf_pads(x.shape[1], x.shape[2], kh, kw, strides[0], strides[1], padding, pads)
        wt = kb.d(w_hwc).permute(2, 0, 1).reshape(c, 1, kh, kw)

        def run(xx, ww):
            return F.conv2d(F.pad(xx.permute(0, 3, 1, 2), [pl, pr, pt, pb]), ww, stride=tuple(strides),
                            groups=c).permute(0, 2, 3, 1)
        return cls(run(kb.d(x), wt), run(kb.d(x).abs(), wt.abs()), kh * kw, bf16_w=False)

    @classmethod
    def gconv(cls, x, w_hwio, strides=(1, 1), padding="SAME", pads=(0, 0, 0, 0)):
        """A grouped conv (the filter's in-depth divides the input's channels): kh kw Cg products per
        output; kernels/gconv.hip adds its zero-filled K padding too (gconv_bounds.k_slots)."""
        kh, kw, cg, _cout = w_hwio.shape
        p = fr.tf_pads(x.shape[1], x.shape[2], kh, kw, strides[0], strides[1], padding, pads)
        zero = torch.zeros(w_hwio.shape[3])
        pre, mag = gb.gconv_parts(x, w_hwio, zero, tuple(strides), p)
        return cls(pre, mag, kh * kw * cg, k_gpu=gb.k_slots(cg))

    @classmethod
    def mm(cls, x, w_kn):
        pre, mag, k = fr.matmul_parts(x, w_kn)
        return cls(pre, mag, k)

    def _next(self, pre, mag, dot, wfold=None):
        a = Aff.__new__(Aff)
        a.pre, a.mag, a.dot, a.k, a.bf16_w, a.k_gpu = pre, mag, dot, self.k, self.bf16_w, self.k_gpu
        a.steps, a.wfold = self.steps + 1, self.wfold if wfold is None else wfold
        return a

    def mul(self, v):
        v = kb.d(v)
        return self._next(self.pre * v, self.mag * v.abs(), self.dot * v.abs(), True)

    def add(self, v, vmag=None):
        v = kb.d(v)
        return self._next(self.pre + v, self.mag + (v.abs() if vmag is None else kb.d(vmag)), self.dot)

    def bn(self, params, eps=BN_EPS):
        gamma, beta, mean, var = (kb.d(p) for p in params)
        inv = gamma / torch.sqrt(var + eps)
        return self.mul(inv).add(beta - mean * inv, beta.abs() + (mean * inv).abs())

    def out(self, act="none", gpu=False, out_f32=None):
        """(ref, bound).  CPU: fp32 output.  GPU: the kernel's epilogue bound
        (bf16 output unless `out_f32`; GPU_SPLITS split-K slabs) plus the bf16
        rounding of folded weights."""
        out_f32 = (not gpu) or bool(out_f32)
        splits = GPU_SPLITS if gpu else 1
        k = (self.k_gpu if gpu else self.k) + STEP * self.steps
        if act == "relu6":        # Lipschitz 1, exact: the pre-activation's bound carries over
            ref, acc = self.pre.clamp(0.0, 6.0), kb.acc_bound(self.pre, self.mag, k, splits, "none")
        else:
            ref, acc = kb.act64(act, self.pre), kb.acc_bound(self.pre, self.mag, k, splits, act)
        if gpu and self.wfold and self.bf16_w:
            acc = acc + kb.L_ACT.get(act, 1.0) * kb.U_BF16 * self.dot
        return ref, kb.out_bound(ref, acc, out_f32)


GPU_SPLITS = 1          # the device leg sets it to the split-K count the op was given


def exact(ref):
    return kb.d(ref), 0.0


def classes_rb(logits, dlogit, axis=-1):
    """argmax over `axis`: exact where the top-2 gap clears twice the logit
    error (kb.argmax_checked's rule), any class elsewhere."""
    lg = kb.d(logits)
    top2 = lg.topk(2, axis).values
    clear = (top2.select(axis, 0) - top2.select(axis, 1)) > 2 * kb.d(dlogit).amax(axis)
    return lg.argmax(axis).double(), torch.where(clear, 0.0, float(lg.shape[axis]))


def mean_rb(x, axes, keep, gpu=False):
    """Mean over `axes`: cnt fp32 additions, the 1/cnt product and one more
    operation (kb.gap_ref's count), stored fp32 -- bf16 where the HIP pool runs
    (rank 4, H and W, C % 8 == 0)."""
    x = kb.d(x)
    axes = sorted({a % x.dim() for a in axes})
    cnt = int(np.prod([x.shape[a] for a in axes]))
    ref = x.mean(axes, keepdim=keep)
    acc = (cnt + 2) * E * x.abs().mean(axes, keepdim=keep)
    hip = gpu and x.dim() == 4 and axes == [1, 2] and x.shape[-1] % 8 == 0
    return ref, kb.out_bound(ref, acc, not hip)


def head_rb(x, w_kn, b, gpu=False):
    """softmax(mean_hw(x) @ w + b) -> (probs, bound, logits, logit error).  On the device
    kb.head_ref (the pooled row is rounded to bf16); in fp32 the pooling error
    goes through |W| and the GEMM adds kb.acc_bound."""
    k, n = w_kn.shape
    if gpu:
        return kb.head_ref(x, kb.d(w_kn).t(), b, n, ks=max(8, GPU_SPLITS))
    pooled, _b, gacc = kb.gap_ref(x)
    pre, mag = kb.gemm_parts(pooled, kb.d(w_kn).t(), b)
    dl = gacc @ kb.d(w_kn).abs() + kb.acc_bound(pre, mag, k, 1, "none")
    p, bound = kb.softmax_ref(pre, dl)
    return p, bound, pre, dl


# ---------------------------------------------------------------- the table
CASES = []


def case(group, gpu=False, **params):
    """Registers fn(**params) under `group` (the pass a failure names)."""
    def deco(fn):
        tag = "-".join(f"{k}={v}" for k, v in params.items())
        name = fn.__name__ + ("-" + tag if tag else "")
        CASES.append(SimpleNamespace(id=f"{group}:{name}", group=group, build=lambda: fn(**params), gpu=gpu))
        return fn
    return deco


def make(b, fetches, must=None, maybe=(), exact=False, ref=None, raises=False, must_gpu=None, ref_gpu=None):
    """must_gpu: the histogram on the device where a device-only pass (fuse_dual_conv,
    fuse_conv_chain) makes it differ.  ref_gpu: the device reference of a case that is
    compared with the interpreter on the CPU; default `ref`.  A reference that takes
    `prog` reads stored intermediates back from the device program's own ops and
    appends (value, ref, bound) checks of them after the fetches' pairs."""
    assert exact or raises or ref is not None
    return SimpleNamespace(b=b, fetches=[f if ":" in f else f + ":0" for f in fetches], must=dict(must or {}),
                           maybe=tuple(maybe), exact=exact, ref=ref, raises=raises, ref_gpu=ref_gpu or ref,
                           must_gpu=dict((must or {}) if must_gpu is None else must_gpu))


def alone(b, fetches, hist):
    """Nothing may be rewritten: the exact unfused histogram, bit-equal outputs."""
    return make(b, fetches, must=hist, exact=True)


# ================================================================== fuse_conv / fuse_depthwise / fuse_grouped_conv
B, H, W, C = 2, 8, 8, 8            # Wo == H == Cout: a scale along the wrong axis type-checks
CG = 4                             # the grouped filter's in-depth: two groups of C = 8 (kernels/gconv.hip takes 4)
LINKS = ["Pad", "Conv2D", "BiasAdd", "FusedBatchNormV3", "Mul", "AddV2", "Relu"]
# The three conv passes share one chain matcher (fused._match_conv_chain), so every near miss of the
# shared head is run for each kind of conv: kind -> (pass, conv op, fused op)
KINDS = {"dense": ("fuse_conv", "Conv2D", "_FusedConv2D"),
         "depthwise": ("fuse_depthwise", "DepthwiseConv2dNative", "_FusedDepthwiseConv2D"),
         "grouped": ("fuse_grouped_conv", "Conv2D", "_FusedGroupedConv2D")}


def conv_data(c=C, k=3, seed=0, cin=None, kind="dense"):
    cin = cin or c
    x = bfv(rnd(B, H, W, cin, seed=seed + 1))
    depth = {"dense": cin, "depthwise": 1, "grouped": CG}[kind]      # products per output: k k depth
    shape = (k, k, cin, 1) if kind == "depthwise" else (k, k, depth, c)
    w = bfv(rnd(*shape, scale=1.0 / math.sqrt(k * k * depth), seed=seed + 2))
    bias = bfv(rnd(c, scale=0.3, seed=seed + 3))
    r = bfv(rnd(B, H, W, c, seed=seed + 4))
    return x, w, bias, r


def kind_conv(b, kind, x, w, **kw):
    """The conv node of `kind` (GB.conv / GB.dw arguments)."""
    return b.dw(x, w, **kw) if kind == "depthwise" else b.conv(x, w, **kw)


def kind_aff(kind, x, w, strides=(1, 1), padding="SAME", pads=(0, 0, 0, 0)):
    if kind == "depthwise":
        return Aff.dwconv(x, w.reshape(w.shape[:3]), strides, padding, pads)
    return (Aff.gconv if kind == "grouped" else Aff.conv)(x, w, strides, padding, pads)


def _chain(tap, mode, act="Relu", kind="dense"):
    """Pad -> Conv -> BiasAdd -> BN -> Mul -> Add -> Relu with link `tap`
    fetched (mode "fetch") or read by a second op (a Tanh, mode "consumer").
    The depthwise and the grouped chain have no scale and no residual: their
    passes absorb neither."""
    _pass, conv_op, fused = KINDS[kind]
    dense = kind == "dense"
    x, w, bias, r = conv_data(seed=10, kind=kind)
    params, sv = bn_params(C, 1), wave([C], 2)
    b = GB()
    xs, rs = b.ph("x", x), b.ph("r", r)
    t = [b.pad(xs, [0, 0, 1, 1, 1, 1, 0, 0])]
    t.append(kind_conv(b, kind, t[-1], w, padding="VALID"))
    t.append(b.bias(t[-1], bias))
    t.append(b.bn(t[-1], params))
    links = ["Pad", conv_op, "BiasAdd", "FusedBatchNormV3"] + (["Mul", "AddV2"] if dense else []) + [act]
    if dense:
        t.append(b.bi("Mul", t[-1], b.c(sv, "scale"), "mul"))
        t.append(b.bi("AddV2", t[-1], rs, "add"))
    t.append(b.un(act, t[-1], "act"))
    fetches = [t[-1]]
    if tap is not None:
        fetches.append(t[tap] if mode == "fetch" else b.un("Tanh", t[tap], "tap"))
    must = {fused: 1}
    maybe = []
    if tap is not None:
        must.update({op: 1 for op in links[tap + 1:]} if tap else {"Pad": 1})
        if mode == "consumer":
            must["Tanh"] = 1
        elif links[tap] == "FusedBatchNormV3":
            must["FusedBatchNormV3"] = 1      # a fetched BatchNorm keeps running as itself
        if mode == "consumer" and dense and links[tap] == "BiasAdd":
            # conv + bias with two readers, one of them a BatchNorm: fuse_post_activation
            # may write the BatchNorm as the conv's second output (CPU; 64-channel convs on the device)
            del must["FusedBatchNormV3"]
            maybe = ["FusedBatchNormV3"]

    def ref(gpu=False):
        base = kind_aff(kind, x, w, (1, 1), "EXPLICIT", (1, 1, 1, 1))
        a = [None, base, base.add(bias)]
        a.append(a[-1].bn(params))
        if dense:
            a.append(a[-1].mul(sv))
            a.append(a[-1].add(r))
        out = [a[-1].out(act.lower(), gpu)]
        if tap is not None:
            if tap == 0:
                padded = F.pad(kb.d(x), [0, 0, 1, 1, 1, 1])
                out.append(exact(padded) if mode == "fetch" else (torch.tanh(padded), kb.act_abs("tanh", padded) +
                                                                  kb.U_F32 * torch.tanh(padded).abs()))
            else:
                out.append(a[tap].out("none" if mode == "fetch" else "tanh", gpu))
        return out
    return make(b, fetches, must, maybe, ref=ref)


@case("fuse_conv", gpu=True)
def conv_positive():
    return _chain(None, "fetch")


@case("fuse_conv", gpu=True)
def conv_positive_relu6():
    """A Relu6 after a residual add."""
    return _chain(None, "fetch", act="Relu6")


@case("fuse_depthwise", gpu=True)
def depthwise_positive():
    return _chain(None, "fetch", act="Relu6", kind="depthwise")


@case("fuse_grouped_conv", gpu=True)
def grouped_positive():
    """C = 8 in two groups of 4: kernels/gconv.hip's smallest shape on the device."""
    return _chain(None, "fetch", kind="grouped")


def conv_chain_link(tap, mode):
    return _chain(LINKS.index(tap), mode)


def depthwise_chain_link(tap, mode):
    return _chain(["Pad", "DepthwiseConv2dNative", "BiasAdd", "FusedBatchNormV3"].index(tap), mode, "Relu6",
                  "depthwise")


def grouped_chain_link(tap, mode):
    return _chain(LINKS.index(tap), mode, kind="grouped")


for _mode in ("fetch", "consumer"):
    for _tap in LINKS[:6]:
        case("fuse_conv", tap=_tap, mode=_mode)(conv_chain_link)
    for _tap in ("Pad", "DepthwiseConv2dNative", "BiasAdd", "FusedBatchNormV3"):
        case("fuse_depthwise", tap=_tap, mode=_mode)(depthwise_chain_link)
    for _tap in LINKS[:4]:
        case("fuse_grouped_conv", tap=_tap, mode=_mode)(grouped_chain_link)


def _conv_then(build_tail, must_tail, ref_tail, k=1, gpu_ok=True, extra_feeds=()):
    """conv k x k (SAME) -> build_tail(b, y, feeds) -> fetch."""
    x, w, _bias, _r = conv_data(k=k, seed=20)
    b = GB()
    xs = b.ph("x", x)
    feeds = [b.ph(n, v, dyn) for n, v, dyn in extra_feeds]
    y = build_tail(b, b.conv(xs, w), feeds)
    must = {"_FusedConv2D": 1}
    must.update(must_tail)
    return make(b, [y], must, ref=lambda gpu=False: [ref_tail(Aff.conv(x, w), gpu)])


SCALE_SHAPES = {"C": [C], "111C": [1, 1, 1, C], "scalar": [], "C1": [C, 1], "1W1": [1, W, 1], "H11": [H, 1, 1]}


@case("fuse_conv", gpu=True, shape="C", first=False)
@case("fuse_conv", gpu=True, shape="C", first=True)
@case("fuse_conv", gpu=True, shape="111C", first=False)
@case("fuse_conv", gpu=True, shape="scalar", first=False)
def conv_mul_const_folds(shape, first):
    sv = wave(SCALE_SHAPES[shape], 3)
    return _conv_then(
        lambda b, y, f: b.un("Relu", b.bi("Mul", *((b.c(sv, "s"), y) if first else (y, b.c(sv, "s"))), "mul")),
        {}, lambda a, gpu: a.mul(sv).out("relu", gpu))


@case("fuse_conv", shape="C1")
@case("fuse_conv", shape="1W1")
@case("fuse_conv", shape="H11")
def conv_mul_const_is_not_per_channel(shape):
    """C elements, but along W or H: folding it as a per-channel scale is wrong."""
    sv = wave(SCALE_SHAPES[shape], 3)
    return _conv_then(lambda b, y, f: b.un("Relu", b.bi("Mul", y, b.c(sv, "s"), "mul")), {"Mul": 1, "Relu": 1},
                      lambda a, gpu: a.mul(sv).out("relu", gpu))


@case("fuse_conv", gpu=True, other="B11C")
@case("fuse_conv", gpu=True, other="111C")
@case("fuse_conv", gpu=True, other="scalar")
def conv_add_broadcast_operand(other):
    """A non-constant operand that broadcasts against the conv output: taken
    as the residual, which the kernels read one element per output element."""
    shape, dyn = {"B11C": ([B, 1, 1, C], True), "111C": ([1, 1, 1, C], False), "scalar": ([], False)}[other]
    r = bfv(rnd(*shape, seed=31)) if shape else bfv(torch.tensor(0.75))
    return _conv_then(lambda b, y, f: b.un("Relu", b.bi("AddV2", y, f[0], "add")), {},
                      lambda a, gpu: a.add(r).out("relu", gpu), extra_feeds=[("r", r, dyn)])


@case("fuse_conv", gpu=True)
def conv_add_operand_larger_than_the_output():
    """conv of a [B,1,1,C] image plus a [B,H,W,C] tensor: the CONV output is
    the one that broadcasts, so the sum cannot be the kernel's residual add."""
    x, w, _bias, r = conv_data(k=1, seed=32)
    x = x[:, :1, :1, :].contiguous()
    b = GB()
    y = b.un("Relu", b.bi("AddV2", b.conv(b.ph("x", x), w), b.ph("r", r), "add"))

    def ref(gpu=False):
        if not gpu:
            return [Aff.conv(x, w).add(r).out("relu")]
        # the conv stores bf16; the add and the ReLU run on torch in fp32 and are stored as bf16 again
        c, d = Aff.conv(x, w).out("none", True)
        s = c + kb.d(r)
        return [(torch.relu(s), kb.out_bound(torch.relu(s), d + E * (c.abs() + kb.d(r).abs()), False))]
    return make(b, [y], {"_FusedConv2D": 1}, ref=ref)


@case("fuse_conv")
def conv_add_constant_plane():
    """A constant [1,H,W,1] is no bias and no residual: the Add stays."""
    cv = wave([1, H, W, 1], 4)
    return _conv_then(lambda b, y, f: b.un("Relu", b.bi("AddV2", y, b.c(cv, "plane"), "add")), {"AddV2": 1, "Relu": 1},
                      lambda a, gpu: a.add(cv).out("relu", gpu))


@case("fuse_conv")
def conv_added_to_itself():
    return _conv_then(lambda b, y, f: b.bi("AddV2", y, y, "add"), {"AddV2": 1}, lambda a, gpu: a.mul(torch.tensor(2.0)).out("none", gpu))


# ---- near misses of the shared head: the dense ones under their own names, then each for the other two kinds
@case("fuse_conv", which="batch")
@case("fuse_conv", which="channel")
def conv_pad_outside_hw(which, kind="dense"):
    """A Pad of the batch or the channel axis is not the conv's padding.  (The
    channel Pad also hides the channel count from _channels_of: the grouped
    conv behind it is fuse_conv's, and runs as Conv2D does.)"""
    full = C if kind == "grouped" else C + 2          # the conv's input channels behind a channel Pad
    x, w, _b, _r = conv_data(k=3, seed=40, cin=full if which == "channel" else C, kind=kind)
    if which == "channel":
        x = x[..., :full - 2]
    pads = [1, 0, 1, 1, 1, 1, 0, 0] if which == "batch" else [0, 0, 1, 1, 1, 1, 1, 1]
    b = GB()
    y = kind_conv(b, kind, b.pad(b.ph("x", x), pads), w, padding="VALID")
    xp = F.pad(x, [pads[6], pads[7], pads[4], pads[5], pads[2], pads[3], pads[0], pads[1]])
    fused = "_FusedConv2D" if (kind, which) == ("grouped", "channel") else KINDS[kind][2]
    return make(b, [y], {"Pad": 1, fused: 1},
                ref=lambda gpu=False: [kind_aff(kind, xp, w, (1, 1), "VALID").out("none", gpu)])


@case("fuse_conv")
def conv_pad_before_same(kind="dense"):
    x, w, _b, _r = conv_data(k=3, seed=41, kind=kind)
    b = GB()
    y = kind_conv(b, kind, b.pad(b.ph("x", x), [0, 0, 1, 1, 1, 1, 0, 0]), w, padding="SAME")
    xp = F.pad(x, [0, 0, 1, 1, 1, 1])
    return make(b, [y], {"Pad": 1, KINDS[kind][2]: 1}, ref=lambda gpu=False: [kind_aff(kind, xp, w).out("none", gpu)])


@case("fuse_conv")
def conv_explicit_paddings_with_a_batch_entry(kind="dense"):
    x, w, _b, _r = conv_data(k=3, seed=42, kind=kind)
    b = GB()
    y = kind_conv(b, kind, b.ph("x", x), w, padding="EXPLICIT", ep=[1, 0, 1, 1, 1, 1, 0, 0])
    return alone(b, [y], {KINDS[kind][1]: 1})


@case("fuse_conv")
def conv_explicit_paddings_with_a_channel_entry(kind="dense"):
    x, w, _b, _r = conv_data(k=3, seed=46, kind=kind)
    b = GB()
    y = kind_conv(b, kind, b.ph("x", x), w, padding="EXPLICIT", ep=[0, 0, 1, 1, 1, 1, 0, 1])
    return alone(b, [y], {KINDS[kind][1]: 1})


@case("fuse_conv")
def conv_nchw(kind="dense"):
    x, w, _b, _r = conv_data(k=3, seed=43, kind=kind)
    b = GB()
    y = b.un("Relu", kind_conv(b, kind, b.ph("x", x), w, fmt="NCHW"))
    return alone(b, [y], {KINDS[kind][1]: 1, "Relu": 1})


@case("fuse_conv")
def conv_dilation_2(kind="dense"):
    x, w, _b, _r = conv_data(k=3, seed=44, kind=kind)
    b = GB()
    y = b.un("Relu", kind_conv(b, kind, b.ph("x", x), w, dil=2))
    return alone(b, [y], {KINDS[kind][1]: 1, "Relu": 1})


@case("fuse_conv")
def conv_filter_is_fed(kind="dense"):
    x, w, _b, _r = conv_data(k=3, seed=45, kind=kind)
    b = GB()
    xs = b.ph("x", x)
    y = b.un("Relu", kind_conv(b, kind, xs, b.ph("w", w, dyn_batch=False)))
    return alone(b, [y], {KINDS[kind][1]: 1, "Relu": 1})


def _conv_bn(kind="dense", c_bn=C):
    """x, a 1x1 conv of `kind` on it, and BatchNorm parameters of `c_bn` elements."""
    x, w, _b, _r = conv_data(k=1, seed=50, kind=kind)
    params = bn_params(c_bn, 5)
    b = GB()
    xs = b.ph("x", x)
    return b, kind_conv(b, kind, xs, w), x, w, params


@case("fuse_conv")
def conv_bn_is_training(kind="dense"):
    b, y, x, w, params = _conv_bn(kind)
    y = b.un("Relu", b.bn(y, params, training=True))
    return make(b, [y], raises=True)


@case("fuse_conv")
def conv_bn_parameter_is_fed(kind="dense"):
    b, y, x, w, params = _conv_bn(kind)
    gamma = b.ph("gamma", bfv(params[0]), dyn_batch=False)
    y = b.un("Relu", b.bn(y, (gamma,) + tuple(params[1:])))
    p = (bfv(params[0]),) + tuple(params[1:])
    return make(b, [y], {KINDS[kind][2]: 1, "FusedBatchNormV3": 1, "Relu": 1},
                ref=lambda gpu=False: [kind_aff(kind, x, w).bn(p).out("relu", gpu)])


@case("fuse_conv", out=1)
@case("fuse_conv", out=2)
@case("fuse_conv", out=3)
@case("fuse_conv", out=4)
def conv_bn_statistic_consumed(out, kind="dense"):
    b, y, x, w, params = _conv_bn(kind)
    bn = b.bn(y, params)
    y = b.un("Relu", bn)
    stat = params[2] if out in (1, 3) else params[3]
    return make(b, [y, f"{bn}:{out}"], {KINDS[kind][2]: 1, "FusedBatchNormV3": 1, "Relu": 1},
                ref=lambda gpu=False: [kind_aff(kind, x, w).bn(params).out("relu", gpu), exact(stat)])


for _kind in ("depthwise", "grouped"):
    for _fn in (conv_pad_before_same, conv_explicit_paddings_with_a_batch_entry,
                conv_explicit_paddings_with_a_channel_entry, conv_nchw, conv_dilation_2, conv_filter_is_fed,
                conv_bn_is_training, conv_bn_parameter_is_fed):
        case(KINDS[_kind][0], kind=_kind)(_fn)
    for _which in ("batch", "channel"):
        case(KINDS[_kind][0], which=_which, kind=_kind)(conv_pad_outside_hw)
    for _out in (1, 2, 3, 4):
        case(KINDS[_kind][0], out=_out, kind=_kind)(conv_bn_statistic_consumed)


@case("fuse_conv")
def conv_bn_has_another_element_count():
    """A BatchNorm of C + 1 elements behind a conv with C outputs is no valid
    graph: the BatchNorm is not folded (the conv fuses without it, as the
    depthwise and the grouped pass always did), stays the interpreter's op, and
    refuses the batch with the same error in both programs."""
    b, y, _x, _w, params = _conv_bn(c_bn=C + 1)
    y = b.un("Relu", b.bn(y, params))
    return make(b, [y], {"_FusedConv2D": 1, "FusedBatchNormV3": 1, "Relu": 1}, raises="OpError")


@case("fuse_conv", gpu=True)
def conv_positive_c64():
    """The zoo shape: 3x3, 64 channels (the halo kernel on the device)."""
    x = bfv(rnd(B, 7, 9, 64, seed=61))
    w = bfv(rnd(3, 3, 64, 64, scale=1 / 24, seed=62))
    params = bn_params(64, 6)
    r = bfv(rnd(B, 7, 9, 64, seed=63))
    b = GB()
    y = b.un("Relu", b.bi("AddV2", b.bn(b.conv(b.ph("x", x), w), params), b.ph("r", r), "add"))
    return make(b, [y], {"_FusedConv2D": 1}, ref=lambda gpu=False: [Aff.conv(x, w).bn(params).add(r).out("relu", gpu)])


# ================================================================== fuse_matmul and the heads
M, K, N = 4, 16, 4                 # batch == N: a column added as a bias row type-checks


def mm_data(seed=0, m=M, k=K, n=N):
    x = bfv(rnd(m, k, seed=seed + 1))
    w = bfv(rnd(k, n, scale=1.6 / math.sqrt(k), seed=seed + 2))
    return x, w


@case("fuse_matmul", gpu=True, shape="N")
@case("fuse_matmul", gpu=True, shape="1N")
def matmul_add_const_folds(shape):
    x, w = mm_data(70)
    bv = wave([N] if shape == "N" else [1, N], 7, -1.0, 1.0)
    b = GB()
    y = b.un("Relu", b.bi("AddV2", b.matmul(b.ph("x", x), w), b.c(bv, "bias"), "add"))
    return make(b, [y], {"_FusedMatMul": 1}, ref=lambda gpu=False: [Aff.mm(x, w).add(bv).out("relu", gpu, out_f32=True)])


@case("fuse_matmul", gpu=True)
def matmul_add_const_column():
    """[N,1] with batch == N has N elements and adds a COLUMN: no bias."""
    x, w = mm_data(71)
    bv = wave([N, 1], 8, -1.0, 1.0)
    b = GB()
    y = b.bi("AddV2", b.matmul(b.ph("x", x), w), b.c(bv, "col"), "add")
    def ref(gpu=False):
        if not gpu:
            return [Aff.mm(x, w).add(bv).out("none")]
        # the GEMM's output feeds no head and is stored as bf16; the Add stays on torch in fp32
        r, bd = Aff.mm(x, w).out("none", True)
        s = r + kb.d(bv)
        return [(s, bd + E * (r.abs() + kb.d(bv).abs()) + kb.U_F32 * s.abs())]
    return make(b, [y], {"_FusedMatMul": 1, "AddV2": 1}, ref=ref)


@case("fuse_matmul")
def matmul_transpose_a():
    x, w = mm_data(72, m=K, k=M, n=N)          # x [K, M] read transposed against w [K, N]
    w = bfv(rnd(K, N, seed=73))
    b = GB()
    y = b.un("Relu", b.matmul(b.ph("x", x, dyn_batch=False), w, ta=True))
    return alone(b, [y], {"MatMul": 1, "Relu": 1})


@case("fuse_matmul", gpu=True)
def matmul_transpose_b():
    x, w = mm_data(74)
    b = GB()
    y = b.un("Tanh", b.matmul(b.ph("x", x), w.t().contiguous(), tb=True))
    return make(b, [y], {"_FusedMatMul": 1}, ref=lambda gpu=False: [Aff.mm(x, w).out("tanh", gpu, out_f32=True)])


@case("fuse_matmul", gpu=True, tap="MatMul")
@case("fuse_matmul", gpu=True, tap="BiasAdd")
@case("fuse_matmul", gpu=True, tap="Relu")
def matmul_intermediate_fetched(tap):
    x, w = mm_data(75)
    bv = wave([N], 9, -1.0, 1.0)
    r = bfv(rnd(M, N, seed=76))
    b = GB()
    t = [b.matmul(b.ph("x", x), w)]
    t.append(b.bias(t[-1], bv))
    t.append(b.un("Relu", t[-1]))
    y = b.bi("AddV2", t[-1], b.ph("r", r), "add")
    i = ["MatMul", "BiasAdd", "Relu"].index(tap)
    must = {"_FusedMatMul": 1, "AddV2": 1}
    must.update({op: 1 for op in ["BiasAdd", "Relu"][i:]})

    def ref(gpu=False):
        a = [Aff.mm(x, w)]
        a.append(a[0].add(bv))
        pre = a[1]
        fin_ref, fin_b = pre.out("relu", gpu, out_f32=True)
        tap_rb = [a[0].out("none", gpu, out_f32=True), a[1].out("none", gpu, out_f32=True), (fin_ref, fin_b)][i]
        return [(fin_ref + kb.d(r), fin_b + E * (fin_ref.abs() + kb.d(r).abs())), tap_rb]
    return make(b, [y, t[i]], must, ref=ref)


@case("fuse_matmul", gpu=True)
def matmul_residual_broadcasts():
    """A [1,N] non-constant operand: the residual, one row for every output row."""
    x, w = mm_data(77)
    bv = wave([N], 10, -1.0, 1.0)
    r = bfv(rnd(1, N, seed=78))
    b = GB()
    y = b.bi("AddV2", b.bias(b.matmul(b.ph("x", x), w), bv), b.ph("r", r, dyn_batch=False), "add")
    return make(b, [y], {"_FusedMatMul": 1},
                ref=lambda gpu=False: [Aff.mm(x, w).add(bv).add(r).out("none", gpu, out_f32=True)])


@case("fuse_matmul", gpu=True)
def matmul_add_operand_larger_than_the_output():
    """One row times W plus an [M,N] tensor: the GEMM output is the operand
    that broadcasts, so the sum cannot be the kernel's residual add."""
    x, w = mm_data(79, m=1)
    r = bfv(rnd(M, N, seed=79))
    b = GB()
    y = b.bi("AddV2", b.matmul(b.ph("x", x), w), b.ph("r", r), "add")

    def ref(gpu=False):
        # (on the device the GEMM's output is fetched through the sum, so it is fp32, and so is the torch add)
        c, d = Aff.mm(x, w).out("none", gpu, out_f32=True)
        s = c + kb.d(r)
        return [(s, d + E * (c.abs() + kb.d(r).abs()) + kb.U_F32 * s.abs())]
    return make(b, [y], {"_FusedMatMul": 1}, ref=ref)


def _gelu(b, x, c0=0.044715, tap=False):
    p = b.bi("Pow", x, b.c(3.0, "three"), "pow")
    m = b.bi("Mul", b.c(c0, "c0"), p, "g_mul")
    a = b.bi("AddV2", x, m, "g_add")
    m1 = b.bi("Mul", b.c(math.sqrt(2 / math.pi), "c1"), a, "g_mul1")
    t = b.un("Tanh", m1, "g_tanh")
    a1 = b.bi("AddV2", b.c(1.0, "one"), t, "g_add1")
    m2 = b.bi("Mul", b.c(0.5, "half"), a1, "g_mul2")
    return b.bi("Mul", x, m2, "g_out"), t


GELU_OPS = {"Pow": 1, "Mul": 4, "AddV2": 2, "Tanh": 1}


@case("fuse_matmul", gpu=True)
def matmul_gelu_positive():
    x, w = mm_data(80)
    bv = wave([N], 11, -1.0, 1.0)
    b = GB()
    y, _t = _gelu(b, b.bias(b.matmul(b.ph("x", x), w), bv))
    return make(b, [y], {"_FusedMatMul": 1},
                ref=lambda gpu=False: [Aff.mm(x, w).add(bv).out("gelu_tanh", gpu, out_f32=True)])


@case("fuse_matmul")
def matmul_gelu_interior_has_an_outside_reader():
    x, w = mm_data(81)
    b = GB()
    y, t = _gelu(b, b.matmul(b.ph("x", x), w))
    must = dict(GELU_OPS, _FusedMatMul=1)
    return make(b, [y, t], must, exact=True)


@case("fuse_matmul", c0=0.0449)
@case("fuse_matmul", c0=0.05)
def matmul_gelu_like_constant_is_off(c0):
    """0.044715 off by more than the matcher's 1e-4 (patterns._close): not GELU."""
    x, w = mm_data(82)
    b = GB()
    y, _t = _gelu(b, b.matmul(b.ph("x", x), w), c0=c0)
    return make(b, [y], dict(GELU_OPS, _FusedMatMul=1), exact=True)


HB, HH, HK, HN = 3, 2, 512, 10      # K = 512: the head kernel's smallest depth


def head_data(seed=90):
    x = bfv(rnd(HB, HH, HH, HK, seed=seed))
    w = bfv(rnd(HK, HN, scale=0.05, seed=seed + 1))
    bv = bfv(rnd(HN, scale=0.1, seed=seed + 2))
    return x, w, bv


def _head(keep=False, via=None, also=None, out="int64", regroup=False):
    x, w, bv = head_data()
    b = GB()
    pooled = b.mean(b.ph("x", x), [1, 2], keep)
    feat = pooled
    if via == "Squeeze":
        feat = b.n("Squeeze", "squeeze", [pooled], squeeze_dims=[1, 2])
    elif via == "Reshape":
        feat = b.reshape(pooled, [-1, HK])
    logits = b.bias(b.matmul(feat, w, "fc"), bv)
    scores = b.reshape(logits, [-1, HN // 2], "regroup") if regroup else logits
    probs, classes = b.un("Softmax", scores), b.argmax(scores, 1, out)
    fetches = [probs, classes] + ({"logits": [logits], "pooled": [pooled], None: []}[also])
    if also is None and not regroup:
        must = {"_ClassifierHead": 1}
    else:
        must = {"_GlobalAvgPool": 1, "_FusedMatMul": 1, "_SoftmaxArgMax": 1}
        if via:
            must[via] = 1
        if regroup:
            must["Reshape"] = 1
    must["Identity"] = 1               # the ArgMax node, now a name for the fused op's second output

    def ref(gpu=False):
        p, bound, logits64, dl = head_rb(x, w, bv, gpu)
        if regroup:
            logits64, dl = logits64.reshape(-1, HN // 2), dl.reshape(-1, HN // 2)
            p, bound = kb.softmax_ref(logits64, dl)
        outs = [(p, bound), classes_rb(logits64, dl)]
        if also == "logits":
            outs.append((logits64, kb.out_bound(logits64, dl, True)))
        elif also == "pooled":
            r, bd = mean_rb(x, [1, 2], keep, gpu)
            outs.append((r, bd))
        return outs
    return make(b, fetches, must, ref=ref)


@case("fuse_classifier_head", gpu=True, out="int64")
@case("fuse_classifier_head", gpu=True, out="int32")
def head_positive(out):
    return _head(out=out)


@case("fuse_classifier_head", gpu=True, via="Squeeze")
@case("fuse_classifier_head", gpu=True, via="Reshape")
def head_keep_dims_then(via):
    return _head(keep=True, via=via)


@case("fuse_classifier_head", gpu=True, also="logits")
@case("fuse_classifier_head", gpu=True, also="pooled")
def head_with_an_interior_fetch(also):
    return _head(also=also)


@case("fuse_classifier_head", gpu=True)
def head_logits_regrouped_before_the_softmax():
    """Reshape of the [B, N] logits to [2 B, N / 2]: the softmax rows are no longer the GEMM's."""
    return _head(regroup=True)


@case("fuse_dense_softmax", gpu=True)
def dense_softmax_positive():
    x, w = mm_data(95, m=3, k=16, n=2)
    bv = bfv(torch.tensor([0.25, -0.5]))
    b = GB()
    y = b.un("Softmax", b.bias(b.matmul(b.ph("x", x), w), bv))

    return make(b, [y], {"_DenseSoftmax": 1},
                ref=lambda gpu=False: [kb.dense_softmax_ref(x, kb.d(w).t().contiguous(), bv, 2)])


# ================================================================== fuse_pools, fuse_softmax_argmax
MEAN_SHAPES = {3: [B, 5, 8], 4: [B, 3, 5, 8], 5: [B, 2, 3, 4, 8]}


def mean_axes(rank, axes, keep):
    x = bfv(rnd(*MEAN_SHAPES[rank], seed=100 + rank))
    b = GB()
    y = b.mean(b.ph("x", x), axes, keep)
    fuses = sorted(axes) in ([1, 2], [-3, -2])
    must = {"_GlobalAvgPool": 1} if fuses else {"Mean": 1}
    return make(b, [y], must, exact=not fuses, ref=lambda gpu=False: [mean_rb(x, axes, keep, gpu)])


for _rank in (3, 4, 5):
    for _axes in ([1, 2], [2, 1], [-3, -2]):
        for _keep in (False, True):
            case("fuse_pools", gpu=True, rank=_rank, axes=_axes, keep=_keep)(mean_axes)
for _axes in ([1], [3], [1, 2, 3]):
    case("fuse_pools", rank=4, axes=_axes, keep=False)(mean_axes)


@case("fuse_pools", gpu=True, padding="SAME")
@case("fuse_pools", gpu=True, padding="VALID")
@case("fuse_pools", gpu=True, padding="EXPLICIT")
def maxpool_padding(padding):
    x = bfv(rnd(B, 6, 6, 8, seed=110))
    ep = [0, 0, 1, 1, 1, 1, 0, 0] if padding == "EXPLICIT" else []
    b = GB()
    y = b.maxpool(b.ph("x", x), 3, 2, padding, ep)
    p = fr.tf_pads(6, 6, 3, 3, 2, 2, padding, (1, 1, 1, 1))
    return make(b, [y], {"_MaxPool": 1}, ref=lambda gpu=False: [exact(kb.maxpool_ref(x, 3, 3, 2, 2, *p))])


@case("fuse_pools")
def maxpool_nchw():
    x = bfv(rnd(B, 8, 6, 6, seed=111))
    b = GB()
    return alone(b, [b.maxpool(b.ph("x", x), 3, 2, "SAME", fmt="NCHW")], {"MaxPool": 1})


@case("fuse_pools", ksize=[2, 3, 3, 1])
@case("fuse_pools", ksize=[1, 3, 3, 2])
def maxpool_window_over_batch_or_channel(ksize):
    x = bfv(rnd(B, 6, 6, 8, seed=112))
    b = GB()
    return alone(b, [b.maxpool(b.ph("x", x), 3, 2, "SAME", ksize=ksize)], {"MaxPool": 1})


def softmax_argmax(rank, axis, other=False):
    shape = [B, 7] if rank == 2 else [B, 5, 7]
    x = bfv(rnd(*shape, seed=120 + rank))
    z = bfv(rnd(*shape, seed=125 + rank))
    b = GB()
    xs = b.ph("x", x)
    src = b.ph("z", z) if other else xs
    probs, classes = b.un("Softmax", xs), b.argmax(src, axis)
    fuses = axis in (1, -1) and not other
    must = {"_SoftmaxArgMax": 1, "Identity": 1} if fuses else {"Softmax": 1, "ArgMax": 1}
    return make(b, [probs, classes], must, exact=not fuses,
                ref=lambda gpu=False: [kb.softmax_ref(x), exact(kb.d(z if other else x).argmax(axis))])


for _rank, _axis in ((2, -1), (2, 1), (3, -1), (3, 1), (3, 2)):
    case("fuse_softmax_argmax", gpu=True, rank=_rank, axis=_axis)(softmax_argmax)


@case("fuse_softmax_argmax")
def argmax_of_another_tensor():
    return softmax_argmax(2, -1, other=True)


# ================================================================== fuse_layernorm
LB, LS, LC = 2, 16, 16              # S == cols: a per-row gamma flattened to a per-column one type-checks
LN_EPS = 1e-5


def _layernorm(b, x, gamma, beta, axis=-1, axis2=None, keep=True, stop=True):
    mean = b.mean(x, [axis], keep, "ln/mean")
    sg = b.un("StopGradient", mean, "ln/sg") if stop else mean
    sqd = b.bi("SquaredDifference", x, sg, "ln/sqd")
    var = b.mean(sqd, [axis if axis2 is None else axis2], keep, "ln/var")
    rs = b.un("Rsqrt", b.bi("AddV2", var, b.c(LN_EPS, "ln/eps"), "ln/add"), "ln/rsqrt")
    m = b.bi("Mul", rs, b.c(gamma, "ln/gamma"), "ln/mul")
    m1, m2 = b.bi("Mul", x, m, "ln/mul1"), b.bi("Mul", mean, m, "ln/mul2")
    return b.bi("AddV2", m1, b.bi("Sub", b.c(beta, "ln/beta"), m2, "ln/sub"), "ln/out"), rs


LN_OPS = {"Mean": 2, "StopGradient": 1, "SquaredDifference": 1, "AddV2": 2, "Rsqrt": 1, "Mul": 3, "Sub": 1}


@case("fuse_layernorm", gpu=True, shape="cols")
@case("fuse_layernorm", gpu=True, shape="11cols")
@case("fuse_layernorm", gpu=True, shape="scalar")
@case("fuse_layernorm", gpu=True, shape="S1")
def layernorm_gamma_shape(shape):
    shp = {"cols": [LC], "11cols": [1, 1, LC], "scalar": [], "S1": [LS, 1]}[shape]
    gamma, beta = wave(shp, 13), wave(shp, 14, -0.5, 0.5)
    x = bfv(rnd(LB, LS, LC, seed=130) * 2 + 0.5)
    b = GB()
    y, _rs = _layernorm(b, b.ph("x", x), gamma, beta)
    fuses = shape != "S1"
    return make(b, [y], {"_LayerNorm": 1} if fuses else LN_OPS, exact=not fuses,
                ref=lambda gpu=False: [kb.layernorm_ref(kb.d(x), gamma.expand(LB, LS, LC) if shp else gamma,
                                                        beta.expand(LB, LS, LC) if shp else beta, LN_EPS,
                                                        out_f32=not (gpu and fuses))])


def _ln_alone(**kw):
    gamma, beta = wave([LC], 13), wave([LC], 14, -0.5, 0.5)
    x = bfv(rnd(LB, LS, LC, seed=131))
    b = GB()
    fetch_rs = kw.pop("fetch_rs", False)
    y, rs = _layernorm(b, b.ph("x", x), gamma, beta, **kw)
    return alone(b, [y] + ([rs] if fetch_rs else []), LN_OPS)


@case("fuse_layernorm")
def layernorm_axis_not_last():
    return _ln_alone(axis=1)


@case("fuse_layernorm")
def layernorm_means_over_different_axes():
    return _ln_alone(axis=-1, axis2=1)


@case("fuse_layernorm")
def layernorm_interior_fetched():
    return _ln_alone(fetch_rs=True)


@case("fuse_layernorm")
def layernorm_without_keep_dims():
    """[B,S,C] - mean[B,S] broadcasts along the wrong axes (S == C, B == 1 make it type-check)."""
    gamma, beta = wave([LC], 13), wave([LC], 14, -0.5, 0.5)
    x = bfv(rnd(1, LS, LC, seed=132))
    b = GB()
    y, _rs = _layernorm(b, b.ph("x", x), gamma, beta, keep=False)
    return alone(b, [y], LN_OPS)


# ================================================================== fuse_attention, fuse_embedding, fuse_key_mask
AB, AS, AHID = 2, 64, 64            # S = 64, head_dim = 64: the HIP attention kernel's shape


def _attention(heads=1, cross=False, fetch_probs=False, mask_after=False, final_rank=2, with_mask=True, batch=AB,
               q_bias_column=False):
    d = AHID // heads
    x = bfv(rnd(batch * AS, AHID, seed=140))
    x2 = bfv(rnd(batch * AS, AHID, seed=141))
    mask = (rnd(batch, AS, seed=142) > -1.0).int()
    mask[:, 0] = 1
    ws = [bfv(rnd(AHID, AHID, scale=1 / 8, seed=143 + i)) for i in range(3)]
    bs = [bfv(rnd(AHID, scale=0.1, seed=147 + i)) for i in range(3)]
    b = GB()
    xs = b.ph("x", x)
    ks = b.ph("x2", x2) if cross else xs
    adder = None
    if with_mask:
        m = b.g.node("Cast", "cast", [b.reshape(b.ph("mask", mask), [-1, 1, AS], "mask3")], SrcT=b.i32, DstT=b.f32,
                     Truncate=False)
        m = b.bi("Mul", b.c(torch.ones(1, AS, 1), "ones"), m, "bmask")
        ex = b.n("ExpandDims", "expand", [m, b.ints(1, "dim")], Tdim=b.i32)
        adder = b.bi("Mul", b.bi("Sub", b.c(1.0, "one"), ex, "sub"), b.c(-10000.0, "neg"), "adder")
    hs = []
    for i, (nm, src) in enumerate((("q", xs), ("k", ks), ("v", ks))):
        if q_bias_column and nm == "q":
            y = b.bi("AddV2", b.matmul(src, ws[i], nm), b.c(wave([batch * AS, 1], 14, -0.5, 0.5), "q_col"), nm + "_b")
        else:
            y = b.bias(b.matmul(src, ws[i], nm), bs[i], nm + "_b")
        y = b.reshape(y, [-1, AS, heads, d], nm + "_r")
        hs.append(b.n("Transpose", nm + "_t", [y, b.ints([0, 2, 1, 3], nm + "_p")], Tperm=b.i32))
    sc = b.n("BatchMatMulV2", "qk", [hs[0], hs[1]], adj_x=False, adj_y=True)
    sc = b.bi("Mul", sc, b.c(1.0 / math.sqrt(d), "scale"), "scaled")
    if adder is not None and not mask_after:
        sc = b.bi("AddV2", sc, adder, "masked")
    pr = b.un("Softmax", sc, "probs")
    pin = b.bi("AddV2", pr, adder, "masked_after") if (adder is not None and mask_after) else pr
    ctx = b.n("BatchMatMulV2", "pv", [pin, hs[2]], adj_x=False, adj_y=False)
    ctx = b.n("Transpose", "ctx_t", [ctx, b.ints([0, 2, 1, 3], "ctx_p")], Tperm=b.i32)
    out = b.reshape(ctx, [-1, AHID] if final_rank == 2 else [-1, AS, AHID], "ctx_r")
    fuses = not (cross or fetch_probs or mask_after or final_rank != 2 or q_bias_column)
    fetches = [out] + ([pr] if fetch_probs else [])
    scale = 1.0 / math.sqrt(d)
    add = None if not with_mask else ((1.0 - kb.d(mask).reshape(batch, 1, 1, AS)) * -10000.0)
    w_cat, b_cat = torch.cat(ws, 1), torch.cat(bs)

    def ref_unfused(gpu=False, prog=None):
        """Device only (on the CPU the case is compared with the interpreter
        bit for bit): the three projections are HIP GEMMs, whose stored bf16
        outputs are read back from the program's own ops and checked; the core
        stays on torch and is bounded by attention_on_torch."""
        assert gpu and not (cross or fetch_probs or mask_after or q_bias_column)
        ops = {node.name: node.attrs["_impl"] for _fn, node, _i, _o in prog.steps if node.op == "_FusedMatMul"}
        xd = x.to(prog.device)
        got, checks = [], []
        for i, nm in enumerate("qkv"):
            y = ops[nm + "_b"](None, None, [xd])[0]
            checks.append((y,) + Aff.mm(x, ws[i]).add(bs[i]).out("none", True))
            got.append(kb.d(y).reshape(batch, AS, heads, d).permute(0, 2, 1, 3))
        r, bd = attention_on_torch(got[0], got[1], got[2], scale, add)
        shape = [batch * AS, AHID] if final_rank == 2 else [batch, AS, AHID]
        return [(r.reshape(shape), bd.reshape(shape))] + checks

    if not fuses:
        return make(b, fetches, {"_FusedMatMul": 3}, maybe=("Reshape", "Transpose", "BatchMatMulV2", "Mul", "AddV2",
                                                            "Softmax", "Cast", "Sub", "ExpandDims"), exact=True,
                    ref_gpu=ref_unfused)

    def ref(gpu=False, prog=None):
        """On the device the attention op reads the QKV GEMM's stored bf16
        output: that output is read back from the program's own _FusedQKV op,
        checked against its own bound, and is what kb.attention_ref starts from."""
        qkv = kb.d(x) @ kb.d(w_cat) + kb.d(b_cat)
        checks = []
        if gpu:
            op, = [node.attrs["_impl"] for _fn, node, _i, _o in prog.steps if node.op == "_FusedQKV"]
            y = op(None, None, [x.to(prog.device)])[0]
            checks.append((y,) + Aff.mm(x, w_cat).add(b_cat).out("none", True))
            qkv = kb.d(y)
        r, bd = kb.attention_ref(qkv.reshape(batch, AS, 3 * AHID), heads, scale, add)
        return [(r.reshape(batch * AS, AHID), bd.reshape(batch * AS, AHID))] + checks
    must = {"_FusedQKV": 1, "_Attention": 1}
    if with_mask:
        must["_KeyMaskAdder"] = 1
        must["Reshape"] = 1
    return make(b, fetches, must, ref=ref)


def attention_on_torch(q, k, v, scale, adder):
    """(ref, bound) [B, S, H D] of the unfused attention core on the device,
    from the stored bf16 q, k, v [B, H, S, D] (fp64 here).  torch multiplies
    bf16 q k^T with fp32 accumulation and stores bf16, scales by the 0-d fp32
    constant in bf16 again, and from the fp32 mask adder on everything is fp32.
    kb.attention_ref's formula with that score error and no bf16 P:

        ds_j  = (D + 4) E (|q| . |k_j|) scale + 2 2^-8 |q . k_j| scale + 2 E |s_j|
        bound = ( sum_j p_j |v_j| ds_j + (P |V|) (sum_j p_j ds_j + (S + 16) E) ) (1 + 2^-24) + 2^-24 |ref|"""
    dh, s = q.shape[-1], q.shape[-2]
    raw = q @ k.transpose(-1, -2) * scale
    sc = raw if adder is None else raw + adder
    p = torch.softmax(sc, -1)
    ds = (dh + 4) * E * (q.abs() @ k.abs().transpose(-1, -2)) * scale + 2 * kb.U_BF16 * raw.abs() + 2 * E * sc.abs()
    ds = torch.where(p > 0, ds, torch.zeros_like(ds))
    ref, pav = p @ v, p @ v.abs()
    bound = ((p * ds) @ v.abs() + pav * ((p * ds).sum(-1, keepdim=True) + (s + 16) * E)) * (1 + kb.U_F32) + \
        kb.U_F32 * ref.abs()
    return ref.permute(0, 2, 1, 3), bound.permute(0, 2, 1, 3)


@case("fuse_attention", gpu=True)
def attention_positive():
    return _attention()


@case("fuse_attention", gpu=True)
def attention_head_dim_32():
    return _attention(heads=2)


@case("fuse_attention")
def attention_query_bias_is_a_column():
    """An [M, 1] constant with B S == N added to the query projection is no bias row."""
    return _attention(batch=1, q_bias_column=True)


@case("fuse_attention")
def attention_cross():
    return _attention(cross=True)


@case("fuse_attention")
def attention_probabilities_fetched():
    return _attention(fetch_probs=True)


@case("fuse_attention")
def attention_mask_added_after_the_softmax():
    return _attention(mask_after=True)


@case("fuse_attention", gpu=True)
def attention_output_keeps_the_sequence_axis():
    """Reshape to [-1, S, H D]: the fused op returns [B S, H D]."""
    return _attention(final_rank=3)


EV, ES, EH = 11, 16, 64          # hidden 64: the smallest row the embed_ln kernel is tested at


def _embedding(with_pos=True, ids_from_op=False, scalar=False):
    ids = torch.randint(0, EV, (LB, ES), generator=torch.Generator().manual_seed(150)).int()
    table = bfv(rnd(EV, EH, seed=151))
    pos = bfv(rnd(1, ES, EH, scale=0.5, seed=152))
    gamma, beta = wave([] if scalar else [EH], 15), wave([] if scalar else [EH], 16, -0.5, 0.5)
    b = GB()
    src = b.ph("ids", ids)
    if ids_from_op:
        src = b.g.node("Identity", "ids_copy", [b.g.node("Maximum", "clip", [src, b.ints(0, "zero")], T=b.i32)], T=b.i32)
    flat = b.g.node("Reshape", "flat", [src, b.ints([-1], "flat/s")], T=b.i32, Tshape=b.i32)
    emb = b.g.node("GatherV2", "gather", [b.c(table, "table"), flat, b.ints(0, "axis")], Tparams=b.f32, Tindices=b.i32,
                   Taxis=b.i32, batch_dims=0)
    emb = b.reshape(emb, [-1, ES, EH], "emb")
    # a sum in front of the LayerNorm is what the pass looks for: with no sum at all the gather stays
    if with_pos is not None:
        emb = b.bi("AddV2", emb, b.c(pos if with_pos else torch.zeros(1, ES, EH), "pos"), "emb_sum")
    y, _rs = _layernorm(b, emb, gamma, beta)

    def ref(gpu=False):
        z = kb.embed_sum(ids, None, table, pos.reshape(ES, EH) if with_pos else None, None, ES)
        r, bd = kb.layernorm_ref(z.reshape(LB, ES, EH), gamma, beta, LN_EPS, out_f32=not gpu)
        return [(r, bd)]
    must = {"_EmbeddingLN": 1, "Reshape": 1}        # (the ids' own Reshape to [-1] is no part of the pattern)
    if with_pos is None:
        must = {"_LayerNorm": 1, "GatherV2": 1, "Reshape": 2}
    maybe = ("Maximum", "Identity") if ids_from_op else ()
    return make(b, [y], must, maybe, ref=ref)


@case("fuse_embedding", gpu=True)
def embedding_positive():
    return _embedding()


@case("fuse_embedding", gpu=True)
def embedding_scalar_gamma_and_beta():
    return _embedding(scalar=True)


@case("fuse_embedding", gpu=True)
def embedding_ids_from_an_op():
    return _embedding(ids_from_op=True)


@case("fuse_embedding", gpu=True)
def embedding_position_term_is_zero():
    return _embedding(with_pos=False)


@case("fuse_embedding", gpu=True)
def embedding_position_term_missing():
    return _embedding(with_pos=None)


# ================================================================== fuse_post_activation, fuse_stem_pool
def _stem(pool_k=3, fetch=None):
    x = bfv(rnd(B, 18, 18, 3, seed=160))
    w = bfv(rnd(7, 7, 3, 16, scale=1 / 12, seed=161))
    bv = bfv(rnd(16, scale=0.2, seed=162))
    b = GB()
    cv = b.bias(b.conv(b.ph("x", x), w, stride=2), bv)
    rl = b.un("Relu", cv)
    y = b.maxpool(rl, pool_k, 2, "SAME")
    fetches = [y] + ({"conv": [cv], "relu": [rl], None: []}[fetch])
    if pool_k == 3 and fetch is None:
        must = {"_StemPool": 1}
    else:
        must = {"_FusedConv2D": 1, "_MaxPool": 1}
        if fetch == "conv":
            must["Relu"] = 1

    def ref(gpu=False):
        a = Aff.conv(x, w, (2, 2), "SAME").add(bv)
        r, bd = a.out("relu", gpu)
        pp = fr.tf_pads(r.shape[1], r.shape[2], pool_k, pool_k, 2, 2, "SAME")
        # rounding is monotone: the pooled value is off by the largest error in its window
        bp = F.max_pool2d(F.pad(bd.permute(0, 3, 1, 2), [pp[2], pp[3], pp[0], pp[1]]), pool_k, 2).permute(0, 2, 3, 1)
        outs = [(kb.maxpool_ref(r, pool_k, pool_k, 2, 2, *pp), bp)]
        if fetch == "conv":
            outs.append(a.out("none", gpu))
        elif fetch == "relu":
            outs.append((r, bd))
        return outs
    return make(b, fetches, must, ref=ref)


@case("fuse_stem_pool", gpu=True)
def stem_positive():
    return _stem()


@case("fuse_stem_pool", gpu=True, fetch="conv")
@case("fuse_stem_pool", gpu=True, fetch="relu")
def stem_interior_fetched(fetch):
    return _stem(fetch=fetch)


@case("fuse_stem_pool")
def stem_followed_by_a_2x2_pool():
    return _stem(pool_k=2)


def _preact(third=False, fetch_sum=False):
    """conv1's sum -> BN -> Relu -> conv2, plus conv2's shortcut add of the sum
    (ResNet v2): conv1 writes [sum, relu(bn(sum))]."""
    c = 64
    x = bfv(rnd(B, 5, 6, c, seed=170))
    w1, w2 = bfv(rnd(3, 3, c, c, scale=1 / 24, seed=171)), bfv(rnd(1, 1, c, c, scale=1 / 8, seed=172))
    params = bn_params(c, 17)
    b = GB()
    y1 = b.conv(b.ph("x", x), w1, name="conv1")
    pre = b.un("Relu", b.bn(y1, params))
    y2 = b.conv(pre, w2, name="conv2")
    out = b.bi("AddV2", y2, y1, "sum")
    fetches = [out] + ([b.un("Tanh", pre, "third")] if third else []) + ([y1] if fetch_sum else [])
    must = {"_FusedConv2D": 2}
    if third:
        must["Tanh"] = 1
    if fetch_sum:
        must.update(FusedBatchNormV3=1, Relu=1)

    def ref(gpu=False):
        a1 = Aff.conv(x, w1)
        r1, d1 = a1.out("none", gpu)
        gamma, beta, mean, var = (kb.d(p) for p in params)
        inv = gamma / torch.sqrt(var + BN_EPS)
        shift, shift_mag = beta - mean * inv, beta.abs() + (mean * inv).abs()
        if not gpu:
            rz, dz = a1.bn(params).out("relu")
        elif not fetch_sum:
            # the conv's second output: the affine of the fp32 epilogue value (kb.post_output), with
            # STEP roundings each for the fp32 scale and shift the pass computes
            rz, dz = kb.post_output(a1.pre, a1.mag, a1.k + 2 * STEP, GPU_SPLITS, inv, shift, "relu")
        else:
            # the fetched sum is stored as bf16 and the BatchNorm stays on torch: fp32 from that value, stored as bf16
            pz = r1 * inv + shift
            rz = torch.relu(pz)
            dz = kb.out_bound(rz, d1 * inv.abs() + STEP * E * ((r1 * inv).abs() + shift_mag), False)
        a2 = Aff.conv(rz, w2)
        # conv2 reads the (slightly wrong) z and adds the (slightly wrong) sum
        acc = kb.acc_bound(a2.pre + r1, a2.mag + r1.abs(), a2.k, GPU_SPLITS if gpu else 1, "none") + \
            (dz.reshape(-1, c) @ kb.d(w2).reshape(c, c).abs()).reshape(d1.shape) + d1
        outs = [(a2.pre + r1, kb.out_bound(a2.pre + r1, acc, not gpu))]
        if third:
            t = torch.tanh(rz)
            outs.append((t, dz + kb.act_abs("tanh", rz) + kb.u_out(not gpu) * t.abs()))
        if fetch_sum:
            outs.append((r1, d1))
        return outs
    return make(b, fetches, must, ref=ref)


@case("fuse_post_activation", gpu=True)
def preactivation_positive():
    return _preact()


@case("fuse_post_activation", gpu=True)
def preactivation_output_has_a_third_reader():
    return _preact(third=True)


@case("fuse_post_activation", gpu=True)
def preactivation_sum_fetched():
    return _preact(fetch_sum=True)


# ================================================================== fuse_dual_conv (a device-only pass)
def _projecting_block(project_k=1, project_broadcasts=False):
    """relu(BN(conv1x1(h)) + BN(conv(x, stride 2))): a ResNet projecting
    block.  64 channels, so that on the device only the guard under test keeps
    (or does not keep) the two convs from becoming one _FusedDualConv."""
    c = 64
    h = bfv(rnd(B, 4, 5, c, seed=180))
    x = bfv(rnd(B, 1, 1, c, seed=181)) if project_broadcasts else bfv(rnd(B, 8, 9, c, seed=181))
    wa = bfv(rnd(1, 1, c, c, scale=1 / 8, seed=182))
    wb = bfv(rnd(project_k, project_k, c, c, scale=1 / (8 * project_k), seed=183))
    pa, pb = bn_params(c, 18), bn_params(c, 19)
    stride = 1 if project_broadcasts else 2
    b = GB()
    ya = b.bn(b.conv(b.ph("h", h), wa, name="expand"), pa, "bn_a")
    yb = b.bn(b.conv(b.ph("x", x), wb, stride=stride, name="project"), pb, "bn_b")
    y = b.un("Relu", b.bi("AddV2", ya, yb, "sum"))

    def ref(gpu=False):
        ea, eb = Aff.conv(h, wa).bn(pa), Aff.conv(x, wb, (stride, stride)).bn(pb)
        if gpu and project_k != 1:
            # two launches: the projection is stored as bf16 and read back as the residual
            rb, db = eb.out("none", True)
            r, d = ea.add(rb).out("relu", True)
            return [(r, d + db * (1 + kb.U_BF16))]
        # one sum of both dot products (on the CPU the projection's fp32 error rides along in the same bound)
        both = Aff(ea.pre + eb.pre, ea.dot + eb.dot, ea.k + eb.k)
        both.mag, both.steps, both.wfold = ea.mag + eb.mag, ea.steps + eb.steps + 1, True
        return [both.out("relu", gpu)]
    dual = {"_FusedDualConv": 1} if project_k == 1 else {"_FusedConv2D": 2}
    return make(b, [y], {"_FusedConv2D": 2}, ref=ref, must_gpu=dual)


@case("fuse_dual_conv", gpu=True)
def dual_positive():
    return _projecting_block()


@case("fuse_dual_conv", gpu=True)
def dual_projection_is_3x3():
    return _projecting_block(project_k=3)


@case("fuse_dual_conv", gpu=True)
def dual_projection_only_broadcasts():
    """Strides that disagree with the shapes: the projection's [B,1,1,C]
    output broadcasts against the expand conv's [B,4,5,C]."""
    return _projecting_block(project_broadcasts=True)


# ================================================================== fuse_conv_chain (a device-only pass)
def _chain_pair(middle=None, residual=None):
    """A bottleneck's expand 1x1 (64 -> 256, bias, [residual,] ReLU) feeding
    the next reduce 1x1 (256 -> 64, bias, ReLU): kernels/chain.hip's stage-1
    shape.  `middle`: the expand output is also fetched, or read by a Tanh."""
    c1, c2 = 64, 256
    x = bfv(rnd(B, 5, 8, c1, seed=190))          # 80 rows: a 64-row tile and a partial one
    wa = bfv(rnd(1, 1, c1, c2, scale=1 / 8, seed=191))
    wb = bfv(rnd(1, 1, c2, c1, scale=1 / 16, seed=192))
    ba, bb = bfv(rnd(c2, scale=0.3, seed=193)), bfv(rnd(c1, scale=0.3, seed=194))
    r = {None: None, "full": bfv(rnd(B, 5, 8, c2, seed=195)), "B11C": bfv(rnd(B, 1, 1, c2, seed=195))}[residual]
    b = GB()
    y1 = b.bias(b.conv(b.ph("x", x), wa, name="expand"), ba, "expand_b")
    if r is not None:
        y1 = b.bi("AddV2", y1, b.ph("r", r), "shortcut")
    y1 = b.un("Relu", y1, "block_out")
    y2 = b.un("Relu", b.bias(b.conv(y1, wb, name="reduce"), bb, "reduce_b"), "reduce_out")
    # (the reduce's output must have a reader of its own: the pass renames outputs, and a fetch keeps its name)
    out = b.un("Tanh", y2, "after")
    fetches = [out] + ({None: [], "fetched": [y1], "third": [b.un("Tanh", y1, "side")]}[middle])
    tanhs = 2 if middle == "third" else 1
    must = {"_FusedConv2D": 2, "Tanh": tanhs}
    must_gpu = {"_FusedConv2D": 2, "Tanh": tanhs} if middle == "fetched" else {"_ChainConv": 1, "Tanh": tanhs}

    def ref(gpu=False):
        a1 = Aff.conv(x, wa).add(ba)
        r1, d1 = (a1 if r is None else a1.add(r)).out("relu", gpu)
        a2 = Aff.conv(r1, wb).add(bb)
        # the reduce reads the stored (slightly wrong) block output: its error goes through |W|
        acc = kb.acc_bound(a2.pre, a2.mag, a2.k + STEP, GPU_SPLITS if gpu else 1, "relu") + \
            (d1.reshape(-1, c2) @ kb.d(wb).reshape(c2, c1).abs()).reshape(a2.pre.shape)
        r2 = torch.relu(a2.pre)
        t2 = torch.tanh(r2)
        outs = [(t2, kb.out_bound(r2, acc, not gpu) + kb.act_abs("tanh", r2) + kb.u_out(not gpu) * t2.abs())]
        if middle == "fetched":
            outs.append((r1, d1))
        elif middle == "third":
            t = torch.tanh(r1)
            outs.append((t, d1 + kb.act_abs("tanh", r1) + kb.u_out(not gpu) * t.abs()))
        return outs
    return make(b, fetches, must, ref=ref, must_gpu=must_gpu)


@case("fuse_conv_chain", gpu=True)
def chain_positive():
    return _chain_pair()


@case("fuse_conv_chain", gpu=True)
def chain_positive_with_a_shortcut():
    return _chain_pair(residual="full")


@case("fuse_conv_chain", gpu=True)
def chain_middle_fetched():
    return _chain_pair(middle="fetched")


@case("fuse_conv_chain", gpu=True)
def chain_middle_read_by_a_third_op():
    return _chain_pair(middle="third")


@case("fuse_conv_chain", gpu=True)
def chain_shortcut_broadcasts():
    """A [B,1,1,C] shortcut: the chain kernel reads one residual element per
    output element, so the op runs its two convs, the first expanding it."""
    return _chain_pair(residual="B11C")
